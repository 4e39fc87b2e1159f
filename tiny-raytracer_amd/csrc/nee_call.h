// nee_call.h - the host side that the next-event units share (nee.hip: trt_nee, trt_nee_mis, trt_nee_pick, trt_nee_mis_pick; nee_samples.hip:
// trt_nee_samples): what a call asks of the device after the checks (NeeCall), the family's parameter check (nee_check), the family's
// labels and the four queries' step lists over their tables (emitter_query.h).  Host code only, no kernel: one copy, so that the sample
// query checks what its folding siblings check, in their order.  Everything here has internal linkage.  Needs gather_draw.h (the checks
// of the path, the source and the table's size) and emitter_query.h.
#pragma once

#include "emitter_query.h"
#include "gather_draw.h"

namespace trt {
namespace {

// What a call asks of the device, after the checks; the variant's fields are emitter_query.h's.
struct NeeCall : EmitterVariant {
    RenderArgs ra;                   // of the path parameters (radiance_check)
    uint32_t samples_per_item, first_stream;
    uint32_t source;
    float spread;
    uint32_t n_emitters;
    float shadow_end;
    uint32_t source_is_diffuse;
    bool nothing() const { return ra.sample_begin == ra.sample_end || ra.max_bounces == 0u; }
};

// What both forms check before any device work: trt_passes' rules on p->gather (radiance_check on the path, the source, the cone's spread,
// the reserved words), trt_direct's on the table's size and on shadow_end, then this struct's own fields.  The table's entries are the
// host form's to check: the device form cannot read them.
int nee_check(const trt_scene* s, const trt_ray* items, uint32_t n, const trt_emitter* emitters, uint32_t n_emitters, const trt_nee_params* p,
              const float* radiance, NeeCall& c) {
    if (!p) return query_fail(TRT_ERR_INVALID_ARG, "null argument");
    const trt_gather_params& g = p->gather;
    int rc = radiance_check(s, items, n, &g.path, radiance, c.ra);
    if (rc != TRT_OK) return rc;
    rc = gather_source_check(g);
    if (rc != TRT_OK) return rc;
    rc = emitter_table_check(n, emitters, n_emitters, p->shadow_end);
    if (rc != TRT_OK) return rc;
    if (p->source_is_diffuse > 1u) return query_fail(TRT_ERR_INVALID_ARG, "source_is_diffuse must be 0 or 1");
    for (uint32_t r : p->reserved)
        if (r != 0u) return query_fail(TRT_ERR_INVALID_ARG, "reserved words must be zero");
    c.samples_per_item = g.path.samples_per_ray;
    c.first_stream = g.path.first_stream;
    c.source = g.lobe;
    c.spread = g.lobe == TRT_PASSES_RAYS ? 0.0f : g.spread;
    c.n_emitters = n_emitters;
    c.shadow_end = p->shadow_end;
    c.source_is_diffuse = p->source_is_diffuse;
    return TRT_OK;
}
// trt_nee_mis' checks before any device work: trt_nee's on p->nee, then the heuristic and this struct's reserved words.
[[maybe_unused]] int nee_check(const trt_scene* s, const trt_ray* items, uint32_t n, const trt_emitter* emitters, uint32_t n_emitters,
                               const trt_nee_mis_params* p, const float* radiance, NeeCall& c) {
    if (!p) return query_fail(TRT_ERR_INVALID_ARG, "null argument");
    const int rc = nee_check(s, items, n, emitters, n_emitters, &p->nee, radiance, c);
    return rc != TRT_OK ? rc : emitter_mis_check(*p, c);
}

constexpr EmitterLabels kNeeLabels{"next-event query buffers", "next-event query launch"};

// THE ORDER OF EACH QUERY'S TABLE CHECKS (tinyrt.h), behind trt_nee's / trt_nee_mis' own.  The host form runs every step, the device
// form the pointer's only: it cannot read a table, and the rules are the caller's to keep (the kernel's clamp keeps a wrong pick table's
// reads inside the E records).  An empty batch reads no table either.
constexpr EmitterStep kNeeSteps[] = {STEP_EMITTER_ENTRIES};
constexpr EmitterStep kNeeMisSteps[] = {STEP_EMITTER_ENTRIES, STEP_TABLE_RULE};
constexpr EmitterStep kNeePickSteps[] = {STEP_PICK_POINTER, STEP_EMITTER_ENTRIES, STEP_PICK_ENTRIES};
// the pick records BEFORE the table rule (trt_direct_mis_pick has them the other way round)
constexpr EmitterStep kNeeMisPickSteps[] = {STEP_PICK_POINTER, STEP_EMITTER_ENTRIES, STEP_PICK_ENTRIES, STEP_TABLE_RULE, STEP_PICK_POWER};

}  // namespace
}  // namespace trt
