// emitter_query.h - the host side that the eight queries over an emitter table share: {direct, nee} x {plain, mis} x {uniform, pick}
// (direct.hip, nee.hip).  Host code only, no kernel.  What a variant adds to a call (EmitterVariant), the weighted queries' own parameter
// check (emitter_mis_check), the checks of the tables as an ordered list of steps per query (EmitterStep, emitter_steps_run) and the two
// forms after the family's parameter check (emitter_query_on_device, emitter_query_on_host), with the family's labels and launcher handed
// in.  THE STEP LISTS BESIDE THE ENTRY POINTS ARE WHERE THE ORDER OF A QUERY'S TABLE CHECKS IS STATED (tinyrt.h documents it).
// The function templates here are static: the library exports nothing of them.  Needs host_stage.h and emitter_pick.h.  The two steps
// that are not the pick table's are defined where the device compiler is needed (gather_draw.h / radiance.hip, mis_weight.h) and only
// declared here, so that tests/native/emitter_query_check.cpp drives all of this on the simulated runtime with steps of its own in their
// place.
#pragma once

#include <stddef.h>

#include "emitter_pick.h"
#include "host_stage.h"

namespace trt {

int emitter_entries_check(const trt_emitter* emitters, uint32_t n_emitters);                              // radiance.hip (gather_draw.h)
inline int nee_mis_table_check(const trt_scene* s, const trt_emitter* emitters, uint32_t n_emitters);     // mis_weight.h

// What the variants add to a call, after the checks: DirectCall and NeeCall derive from it.
struct EmitterVariant {
    bool mis = false;                // the weighted kernels, with `heuristic`
    uint32_t heuristic = 0u;
    bool pick = false;               // the PICK kernels, with an alias table (and, weighted, `total_power`)
    float total_power = 0.0f;
};

// The weighted queries' own parameters (trt_direct_mis_params, trt_nee_mis_params), after the check of the struct they wrap.
template <class MisParams>
static int emitter_mis_check(const MisParams& p, EmitterVariant& v) {
    if (p.heuristic > TRT_MIS_POWER) return query_fail(TRT_ERR_INVALID_ARG, "heuristic must be TRT_MIS_BALANCE or TRT_MIS_POWER");
    for (uint32_t r : p.reserved)
        if (r != 0u) return query_fail(TRT_ERR_INVALID_ARG, "reserved words must be zero");
    v.mis = true;
    v.heuristic = p.heuristic;
    return TRT_OK;
}

// The tables of a call as the entry point was handed them (host or device pointers), and the checks of them.  STEP_PICK_POINTER looks
// at the pointer only: both forms, and it looks at n itself.  The other steps read the tables: host form only, n > 0 only.
struct EmitterTables {
    const trt_emitter* emitters;
    const trt_emitter_pick* pick;    // nullptr: no PICK query
    uint32_t n_emitters;
    float total_power;               // of the weighted PICK queries
};
enum EmitterStep {
    STEP_PICK_POINTER,               // emitter_pick.h pick_pointer_check; the query is a PICK query
    STEP_EMITTER_ENTRIES,            // emitter_entries_check: every record's kind and reserved words
    STEP_TABLE_RULE,                 // nee_mis_table_check: the records with a geometry are the scene's lights, each once
    STEP_PICK_ENTRIES,               // emitter_pick.h pick_entries_check: every pick record, then "can be chosen with prob 0"
    STEP_PICK_POWER,                 // emitter_pick.h pick_power_check: total_power, then prob bit for bit; the query takes total_power
};
enum EmitterForm { FORM_HOST, FORM_DEVICE };

// Runs the steps in the order listed and stops at the first that fails; sets v.pick / v.total_power for the steps that say so.
template <size_t K>
static int emitter_steps_run(const trt_scene* s, uint32_t n, const EmitterTables& t, EmitterForm form, const EmitterStep (&steps)[K], EmitterVariant& v) {
    const bool reads = form == FORM_HOST && n > 0u;
    for (const EmitterStep step : steps) {
        int rc = TRT_OK;
        switch (step) {
        case STEP_PICK_POINTER: rc = pick_pointer_check(n, t.pick); v.pick = true; break;
        case STEP_EMITTER_ENTRIES: if (reads) rc = emitter_entries_check(t.emitters, t.n_emitters); break;
        case STEP_TABLE_RULE: if (reads) rc = nee_mis_table_check(s, t.emitters, t.n_emitters); break;
        case STEP_PICK_ENTRIES: if (reads) rc = pick_entries_check(t.pick, t.n_emitters); break;
        case STEP_PICK_POWER: if (reads) rc = pick_power_check(t.emitters, t.pick, t.n_emitters, t.total_power); v.total_power = t.total_power; break;
        }
        if (rc != TRT_OK) return rc;
    }
    return TRT_OK;
}

// What a family's failures are called.
struct EmitterLabels {
    const char *buffers, *launch;
};

// The two forms after the family's parameter check.  `c` is the family's call (an EmitterVariant with `ra` and nothing()); launch is its
// launcher: launch(qs, c, d_items, n, d_emitters, d_pick, d_radiance, d_moment2, d_counters, stream).
template <class Call, size_t K, class Launch>
static int emitter_query_on_device(trt_scene* s, Call& c, const EmitterStep (&steps)[K], const EmitterLabels& what, Launch&& launch,
                                   const trt_ray* d_items, uint32_t n, const EmitterTables& t, float* d_radiance, float* d_moment2, uint64_t* d_counters,
                                   void* stream) {
    const int rc = emitter_steps_run(s, n, t, FORM_DEVICE, steps, c);
    if (rc != TRT_OK) return rc;
    return sample_query_on_device(s, n, what.launch, [&](const QueryScene& qs) {
        return launch(qs, c, reinterpret_cast<const float*>(d_items), n, reinterpret_cast<const float*>(t.emitters), reinterpret_cast<const float*>(t.pick),
                      d_radiance, d_moment2, reinterpret_cast<unsigned long long*>(d_counters), static_cast<hipStream_t>(stream));
    });
}
// Host buffers (inside host_form): staged by host_stage.h sample_query_on_host (items | table | sums | second moments, if wanted |
// counters | pick table, if any).
template <class Call, size_t K, class Launch>
static int emitter_query_on_host(trt_scene* s, Call& c, const EmitterStep (&steps)[K], const EmitterLabels& what, Launch&& launch,
                                 const trt_ray* items, uint32_t n, const EmitterTables& t, float* radiance, float* moment2, trt_stats* stats) {
    const int rc = emitter_steps_run(s, n, t, FORM_HOST, steps, c);
    if (rc != TRT_OK) return rc;
    const size_t sums = (size_t)n * 12u;
    SampleHost h{items, (size_t)n * sizeof(trt_ray), "hipMemcpy of the items", t.emitters, (size_t)t.n_emitters * sizeof(trt_emitter),
                 "hipMemcpy of the emitters", radiance, sums, moment2, sums, "hipMemcpy of the second moments"};
    if (c.pick) { h.table2 = t.pick; h.table2_b = (size_t)t.n_emitters * sizeof(trt_emitter_pick); h.table2_what = "hipMemcpy of the pick table"; }
    return sample_query_on_host(s, n, h, c.ra.accumulate != 0u, c.nothing(), what.buffers, what.launch, stats, [&](const QueryScene& qs, const SampleDev& d) {
        return launch(qs, c, d.items, n, d.table, d.table2, d.sums, d.sums2, d.counters, nullptr);
    });
}

}  // namespace trt
