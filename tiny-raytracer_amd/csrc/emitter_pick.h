// emitter_pick.h - the alias table of the direct-light queries that choose their emitter by power (tinyrt.h trt_emitter_pick,
// trt_emitter_pick_build, trt_direct_pick, trt_direct_mis_pick): host code only, no kernel.  The builder - the header's rules for the
// weights, the total and prob, Vose's construction in double with the header's list order - and what the host forms check of a table
// before any device work.  Needs scene_query.h (query_fail) and nothing of the kernel units: tests/native/emitter_pick_check.cpp drives
// all of it under the sanitizers.  The device side of the table is gather_draw.h AliasPick.
#pragma once

#include <cstddef>
#include <cstring>
#include <vector>

#include "scene_query.h"

namespace trt {

static_assert(sizeof(trt_emitter_pick) == 16 && offsetof(trt_emitter_pick, q) == 0 && offsetof(trt_emitter_pick, alias) == 4 &&
              offsetof(trt_emitter_pick, prob) == 8 && offsetof(trt_emitter_pick, reserved) == 12, "trt_emitter_pick layout (tinyrt.h; gather_draw.h AliasPick)");

// An emitter's power as the header states it: f32, one IEEE operation per operator (-ffp-contract=off: nothing fused).  mis_weight.h repeats
// these operations on the device.
inline float emitter_power(const trt_emitter& e) {
    return ((0.2126f * e.color.x + 0.7152f * e.color.y) + 0.0722f * e.color.z) * e.area;
}
// The weights' sum in double in table order, rounded once; 0 with `ok` false where a weight is negative or no number.
inline float weights_total(const trt_emitter* emitters, const float* weights, uint32_t n_emitters, bool& ok) {
    double sum = 0.0;
    ok = true;
    for (uint32_t e = 0; e < n_emitters; e++) {
        const float w = weights ? weights[e] : emitter_power(emitters[e]);
        if (!(w >= 0.0f) || !(w < __builtin_inff())) { ok = false; return 0.0f; }
        sum += (double)w;
    }
    return (float)sum;
}

inline int pick_build(const trt_emitter* emitters, uint32_t n_emitters, const float* weights, trt_emitter_pick* out, float* total_out) {
    if (!emitters || !out) return query_fail(TRT_ERR_INVALID_ARG, "null argument");
    if (n_emitters == 0u || n_emitters > (1u << 20)) return query_fail(TRT_ERR_INVALID_ARG, "n_emitters must be 1 .. 2^20");
    bool ok;
    const float total = weights_total(emitters, weights, n_emitters, ok);
    if (!ok) return query_fail(TRT_ERR_INVALID_ARG, "a weight is negative or not finite");
    if (!(total > 0.0f) || !(total < __builtin_inff())) return query_fail(TRT_ERR_INVALID_ARG, "the weights' total must be positive and finite");
    // prob, and the construction's weights: an emitter whose prob is 0 (its own weight is, or the division underflows) is never chosen
    // (their sum S is compensated, Neumaier's way: a plain sum's error, times E, would all land on the slot the construction ends with)
    std::vector<double> scaled(n_emitters);
    double sum = 0.0, lost = 0.0;
    uint32_t heaviest = 0;
    for (uint32_t e = 0; e < n_emitters; e++) {
        const float w = weights ? weights[e] : emitter_power(emitters[e]);
        out[e] = trt_emitter_pick{0.0f, e, w / total, 0u};
        scaled[e] = out[e].prob > 0.0f ? (double)w : 0.0;
        const double x = scaled[e], t = sum + x;
        lost += sum >= x ? (sum - t) + x : (x - t) + sum;
        sum = t;
        if (scaled[e] > scaled[heaviest]) heaviest = e;
    }
    sum += lost;
    for (double& x : scaled) x = (x * (double)n_emitters) / sum;
    // Vose: both lists filled in index order, emptied from the back; what is left of a large one goes to the back of its new list
    std::vector<uint32_t> small, large;
    for (uint32_t e = 0; e < n_emitters; e++) (scaled[e] < 1.0 ? small : large).push_back(e);
    std::vector<double> q(n_emitters, 1.0);
    while (!small.empty() && !large.empty()) {
        const uint32_t sm = small.back(), lg = large.back();
        small.pop_back();
        large.pop_back();
        q[sm] = scaled[sm];
        out[sm].alias = lg;
        scaled[lg] = (scaled[lg] + scaled[sm]) - 1.0;
        (scaled[lg] < 1.0 ? small : large).push_back(lg);
    }
    // left over by rounding: q = 1 and its own alias - but an emitter of no weight stays unchosen
    for (const uint32_t sm : small)
        if (scaled[sm] == 0.0) { q[sm] = 0.0; out[sm].alias = heaviest; }
    for (uint32_t e = 0; e < n_emitters; e++) {
        const float f = (float)q[e];
        out[e].q = f < 0.0f ? 0.0f : (f > 1.0f ? 1.0f : f);
    }
    if (total_out) *total_out = total;
    return TRT_OK;
}

// What a PICK query checks besides: the pointer (both forms, n > 0) ...
inline int pick_pointer_check(uint32_t n, const trt_emitter_pick* pick) {
    if (n > 0u && !pick) return query_fail(TRT_ERR_INVALID_ARG, "null argument");
    return TRT_OK;
}
// ... and the records, which only a host form can read.
inline int pick_entries_check(const trt_emitter_pick* pick, uint32_t n_emitters) {
    for (uint32_t k = 0; k < n_emitters; k++) {
        const trt_emitter_pick& r = pick[k];
        if (!(r.q >= 0.0f && r.q <= 1.0f)) return query_fail(TRT_ERR_INVALID_ARG, "pick: q must be in [0, 1]");
        if (r.alias >= n_emitters) return query_fail(TRT_ERR_INVALID_ARG, "pick: alias must be below n_emitters");
        if (!(r.prob >= 0.0f && r.prob <= 1.0f)) return query_fail(TRT_ERR_INVALID_ARG, "pick: prob must be in [0, 1]");
        if (r.reserved != 0u) return query_fail(TRT_ERR_INVALID_ARG, "reserved words must be zero");
    }
    for (uint32_t k = 0; k < n_emitters; k++) {
        const trt_emitter_pick& r = pick[k];
        if ((r.q > 0.0f && r.prob == 0.0f) || (r.q < 1.0f && pick[r.alias].prob == 0.0f))
            return query_fail(TRT_ERR_INVALID_ARG, "pick: an emitter that can be chosen has prob 0");
    }
    return TRT_OK;
}
// The weighted PICK query's table rule besides trt_direct_mis': prob is the power rule's, bit for bit, under this total_power.
inline int pick_power_check(const trt_emitter* emitters, const trt_emitter_pick* pick, uint32_t n_emitters, float total_power) {
    if (!(total_power > 0.0f) || !(total_power < __builtin_inff())) return query_fail(TRT_ERR_INVALID_ARG, "total_power must be positive and finite");
    for (uint32_t e = 0; e < n_emitters; e++) {
        const float want = emitter_power(emitters[e]) / total_power;
        if (std::memcmp(&want, &pick[e].prob, sizeof(float)) != 0)
            return query_fail(TRT_ERR_INVALID_ARG, "pick: prob must be power / total_power of the table (trt_emitter_pick_build with weights == NULL)");
    }
    return TRT_OK;
}

}  // namespace trt
