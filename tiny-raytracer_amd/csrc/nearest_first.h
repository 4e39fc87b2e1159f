// nearest_first.h — the leaf phase of the lock-step walk tests the NEAREST pending leaf first and skips the rest without a test (rt_path.h
// leaf_phase_nearest), on scenes whose primitives are all axis-exact quads (axis_quads.h).  The rule, its margin and the scene-level switch.
//
// A leaf phase starts from (T0, P0) - t_best and prim_best on entry - with pending slots k = 0..m-1 in walk order, each (leaf_k, start_k).
// Every slot passed its box with T0, so far_k > start_k and T0 > start_k hold for the whole phase (rt_path.h walk_fast).
//   REFERENCE PHASE (leaf_phase): for k in order, if t_best > start_k, run the quad test on [t_min, t_best).
//   NEAREST-FIRST PHASE:
//     1. scan: s = the slot with the smallest start (the lowest k on equal start), start2 = the second smallest start;
//     2. test slot s on [t_min, t_best);
//     3. a lane needs more iff it has a second slot and start2 - E <= t_best; if no lane of the wave does, the phase is over;
//     4. residual, needing lanes only: the other slots in walk order; slot k is skipped iff start_k - E > t_best (strictly), otherwise
//        tested and accepted iff t_k < t_best, or t_k == t_best and k precedes the current winner's slot (a winner carried in from an
//        earlier phase, P0, precedes every slot: t_k == T0 never replaces it - it is outside [t_min, T0) anyway);
//     5. safety: if the phase produced a winner m and start_m > t_m, (T0, P0) are restored and the lane runs the reference phase.
// On Cornell the wave used to run 3.4 trips of the quad test per phase, all but the first for a handful of lanes whose hit was then
// superseded (walk order is unrelated to distance); now it runs one, and a second one where some lane needs the residual loop (0.97 % of
// Cornell's rays, mostly those that reach the light, whose leaf ties with the coplanar ceiling's: about every other wave round).
//
// WHY IT IS EXACT.  Let t_k be slot k's own hit distance on [t_min, T0) (none if it misses).  Step 4 skips only leaves with
// t_k >= start_k - E > t_best >= the final t_best (THE MARGIN, below), so after step 4 the winner m is the arg-min of t over ALL pending
// hits in [t_min, T0), ties going to walk order.  That is the premise of the ordered-traversal theorem (checked on millions
// of rays by tests/native/ordered_theorem_check.c): if start_m <= t_m the reference accepts m at its turn - any h accepted before it has
// t_h > t_m >= start_m (t_h == t_m with h earlier would have made h the winner), so t_best > start_m when m's turn comes - and nothing
// displaces it afterwards (a later k needs t_k < t_m).  Otherwise step 5 runs the reference itself.  If no pending leaf is hit, neither
// phase changes (T0, P0).  The only floating-point statement is therefore the margin.
//
// THE MARGIN: t_k >= start_k - E for every axis-exact quad hit the test accepts, with
//     E = 2^-19 max over the axes of fl(fl(P_axis + |o_axis|) |inv_axis|),     P_axis >= |every leaf-box plane on that axis|, P_axis >= 2^-32.
// u = 2^-24; rays in the DOMAIN 2^-60 <= |inv_axis| <= 2^60 on every axis with a finite origin (closest_hit sends the others through the
// reference walk), so d = the ray's direction component is finite, non-zero, and inv = (1/d)(1 + e), |e| <= u, is normal.  start_k is
// max(t_min, the three near slab distances) and an accepted t is >= t_min, so it suffices to bound near_axis - t per axis.  Each near slab
// distance is min over the box's two planes p of fl(fl(p - o) inv) = (p - o)/d (1 + e)^3: within 3 u (P + |o|) |1/d| of the real entry
// distance of the slab [lo, hi] (plus 2^-150 where a product is subnormal).  What the HOST has checked in double precision for every leaf
// before it sets the switch (nearest_first_flag: stored box against the stored constants the test uses, each to 4 u P):
//   * normal axis a: the plane Q' = D/N (record elements n_a = N, d = D) lies in [lo_a - 4uP, hi_a + 4uP] and 2^-32 <= |N| <= 2^32.
//     t = fl(fl(D - fl(o_a N)) / fl(d_a N)) (the other two products of each dot product are +-0: axis_quads.h) = (Q' - o_a(1 + e1)) (1 + e2)
//     (1 + e3) / (d_a (1 + e4)): within 4 u (P + |o|) |1/d_a| of (Q' - o_a)/d_a, which is at least the slab's real entry distance minus
//     4 u P |1/d_a|.  |d_a N| >= 2^-93 and |N| >= 2^-32 keep the quotient's relative bound; a subnormal D or o_a N adds 2^-117 |1/d_a|.
//     Normal axis: near_a - t <= 11 u (P + |o|) |1/d_a|.
//   * in-plane axis b: the accepted inside test says 0 <= fl(w_a fl(p_b A_b)) < 1, i.e. p_b / e_b in [0, 1 + 2u) with the edge
//     e_b = 1/(w_a A_b), and the host has checked [c_b, c_b + e_b] inside [lo_b - 4uP, hi_b + 4uP] (|e_b| <= 2P + 8uP).  p_b =
//     fl(fl(o_b + fl(t d_b)) - c_b) is within u (|t d_b| + |o_b + t d_b| + |p_b|) <= 4 u (P + |o|) of x_b - c_b, x_b = o_b + t d_b in REAL
//     arithmetic at the COMPUTED t (so no further error of t enters).  Hence x_b lies within (4 + 4 + 4) u (P + |o|) of the slab, the real
//     entry distance is at most t + 12 u (P + |o|) |1/d_b|, and near_b - t <= 15 u (P + |o|) |1/d_b|.  An underflow in t d_b, p_b A_b or
//     the product with w_a (|A_b| >= 2^-64, |w_a| >= 2^-32) moves p_b by less than 2^-86: the floor P >= 2^-32 makes 1 u P = 2^-56.
//   * E and the comparison: |inv| <= |1/d| (1 + u); fl(fl(P + |o|) |inv|) loses 2 u of E; fl(start - E) is within u |start| <= 1.0001 u
//     (P + |o|) |inv| of start - E.  In all start_k - t_k <= 17.1 u max((P + |o|) |inv|) against E >= 31.9 u of it: (start - t)/E <= 0.54.
// A margin that is too large costs only time (more residual tests); +inf (overflow of P + |o| times |inv|) disables skipping.  Where the
// scene does not have the switch the kernel runs leaf_phase as before.  Plain C++: the scene layer, the kernels and the host tests
// (tests/test_nearest_first.py, tests/native/nearest_first_check.c: 2 M rays per scene against the reference phase) include it.
#pragma once

#include <stdint.h>
#include <string.h>

#include "axis_quads.h"

#if defined(__HIPCC__)
#define TRT_NF_FN __host__ __device__ inline
#else
#define TRT_NF_FN inline
#endif

namespace trt {

constexpr float kNfInvLo = 8.67361737988403547e-19f, kNfInvHi = 1152921504606846976.0f;      // 2^-60, 2^60: the ray domain of the margin
constexpr float kNfPlaneFloor = 2.3283064365386963e-10f, kNfPlaneMax = 1048576.0f;           // 2^-32 <= P_axis <= 2^20
constexpr float kNfScale = 1.9073486328125e-06f;                                             // 2^-19 = 32 u

// E for one walk (P_axis: nearest_first_flag).  Unfused, in this order.
TRT_NF_FN float nf_margin(float px, float py, float pz, float ox, float oy, float oz, float ix, float iy, float iz) {
    const float ax = (px + __builtin_fabsf(ox)) * __builtin_fabsf(ix);
    const float ay = (py + __builtin_fabsf(oy)) * __builtin_fabsf(iy);
    const float az = (pz + __builtin_fabsf(oz)) * __builtin_fabsf(iz);
    return kNfScale * __builtin_fmaxf(__builtin_fmaxf(ax, ay), az);
}
TRT_NF_FN bool nf_in_domain(float ix, float iy, float iz) {
    const float hi = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(ix), __builtin_fabsf(iy)), __builtin_fabsf(iz));
    const float lo = __builtin_fminf(__builtin_fminf(__builtin_fabsf(ix), __builtin_fabsf(iy)), __builtin_fabsf(iz));
    return (hi <= kNfInvHi) & (lo >= kNfInvLo);
}

// Step 1, one slot: branch-free.  `leaf` ends as the leaf of the slot with the smallest start, the first of equal ones.
struct NfScan {
    float smallest, start2;
    uint32_t leaf;
};
TRT_NF_FN NfScan nf_scan_begin() { return NfScan{__builtin_inff(), __builtin_inff(), 0xFFFFFFFFu}; }
// (start2 = min(start2, max(smallest, start)) before smallest = min(smallest, start), written as comparisons and selects: a start is
// never NaN, and fminf / fmaxf on a value read from memory cost a canonicalising instruction each on the device.)
TRT_NF_FN void nf_scan_step(NfScan& s, uint32_t leaf, float start) {
    const bool nearer = start < s.smallest;
    const float other = nearer ? s.smallest : start;
    s.start2 = other < s.start2 ? other : s.start2;
    s.leaf = nearer ? leaf : s.leaf;
    s.smallest = nearer ? start : s.smallest;
}
// Step 3 (a real start is finite: its box passed, far > start; +inf = the lane has no second slot).
TRT_NF_FN bool nf_needs_more(float start2, float E, float t_best) { return (start2 - E <= t_best) & (start2 < __builtin_inff()); }
// Step 4: the skip and the acceptance (`before_winner`: this slot precedes the current winner's slot, and that winner is of this phase).
TRT_NF_FN bool nf_skip(float start, float E, float t_best) { return start - E > t_best; }
TRT_NF_FN bool nf_accept(float t, float t_best, bool before_winner) { return (t < t_best) | (before_winner & (t == t_best)); }
// Step 5.
TRT_NF_FN bool nf_unsafe(uint32_t prim_best, uint32_t p0, float win_start, float t_best) { return (prim_best != p0) & (win_start > t_best); }

// Steps 4 and 5 for one lane (cold code behind the wave's ballot).  slot(k, leaf, start) reads slot k; test(leaf, t) is the
// quad's own hit on [t_min, +inf): whether it is hit, and t.  `leaf_s`, `win_start`: the slot step 2 tested and the start of the current
// winner's slot (step 2's if it hit).  `residual`: the lane needs step 4 (nf_needs_more).  Returns 1 if the reference phase was run.
template <typename Slot, typename Test>
TRT_NF_FN uint32_t nf_cold_phase(uint32_t m, Slot&& slot, Test&& test, bool residual, uint32_t leaf_s, float E, float t0, uint32_t p0,
                                 float win_start, float& t_best, uint32_t& prim_best) {
    if (residual) {
        bool before_s = true;                                        // slots walked so far precede s
        for (uint32_t k = 0; k < m; k++) {
            uint32_t leaf; float start, t;
            slot(k, leaf, start);
            if (leaf == leaf_s) { before_s = false; continue; }
            if (nf_skip(start, E, t_best)) continue;
            if (test(leaf, t) && nf_accept(t, t_best, before_s & (prim_best == leaf_s))) { t_best = t; prim_best = leaf; win_start = start; }
        }
    }
    if (!nf_unsafe(prim_best, p0, win_start, t_best)) return 0u;
    t_best = t0; prim_best = p0;                                     // the reference phase itself
    for (uint32_t k = 0; k < m; k++) {
        uint32_t leaf; float start, t;
        slot(k, leaf, start);
        if (t_best > start && test(leaf, t) && t < t_best) { t_best = t; prim_best = leaf; }
    }
    return 1u;
}

// The whole phase for one lane, steps 1 to 5 (the kernel runs the same pieces with a ballot between steps 3 and 4).  Returns bit 0: the
// lane took step 4, bit 1: it ran the reference phase.
template <typename Slot, typename Test>
TRT_NF_FN uint32_t nearest_first_phase(uint32_t m, Slot&& slot, Test&& test, float E, float& t_best, uint32_t& prim_best) {
    if (m == 0u) return 0u;
    const float t0 = t_best;
    const uint32_t p0 = prim_best;
    NfScan sc = nf_scan_begin();
    for (uint32_t k = 0; k < m; k++) {
        uint32_t leaf; float start;
        slot(k, leaf, start);
        nf_scan_step(sc, leaf, start);
    }
    float t;
    if (test(sc.leaf, t) && nf_accept(t, t_best, false)) { t_best = t; prim_best = sc.leaf; }
    const bool residual = nf_needs_more(sc.start2, E, t_best);
    const uint32_t rerun = nf_cold_phase(m, slot, test, residual, sc.leaf, E, t0, p0, sc.smallest, t_best, prim_best);
    return (residual ? 1u : 0u) | (rerun << 1);
}

// The scene-level switch and P_axis (out[0..2], each >= 2^-32), from the packed leaf list (n_leaves leaves of 32 bytes in walk order:
// (lo.x lo.y lo.z hi.x) (hi.y hi.z skip link), scene.h off_leaf_list) and the packed quad records (80 bytes each, axis_quads.h).
// 1 iff `enabled` (TRT_NEAREST_FIRST), the axis-exact-quads switch is on (`axis_quads`: every quad axis-exact, lock-step walk on an LDS
// copy), the scene has no sphere, every leaf is a quad whose box holds what THE MARGIN needs of it (header comment), and every P_axis is
// finite and at most 2^20.  P is written whatever the flag.
inline uint32_t nearest_first_flag(const void* leaf_list, uint32_t n_leaves, const void* quads, uint32_t n_quads, uint32_t n_spheres,
                                   uint32_t axis_quads, bool enabled, float out[3]) {
    out[0] = out[1] = out[2] = kNfPlaneFloor;
    if (leaf_list == nullptr || n_leaves == 0u || n_leaves > 32u) return 0u;
    const unsigned char* lp = static_cast<const unsigned char*>(leaf_list);
    bool ok = enabled && axis_quads != 0u && n_spheres == 0u && quads != nullptr && n_quads > 0u;
    for (uint32_t i = 0; i < n_leaves; i++) {
        float box[6];
        memcpy(box, lp + 32u * (size_t)i, sizeof box);
        for (int k = 0; k < 6; k++) {
            const float a = __builtin_fabsf(box[k]);
            if (!(a <= kNfPlaneMax)) ok = false;                     // NaN, inf or beyond 2^20
            if (a > out[k % 3]) out[k % 3] = a;
        }
    }
    if (!ok) return 0u;
    const double u4 = 4.0 / 16777216.0;
    for (uint32_t i = 0; i < n_leaves; i++) {
        float box[6], rec[20], c[8];
        uint32_t link;
        memcpy(box, lp + 32u * (size_t)i, sizeof box);
        memcpy(&link, lp + 32u * (size_t)i + 28u, sizeof link);
        if ((link & 0x40000000u) == 0u || (link & 0x3FFFFFFFu) >= n_quads) return 0u;               // PRIM_QUAD_BIT, PRIM_INDEX_MASK (scene.h)
        memcpy(rec, static_cast<const unsigned char*>(quads) + 80u * (size_t)(link & 0x3FFFFFFFu), sizeof rec);
        if (!axis_quad_constants(rec, c)) return 0u;
        const int a = rec[0] != 0.0f ? 0 : rec[1] != 0.0f ? 1 : 2;
        const double N = rec[a], D = rec[3], wa = c[3];
        if (!(__builtin_fabs(N) >= 2.3283064365386963e-10 && __builtin_fabs(N) <= 4294967296.0)) return 0u;
        for (int k = 0; k < 3; k++) {
            const double tol = u4 * out[k], lo = (double)box[k] - tol, hi = (double)box[3 + k] + tol, corner = rec[4 + k];
            double x0, x1;
            if (k == a) {
                x0 = D / N; x1 = corner;                             // the plane the test uses, and the corner p is taken from
            } else {
                const double g = (double)c[k] != 0.0 ? (double)c[k] : (double)c[4 + k];            // A_k or B_k: one of them is the edge's
                x0 = corner; x1 = corner + 1.0 / (wa * g);
            }
            if (!(x0 >= lo && x0 <= hi && x1 >= lo && x1 <= hi)) return 0u;
        }
    }
    return 1u;
}

}  // namespace trt
