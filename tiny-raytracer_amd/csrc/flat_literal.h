// flat_literal.h - the box phase of the lock-step leaf walk written out for ONE scene: the text of the asm block that stands in for
// rt_path.h box_loop_flat in a kernel compiled at run time for that scene (streamed.hip, stream_pool.h).  Host code only, plain C++.
//
// box_loop_flat takes every leaf plane from an SGPR, and a vector instruction with an SGPR operand issues in 4.2-4.5 cycles where the
// same instruction on VGPR, literal or inline-constant operands takes 2.4-2.6 (profiles/r03_valu_forms_microbenchmark.txt).  A scene's
// planes do not change between renders, so here they are 32-bit literals in the instruction stream: no register, no LDS, no scalar load.
//
// The block is box_loop_flat unrolled over the leaf list, operation for operation (TRT_FLAT_BOX): per computed axis
//   v_sub t0, <lo bits>, o   v_sub t1, <hi bits>, o   v_mul t0, inv, t0   v_mul t1, inv, t1   and x: two v_med3 with t_min / t_best,
//   y / z: v_min, v_max;   then v_max3, v_min3, v_cmp_nle and the push of (link, start) under s_and_saveexec with the link a literal.
// Planes and links are written as eight hex digits, never as decimal text: -0, +0, inf and NaN planes keep their bits.
//
// WHAT IS DECIDED HERE INSTEAD OF AT RUN TIME
//   * interval reuse: an axis whose bit is set in the masks of flat_reuse.h emits nothing - the interval of the previous leaf is still in
//     its registers (the three s_bitcmp1 + s_cbranch per box are gone);
//   * the pair loop: straight-line code, the stack-full ballot after every second leaf as before, `i` written only where the block ends;
//   * the leaf planes' scalar load and its wait.
//
// ENTRIES.  The block is left with i < n only behind the second leaf of a pair (some lane's stack cannot hold another pair), so it is
// entered at EVEN i only, and the first box of every entry computes all three axes whatever its bits say (no interval outlives the t_best
// it was folded with: box_loop_flat's rule).  Form chosen: one straight main stream that reuses, plus, out of line, a FRESH copy of every
// even leaf that reuses something; an entry at i > 0 goes through a scalar jump table (s_getpc, add 2 i, s_setpc into a row of s_branch)
// to the fresh copy, which falls back into the main stream at leaf i + 1.  An even leaf that reuses nothing is its own fresh copy: the
// table points into the main stream.  Odd leaves need no entry - no exit leaves i odd except i == n - and get none: dead code would only
// cost instruction cache.  i == 0, the entry of every new ray, skips the table (one s_cmp + one s_cbranch not taken).
// Against two whole copies of every pair this duplicates one box per pair at most, and nothing where nothing is reused.
//
// Operands of the block (names as in box_loop_flat): [i] "+s", [top] "+v", [m] "=&s" (64 bit), [t0] [t1] [xe] [xx] [ye] [yx] [ze] [zx] [st]
// [lk] "=&v", [lim] [ox] [oy] [oz] [ix] [iy] [iz] [tb] "v", [tmin] "s"; clobbers vcc, scc, memory, s36, s37, s38 (the jump).
// Local labels: 200 + k main-stream leaf k, 100 + k fresh copy of leaf k, 400 + k the exit with i = k, 900 the table, 990 the end.
#pragma once

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>

#include "flat_reuse.h"

namespace trt {

constexpr uint32_t kFlatLiteralMaxLeaves = 32u;

namespace flat_literal_detail {

inline void hex(std::string& s, uint32_t bits) {
    char b[16];
    snprintf(b, sizeof b, "0x%08x", bits);
    s += b;
}

// One leaf box: the axes of `axes` (bit 0 x, 1 y, 2 z) computed, then the combination and the push.  w: the leaf's eight words.
inline void box(std::string& s, const uint32_t w[8], uint32_t axes) {
    static const char* const o[3] = {"%[ox]", "%[oy]", "%[oz]"};
    static const char* const inv[3] = {"%[ix]", "%[iy]", "%[iz]"};
    static const char* const lo_out[3] = {"%[xe]", "%[ye]", "%[ze]"};
    static const char* const hi_out[3] = {"%[xx]", "%[yx]", "%[zx]"};
    for (int k = 0; k < 3; k++) {
        if (!(axes & (1u << k))) continue;
        s += "v_sub_f32_e32 %[t0], "; hex(s, w[k]); s += ", "; s += o[k]; s += "\n";
        s += "v_sub_f32_e32 %[t1], "; hex(s, w[3 + k]); s += ", "; s += o[k]; s += "\n";
        s += "v_mul_f32_e32 %[t0], "; s += inv[k]; s += ", %[t0]\n";
        s += "v_mul_f32_e32 %[t1], "; s += inv[k]; s += ", %[t1]\n";
        if (k == 0) {
            s += "v_med3_f32 %[xe], %[t0], %[t1], %[tmin]\n";
            s += "v_med3_f32 %[xx], %[t0], %[t1], %[tb]\n";
        } else {
            s += "v_min_f32_e32 "; s += lo_out[k]; s += ", %[t0], %[t1]\n";
            s += "v_max_f32_e32 "; s += hi_out[k]; s += ", %[t0], %[t1]\n";
        }
    }
    s += "v_max3_f32 %[st], %[xe], %[ye], %[ze]\n";
    s += "v_min3_f32 %[t0], %[xx], %[yx], %[zx]\n";
    s += "v_cmp_nle_f32_e32 vcc, %[t0], %[st]\n";
    s += "s_and_saveexec_b64 %[m], vcc\n";
    s += "v_mov_b32_e32 %[lk], "; hex(s, w[7]); s += "\n";
    s += "ds_write2_b32 %[top], %[lk], %[st] offset1:1\n";
    s += "v_add_u32_e32 %[top], 0x200, %[top]\n";
    s += "s_mov_b64 exec, %[m]\n";
}

inline void label(std::string& s, uint32_t base, uint32_t k) { s += std::to_string(base + k); s += ":\n"; }
inline void ref(std::string& s, uint32_t base, uint32_t k, char dir) { s += std::to_string(base + k); s += dir; }

}  // namespace flat_literal_detail

// The asm text for this leaf list (n_leaves leaves of 32 bytes in walk order: flat_reuse.h) with the reuse schedule `masks` (what
// flat_reuse_masks gives for the list, or zeros: every box in full).  False - nothing written - for an empty list, a list of more than
// kFlatLiteralMaxLeaves leaves, or a null pointer.  Deterministic: the text is a function of the bytes and the masks alone.
inline bool flat_literal_asm(const void* leaf_list, uint32_t n_leaves, const uint32_t masks[3], std::string& out) {
    using namespace flat_literal_detail;
    if (leaf_list == nullptr || n_leaves == 0u || n_leaves > kFlatLiteralMaxLeaves) return false;
    const unsigned char* p = static_cast<const unsigned char*>(leaf_list);
    const uint32_t n = n_leaves;
    auto leaf = [&](uint32_t k, uint32_t w[8]) { memcpy(w, p + 32u * (size_t)k, 32u); };
    // axes leaf k computes in the main stream; leaf 0 computes all
    auto axes_of = [&](uint32_t k) {
        const uint32_t b = 1u << k;
        return k == 0u ? 7u : (((masks[0] & b) ? 0u : 1u) | ((masks[1] & b) ? 0u : 2u) | ((masks[2] & b) ? 0u : 4u));
    };
    std::string s;
    uint32_t w[8];
    s += "s_cmp_lg_u32 %[i], 0\n";
    s += "s_cbranch_scc1 900f\n";
    // ---- main stream ----
    for (uint32_t k = 0; k < n; k++) {
        label(s, 200u, k);
        leaf(k, w);
        box(s, w, axes_of(k));
        if ((k & 1u) && k + 1u < n) {                          // behind a pair that is not the last: can every lane hold another pair?
            s += "v_cmp_gt_u32_e32 vcc, %[top], %[lim]\n";
            s += "s_cbranch_vccnz "; ref(s, 400u, k + 1u, 'f'); s += "\n";
        }
    }
    s += "s_mov_b32 %[i], "; hex(s, n); s += "\n";
    s += "s_branch 990f\n";
    // ---- exits with i < n ----
    for (uint32_t k = 2; k < n; k += 2u) {
        label(s, 400u, k);
        s += "s_mov_b32 %[i], "; hex(s, k); s += "\n";
        s += "s_branch 990f\n";
    }
    // ---- fresh copies of the even leaves that reuse something ----
    for (uint32_t k = 2; k < n; k += 2u) {
        if (axes_of(k) == 7u) continue;
        label(s, 100u, k);
        leaf(k, w);
        box(s, w, 7u);
        if (k + 1u < n) { s += "s_branch "; ref(s, 200u, k + 1u, 'b'); s += "\n"; }
        else { s += "s_mov_b32 %[i], "; hex(s, n); s += "\n"; s += "s_branch 990f\n"; }
    }
    // ---- entry at even i > 0: row i / 2 of the table (4 bytes a row) ----
    s += "900:\n";
    s += "s_lshl_b32 s38, %[i], 1\n";
    s += "s_add_u32 s38, s38, 12\n";                            // the three instructions between s_getpc's result and the table
    s += "s_getpc_b64 s[36:37]\n";
    s += "s_add_u32 s36, s36, s38\n";
    s += "s_addc_u32 s37, s37, 0\n";
    s += "s_setpc_b64 s[36:37]\n";
    for (uint32_t k = 0; k < n; k += 2u) {
        s += "s_branch "; ref(s, axes_of(k) == 7u ? 200u : 100u, k, 'b'); s += "\n";
    }
    s += "990:\n";
    out.swap(s);
    return true;
}

// ---- the interval cache ----
// flat_literal_asm keeps an interval only from leaf i-1 to leaf i: the rule of the run-time loop, which held three intervals and chose
// per box with scalar branches.  A text written per scene can keep more, because which interval sits in which register is decided while
// the text is written: flat_literal_cached_asm puts a CACHED STREAM in front of flat_literal_asm's text.
//   * It is entered only at i == 0 - where every new ray starts - and runs the leaves in walk order to the end or to a stack-full exit.
//     t_best is constant within one call of the block, so an x interval (folded with t_min / t_best) is as good at leaf 17 as at leaf 1.
//   * `interval_pairs` register pairs hold intervals: (xe xx) (ye yx) (ze zx), then (c0 c1) (c2 c3) ...  Any pair holds any axis' interval;
//     each leaf's v_max3 / v_min3 name the pairs that hold its three.  No moves.
//   * An interval is found again only if both plane words are the earlier ones bit for bit, on the same axis, both finite (flat_reuse.h).
//   * A pair is taken by farthest next use (optimal for a fixed sequence: Belady), ties by the lowest pair, never one the current leaf
//     needs.  An empty pair, and one whose interval no later leaf uses, count as never used again.
//   * `plane_regs` further registers (behind the pairs among c0 ...) hold single plane distances fl(fl(p - o) * inv): a finite plane that
//     a LATER COMPUTED interval of the same axis names again is written there instead of t0 / t1 - the same two instructions on the same
//     operands - and read from there.  Taken by farthest next use as well; a plane whose next use lies farther than every resident's goes
//     through t0 / t1.  The interval's two instructions keep their operand order: the lo plane's distance, then the hi plane's.
//   * The push, the link, the ballot behind every second leaf: as in flat_literal_asm, and the ballot's exit IS that text's exit (400 + k).
// An entry at i > 0 (after a stack-full exit) goes to flat_literal_asm's text, which follows whole and unchanged behind label 1000: its
// table, its fresh copies, its stream that reuses from leaf i-1 only.  Local labels of the new part: 1000, and 1200 + k for cached leaf k.
// Operands beyond flat_literal_asm's: [c0] ... "=&v", FlatCacheStats::extra_operands of them.
struct FlatCacheStats {
    uint32_t intervals = 0;             // intervals the stream entered at i == 0 computes
    uint32_t plane_distances = 0;       // plane distances it computes (two instructions each)
    uint32_t evictions = 0;             // intervals dropped from a pair although a later leaf names them again
    uint32_t far_reuses = 0;            // intervals read from a pair that leaf i-1 did not use on that axis (what flat_literal_asm cannot do)
    uint32_t extra_operands = 0;        // [c0] ... the text names; 0: the text is flat_literal_asm's
    bool cached = false;                // a cached stream was written
};
constexpr uint32_t kFlatCacheMinPairs = 3u, kFlatCacheMaxPairs = 8u, kFlatCacheMaxPlanes = 8u;
constexpr uint32_t kFlatCacheMaxExtra = 2u * (kFlatCacheMaxPairs - 3u) + kFlatCacheMaxPlanes;

// False - nothing written - where flat_literal_asm refuses, or for interval_pairs outside 3 ... 8 or plane_regs beyond 8.  The text is
// flat_literal_asm's own, byte for byte, for (3, 0) and for a list on which the cached stream would compute no fewer intervals and no fewer
// plane distances than the masks' schedule (then stats.cached is false and the counts are that schedule's).
inline bool flat_literal_cached_asm(const void* leaf_list, uint32_t n_leaves, const uint32_t masks[3], uint32_t interval_pairs, uint32_t plane_regs,
                                    std::string& out, FlatCacheStats& stats) {
    using namespace flat_literal_detail;
    if (interval_pairs < kFlatCacheMinPairs || interval_pairs > kFlatCacheMaxPairs || plane_regs > kFlatCacheMaxPlanes) return false;
    std::string plain;
    if (!flat_literal_asm(leaf_list, n_leaves, masks, plain)) return false;
    const unsigned char* p = static_cast<const unsigned char*>(leaf_list);
    const uint32_t n = n_leaves, kNever = 0xffffffffu;
    uint32_t w[kFlatLiteralMaxLeaves][8];
    for (uint32_t k = 0; k < n; k++) memcpy(w[k], p + 32u * (size_t)k, 32u);
    auto finite = [](uint32_t b) { return (b & 0x7f800000u) != 0x7f800000u; };
    auto shareable = [&](uint32_t k, int a) { return finite(w[k][a]) && finite(w[k][3 + a]); };
    auto same = [&](uint32_t k, uint32_t j, int a) { return w[k][a] == w[j][a] && w[k][3 + a] == w[j][3 + a]; };
    FlatCacheStats st;
    // the masks' schedule, for the comparison and for the plain case
    uint32_t plain_intervals = 0;
    for (uint32_t k = 0; k < n; k++)
        for (int a = 0; a < 3; a++) plain_intervals += (k == 0u || !(masks[a] & (1u << k))) ? 1u : 0u;
    // ---- pass 1: which pair holds each leaf's three intervals, and which of them are computed there ----
    struct Pair { bool used = false; int axis = 0; uint32_t leaf = 0; bool share = false; };       // the interval of `leaf` on `axis`
    Pair pairs[kFlatCacheMaxPairs];
    uint32_t slot_of[kFlatLiteralMaxLeaves][3];
    bool computed[kFlatLiteralMaxLeaves][3];
    // when q's interval is named next behind leaf `after`, in steps of one axis of one leaf (x, y, z of leaf 0, x of leaf 1 ...): no two
    // intervals share a step, so only pairs that are never used again tie
    auto next_use = [&](const Pair& q, uint32_t after) {
        if (!q.used || !q.share) return kNever;
        for (uint32_t j = after + 1u; j < n; j++) if (shareable(j, q.axis) && same(j, q.leaf, q.axis)) return 3u * j + (uint32_t)q.axis;
        return kNever;
    };
    for (uint32_t k = 0; k < n; k++) {
        bool needed[kFlatCacheMaxPairs] = {};
        uint32_t found[3] = {kNever, kNever, kNever};
        for (int a = 0; a < 3; a++) {                                                               // what is there is kept before anything is taken
            if (!shareable(k, a)) continue;
            for (uint32_t s = 0; s < interval_pairs; s++)
                if (pairs[s].used && pairs[s].share && pairs[s].axis == a && same(k, pairs[s].leaf, a)) { found[a] = s; needed[s] = true; break; }
        }
        for (int a = 0; a < 3; a++) {
            if (found[a] != kNever) {
                slot_of[k][a] = found[a]; computed[k][a] = false;
                if (k == 0u || !(masks[a] & (1u << k))) st.far_reuses++;
                continue;
            }
            uint32_t best = kNever, best_use = 0;
            for (uint32_t s = 0; s < interval_pairs; s++) {
                if (needed[s]) continue;
                const uint32_t u = next_use(pairs[s], k);
                if (best == kNever || u > best_use) { best = s; best_use = u; }
            }
            if (best_use != kNever) st.evictions++;
            pairs[best] = Pair{true, a, k, shareable(k, a)};
            needed[best] = true;
            slot_of[k][a] = best; computed[k][a] = true;
            st.intervals++;
        }
    }
    // ---- pass 2: where each plane distance of the computed intervals comes from ----
    struct Use { uint32_t leaf; int axis; int hi; uint32_t bits; bool share; };
    Use uses[6u * kFlatLiteralMaxLeaves];
    uint32_t n_uses = 0;
    for (uint32_t k = 0; k < n; k++)
        for (int a = 0; a < 3; a++)
            if (computed[k][a])
                for (int h = 0; h < 2; h++) { const uint32_t b = w[k][3 * h + a]; uses[n_uses++] = Use{k, a, h, b, finite(b)}; }
    auto plane_next = [&](int axis, uint32_t bits, uint32_t after) {
        for (uint32_t j = after + 1u; j < n_uses; j++) if (uses[j].share && uses[j].axis == axis && uses[j].bits == bits) return j;
        return kNever;
    };
    struct Plane { bool used = false; int axis = 0; uint32_t bits = 0; };
    Plane planes[kFlatCacheMaxPlanes];
    // per use: the register read (0 ... plane_regs - 1, or kNever: t0 / t1) and whether it is written here
    uint32_t reg_of[6u * kFlatLiteralMaxLeaves];
    bool written[6u * kFlatLiteralMaxLeaves];
    for (uint32_t u = 0; u < n_uses; u++) {
        reg_of[u] = kNever; written[u] = true;
        if (!uses[u].share || plane_regs == 0u) { st.plane_distances++; continue; }
        uint32_t hit = kNever;
        for (uint32_t r = 0; r < plane_regs; r++) if (planes[r].used && planes[r].axis == uses[u].axis && planes[r].bits == uses[u].bits) { hit = r; break; }
        if (hit != kNever) { reg_of[u] = hit; written[u] = false; continue; }
        st.plane_distances++;
        const uint32_t mine = plane_next(uses[u].axis, uses[u].bits, u);
        if (mine == kNever) continue;
        const uint32_t partner = uses[u].hi ? reg_of[u - 1u] : kNever;                              // the lo plane of this interval is read with this one
        uint32_t best = kNever, best_use = 0;
        for (uint32_t r = 0; r < plane_regs; r++) {
            if (r == partner) continue;
            const uint32_t v = planes[r].used ? plane_next(planes[r].axis, planes[r].bits, u) : kNever;
            if (best == kNever || v > best_use) { best = r; best_use = v; }
        }
        if (best == kNever || best_use <= mine) continue;                                           // every resident is needed sooner
        planes[best] = Plane{true, uses[u].axis, uses[u].bits};
        reg_of[u] = best;
    }
    const bool gains = st.intervals < plain_intervals || st.plane_distances < 2u * plain_intervals;
    if ((interval_pairs == kFlatCacheMinPairs && plane_regs == 0u) || !gains) {
        stats = FlatCacheStats{};
        stats.intervals = plain_intervals; stats.plane_distances = 2u * plain_intervals;
        out.swap(plain);
        return true;
    }
    // ---- the text ----
    static const char* const o[3] = {"%[ox]", "%[oy]", "%[oz]"};
    static const char* const inv[3] = {"%[ix]", "%[iy]", "%[iz]"};
    static const char* const first_lo[3] = {"%[xe]", "%[ye]", "%[ze]"};
    static const char* const first_hi[3] = {"%[xx]", "%[yx]", "%[zx]"};
    auto c = [](uint32_t j) { return "%[c" + std::to_string(j) + "]"; };
    auto pair_lo = [&](uint32_t s) { return s < 3u ? std::string(first_lo[s]) : c(2u * (s - 3u)); };
    auto pair_hi = [&](uint32_t s) { return s < 3u ? std::string(first_hi[s]) : c(2u * (s - 3u) + 1u); };
    auto plane_reg = [&](uint32_t r) { return c(2u * (interval_pairs - 3u) + r); };
    std::string s;
    s += "s_cmp_lg_u32 %[i], 0\n";
    s += "s_cbranch_scc1 1000f\n";
    uint32_t u = 0;
    for (uint32_t k = 0; k < n; k++) {
        label(s, 1200u, k);
        for (int a = 0; a < 3; a++) {
            if (!computed[k][a]) continue;
            std::string d[2];
            for (int h = 0; h < 2; h++) {
                d[h] = reg_of[u + h] != kNever ? plane_reg(reg_of[u + h]) : (h ? "%[t1]" : "%[t0]");
                if (written[u + h]) { s += "v_sub_f32_e32 " + d[h] + ", "; hex(s, uses[u + h].bits); s += ", "; s += o[a]; s += "\n"; }
            }
            for (int h = 0; h < 2; h++)
                if (written[u + h]) { s += "v_mul_f32_e32 " + d[h] + ", "; s += inv[a]; s += ", " + d[h] + "\n"; }
            const std::string lo = pair_lo(slot_of[k][a]), hi = pair_hi(slot_of[k][a]);
            if (a == 0) {
                s += "v_med3_f32 " + lo + ", " + d[0] + ", " + d[1] + ", %[tmin]\n";
                s += "v_med3_f32 " + hi + ", " + d[0] + ", " + d[1] + ", %[tb]\n";
            } else {
                s += "v_min_f32_e32 " + lo + ", " + d[0] + ", " + d[1] + "\n";
                s += "v_max_f32_e32 " + hi + ", " + d[0] + ", " + d[1] + "\n";
            }
            u += 2u;
        }
        s += "v_max3_f32 %[st], " + pair_lo(slot_of[k][0]) + ", " + pair_lo(slot_of[k][1]) + ", " + pair_lo(slot_of[k][2]) + "\n";
        s += "v_min3_f32 %[t0], " + pair_hi(slot_of[k][0]) + ", " + pair_hi(slot_of[k][1]) + ", " + pair_hi(slot_of[k][2]) + "\n";
        s += "v_cmp_nle_f32_e32 vcc, %[t0], %[st]\n";
        s += "s_and_saveexec_b64 %[m], vcc\n";
        s += "v_mov_b32_e32 %[lk], "; hex(s, w[k][7]); s += "\n";
        s += "ds_write2_b32 %[top], %[lk], %[st] offset1:1\n";
        s += "v_add_u32_e32 %[top], 0x200, %[top]\n";
        s += "s_mov_b64 exec, %[m]\n";
        if ((k & 1u) && k + 1u < n) {
            s += "v_cmp_gt_u32_e32 vcc, %[top], %[lim]\n";
            s += "s_cbranch_vccnz "; ref(s, 400u, k + 1u, 'f'); s += "\n";
        }
    }
    s += "s_mov_b32 %[i], "; hex(s, n); s += "\n";
    s += "s_branch 990f\n";
    s += "1000:\n";
    s += plain;
    st.extra_operands = 2u * (interval_pairs - 3u) + plane_regs;
    st.cached = true;
    stats = st;
    out.swap(s);
    return true;
}

// The same text as a C string literal, one quoted line per instruction, for a `#define NAME \` in the run-time compiled unit.
inline std::string flat_literal_define(const std::string& name, const std::string& asm_text) {
    std::string d = "#define " + name + " \\\n";
    size_t a = 0;
    while (a < asm_text.size()) {
        size_t b = asm_text.find('\n', a);
        if (b == std::string::npos) b = asm_text.size();
        d += "\""; d.append(asm_text, a, b - a); d += "\\n\" \\\n";
        a = b + 1u;
    }
    d += "\"\"\n";
    return d;
}

}  // namespace trt
