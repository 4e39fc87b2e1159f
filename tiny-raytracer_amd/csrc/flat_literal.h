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
