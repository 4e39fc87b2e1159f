// scene_common.h — the scene compiler's scalar rules, shared by the host compiler (scene_host.cpp, plain C++) and the device
// compiler (scene_build.hip): sort keys, surface areas, f16 rounding of the compact nodes and their eps rule.  One definition
// each, so that the two compilers cannot drift apart.  Compiles with plain g++ (no HIP headers): TRT_SHARED is plain inline there.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define TRT_SHARED __host__ __device__ inline
#else
#define TRT_SHARED inline
#endif

namespace trt {

TRT_SHARED float bits_to_f32(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
TRT_SHARED uint32_t f32_to_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// f32::total_cmp as an integer key (aabb.rs:80-82)
TRT_SHARED int32_t total_order_key(float f) {
    int32_t bits;
    memcpy(&bits, &f, 4);
    return bits ^ (int32_t)((uint32_t)(bits >> 31) >> 1);
}
// the same order as an unsigned key (what the reference tree's sort compares)
TRT_SHARED uint32_t total_order_key_u32(float f) { return (uint32_t)total_order_key(f) ^ 0x80000000u; }

// AABB::longest_axis (aabb.rs:63-78) of the box lo..hi: ties go to the later axis.
TRT_SHARED int box_longest_axis6(const float lo[3], const float hi[3]) {
    float sx = hi[0] - lo[0], sy = hi[1] - lo[1], sz = hi[2] - lo[2];
    if (sx > sy) return sx > sz ? 0 : 2;
    return sy > sz ? 1 : 2;
}

// surface area in double (the culling tree's SAH); an empty or NaN extent counts as 0
TRT_SHARED double surface_area6(const float lo[3], const float hi[3]) {
    double dx = (double)hi[0] - lo[0], dy = (double)hi[1] - lo[1], dz = (double)hi[2] - lo[2];
    if (!(dx > 0)) dx = 0;
    if (!(dy > 0)) dy = 0;
    if (!(dz > 0)) dz = 0;
    return 2.0 * (dx * dy + dy * dz + dz * dx);
}

TRT_SHARED bool tame(float v) { return fabsf(v) < 1e30f; }

// f32 -> f16 bits rounded toward -inf (up = false) or +inf (up = true): the nearest-even conversion, stepped by one
// f16 if it landed on the wrong side.  |x| beyond the f16 range becomes +-inf or +-65504, whichever is conservative.
TRT_SHARED float f16_bits_to_f32(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 0x1Fu, m = h & 0x3FFu;
    uint32_t out;
    if (e == 0u) {
        if (m == 0u) out = sign;
        else {                                              // subnormal: m * 2^-24
            float v = (float)m * 5.9604644775390625e-08f;
            uint32_t b; memcpy(&b, &v, 4); out = b | sign;
        }
    } else if (e == 31u) out = sign | 0x7F800000u | (m << 13);
    else out = sign | ((e + 112u) << 23) | (m << 13);
    float f; memcpy(&f, &out, 4); return f;
}
TRT_SHARED uint16_t f32_to_f16_nearest(float x) {
    uint32_t b; memcpy(&b, &x, 4);
    const uint32_t sign = (b >> 16) & 0x8000u;
    const uint32_t a = b & 0x7FFFFFFFu;
    if (a >= 0x7F800000u) return (uint16_t)(sign | 0x7C00u | (a > 0x7F800000u ? 0x200u : 0u));
    if (a >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);            // >= 65520 rounds to inf
    if (a < 0x33000001u) return (uint16_t)sign;                           // <= 2^-25 rounds to zero
    int32_t e = (int32_t)(a >> 23) - 127;
    uint32_t m = (a & 0x7FFFFFu) | 0x800000u;
    uint32_t shift = e < -14 ? (uint32_t)(13 + (-14 - e)) : 13u;          // subnormal results lose more bits
    uint32_t half = m >> shift, rem = m & ((1u << shift) - 1u), mid = 1u << (shift - 1u);
    if (rem > mid || (rem == mid && (half & 1u))) half++;
    uint32_t he = e < -14 ? 0u : (uint32_t)(e + 15);
    uint32_t out = e < -14 ? half : ((he << 10) + (half - 0x400u));       // a mantissa carry rolls into the exponent
    return (uint16_t)(sign | out);
}
TRT_SHARED uint16_t f32_to_f16_dir(float x, bool up) {
    if (x != x) return up ? 0x7C00u : 0xFC00u;                            // NaN: the conservative infinity
    uint16_t h = f32_to_f16_nearest(x);
    const float back = f16_bits_to_f32(h);
    if (up ? back >= x : back <= x) return h;
    // step one f16 toward the wanted side
    if (up) {
        if (h & 0x8000u) return (h & 0x7FFFu) == 0u ? (uint16_t)0x0001u : (uint16_t)(h - 1u);   // negative: smaller magnitude
        return (uint16_t)(h + 1u);                                                           // positive: larger magnitude (0x7BFF -> inf)
    }
    if (h & 0x8000u) return (uint16_t)(h + 1u);
    return (h & 0x7FFFu) == 0u ? (uint16_t)0x8001u : (uint16_t)(h - 1u);
}

// The compact nodes' growth eps per axis and the ray-origin limit up to which the fused slab arithmetic is conservative, from
// the culling root's box (scene_host.cpp explains the 2^-19 B rule).  limit is all zero unless every axis has a positive one.
TRT_SHARED void compact_eps_rule(const float root_lo[3], const float root_hi[3], bool all_finite, float eps[3], float limit[3]) {
    const float b3[3] = {fmaxf(fabsf(root_lo[0]), fabsf(root_hi[0])), fmaxf(fabsf(root_lo[1]), fabsf(root_hi[1])),
                         fmaxf(fabsf(root_lo[2]), fabsf(root_hi[2]))};
    for (int a = 0; a < 3; a++) {
        const bool ok = all_finite && b3[a] <= 1.0e12f;                           // (products with 1/d <= 2^60 and 4 B stay far from overflow)
        eps[a] = ok ? b3[a] * 1.9073486328125e-06f : 0.0f;                       // 2^-19 B
        limit[a] = ok ? 4.0f * b3[a] : 0.0f;
    }
    if (!(limit[0] > 0.0f && limit[1] > 0.0f && limit[2] > 0.0f)) limit[0] = limit[1] = limit[2] = 0.0f;
}

// One compact node (16 bytes): f16 box grown by eps and rounded outward, then the link word.
TRT_SHARED void compact_node_words(const float lo[3], const float hi[3], const float eps[3], uint32_t link, uint32_t out[4]) {
    const uint32_t lx = f32_to_f16_dir(lo[0] - eps[0], false), ly = f32_to_f16_dir(lo[1] - eps[1], false), lz = f32_to_f16_dir(lo[2] - eps[2], false);
    const uint32_t hx = f32_to_f16_dir(hi[0] + eps[0], true), hy = f32_to_f16_dir(hi[1] + eps[1], true), hz = f32_to_f16_dir(hi[2] + eps[2], true);
    out[0] = lx | ly << 16;
    out[1] = lz | hx << 16;
    out[2] = hy | hz << 16;
    out[3] = link;
}

}  // namespace trt
