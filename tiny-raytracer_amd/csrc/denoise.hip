// denoise.hip — feature-guided edge-avoiding à-trous wavelet filter for rendered frames (tinyrt.h trt_denoise / trt_denoise_device),
// written for gfx950 (CDNA4) only.  It consumes what trt_render and trt_render_aov leave in HBM: radiance plus albedo, normal, depth.
//
// The filter (tinyrt.h has the definition): pass i = 0 .. iterations-1 has step = 1 << i and folds the 25 taps
// q = p + (dx, dy) * step of a 5 x 5 B3-spline (dy outer, dx inner) with weights that depend on the guides only.  Every f32 operation
// is written once, in the order of the definition, and compiled without contraction, so every output bit is determined; the three forms
// of the pass below share one function (dn_filter) and differ only in where a tap's three records come from.
//
// Data layout of the tuned forms.  A prologue kernel packs the inputs into 16-byte records in the caller's scratch - G0 = normal.xyz |
// depth, G1 = albedo.rgb | 0 - and the colour into a padded 16-byte image; the passes ping-pong between two such images and the last one
// writes the caller's 12-byte pixels.  A tap is then three 16-byte loads instead of ten dword loads.
//   dn_lds_kernel    steps 1, 2 (and 4 on request): a 1024-thread workgroup owns a 32 x 32 tile and stages the tile plus a halo of
//                    2 * step records per image in LDS ((32 + 4 step)^2 x 48 bytes: 62, 77 and 111 KiB of the 160 KiB); a wave is two
//                    rows of 32 pixels, so the 16-lane groups of a ds_read_b128 read 16 consecutive 16-byte slots of one row: all 64
//                    banks once, whatever the pitch.
//   dn_packed_kernel every step: 64 x 4 pixels per 256-thread workgroup, the records straight from global memory (a wave's tap is
//                    1 KiB contiguous), reuse between taps and rows left to L1 / L2.
//   dn_plain_kernel  the plain partner: no packing, no LDS, dword loads from the caller's own buffers, 12-byte ping-pong images.
// One thread per pixel, no atomics, no dependency between workgroups inside a pass; passes are separate launches on the stream.
// Out-of-image taps are read at clamped coordinates (global forms) or from unwritten halo records (LDS form) and discarded by a
// select, as NaN and non-positive weights are: no tap branches, so the compiler hoists the loads of a row of taps together.
//
// The variance-guided colour stop (trt_denoise_ex) is a fourth term (kDnColour): the variance image v_i travels with the
// colour - in the tuned forms in the fourth word of the 16-byte colour records, which the three forms load anyway, in the plain form in two
// 4-byte ping-pong images behind the 12-byte ones - so the scratch is the same.  A prologue kernel (dn_var0_kernel) writes the 3 x 3
// prefiltered v_0; every pass but the last writes v_{i+1} beside its colour.  With the term off nothing of this runs.
//
// Which form runs a pass: dn_choose below.  TRT_DENOISE_VARIANT = plain | packed | lds overrides it (the A/B switch of
// tools/denoise_bench.py and the byte-equality test); it is not part of the ABI.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/tinyrt.h"
#include "host_stage.h"

namespace trt {
namespace {

static_assert(sizeof(trt_denoise_params) == 32, "trt_denoise_params layout (tinyrt.h)");
static_assert(sizeof(trt_denoise_inputs) == 32, "trt_denoise_inputs layout (tinyrt.h)");
static_assert(sizeof(trt_denoise_color) == 32, "trt_denoise_color layout (tinyrt.h)");

constexpr uint32_t kDnNormal = 1u, kDnAlbedo = 2u, kDnDepth = 4u, kDnColour = 8u;      // which terms are on (template parameter F)
constexpr uint32_t kDnMaxSide = 65536u;                                   // width, height: keeps every grid and every int coordinate in range
constexpr int kDnTile = 32;                                               // LDS form: tile side; a wave = two rows of it
constexpr int kDnLdsMaxStep = 4;                                          // (32 + 16)^2 x 48 B = 110 592 B; step 8 would need 196 KiB
constexpr uint32_t kDnLdsPerCu = 160u * 1024u;
constexpr float kDnSigmaColourDefault = 8.0f;                             // trt_denoise_color_default: chosen from the table of DESIGN.md 6.4

struct DnPass {
    int width, height, step;
    uint32_t npow;               // normal_power_log2
    float inv_a;                 // 1 / (sigma_albedo * sigma_albedo), computed once on the host
    float sigma_depth;
    float sigma_c2;              // sigma_color * sigma_color, computed once on the host
};

struct DnTap {
    float4 g0;                   // normal.xyz | depth
    float4 g1;                   // albedo.rgb | -
    float4 c;                    // colour.rgb | variance v_i (colour term on)
};

__device__ __forceinline__ int dn_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// Records from the packed images in global memory.
template <uint32_t F>
struct DnPackedFetch {
    const float4* g0;
    const float4* g1;
    const float4* c;
    int width, height;
    __device__ __forceinline__ size_t at(int x, int y) const { return (size_t)dn_clamp(y, height - 1) * (size_t)width + (size_t)dn_clamp(x, width - 1); }
    __device__ __forceinline__ void guides(int x, int y, DnTap& t) const {
        const size_t i = at(x, y);
        if (F & (kDnNormal | kDnDepth)) t.g0 = g0[i];
        if (F & kDnAlbedo) t.g1 = g1[i];
    }
    __device__ __forceinline__ void colour(int x, int y, DnTap& t) const { t.c = c[at(x, y)]; }
};

// Records from the caller's own buffers, dword by dword (the plain form).
template <uint32_t F>
struct DnPlainFetch {
    const float* normal;
    const float* albedo;
    const float* depth;
    const float* c;              // 3 f32 per pixel
    const float* v;              // 1 f32 per pixel: v_i (colour term on)
    int width, height;
    __device__ __forceinline__ size_t at(int x, int y) const { return (size_t)dn_clamp(y, height - 1) * (size_t)width + (size_t)dn_clamp(x, width - 1); }
    __device__ __forceinline__ void guides(int x, int y, DnTap& t) const {
        const size_t i = at(x, y);
        if (F & kDnNormal) { t.g0.x = normal[3 * i]; t.g0.y = normal[3 * i + 1]; t.g0.z = normal[3 * i + 2]; }
        if (F & kDnDepth) t.g0.w = depth[i];
        if (F & kDnAlbedo) { t.g1.x = albedo[3 * i]; t.g1.y = albedo[3 * i + 1]; t.g1.z = albedo[3 * i + 2]; }
    }
    __device__ __forceinline__ void colour(int x, int y, DnTap& t) const {
        const size_t i = at(x, y);
        t.c.x = c[3 * i]; t.c.y = c[3 * i + 1]; t.c.z = c[3 * i + 2];
        if (F & kDnColour) t.c.w = v[i];
    }
};

// Records from the workgroup's LDS tile: (ox, oy) is the image position of record 0, `pitch` the records per row.  A tap of a pixel of
// the tile lies inside the staged area by construction; a record outside the image was never written and its tap is discarded.
template <uint32_t F>
struct DnLdsFetch {
    const float4* g0;
    const float4* g1;
    const float4* c;
    int ox, oy, pitch;
    __device__ __forceinline__ int at(int x, int y) const { return (y - oy) * pitch + (x - ox); }
    __device__ __forceinline__ void guides(int x, int y, DnTap& t) const {
        const int i = at(x, y);
        if (F & (kDnNormal | kDnDepth)) t.g0 = g0[i];
        if (F & kDnAlbedo) t.g1 = g1[i];
    }
    __device__ __forceinline__ void colour(int x, int y, DnTap& t) const { t.c = c[at(x, y)]; }
};

// One pixel of one pass: the definition, operation by operation.  (x, y) is inside the image.
template <uint32_t F, class Fetch>
__device__ __forceinline__ float4 dn_filter(const Fetch& f, const DnPass& a, int x, int y) {
    const float kH[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    DnTap p;
    p.g0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    p.g1 = p.g0;
    f.guides(x, y, p);
    float inv_z = 0.0f;
    if (F & kDnDepth) {
        const float s = (a.sigma_depth * p.g0.w) * (float)a.step;
        inv_z = 1.0f / (s * s);                                               // one division per pixel and pass
    }
    float inv_c = 0.0f;
    if (F & kDnColour) {
        p.c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        f.colour(x, y, p);
        inv_c = 1.0f / (a.sigma_c2 * p.c.w);                                  // one division per pixel and pass
    }
    float ar = 0.0f, ag = 0.0f, ab = 0.0f, ws = 0.0f, va = 0.0f;
    // The rows of taps are a real loop, the five taps of a row are unrolled: fully unrolled, the scheduler hoists the loads of all 25 taps
    // (75 records, 226 VGPRs, spills under the 128 of a 1024-thread workgroup); a row in flight is 15 records.  What depends on dy comes
    // from selects over constants, so no operation of the definition is computed differently.
#pragma unroll 1
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + dy * a.step;
        const int ady = dy < 0 ? -dy : dy;
        const float hy = ady == 0 ? 0.375f : (ady == 1 ? 0.25f : 0.0625f);
        const bool row_ok = qy >= 0 && qy < a.height;
        DnTap q[5];
        float d[5];
#pragma unroll
        for (int k = 0; k < 5; k++) {
            const int qx = x + (k - 2) * a.step;
            q[k].g0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            q[k].g1 = q[k].g0;
            f.guides(qx, qy, q[k]);
            f.colour(qx, qy, q[k]);
            d[k] = 0.0f;
            if (F & kDnNormal) {
                const float dot = (p.g0.x * q[k].g0.x + p.g0.y * q[k].g0.y) + p.g0.z * q[k].g0.z;
                d[k] = dot > 0.0f ? dot : 0.0f;
            }
        }
        if (F & kDnNormal) {
            // normal_power_log2 squarings, the five taps of the row side by side
            for (uint32_t n = 0; n < a.npow; n++) {
#pragma unroll
                for (int k = 0; k < 5; k++) d[k] = d[k] * d[k];
            }
        }
#pragma unroll
        for (int k = 0; k < 5; k++) {
            const int dx = k - 2;
            const int qx = x + dx * a.step;
            const float w0 = hy * kH[k];
            float w = w0;
            if (F & kDnNormal) w = w * d[k];
            if (F & kDnAlbedo) {
                const float er = p.g1.x - q[k].g1.x, eg = p.g1.y - q[k].g1.y, eb = p.g1.z - q[k].g1.z;
                const float e = (er * er + eg * eg) + eb * eb;
                float m = 1.0f - e * a.inv_a;
                m = m > 0.0f ? m : 0.0f;
                w = w * (m * m);
            }
            if (F & kDnDepth) {
                // 1.0f / float(dx*dx + dy*dy): constants, rounded by the compiler as the division rounds (the centre's slot is not used)
                const float inv_r2 = ady == 0 ? 1.0f / (float)(dx * dx + (dx == 0 ? 1 : 0))
                                              : (ady == 1 ? 1.0f / (float)(dx * dx + 1) : 1.0f / (float)(dx * dx + 4));
                const float dz = p.g0.w - q[k].g0.w;
                float m = 1.0f - ((dz * dz) * inv_z) * inv_r2;
                m = m > 0.0f ? m : 0.0f;
                w = w * (m * m);
            }
            if (F & kDnColour) {
                const float er = p.c.x - q[k].c.x, eg = p.c.y - q[k].c.y, eb = p.c.z - q[k].c.z;
                const float e = (er * er + eg * eg) + eb * eb;
                float m = 1.0f - e * inv_c;
                m = m > 0.0f ? m : 0.0f;
                w = w * (m * m);
            }
            if (dx == 0) w = dy == 0 ? w0 : w;                                // the centre tap keeps h * h whatever its guides hold
            // taken only if inside the image and w > 0: a zero or NaN weight adds nothing, not 0 * c
            const bool take = row_ok && qx >= 0 && qx < a.width && w > 0.0f;
            const float nr = ar + w * q[k].c.x, ng = ag + w * q[k].c.y, nb = ab + w * q[k].c.z, nw = ws + w;
            ar = take ? nr : ar;
            ag = take ? ng : ag;
            ab = take ? nb : ab;
            ws = take ? nw : ws;
            if (F & kDnColour) {
                const float nv = va + (w * w) * q[k].c.w;                      // the variance of the weighted mean, carried to the next pass
                va = take ? nv : va;
            }
        }
    }
    const float r = 1.0f / ws;                                                // the centre tap is always taken: ws > 0
    return make_float4(ar * r, ag * r, ab * r, (F & kDnColour) ? va * (r * r) : 0.0f);
}

// The prologue of the tuned forms: caller's buffers -> 16-byte records.  A guide that is off leaves zeros nobody reads.
__global__ __launch_bounds__(256) void dn_pack_kernel(const float* color, const float* albedo, const float* normal, const float* depth, size_t n,
                                                      float4* c0, float4* g0, float4* g1) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    c0[i] = make_float4(color[3 * i], color[3 * i + 1], color[3 * i + 2], 0.0f);
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
    if (normal) { a.x = normal[3 * i]; a.y = normal[3 * i + 1]; a.z = normal[3 * i + 2]; }
    if (depth) a.w = depth[i];
    if (albedo) { b.x = albedo[3 * i]; b.y = albedo[3 * i + 1]; b.z = albedo[3 * i + 2]; }
    g0[i] = a;
    g1[i] = b;
}

// The prologue of the colour term: v_0 = the 3 x 3 average of the caller's variance, weights {0.25, 0.5, 0.25} per axis, dy outer, dx inner,
// over the taps inside the image, divided by the sum of the weights used through one reciprocal.  out[i * stride]: the fourth word of the
// packed colour records (stride 4) or the plain form's 4-byte image (stride 1).
__global__ __launch_bounds__(256) void dn_var0_kernel(const float* variance, int width, int height, float* out, int stride) {
    const int x = (int)(blockIdx.x * 64u + threadIdx.x), y = (int)(blockIdx.y * 4u + threadIdx.y);
    if (x >= width || y >= height) return;
    const float kB[3] = {0.25f, 0.5f, 0.25f};
    float sv = 0.0f, sw = 0.0f;
    for (int dy = -1; dy <= 1; dy++) {
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx, qy = y + dy;
            if (qx < 0 || qx >= width || qy < 0 || qy >= height) continue;
            const float wt = kB[dy + 1] * kB[dx + 1];
            sv = sv + wt * variance[(size_t)qy * (size_t)width + (size_t)qx];
            sw = sw + wt;
        }
    }
    out[((size_t)y * (size_t)width + (size_t)x) * (size_t)stride] = sv * (1.0f / sw);
}

// out3 != nullptr: the last pass, 12-byte pixels for the caller; else the padded ping-pong image (fourth word: v_{i+1}, or 0 with the colour term off).
__device__ __forceinline__ void dn_store(const float4& v, size_t i, float4* out4, float* out3) {
    if (out3) { out3[3 * i] = v.x; out3[3 * i + 1] = v.y; out3[3 * i + 2] = v.z; }
    else out4[i] = v;
}

template <uint32_t F>
__global__ __launch_bounds__(256) void dn_packed_kernel(DnPass a, const float4* g0, const float4* g1, const float4* c, float4* out4, float* out3) {
    const int x = (int)(blockIdx.x * 64u + threadIdx.x), y = (int)(blockIdx.y * 4u + threadIdx.y);
    if (x >= a.width || y >= a.height) return;
    const DnPackedFetch<F> f{g0, g1, c, a.width, a.height};
    dn_store(dn_filter<F>(f, a, x, y), (size_t)y * (size_t)a.width + (size_t)x, out4, out3);
}

// v_in / v_out (colour term on): the 4-byte images of v_i and v_{i+1}; v_out == nullptr in the last pass.
template <uint32_t F>
__global__ __launch_bounds__(256) void dn_plain_kernel(DnPass a, const float* normal, const float* albedo, const float* depth, const float* c, float* out3,
                                                       const float* v_in, float* v_out) {
    const int x = (int)(blockIdx.x * 64u + threadIdx.x), y = (int)(blockIdx.y * 4u + threadIdx.y);
    if (x >= a.width || y >= a.height) return;
    const DnPlainFetch<F> f{normal, albedo, depth, c, v_in, a.width, a.height};
    const size_t i = (size_t)y * (size_t)a.width + (size_t)x;
    const float4 r = dn_filter<F>(f, a, x, y);
    dn_store(r, i, nullptr, out3);
    if ((F & kDnColour) && v_out) v_out[i] = r.w;
}

// Dynamic LDS: colour tile | G0 tile (normal or depth on) | G1 tile (albedo on), each pitch * pitch records, pitch = 32 + 4 * step.
template <uint32_t F>
__global__ __launch_bounds__(1024) void dn_lds_kernel(DnPass a, const float4* g0, const float4* g1, const float4* c, float4* out4, float* out3) {
    extern __shared__ float4 dn_tile[];
    const int pitch = kDnTile + 4 * a.step, records = pitch * pitch;
    float4* const lc = dn_tile;
    float4* const l0 = lc + records;
    float4* const l1 = l0 + ((F & (kDnNormal | kDnDepth)) ? records : 0);
    const int x0 = (int)blockIdx.x * kDnTile, y0 = (int)blockIdx.y * kDnTile;
    const int ox = x0 - 2 * a.step, oy = y0 - 2 * a.step;
    const int tid = (int)(threadIdx.y * (uint32_t)kDnTile + threadIdx.x);
    for (int r = tid; r < records; r += kDnTile * kDnTile) {
        const int ly = r / pitch, lx = r - ly * pitch;
        const int gx = ox + lx, gy = oy + ly;
        if (gx < 0 || gx >= a.width || gy < 0 || gy >= a.height) continue;
        const size_t i = (size_t)gy * (size_t)a.width + (size_t)gx;
        lc[r] = c[i];
        if (F & (kDnNormal | kDnDepth)) l0[r] = g0[i];
        if (F & kDnAlbedo) l1[r] = g1[i];
    }
    __syncthreads();
    const int x = x0 + (int)threadIdx.x, y = y0 + (int)threadIdx.y;
    if (x >= a.width || y >= a.height) return;
    const DnLdsFetch<F> f{l0, l1, lc, ox, oy, pitch};
    dn_store(dn_filter<F>(f, a, x, y), (size_t)y * (size_t)a.width + (size_t)x, out4, out3);
}

uint32_t dn_lds_bytes(uint32_t flags, int step) {
    const uint32_t pitch = (uint32_t)(kDnTile + 4 * step);
    const uint32_t images = 1u + ((flags & (kDnNormal | kDnDepth)) ? 1u : 0u) + ((flags & kDnAlbedo) ? 1u : 0u);
    return pitch * pitch * 16u * images;
}

enum DnVariant { DN_AUTO = 0, DN_PLAIN, DN_PACKED, DN_LDS };

DnVariant dn_variant_from_env() {
    const char* e = getenv("TRT_DENOISE_VARIANT");
    if (!e || !*e) return DN_AUTO;
    if (!strcmp(e, "plain")) return DN_PLAIN;
    if (!strcmp(e, "packed")) return DN_PACKED;
    if (!strcmp(e, "lds")) return DN_LDS;
    return DN_AUTO;
}

// Which tuned form runs the pass of this step.  The default is the LDS tile for steps 1 and 2 and the global records beyond (the
// layout the halo overhead suggests: 1.27 x and 1.56 x the tile's records staged, 2.25 x at step 4); tools/denoise_bench.py times both.
bool dn_choose_lds(DnVariant v, int step) {
    if (step > kDnLdsMaxStep) return false;
    if (v == DN_LDS) return true;
    return v == DN_AUTO && step <= 2;
}

#define DN_FOR_FLAGS(flags, CALL)                                                                  \
    switch (flags) {                                                                               \
        case 0u: CALL(0u); break;                                                                  \
        case 1u: CALL(1u); break;                                                                  \
        case 2u: CALL(2u); break;                                                                  \
        case 3u: CALL(3u); break;                                                                  \
        case 4u: CALL(4u); break;                                                                  \
        case 5u: CALL(5u); break;                                                                  \
        case 6u: CALL(6u); break;                                                                  \
        case 7u: CALL(7u); break;                                                                  \
        case 8u: CALL(8u); break;                                                                  \
        case 9u: CALL(9u); break;                                                                  \
        case 10u: CALL(10u); break;                                                                \
        case 11u: CALL(11u); break;                                                                \
        case 12u: CALL(12u); break;                                                                \
        case 13u: CALL(13u); break;                                                                \
        case 14u: CALL(14u); break;                                                                \
        default: CALL(15u); break;                                                                 \
    }

// The caller's scratch: up to 15 bytes to reach a 16-byte boundary, then four images of 16 bytes per pixel - colour A, colour B, G0, G1.
// (The plain form uses the first two as 12-byte images and, with the colour term on, the first 4 bytes per pixel of the other two for v_i.)
uint64_t dn_scratch_bytes(uint32_t width, uint32_t height) { return 16u + 4u * (uint64_t)q_align16((size_t)width * height * 16u); }

struct DnPlan {
    trt_denoise_params p;
    uint32_t flags;
    float inv_a;
    float sigma_c2 = 0.0f;               // colour term on: sigma_color * sigma_color
    const float* variance = nullptr;     // colour term on: the caller's variance image
};

int dn_check_params(const trt_denoise_params* params, DnPlan& plan) {
    if (params) plan.p = *params;
    else trt_denoise_params_default(&plan.p);
    const trt_denoise_params& p = plan.p;
    if (p.iterations < 1u || p.iterations > 8u) return query_fail(TRT_ERR_INVALID_ARG, "iterations must be 1..8");
    if (p.normal_power_log2 > 10u) return query_fail(TRT_ERR_INVALID_ARG, "normal_power_log2 must be 0..10");
    if (p.sigma_albedo != p.sigma_albedo || p.sigma_depth != p.sigma_depth) return query_fail(TRT_ERR_INVALID_ARG, "a sigma is NaN");
    for (int i = 0; i < 4; i++)
        if (p.reserved[i] != 0u) return query_fail(TRT_ERR_INVALID_ARG, "trt_denoise_params.reserved must be zero");
    return TRT_OK;
}

bool dn_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// Everything that is TRT_ERR_INVALID_ARG, before any device work.
int dn_check(const trt_denoise_inputs* in, uint32_t width, uint32_t height, const trt_denoise_params* params, const float* out, DnPlan& plan) {
    if (!in || !in->color || !out) return query_fail(TRT_ERR_INVALID_ARG, "null argument");
    if (width == 0u || height == 0u) return query_fail(TRT_ERR_INVALID_ARG, "width and height must be positive");
    if (width > kDnMaxSide || height > kDnMaxSide) return query_fail(TRT_ERR_INVALID_ARG, "width and height must not exceed 65536");
    const int rc = dn_check_params(params, plan);
    if (rc != TRT_OK) return rc;
    const size_t n = (size_t)width * height;
    if (dn_overlap(out, n * 12u, in->color, n * 12u) || (in->albedo && dn_overlap(out, n * 12u, in->albedo, n * 12u)) ||
        (in->normal && dn_overlap(out, n * 12u, in->normal, n * 12u)) || (in->depth && dn_overlap(out, n * 12u, in->depth, n * 4u)))
        return query_fail(TRT_ERR_INVALID_ARG, "the output must not overlap an input");
    plan.flags = (in->normal ? kDnNormal : 0u) | ((in->albedo && plan.p.sigma_albedo > 0.0f) ? kDnAlbedo : 0u) |
                 ((in->depth && plan.p.sigma_depth > 0.0f) ? kDnDepth : 0u);
    plan.inv_a = (plan.flags & kDnAlbedo) ? 1.0f / (plan.p.sigma_albedo * plan.p.sigma_albedo) : 0.0f;
    return TRT_OK;
}

// trt_denoise_ex's extra argument, after dn_check: NULL, a NULL variance or sigma_color <= 0 leave the plan as trt_denoise's.
int dn_check_colour(const trt_denoise_color* col, uint32_t width, uint32_t height, const float* out, DnPlan& plan) {
    if (!col) return TRT_OK;
    if (col->sigma_color != col->sigma_color) return query_fail(TRT_ERR_INVALID_ARG, "sigma_color is NaN");
    for (int i = 0; i < 5; i++)
        if (col->reserved[i] != 0u) return query_fail(TRT_ERR_INVALID_ARG, "trt_denoise_color.reserved must be zero");
    const size_t n = (size_t)width * height;
    if (col->variance && dn_overlap(out, n * 12u, col->variance, n * 4u)) return query_fail(TRT_ERR_INVALID_ARG, "the output must not overlap an input");
    if (col->variance && col->sigma_color > 0.0f) {
        plan.flags |= kDnColour;
        plan.sigma_c2 = col->sigma_color * col->sigma_color;
        plan.variance = col->variance;
    }
    return TRT_OK;
}

template <uint32_t F>
hipError_t dn_launch_lds(const DnPass& a, dim3 grid, uint32_t lds, const float4* g0, const float4* g1, const float4* c, float4* out4, float* out3,
                         hipStream_t stream) {
    if (lds > 48u * 1024u) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&dn_lds_kernel<F>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    dn_lds_kernel<F><<<grid, dim3(kDnTile, kDnTile), lds, stream>>>(a, g0, g1, c, out4, out3);
    return hipGetLastError();
}

// All passes on `stream`; every buffer is on the device.  Nothing is allocated.
hipError_t dn_launch(const trt_denoise_inputs& in, uint32_t width, uint32_t height, const DnPlan& plan, float* d_out, void* d_scratch, hipStream_t stream) {
    const size_t n = (size_t)width * height;
    const size_t image = q_align16(n * 16u);
    char* const base = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(d_scratch) + 15u) & ~(uintptr_t)15u);
    const DnVariant variant = dn_variant_from_env();
    const uint32_t flags = plan.flags;
    // a guide whose term is off is not read at all
    const float* const normal = (flags & kDnNormal) ? in.normal : nullptr;
    const float* const albedo = (flags & kDnAlbedo) ? in.albedo : nullptr;
    const float* const depth = (flags & kDnDepth) ? in.depth : nullptr;
    DnPass a;
    a.width = (int)width;
    a.height = (int)height;
    a.npow = plan.p.normal_power_log2;
    a.inv_a = plan.inv_a;
    a.sigma_depth = plan.p.sigma_depth;
    a.sigma_c2 = plan.sigma_c2;
    const bool colour = (flags & kDnColour) != 0u;
    const float* const variance = plan.variance;           // (a device pointer: dn_launch's callers put it there)
    const dim3 rows_grid((width + 63u) / 64u, (height + 3u) / 4u), rows_block(64, 4);
    hipError_t e = hipSuccess;
    if (variant == DN_PLAIN) {
        float* const img[2] = {reinterpret_cast<float*>(base), reinterpret_cast<float*>(base + image)};
        float* const vimg[2] = {reinterpret_cast<float*>(base + 2u * image), reinterpret_cast<float*>(base + 3u * image)};
        if (colour) {
            dn_var0_kernel<<<rows_grid, rows_block, 0, stream>>>(variance, a.width, a.height, vimg[0], 1);
            e = hipGetLastError();
        }
        const float* src = in.color;
        for (uint32_t i = 0; i < plan.p.iterations && e == hipSuccess; i++) {
            a.step = 1 << i;
            const bool last = i + 1u == plan.p.iterations;
            float* const dst = last ? d_out : img[i & 1u];
            const float* const v_in = colour ? vimg[i & 1u] : nullptr;
            float* const v_out = colour && !last ? vimg[(i + 1u) & 1u] : nullptr;
#define DN_CALL(F) dn_plain_kernel<F><<<rows_grid, rows_block, 0, stream>>>(a, normal, albedo, depth, src, dst, v_in, v_out)
            DN_FOR_FLAGS(flags, DN_CALL)
#undef DN_CALL
            e = hipGetLastError();
            src = dst;
        }
        return e;
    }
    float4* const col[2] = {reinterpret_cast<float4*>(base), reinterpret_cast<float4*>(base + image)};
    float4* const g0 = reinterpret_cast<float4*>(base + 2u * image);
    float4* const g1 = reinterpret_cast<float4*>(base + 3u * image);
    dn_pack_kernel<<<dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, stream>>>(in.color, albedo, normal, depth, n, col[0], g0, g1);
    e = hipGetLastError();
    if (colour && e == hipSuccess) {
        dn_var0_kernel<<<rows_grid, rows_block, 0, stream>>>(variance, a.width, a.height, &col[0]->w, 4);
        e = hipGetLastError();
    }
    const dim3 tile_grid((width + kDnTile - 1u) / kDnTile, (height + kDnTile - 1u) / kDnTile);
    for (uint32_t i = 0; i < plan.p.iterations && e == hipSuccess; i++) {
        a.step = 1 << i;
        const bool last = i + 1u == plan.p.iterations;
        const float4* const src = col[i & 1u];
        float4* const dst4 = last ? nullptr : col[(i + 1u) & 1u];
        float* const dst3 = last ? d_out : nullptr;
        if (dn_choose_lds(variant, a.step)) {
            const uint32_t lds = dn_lds_bytes(flags, a.step);
            if (lds > kDnLdsPerCu) return hipErrorInvalidConfiguration;                // what the kernel assumes, checked where the launch is made
#define DN_CALL(F) e = dn_launch_lds<F>(a, tile_grid, lds, g0, g1, src, dst4, dst3, stream)
            DN_FOR_FLAGS(flags, DN_CALL)
#undef DN_CALL
        } else {
#define DN_CALL(F) dn_packed_kernel<F><<<rows_grid, rows_block, 0, stream>>>(a, g0, g1, src, dst4, dst3)
            DN_FOR_FLAGS(flags, DN_CALL)
#undef DN_CALL
            e = hipGetLastError();
        }
    }
    return e;
}

}  // namespace
}  // namespace trt

extern "C" {

void trt_denoise_params_default(trt_denoise_params* out) {
    if (!out) return;
    memset(out, 0, sizeof(*out));
    out->iterations = 4u;
    out->normal_power_log2 = 7u;
    out->sigma_albedo = 0.1f;
    out->sigma_depth = 0.05f;
}

void trt_denoise_color_default(trt_denoise_color* out) {
    if (!out) return;
    memset(out, 0, sizeof(*out));
    out->variance = nullptr;
    out->sigma_color = trt::kDnSigmaColourDefault;                 // the table it was chosen from
}

// Host arithmetic only: works without a device.  0 = invalid arguments.
uint64_t trt_denoise_scratch_bytes(uint32_t width, uint32_t height, const trt_denoise_params* params) {
    trt::DnPlan plan;
    if (width == 0u || height == 0u || width > trt::kDnMaxSide || height > trt::kDnMaxSide) return 0u;
    if (trt::dn_check_params(params, plan) != TRT_OK) return 0u;
    return trt::dn_scratch_bytes(width, height);
}

int trt_denoise_ex_device(const trt_denoise_inputs* d_in, const trt_denoise_color* color, uint32_t width, uint32_t height,
                          const trt_denoise_params* params, float* d_out, void* d_scratch, uint64_t scratch_bytes, void* stream) {
    trt::DnPlan plan;
    int rc = trt::dn_check(d_in, width, height, params, d_out, plan);
    if (rc != TRT_OK) return rc;
    rc = trt::dn_check_colour(color, width, height, d_out, plan);
    if (rc != TRT_OK) return rc;
    if (!d_scratch) return trt::query_fail(TRT_ERR_INVALID_ARG, "null scratch");
    if (scratch_bytes < trt::dn_scratch_bytes(width, height))
        return trt::query_fail(TRT_ERR_INVALID_ARG, "scratch is smaller than trt_denoise_scratch_bytes");
    rc = trt::query_require_device();
    if (rc != TRT_OK) return rc;
    const hipError_t e = trt::dn_launch(*d_in, width, height, plan, d_out, d_scratch, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return trt::query_fail_hip(e, "denoise launch");
    return TRT_OK;
}

int trt_denoise_device(const trt_denoise_inputs* d_in, uint32_t width, uint32_t height, const trt_denoise_params* params, float* d_out,
                       void* d_scratch, uint64_t scratch_bytes, void* stream) {
    return trt_denoise_ex_device(d_in, nullptr, width, height, params, d_out, d_scratch, scratch_bytes, stream);
}

// Host buffers: device copies of the call's own, one stream-ordered sequence on the default stream, complete when the call returns.
int trt_denoise_ex(const trt_denoise_inputs* in, const trt_denoise_color* color, uint32_t width, uint32_t height, const trt_denoise_params* params,
                   float* out) {
    return trt::host_form([&]() -> int {
        trt::DnPlan plan;
        int rc = trt::dn_check(in, width, height, params, out, plan);
        if (rc != TRT_OK) return rc;
        rc = trt::dn_check_colour(color, width, height, out, plan);
        if (rc != TRT_OK) return rc;
        rc = trt::query_require_device();
        if (rc != TRT_OK) return rc;
        const size_t n = (size_t)width * height;
        const void* const host[5] = {in->color, (plan.flags & trt::kDnAlbedo) ? in->albedo : nullptr, (plan.flags & trt::kDnNormal) ? in->normal : nullptr,
                                     (plan.flags & trt::kDnDepth) ? in->depth : nullptr, (plan.flags & trt::kDnColour) ? plan.variance : nullptr};
        const size_t item[5] = {12u, 12u, 12u, 4u, 4u};
        trt::HostStage st("denoise buffers");
        size_t r[5];
        for (int i = 0; i < 5; i++) r[i] = st.reserve(n * item[i], host[i] != nullptr);
        const size_t r_out = st.reserve(n * 12u), r_scratch = st.reserve((size_t)trt::dn_scratch_bytes(width, height));
        st.alloc();
        for (int i = 0; i < 5; i++) st.up(r[i], host[i], n * item[i], "hipMemcpy of the inputs");
        const trt_denoise_inputs din{st.ptr<float>(r[0]), st.ptr<float>(r[1]), st.ptr<float>(r[2]), st.ptr<float>(r[3])};
        plan.variance = st.ptr<float>(r[4]);
        if (st.ok()) st.run(trt::dn_launch(din, width, height, plan, st.ptr<float>(r_out), st.ptr<char>(r_scratch), nullptr), "denoise launch");
        st.down(out, r_out, n * 12u, "hipMemcpy of the result");
        return st.finish();
    });
}

int trt_denoise(const trt_denoise_inputs* in, uint32_t width, uint32_t height, const trt_denoise_params* params, float* out) {
    return trt_denoise_ex(in, nullptr, width, height, params, out);
}

}  // extern "C"
