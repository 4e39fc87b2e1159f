// pixels.hip — sparse rendering of caller-chosen pixels (tinyrt.h trt_render_pixels / trt_render_pixels_device) and the selection of the
// pixels whose estimate is still too noisy (trt_select_pixels / trt_select_pixels_device), written for gfx950 (CDNA4) only.
//
// The render entry points trace every pixel of their rows for a whole sample range; the band fields cut rows, never columns.  This unit
// traces a LIST of pixels and leaves, for each of them, the bytes trt_render_moments_device would have left: the same RNG stream
// (seed, image pixel, sample), the same bounce loop (closest hit, shade_hit of rt_path.h), and the imager's fold
//   acc.ch = acc.ch + c.ch * inv_spp;   m2.ch = m2.ch + (c.ch * c.ch) * inv_spp
// in sample order, one IEEE f32 operation per operator (streamed.hip stream_fold_moments_kernel), here in registers: a lane owns a pixel
// for all samples of the call, so no radiance record goes through memory and there is no second kernel.  Every other byte of the two
// buffers is left alone.  Adaptive sampling is then a host loop over two primitives: render a list, select the next one (api.py).
//
// There is no walk code in this file and none of the render kernels is touched: the kernel calls the entry points of rt_path.h with the
// dynamic LDS laid out as the queries lay it out (scene copy | leaf stack: threads x slots x 8 bytes; the run, the place of the stack and the refill's
// cursor step are wave_run.h's), and is launched by the rule of the queries (query_plan.h) with list entries in place of rays: a wave owns a
// contiguous run of the list.
//
// Work: the wave runs in rounds.  At the top of a round every lane without a pixel takes the next entry of the run, every lane without a
// path starts its pixel's next sample; then all lanes that own a pixel trace one bounce.  A lane whose path ended in a round therefore has
// a new one in the next, whatever the walk: no lane idles while its neighbours finish longer paths.  With the two resumable walks (LDS
// tree, 16-byte nodes) a walk still under way when at most `stragglers` lanes walk is parked in the lane's leaf stack and resumed beside
// the fresh rays, as the feature buffers' and the queries' kernels do.
#include <vector>

#include "kernels.h"
#include "query_plan.h"
#include "rt_path.h"
#include "scene_query.h"
#include "wave_run.h"

namespace trt {

struct PixelsArgs {
    const uint32_t* pixels;          // n local pixel indices r * width + x
    const uint32_t* d_count;         // nullptr, or the number of entries to use (at most n)
    float* accum;                    // npixels x 3
    float* moment2;                  // npixels x 3, or nullptr: not wanted
    unsigned long long* counters;    // nullptr, or [CTR_SAMPLES], [CTR_RAYS] are added to
    uint32_t n, npixels;             // list length; pixels of the local image (rows x width): an entry >= npixels is skipped
    uint32_t pixels_per_wave;        // wave w owns entries [w * pixels_per_wave, ...)
    uint32_t slots, stragglers;      // as in query.hip QueryArgs
};

// Entries the launch uses: min(*d_count, n).  The count may have been written by the kernel before this one on the stream
// (select_write_kernel), so it is read with a vector load from memory (volatile: never through the scalar cache) and made wave-uniform.
TRT_DEV uint32_t px_entries(const uint32_t* d_count, uint32_t n) {
    if (d_count == nullptr) return n;
    const uint32_t c = __builtin_amdgcn_readfirstlane(*reinterpret_cast<const volatile uint32_t*>(d_count));
    return c < n ? c : n;
}

// ra.sample_begin < ra.sample_end and ra.max_bounces > 0 (launch_pixels: nothing to trace launches pixels_zero_kernel or nothing)
template <int MODE, int WALK, int THREADS, int MINW>
__global__ __launch_bounds__(THREADS, MINW) void pixels_kernel(SceneDev scd, CameraDev cam, RenderArgs ra, PixelsArgs pa, const float4* __restrict__ leaf_list,
                                                                    const uint4* __restrict__ nodes16) {
    stage_scene_to_lds<MODE>(scd);
    const FlatReuse flat_reuse = axis_quads_to_lds<MODE, false, WALK>(scd, ra.flat_reuse);
    const SceneAcc<MODE> sc{scd.blob, scd.L};
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n = px_entries(pa.d_count, pa.n);
    const unsigned long long begin64 = wave_begin<THREADS>(pa.pixels_per_wave);
    if (begin64 >= n) return;                                               // (after the barriers above)
    const uint32_t begin = (uint32_t)begin64;
    const uint32_t count = wave_count(n, pa.pixels_per_wave, begin);
    // this lane's postponed-leaf stack: behind the scene copy, slots x 64 x 8 bytes per wave
    float2* const stack = WALK != WALK_REGS ? reinterpret_cast<float2*>(lds_behind_scene(sc)) + (threadIdx.x >> 6) * (64u * pa.slots) + lane : nullptr;
    const V3 background = v3(ra.background[0], ra.background[1], ra.background[2]);
    Counters<false> ctr;
    constexpr bool kResumable = WALK == WALK_COMPACT || WALK == WALK_LDS_STACK;

    uint32_t cursor = 0;                                                    // wave-uniform
    bool own = false, has_path = false, walking = false;                    // the lane owns a pixel; a path of it is under way; its walk is parked
    uint32_t pix = 0, s = 0;
    uint32_t n_samples = 0, n_rays = 0;
    V3 acc = v3(0.0f, 0.0f, 0.0f), m2 = v3(0.0f, 0.0f, 0.0f);
    Path p;
    p.ray.o = v3(0.0f, 0.0f, 0.0f); p.ray.d = v3(0.0f, 0.0f, 0.0f);
    p.color = v3(0.0f, 0.0f, 0.0f); p.atten = v3(0.0f, 0.0f, 0.0f);
    p.remain = 0u;
    p.rng.s0 = 0u; p.rng.s1 = 0u;
    for (;;) {
        // ---- refill: every lane without a pixel takes the next entry of the run ----
        const uint64_t need = __builtin_amdgcn_ballot_w64(!own);
        if (need != 0ull && cursor < count) {
            const uint32_t item = cursor + wave_rank(need);
            if (!own && item < count) {
                pix = pa.pixels[begin + item];
                if (pix < pa.npixels) {                                     // an entry past the local image is skipped: neither read nor written
                    s = ra.sample_begin;
                    if (ra.accumulate) {
                        const float* const a = pa.accum + 3ull * pix;
                        acc = v3(a[0], a[1], a[2]);
                        if (pa.moment2) { const float* const m = pa.moment2 + 3ull * pix; m2 = v3(m[0], m[1], m[2]); }
                    } else {
                        acc = v3(0.0f, 0.0f, 0.0f);
                        m2 = v3(0.0f, 0.0f, 0.0f);
                    }
                    own = true;
                }
            }
            cursor = wave_advance(cursor, need, count);
        }
        if (__builtin_amdgcn_ballot_w64(own) == 0ull) {
            if (cursor >= count) break;                                     // the run is done
            continue;                                                       // 64 skipped entries: take the next ones
        }
        if (own) {
            if (!has_path) {                                                // cpu.rs:42-45
                const uint32_t row = pix / cam.width, x = pix - row * cam.width;
                path_begin(p, cam, ra, x, image_row(ra, row), s);
                has_path = true;
                n_samples++;
            }
            bool ended = false;
            if constexpr (kResumable) {
                Trav tr = trav_begin<MODE, WALK == WALK_COMPACT>(sc, p.ray, false);      // a new walk, or the frame of a parked one
                if (walking) trav_unpark(stack, tr); else { tr.t_best = __builtin_inff(); n_rays++; }
                const uint32_t entered = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(true));
                walking = !closest_hit_resume<MODE, false, WALK, false>(sc, p.ray, tr, ctr, pa.slots, stack, leaf_list, nodes16, pa.stragglers, entered);
                if (!walking) ended = shade_hit<MODE, false>(sc, p, tr.prim_best, tr.t_best, background, ctr);
            } else {
                n_rays++;
                float t = 0.0f;
                const uint32_t prim = closest_hit<MODE, false, WALK, false>(sc, p.ray, false, t, ctr, pa.slots, stack, leaf_list, nodes16, flat_reuse);
                ended = shade_hit<MODE, false>(sc, p, prim, t, background, ctr);
            }
            if (ended) {
                // imager.rs:35,50 and the second moment beside it, in the operation order of stream_fold_moments_kernel
                acc = acc + p.color * ra.inv_spp;
                m2.x = m2.x + (p.color.x * p.color.x) * ra.inv_spp;
                m2.y = m2.y + (p.color.y * p.color.y) * ra.inv_spp;
                m2.z = m2.z + (p.color.z * p.color.z) * ra.inv_spp;
                has_path = false;
                s += 1u;
                if (s == ra.sample_end) {
                    float* const a = pa.accum + 3ull * pix;
                    a[0] = acc.x; a[1] = acc.y; a[2] = acc.z;
                    if (pa.moment2) { float* const m = pa.moment2 + 3ull * pix; m[0] = m2.x; m[1] = m2.y; m[2] = m2.z; }
                    own = false;
                }
            }
        }
    }
    flush_counters<false>(pa.counters, n_samples, n_rays, ctr);
}

// Nothing to trace (an empty sample range, max_bounces == 0) without accumulate: the listed pixels become 0, as the frame of trt_render_moments does.
__global__ __launch_bounds__(256) void pixels_zero_kernel(const uint32_t* __restrict__ pixels, const uint32_t* d_count, uint32_t n, uint32_t npixels,
                                                          float* __restrict__ accum, float* __restrict__ moment2) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= px_entries(d_count, n)) return;
    const uint32_t pix = pixels[i];
    if (pix >= npixels) return;
    float* const a = accum + 3ull * pix;
    a[0] = 0.0f; a[1] = 0.0f; a[2] = 0.0f;
    if (moment2) { float* const m = moment2 + 3ull * pix; m[0] = 0.0f; m[1] = 0.0f; m[2] = 0.0f; }
}

// ------------------------------------------------------------------------------------------------------------------
// Selection (tinyrt.h trt_select_pixels): from a candidate list, the pixels whose estimate after `samples_done` samples is still too
// noisy, in candidate order.  Three launches, no atomic anywhere, so the output is the same list on every run:
//   select_count_kernel   a workgroup counts the kept candidates of its tile of kSelectTile
//   select_scan_kernel    ONE workgroup turns the tile counts into exclusive offsets (chunks of kSelectTile, carried in order) and writes the total
//   select_write_kernel   a workgroup evaluates its tile again and writes the kept indices from its offset on, ranked by ballot within a wave
// The test is evaluated twice rather than kept: 24 bytes read per candidate against a flag written and read back, and no scratch per candidate.
// ------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kSelectTile = 256u;

struct SelectArgs {
    const float* accum;
    const float* moment2;
    const uint32_t* candidates;      // nullptr: candidate i is pixel i
    uint32_t n, npixels;
    float k, inv, rel2, abs2;        // N / n, 1 / (n - 1), rel_tol^2, abs_tol^2: computed once on the host
    uint32_t known;                  // 0: samples_done <= 1, the variance is unknown and every candidate is kept
};

// all f32, one IEEE operation per operator, nothing fused (-ffp-contract=off); the sums of tinyrt.h trt_select_pixels
TRT_DEV bool select_keep(const SelectArgs& sa, uint32_t i) {
    const uint32_t pix = sa.candidates ? sa.candidates[i] : i;
    if (pix >= sa.npixels) return false;                                    // not kept and not read
    if (!sa.known) return true;
    const float* const S = sa.accum + 3ull * pix;
    const float* const M = sa.moment2 + 3ull * pix;
    const float sr = S[0] * sa.k, sg = S[1] * sa.k, sb = S[2] * sa.k;
    const float qr = M[0] * sa.k, qg = M[1] * sa.k, qb = M[2] * sa.k;
    float dr = qr - sr * sr, dg = qg - sg * sg, db = qb - sb * sb;
    dr = dr > 0.0f ? dr : 0.0f;
    dg = dg > 0.0f ? dg : 0.0f;
    db = db > 0.0f ? db : 0.0f;
    const float v = ((dr + dg) + db) * sa.inv;
    const float l = (sr + sg) + sb;
    float b = sa.rel2 * (l * l);
    b = b + sa.abs2;
    return v > b;                                                           // a NaN on either side: not kept
}

// Kept candidates of the workgroup's tile before this lane (exclusive), and the tile's total; `waves`: LDS, 4 words.
TRT_DEV uint32_t select_tile_rank(bool keep, uint32_t* waves, uint32_t& total) {
    const uint64_t mask = __builtin_amdgcn_ballot_w64(keep);
    const uint32_t w = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) waves[w] = (uint32_t)__builtin_popcountll(mask);
    __syncthreads();
    uint32_t before = 0;
    total = 0;
    for (uint32_t k = 0; k < kSelectTile / 64u; k++) { if (k < w) before += waves[k]; total += waves[k]; }
    return before + wave_rank(mask);
}

__global__ __launch_bounds__(kSelectTile) void select_count_kernel(SelectArgs sa, uint32_t* __restrict__ tile_counts) {
    __shared__ uint32_t waves[kSelectTile / 64u];
    const uint32_t i = blockIdx.x * kSelectTile + threadIdx.x;
    const bool keep = i < sa.n && select_keep(sa, i);
    uint32_t total = 0;
    (void)select_tile_rank(keep, waves, total);
    if (threadIdx.x == 0u) tile_counts[blockIdx.x] = total;
}

// one workgroup: tile_counts[t] becomes the number of kept candidates in the tiles before t; *count the number kept in all
__global__ __launch_bounds__(kSelectTile) void select_scan_kernel(uint32_t* __restrict__ tile_counts, uint32_t n_tiles, uint32_t* __restrict__ count) {
    __shared__ uint32_t part[kSelectTile];
    uint32_t carry = 0;                                                     // the same in every lane
    for (uint32_t base = 0; base < n_tiles; base += kSelectTile) {
        const uint32_t t = base + threadIdx.x;
        const uint32_t c = t < n_tiles ? tile_counts[t] : 0u;
        part[threadIdx.x] = c;
        __syncthreads();
        // inclusive scan of the chunk (Hillis-Steele: 8 steps of 256 lanes)
        for (uint32_t off = 1; off < kSelectTile; off <<= 1) {
            const uint32_t add = threadIdx.x >= off ? part[threadIdx.x - off] : 0u;
            __syncthreads();
            part[threadIdx.x] += add;
            __syncthreads();
        }
        if (t < n_tiles) tile_counts[t] = carry + part[threadIdx.x] - c;
        carry += part[kSelectTile - 1u];
        __syncthreads();                                                    // (before the next chunk overwrites part[])
    }
    if (threadIdx.x == 0u) *count = carry;
}

__global__ __launch_bounds__(kSelectTile) void select_write_kernel(SelectArgs sa, const uint32_t* __restrict__ tile_offsets, uint32_t* __restrict__ selected) {
    __shared__ uint32_t waves[kSelectTile / 64u];
    const uint32_t i = blockIdx.x * kSelectTile + threadIdx.x;
    const bool keep = i < sa.n && select_keep(sa, i);
    uint32_t total = 0;
    const uint32_t rank = select_tile_rank(keep, waves, total);
    // offset + rank < number kept <= n: within the caller's n entries
    if (keep) selected[tile_offsets[blockIdx.x] + rank] = sa.candidates ? sa.candidates[i] : i;
}

namespace {

#define TRT_PIXELS(MODE, WALK, THREADS, MINW) \
    BatchKernel{reinterpret_cast<const void*>(&pixels_kernel<MODE, WALK, THREADS, MINW>), MODE, WALK, THREADS, MINW}
// the (scene mode, walk, workgroup shape) set of the queries' table, with the register-slot fallback (query_plan.h), so that every scene
// has a kernel.  A lane carries a whole path (ray, colour, attenuation, RNG) and two running sums across the walk, where the feature
// buffers carry a ray and eight sums: the launch bounds are the highest at which the instantiation uses no scratch memory
// (profiles/pixels_resource_usage.txt).  The plan reports the bound (kernel_waves_per_simd).
const BatchKernel kPixelsKernels[] = {
    TRT_PIXELS(MODE_LDS, WALK_FLAT, 256, 5),
    TRT_PIXELS(MODE_LDS, WALK_LDS_STACK, 256, 5),
    TRT_PIXELS(MODE_LDS, WALK_LDS_STACK, 768, 5),
    TRT_PIXELS(MODE_LDS, WALK_REGS, 512, 5),
    TRT_PIXELS(MODE_GLOBAL, WALK_COMPACT, 256, 5),
    TRT_PIXELS(MODE_GLOBAL, WALK_REGS, 256, 5),
};
#undef TRT_PIXELS
constexpr size_t kPixelsShapes = sizeof(kPixelsKernels) / sizeof(kPixelsKernels[0]);

// npixels = rows x width of the local image
hipError_t launch_pixels(const QueryScene& qs, const CameraDev& cd, RenderArgs ra, uint32_t npixels, const uint32_t* d_pixels, uint32_t n,
                         const uint32_t* d_count, float* d_accum, float* d_moment2, unsigned long long* d_counters, hipStream_t stream) {
    if (n == 0 || npixels == 0) return hipSuccess;
    if (ra.sample_begin == ra.sample_end || ra.max_bounces == 0) {
        // nothing to trace: a path with no bounce budget returns colour 0 (cpu.rs:43-47,64); the sums start at 0, or stay
        if (ra.accumulate) return hipSuccess;
        hipLaunchKernelGGL(pixels_zero_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, d_pixels, d_count, n, npixels, d_accum, d_moment2);
        return hipGetLastError();
    }
    SceneDev scd = qs.scene;
    BatchLaunch b;
    const hipError_t e = batch_prepare(scd, n, kPixelsKernels, kPixelsShapes, b);
    if (e != hipSuccess) return e;
    const trt_query_plan& q = b.q;
    CameraDev cam = cd;
    ra.flat_reuse = qs.flat_reuse;
    PixelsArgs pa{d_pixels, d_count, d_accum, d_moment2, d_counters, n, npixels, q.rays_per_wave, q.leaf_slots, q.stragglers};
    void* args[] = {&scd, &cam, &ra, &pa, &b.leaf_list, &b.nodes16};
    return batch_launch(b, args, stream);
}

// What both forms check before any device work.  npixels = pixels of the local image.
int pixels_check(const trt_scene* s, const trt_camera* cam, const trt_render_params* p, const uint32_t* pixels, uint32_t n, const float* accum,
                 RenderArgs& ra, uint32_t& npixels, CameraDev& cd) {
    if (!s || !cam || !p) return query_fail(TRT_ERR_INVALID_ARG, "null argument");
    if (p->collect_stats != 0u) return query_fail(TRT_ERR_INVALID_ARG, "the sparse render has no counting kernels: collect_stats must be 0");
    uint32_t rows = 0;
    const int rc = batch_render_args(cam, p, ra, rows, cd);
    if (rc != TRT_OK) return rc;
    npixels = rows * cam->width;
    if (n > 0u && (!pixels || !accum)) return query_fail(TRT_ERR_INVALID_ARG, "null buffer");
    return TRT_OK;
}

size_t select_tiles(uint32_t n) { return ((size_t)n + kSelectTile - 1u) / kSelectTile; }

int select_check(const float* accum, const float* moment2, uint32_t samples_per_pixel, uint32_t samples_done, uint32_t n, const uint32_t* selected,
                 const uint32_t* count) {
    if (!count) return query_fail(TRT_ERR_INVALID_ARG, "count is null");
    if (samples_per_pixel == 0u) return query_fail(TRT_ERR_INVALID_ARG, "samples_per_pixel must be positive");
    if (samples_done > samples_per_pixel) return query_fail(TRT_ERR_INVALID_ARG, "samples_done must not exceed samples_per_pixel");
    if (n > 0u && (!accum || !moment2 || !selected)) return query_fail(TRT_ERR_INVALID_ARG, "null buffer");
    return TRT_OK;
}

SelectArgs select_args(const float* d_accum, const float* d_moment2, uint32_t npixels, uint32_t samples_per_pixel, uint32_t samples_done,
                       const uint32_t* d_candidates, uint32_t n, float rel_tol, float abs_tol) {
    SelectArgs sa{};
    sa.accum = d_accum; sa.moment2 = d_moment2; sa.candidates = d_candidates;
    sa.n = n; sa.npixels = npixels;
    sa.known = samples_done > 1u ? 1u : 0u;
    sa.k = sa.known ? (float)samples_per_pixel / (float)samples_done : 0.0f;
    sa.inv = sa.known ? 1.0f / (float)(samples_done - 1u) : 0.0f;
    sa.rel2 = rel_tol * rel_tol;
    sa.abs2 = abs_tol * abs_tol;
    return sa;
}

// n > 0; d_scratch holds select_tiles(n) words
hipError_t launch_select(const SelectArgs& sa, uint32_t* d_selected, uint32_t* d_count, uint32_t* d_scratch, hipStream_t stream) {
    const uint32_t tiles = (uint32_t)select_tiles(sa.n);
    hipLaunchKernelGGL(select_count_kernel, dim3(tiles), dim3(kSelectTile), 0, stream, sa, d_scratch);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(kSelectTile), 0, stream, d_scratch, tiles, d_count);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(select_write_kernel, dim3(tiles), dim3(kSelectTile), 0, stream, sa, static_cast<const uint32_t*>(d_scratch), d_selected);
    return hipGetLastError();
}

}  // namespace
}  // namespace trt

extern "C" {

int trt_render_pixels_device(trt_scene* s, const trt_camera* cam, const trt_render_params* p, const uint32_t* d_pixels, uint32_t n,
                             const uint32_t* d_count, float* d_accum, float* d_moment2, uint64_t* d_counters, void* stream) {
    trt::RenderArgs ra;
    trt::CameraDev cd;
    uint32_t npixels = 0;
    int rc = trt::pixels_check(s, cam, p, d_pixels, n, d_accum, ra, npixels, cd);
    if (rc != TRT_OK) return rc;
    if (n == 0u) return TRT_OK;
    rc = trt::query_require_device();
    if (rc != TRT_OK) return rc;
    trt::QueryScene qs;
    rc = trt::query_scene_on_device(s, qs);
    if (rc != TRT_OK) return rc;
    const hipError_t e = trt::launch_pixels(qs, cd, ra, npixels, d_pixels, n, d_count, d_accum, d_moment2,
                                            reinterpret_cast<unsigned long long*>(d_counters), static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return trt::query_fail_hip(e, "sparse render launch");
    return TRT_OK;
}

// Host buffers: the list is validated, then device copies of the list and of the two frames are the call's own, one stream-ordered sequence
// on the default stream, complete when the call returns.  Only the listed pixels are copied back into the caller's buffers.
int trt_render_pixels(trt_scene* s, const trt_camera* cam, const trt_render_params* p, const uint32_t* pixels, uint32_t n, float* accum,
                      float* moment2, trt_stats* stats) {
    return trt::host_form([&]() -> int {
        trt::RenderArgs ra;
        trt::CameraDev cd;
        uint32_t npixels = 0;
        int rc = trt::pixels_check(s, cam, p, pixels, n, accum, ra, npixels, cd);
        if (rc != TRT_OK) return rc;
        {
            std::vector<uint64_t> seen(((size_t)npixels + 63u) / 64u, 0ull);
            for (uint32_t i = 0; i < n; i++) {
                const uint32_t pix = pixels[i];
                if (pix >= npixels) return trt::query_fail(TRT_ERR_INVALID_ARG, "pixel index " + std::to_string(pix) + " at entry " + std::to_string(i) + " is outside the local image");
                if (seen[pix >> 6] >> (pix & 63u) & 1ull) return trt::query_fail(TRT_ERR_INVALID_ARG, "pixel index " + std::to_string(pix) + " is listed twice");
                seen[pix >> 6] |= 1ull << (pix & 63u);
            }
        }
        if (n == 0u) {
            if (stats) *stats = trt_stats{};
            return TRT_OK;
        }
        rc = trt::query_require_device();
        if (rc != TRT_OK) return rc;
        trt::QueryScene qs;
        rc = trt::query_scene_on_device(s, qs);
        if (rc != TRT_OK) return rc;
        const size_t frame = (size_t)npixels * 12u, list = (size_t)n * 4u;
        trt::HostStage st("sparse render buffers");
        const size_t r_list = st.reserve(list), r_acc = st.reserve(frame), r_m2 = st.reserve(frame, moment2 != nullptr);
        st.reserve_counters();
        st.alloc();
        std::vector<float> back(3u * (size_t)npixels);
        st.up(r_list, pixels, list, "hipMemcpy of the list");
        st.zero_counters();
        // the running sums a pass continues go up; a pass that starts them reads nothing
        if (ra.accumulate) st.up(r_acc, accum, frame, "hipMemcpy of the frame");
        if (ra.accumulate) st.up(r_m2, moment2, frame, "hipMemcpy of the second moments");
        st.time_begin();
        if (st.ok())
            st.run(trt::launch_pixels(qs, cd, ra, npixels, st.ptr<uint32_t>(r_list), n, nullptr, st.ptr<float>(r_acc), st.ptr<float>(r_m2), st.counters(), nullptr),
                   "sparse render launch");
        const bool wrote = !(ra.accumulate && (ra.sample_begin == ra.sample_end || ra.max_bounces == 0u));
        for (int b = 0; b < 2 && wrote; b++) {
            float* const host = b == 0 ? accum : moment2;
            if (!host) continue;
            st.down(back.data(), b == 0 ? r_acc : r_m2, frame, "hipMemcpy of the results");
            for (uint32_t i = 0; i < n && st.ok(); i++) {
                const size_t o = 3u * (size_t)pixels[i];
                host[o] = back[o]; host[o + 1u] = back[o + 1u]; host[o + 2u] = back[o + 2u];
            }
        }
        st.read_stats(stats);
        return st.finish();
    });
}

// How launch_pixels would launch a list of n pixels on this scene.
int trt_pixels_launch_plan(const trt_scene* s, uint32_t n, uint32_t compute_units, trt_query_plan* out) {
    return trt::batch_launch_plan(s, n, compute_units, trt::kPixelsKernels, trt::kPixelsShapes, out);
}

uint64_t trt_select_scratch_bytes(uint32_t n) { return (uint64_t)trt::q_align16(trt::select_tiles(n) * sizeof(uint32_t)); }

int trt_select_pixels_device(const float* d_accum, const float* d_moment2, uint32_t npixels, uint32_t samples_per_pixel, uint32_t samples_done,
                             const uint32_t* d_candidates, uint32_t n, float rel_tol, float abs_tol, uint32_t* d_selected, uint32_t* d_count,
                             void* d_scratch, uint64_t scratch_bytes, void* stream) {
    int rc = trt::select_check(d_accum, d_moment2, samples_per_pixel, samples_done, n, d_selected, d_count);
    if (rc != TRT_OK) return rc;
    if (n > 0u && d_candidates) {
        // select_write_kernel writes selected[offset + rank] while other workgroups still read candidates[i]: offset + rank <= i, but that
        // slot may be a candidate of an earlier tile that has not been read yet - compacting in place is a race, so overlap is refused
        const uintptr_t c0 = reinterpret_cast<uintptr_t>(d_candidates), s0 = reinterpret_cast<uintptr_t>(d_selected), bytes = (uintptr_t)n * 4u;
        if (c0 < s0 ? s0 - c0 < bytes : c0 - s0 < bytes)
            return trt::query_fail(TRT_ERR_INVALID_ARG, "d_selected overlaps d_candidates: the device form does not select in place");
    }
    if (n > 0u && (!d_scratch || scratch_bytes < trt_select_scratch_bytes(n)))
        return trt::query_fail(TRT_ERR_INVALID_ARG, "scratch is null or smaller than trt_select_scratch_bytes(n)");
    if (n == 0u) {
        // count 0 and nothing else; without a device there is no buffer to write it to
        if (trt_device_count() > 0) {
            const hipError_t e = hipMemsetAsync(d_count, 0, sizeof(uint32_t), static_cast<hipStream_t>(stream));
            if (e != hipSuccess) return trt::query_fail_hip(e, "hipMemsetAsync of the count");
        }
        return TRT_OK;
    }
    rc = trt::query_require_device();
    if (rc != TRT_OK) return rc;
    const trt::SelectArgs sa = trt::select_args(d_accum, d_moment2, npixels, samples_per_pixel, samples_done, d_candidates, n, rel_tol, abs_tol);
    const hipError_t e = trt::launch_select(sa, d_selected, d_count, static_cast<uint32_t*>(d_scratch), static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return trt::query_fail_hip(e, "selection launch");
    return TRT_OK;
}

// Host buffers: device copies of the call's own on the default stream, complete when the call returns.
int trt_select_pixels(const float* accum, const float* moment2, uint32_t npixels, uint32_t samples_per_pixel, uint32_t samples_done,
                      const uint32_t* candidates, uint32_t n, float rel_tol, float abs_tol, uint32_t* selected, uint32_t* count) {
    return trt::host_form([&]() -> int {
        int rc = trt::select_check(accum, moment2, samples_per_pixel, samples_done, n, selected, count);
        if (rc != TRT_OK) return rc;
        if (n == 0u) { *count = 0u; return TRT_OK; }
        rc = trt::query_require_device();
        if (rc != TRT_OK) return rc;
        const size_t frame = (size_t)npixels * 12u, list = (size_t)n * 4u;
        trt::HostStage st("selection buffers");
        const size_t r_acc = st.reserve(frame), r_m2 = st.reserve(frame), r_cand = st.reserve(list, candidates != nullptr), r_sel = st.reserve(list);
        const size_t r_scratch = st.reserve((size_t)trt_select_scratch_bytes(n)), r_count = st.reserve(16u);
        st.alloc();
        if (frame) st.up(r_acc, accum, frame, "hipMemcpy of the sums");
        if (frame) st.up(r_m2, moment2, frame, "hipMemcpy of the sums");
        st.up(r_cand, candidates, list, "hipMemcpy of the candidates");
        const trt::SelectArgs sa = trt::select_args(st.ptr<float>(r_acc), st.ptr<float>(r_m2), npixels, samples_per_pixel, samples_done,
                                                    st.ptr<uint32_t>(r_cand), n, rel_tol, abs_tol);
        if (st.ok()) st.run(trt::launch_select(sa, st.ptr<uint32_t>(r_sel), st.ptr<uint32_t>(r_count), st.ptr<uint32_t>(r_scratch), nullptr), "selection launch");
        uint32_t kept = 0;
        st.down(&kept, r_count, sizeof(kept), "hipMemcpy of the count");
        if (st.ok() && kept > n) return trt::query_fail(TRT_ERR_HIP, "selection kept more candidates than it was given");
        if (kept) st.down(selected, r_sel, (size_t)kept * 4u, "hipMemcpy of the selection");
        if (st.ok()) *count = kept;
        return st.finish();
    });
}

}  // extern "C"
