// streamed.hip — "streamed" backend (TRT_BACKEND_STREAMED), written for gfx950 (CDNA4) only.
//
// The megakernel binds a lane to one pixel for a whole launch.  That ties the length of a launch to the most
// expensive pixel (in the Cornell box the per-pixel cost varies ~2x across the image) and to the longest of a
// wave's 64 sample chains; both hurt exactly when the launch is small: a short progressive pass, or one of 8 GPUs'
// share of the frame (2048 workgroups for 1792 resident ones: measured 16.5 Gray/s per GPU against 25.0 on the
// whole frame).  Here a SAMPLE, not a pixel, is the unit of work:
//
//  * SAMPLE kernel: a persistent grid of waves pulls batches (one 8x8 pixel tile x 8 consecutive samples = 512 items,
//    ~3.6 k rays: small against a wave's share even of one GPU's eighth of a frame) from a global counter, one
//    returning atomic per batch (<10 per us, the counter word saturates near 88); inside a wave every lane takes the next item of
//    the batch whenever its path ends (ballot + mbcnt ranks on a wave-uniform cursor, no atomics), so no lane waits
//    for a neighbour's longer chain or a more expensive pixel.  The finished sample's radiance (12 B, one store) goes to an HBM
//    buffer laid out [tile][sample][lane of the tile] (stream_fold_kernel).
//  * FOLD kernel: one lane per pixel adds that pixel's radiances in sample order,
//    `pixels[idx] += color * (1/spp)` (imager.rs:50): the same sequence of f32 additions as the reference, so the
//    frame is bit-identical to the megakernel's and the oracle's whatever lane computed which sample.
//
// Cost: 12 B written + 12 B read per sample (a sample is ~7 rays, ~4.6 KB algorithmic), i.e. <1 % extra traffic, and
// two launches per chunk of samples (sized to a radiance buffer of at most 16 GB: streamed_chunk_spp) instead of one.  stream_sample_kernel keeps the
// primary-ray stock of kernels.hip (items are taken ahead); stream_pool_kernel, used for small LDS scenes, generates the
// primary rays of a whole wave at once into an LDS pool.
#include <mutex>
#include <string>

#include "flat_literal_rtc.h"
#include "host_stage.h"
#include "kernels.h"
#include "literal_kernel.h"
#include "rt_path.h"
#include "stream_plan.h"
#include "stream_pool.h"
#include "wave_run.h"

namespace trt {

template <int MODE, bool STATS, int MINW = 1, int THREADS = 256, int WALK = WALK_RUNTIME, bool LAZY = false>
__global__ __launch_bounds__(THREADS, MINW) void stream_sample_kernel(SceneDev scd, CameraDev cam, RenderArgs ra,
                                                                             float* __restrict__ colors,
                                                                             uint32_t* __restrict__ batch_counter,
                                                                             unsigned long long* __restrict__ counters,
                                                                             uint32_t tiles_x, uint32_t n_tiles, uint32_t n_batches, uint32_t batch_spp,
                                                                             const float4* __restrict__ leaf_list,
                                                                             const uint4* __restrict__ nodes16) {
    stage_scene_to_lds<MODE>(scd);
    const FlatReuse flat_reuse = axis_quads_to_lds<MODE, STATS, WALK>(scd, ra.flat_reuse);      // axis-exact quads: the LDS copy's records rewritten (rt_path.h)
    const SceneAcc<MODE> sc{scd.blob, scd.L};
    const uint32_t lane = threadIdx.x & 63u;
    const V3 background = v3(ra.background[0], ra.background[1], ra.background[2]);
    const uint32_t n_spp = ra.sample_end - ra.sample_begin;
    // postponed-leaf stack (rt_path.h walk_fast_lds): behind the scene copy, leaf_slots x 64 x 8 bytes per wave
    float2* const leaf_stack = (WALK != WALK_REGS && (WALK != WALK_RUNTIME || ra.lds_leaf_stack))
        ? reinterpret_cast<float2*>(lds_behind_scene(sc)) + (threadIdx.x >> 6) * (64u * ra.leaf_slots) + lane
        : nullptr;

    // wave-uniform work cursor
    uint32_t tile_x0 = 0, tile_row0 = 0, tile_slot0 = 0, ds0 = 0, items_per_batch = 0, cursor = 0;    // cursor == items_per_batch: batch used up
    bool exhausted = false;

    Path p;
    p.remain = 0u;
    bool has_path = false, stocked = false;
    uint32_t out_idx = 0, stock_idx = 0;                                  // radiance record of the sample (radiance_slot below): < 2^32 (see streamed_chunk_spp)
    Ray stock_ray;
    Rng stock_rng;
    uint32_t n_samples = 0, n_rays = 0;
    Counters<STATS> ctr;
    // resumable walks (rt_path.h walk_compact, walk_fast_lds): a round's walk phase ends once only a few lanes still walk; they carry
    // their walk into the next round (100 k spheres: 324 trips per round for 222 box steps per ray, +10 %; random-spheres: see DESIGN 13)
    constexpr bool kResumable = !STATS && (WALK == WALK_COMPACT || WALK == WALK_LDS_STACK);
    bool walking = false;                                                         // this lane's walk is parked in its leaf stack (kResumable only)

    TRT_CLK_START(ctr);
    for (;;) {
        // ---- take items ahead: whenever a lane has neither a path nor a stocked ray, every lane without stock takes one ----
        if (!exhausted && __builtin_amdgcn_ballot_w64(!has_path && !stocked) != 0ull) {
            if (cursor >= items_per_batch) {
                uint32_t b = 0;
                if (lane == 0u) b = atomicAdd(batch_counter, 1u);
                b = __builtin_amdgcn_readfirstlane(b);
                if (b >= n_batches) {
                    exhausted = true;
                } else {
                    const uint32_t tile = b % n_tiles;                                // consecutive batches: neighbouring tiles, same samples
                    ds0 = (b / n_tiles) * batch_spp;
                    tile_x0 = (tile % tiles_x) * 8u;
                    tile_row0 = (tile / tiles_x) * 8u;
                    tile_slot0 = tile * n_spp * 64u;                                  // the tile's radiance records (radiance_slot)
                    items_per_batch = 64u * (n_spp - ds0 < batch_spp ? n_spp - ds0 : batch_spp);
                    cursor = 0;
                }
            }
            if (!exhausted) {
                const uint64_t want = __builtin_amdgcn_ballot_w64(!stocked);
                const uint32_t item = cursor + wave_rank(want);
                cursor += (uint32_t)__builtin_popcountll(want);
                if (!stocked && item < items_per_batch) {
                    const uint32_t l = item & 63u, ds = ds0 + (item >> 6);         // neighbouring items = neighbouring pixels, same sample
                    const uint32_t x = tile_x0 + (l & 7u), row = tile_row0 + (l >> 3);
                    if (x < cam.width && row < ra.rows_local) {
                        if constexpr (STATS) { if (first_active_lane()) ctr.w_gen++; }
                        const uint32_t y = image_row(ra, row);
                        stock_rng = rng_seed(ra.seed_key, y * cam.width + x, ra.sample_begin + ds);
                        stock_ray = primary_ray(cam, x, y, stock_rng);
                        stock_idx = tile_slot0 + ds * 64u + l;
                        stocked = true;
                    }
                }
            }
        }
        if (!has_path && stocked) {                                               // cpu.rs:42-45
            p.ray = stock_ray;
            p.rng = stock_rng;
            p.color = v3(0.0f, 0.0f, 0.0f);
            p.atten = v3(1.0f, 1.0f, 1.0f);
            p.remain = ra.max_bounces;
            out_idx = stock_idx;
            has_path = true;
            stocked = false;
            n_samples++;
        }
        if (__builtin_amdgcn_ballot_w64(has_path) == 0ull) {
            if (exhausted) break;
            continue;                                                             // a batch of off-image items: fetch the next
        }
        TRT_CLK(ctr, 0);
        if (has_path) {
            if constexpr (STATS) { if (first_active_lane()) ctr.w_rounds++; }
            if constexpr (kResumable) {
                // per-lane tree walk: a lane whose walk is still under way when most of the wave has finished carries it into the
                // next round (rt_path.h walk_compact) and is not shaded in this one
                Trav tr = trav_begin<MODE, WALK == WALK_COMPACT>(sc, p.ray, false);                              // every lane: a new walk, or the frame of a parked one
                if (walking) trav_unpark(leaf_stack, tr); else n_rays++;
                const uint32_t entered = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(true));
                walking = !closest_hit_resume<MODE, STATS, WALK>(sc, p.ray, tr, ctr, ra.leaf_slots, leaf_stack, leaf_list, nodes16, ra.stragglers, entered);
                if (!walking) {
                    if (shade_hit<MODE, STATS, LAZY>(sc, p, tr.prim_best, tr.t_best, background, ctr)) {
                        radiance_store(colors, out_idx, p.color);
                        has_path = false;
                    }
                }
            } else {
                n_rays++;
                float t;
                const uint32_t prim = closest_hit<MODE, STATS, WALK>(sc, p.ray, STATS && ra.ref_tree != 0u, t, ctr, ra.leaf_slots, leaf_stack, leaf_list, nodes16, flat_reuse);
                if (shade_hit<MODE, STATS, LAZY>(sc, p, prim, t, background, ctr)) {
                    radiance_store(colors, out_idx, p.color);
                    has_path = false;
                }
            }
        }
        TRT_CLK(ctr, 3);
    }
    flush_counters<STATS>(counters, n_samples, n_rays, ctr);
}


// ------------------------------------------------------------------------------------------------------------------
// The pool kernel for scenes in global memory with TWO paths per lane (rt_path.h walk_compact2): slot A and slot B of a lane are two
// independent paths - each takes its primary rays from the wave's pool, walks, is shaded and stores its radiance exactly as the one
// path of stream_pool_kernel does - and a round steps both walks in one loop that keeps two node loads in flight per wave.  LDS per
// wave: two postponed-leaf stacks (slot A's, then slot B's) and the ray pool.  The launch plan takes it for scenes beyond L2 (trt_tuning.dual_walk = 0: by
// scene): -2.6 % where the tree fits L2, +2.7 % / +4.2 % on sphere_field 1 M / 4 M (rt_path.h box_loop_compact2 has the finding).  Which lane and which slot
// traces which sample changes; no sample's radiance does (RNG keyed by pixel and sample, radiance stored per sample, folded in order).
// ------------------------------------------------------------------------------------------------------------------
struct DualSlot {
    Path p;
    uint32_t out_idx = 0;
    bool has_path = false;
    bool walking = false;          // the slot's walk is parked in its leaf stack
};

template <int MINW, int THREADS = 256>
__global__ __launch_bounds__(THREADS, MINW) void stream_dual_kernel(SceneDev scd, CameraDev cam, RenderArgs ra,
                                                                           float* __restrict__ colors,
                                                                           uint32_t* __restrict__ batch_counter,
                                                                           unsigned long long* __restrict__ counters,
                                                                           uint32_t tiles_x, uint32_t n_tiles, uint32_t n_batches, uint32_t batch_spp,
                                                                           const float4* __restrict__ leaf_list,
                                                                           const uint4* __restrict__ nodes16) {
    constexpr int MODE = MODE_GLOBAL;
    const SceneAcc<MODE> sc{scd.blob, scd.L};
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const V3 background = v3(ra.background[0], ra.background[1], ra.background[2]);
    const uint32_t n_spp = ra.sample_end - ra.sample_begin;
    char* const lds_tail = reinterpret_cast<char*>(g_lds);
    float2* const stkA = reinterpret_cast<float2*>(lds_tail) + (2u * wave) * (64u * ra.leaf_slots) + lane;
    float2* const stkB = stkA + 64u * ra.leaf_slots;
    uint32_t* const pool = reinterpret_cast<uint32_t*>(lds_tail + (size_t)THREADS * 2u * ra.leaf_slots * sizeof(float2)) + wave * (64u * kPoolDwords);      // behind the two leaf stacks (stream_plan.h LdsLayout::stack_bytes)

    uint32_t tile_x0 = 0, tile_row0 = 0, tile_slot0 = 0, ds0 = 0, items_per_batch = 0, cursor = 0;    // wave-uniform work cursor
    uint32_t pool_head = 0, pool_count = 0;                                            // wave-uniform
    bool exhausted = false;
    uint32_t n_samples = 0, n_rays = 0;
    Counters<false> ctr;
    DualSlot A, B;
    A.p.remain = 0u; B.p.remain = 0u;

    // lanes whose slot has no path take pool entries; an empty pool is refilled by the whole wave (stream_pool_kernel)
    auto take = [&](DualSlot& S) {
        for (;;) {
            const uint64_t need = __builtin_amdgcn_ballot_w64(!S.has_path);
            if (need == 0ull) break;
            if (pool_count == 0u) {
                if (exhausted) break;
                if (cursor >= items_per_batch) {
                    uint32_t b = 0;
                    if (lane == 0u) b = atomicAdd(batch_counter, 1u);
                    b = __builtin_amdgcn_readfirstlane(b);
                    if (b >= n_batches) { exhausted = true; break; }
                    const uint32_t tile = b % n_tiles;
                    ds0 = (b / n_tiles) * batch_spp;
                    tile_x0 = (tile % tiles_x) * 8u;
                    tile_row0 = (tile / tiles_x) * 8u;
                    tile_slot0 = tile * n_spp * 64u;
                    items_per_batch = 64u * (n_spp - ds0 < batch_spp ? n_spp - ds0 : batch_spp);
                    cursor = 0;
                }
                const uint32_t item = cursor + lane;
                cursor += 64u;
                const uint32_t ds = ds0 + (item >> 6);
                const uint32_t x = tile_x0 + (lane & 7u), row = tile_row0 + (lane >> 3);
                const bool valid = x < cam.width && row < ra.rows_local;
                const uint64_t vmask = __builtin_amdgcn_ballot_w64(valid);
                if (valid) {
                    const uint32_t y = image_row(ra, row);
                    Rng rng = rng_seed(ra.seed_key, y * cam.width + x, ra.sample_begin + ds);        // cpu.rs:42-45
                    const Ray ray = primary_ray(cam, x, y, rng);
                    const uint32_t e = wave_rank(vmask);
                    pool[0u * 64u + e] = __float_as_uint(ray.o.x); pool[1u * 64u + e] = __float_as_uint(ray.o.y); pool[2u * 64u + e] = __float_as_uint(ray.o.z);
                    pool[3u * 64u + e] = __float_as_uint(ray.d.x); pool[4u * 64u + e] = __float_as_uint(ray.d.y); pool[5u * 64u + e] = __float_as_uint(ray.d.z);
                    pool[6u * 64u + e] = rng.s0; pool[7u * 64u + e] = rng.s1;
                    pool[8u * 64u + e] = tile_slot0 + ds * 64u + lane;
                }
                pool_head = 0u;
                pool_count = (uint32_t)__builtin_popcountll(vmask);
                if (pool_count == 0u) continue;
            }
            const uint32_t rank = wave_rank(need);
            if (!S.has_path && rank < pool_count) {
                const uint32_t e = pool_head + rank;
                S.p.ray.o = v3(__uint_as_float(pool[0u * 64u + e]), __uint_as_float(pool[1u * 64u + e]), __uint_as_float(pool[2u * 64u + e]));
                S.p.ray.d = v3(__uint_as_float(pool[3u * 64u + e]), __uint_as_float(pool[4u * 64u + e]), __uint_as_float(pool[5u * 64u + e]));
                S.p.rng.s0 = pool[6u * 64u + e]; S.p.rng.s1 = pool[7u * 64u + e];
                S.out_idx = pool[8u * 64u + e];
                S.p.color = v3(0.0f, 0.0f, 0.0f);
                S.p.atten = v3(1.0f, 1.0f, 1.0f);
                S.p.remain = ra.max_bounces;
                S.has_path = true;
                n_samples++;
            }
            const uint32_t wanted = (uint32_t)__builtin_popcountll(need);
            const uint32_t taken = wanted < pool_count ? wanted : pool_count;
            pool_head += taken;
            pool_count -= taken;
        }
    };
    // a finished walk: shade, store the radiance of a finished path; an unfinished one: park it in the slot's leaf stack
    auto settle = [&](DualSlot& S, Trav& tr, bool done, float2* stk) {
        if (!S.has_path) return;
        if (!done) { trav_park(stk, tr); S.walking = true; return; }
        S.walking = false;
        if (shade_hit<MODE, false, true>(sc, S.p, tr.prim_best, tr.t_best, background, ctr)) {
            radiance_store(colors, S.out_idx, S.p.color);
            S.has_path = false;
        }
    };

    TRT_CLK_START(ctr);
    for (;;) {
        take(A);
        take(B);
        if (__builtin_amdgcn_ballot_w64(A.has_path || B.has_path) == 0ull) break;          // the batches are used up
        TRT_CLK(ctr, 0);
        Trav trA = trav_begin<MODE, true>(sc, A.p.ray, false), trB = trav_begin<MODE, true>(sc, B.p.ray, false);   // a new walk, or the frame of a parked one (fused-slab domain: rt_path.h)
        if (A.has_path) { if (A.walking) trav_unpark(stkA, trA); else n_rays++; }
        if (B.has_path) { if (B.walking) trav_unpark(stkB, trB); else n_rays++; }
        const uint32_t entered = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(A.has_path)) +
                                 (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(B.has_path));
        bool doneA = false, doneB = false;
        walk_compact2<MODE>(sc, nodes16, leaf_list, A.p.ray, trA, A.has_path, B.p.ray, trB, B.has_path, ctr, stkA, stkB, ra.leaf_slots, ra.stragglers,
                            entered, doneA, doneB);
        settle(A, trA, doneA, stkA);
        settle(B, trB, doneB, stkB);
        TRT_CLK(ctr, 3);
    }
    flush_counters<false>(counters, n_samples, n_rays, ctr);
}

// pixels[idx] += color * (1/spp), samples in order (imager.rs:35,50).
// Radiance records are TILE-MAJOR (round 4): record (tile, sample, lane) at ((tile * n_spp + sample) * 64 + lane) x 12 bytes, tile = the 8x8-pixel
// tile of the work batches, lane = (row % 8) * 8 + x % 8.  The 64 records of a tile and sample - what one wave finishes within one batch - are 768
// contiguous bytes, twelve whole 64-byte lines that no other wave writes; in rounds 1-3 ([sample][pixel]) they were eight runs of 96 bytes, each
// sharing its lines with neighbouring tiles that other waves finish at other times, and the L2 wrote the partial lines back: WRITE_SIZE 1.8x the
// records' bytes on Cornell, 4.3x on the 100 k-sphere scene (profiles/r03_*_pmc.json).  The fold reads a tile-sample as one 768-byte wave load.
__global__ __launch_bounds__(256) void stream_fold_kernel(const float* __restrict__ colors, float* __restrict__ accum, uint32_t width, uint32_t rows,
                                                          uint32_t tiles_x, uint32_t n_tiles, uint32_t n_spp, float inv_spp, uint32_t accumulate) {
    const uint32_t tile = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (tile >= n_tiles) return;
    const uint32_t x = (tile % tiles_x) * 8u + (lane & 7u), row = (tile / tiles_x) * 8u + (lane >> 3);
    if (x >= width || row >= rows) return;                                      // an edge tile's off-image lanes: records never written, never read
    float* out = accum + 3ull * ((unsigned long long)row * width + x);
    V3 acc = v3(0.0f, 0.0f, 0.0f);
    if (accumulate) acc = v3(out[0], out[1], out[2]);
    const float* rec = colors + 3ull * ((unsigned long long)tile * n_spp * 64ull + lane);
    for (uint32_t s = 0; s < n_spp; s++) {
        const Radiance c = *reinterpret_cast<const Radiance*>(rec + 3ull * 64ull * s);      // one global_load_dwordx3
        acc = acc + v3(c.r, c.g, c.b) * inv_spp;
    }
    out[0] = acc.x; out[1] = acc.y; out[2] = acc.z;
}

// The same fold that also keeps the per-pixel second moment (tinyrt.h trt_render_moments): moment2[idx].ch += (c.ch * c.ch) * (1/spp), in the
// same pass over the records, samples in order, one f32 operation per operator (nothing fused: -ffp-contract=off).  `moment2` has the frame's
// layout; `accumulate` applies to both buffers.  The frame it writes is stream_fold_kernel's, bit for bit: the same operations in the same order.
__global__ __launch_bounds__(256) void stream_fold_moments_kernel(const float* __restrict__ colors, float* __restrict__ accum, float* __restrict__ moment2,
                                                                  uint32_t width, uint32_t rows, uint32_t tiles_x, uint32_t n_tiles, uint32_t n_spp,
                                                                  float inv_spp, uint32_t accumulate) {
    const uint32_t tile = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (tile >= n_tiles) return;
    const uint32_t x = (tile % tiles_x) * 8u + (lane & 7u), row = (tile / tiles_x) * 8u + (lane >> 3);
    if (x >= width || row >= rows) return;                                      // an edge tile's off-image lanes: records never written, never read
    const unsigned long long px = 3ull * ((unsigned long long)row * width + x);
    float* out = accum + px;
    float* out2 = moment2 + px;
    V3 acc = v3(0.0f, 0.0f, 0.0f), m2 = v3(0.0f, 0.0f, 0.0f);
    if (accumulate) { acc = v3(out[0], out[1], out[2]); m2 = v3(out2[0], out2[1], out2[2]); }
    const float* rec = colors + 3ull * ((unsigned long long)tile * n_spp * 64ull + lane);
    for (uint32_t s = 0; s < n_spp; s++) {
        const Radiance c = *reinterpret_cast<const Radiance*>(rec + 3ull * 64ull * s);      // one global_load_dwordx3
        acc = acc + v3(c.r, c.g, c.b) * inv_spp;
        m2.x = m2.x + (c.r * c.r) * inv_spp;
        m2.y = m2.y + (c.g * c.g) * inv_spp;
        m2.z = m2.z + (c.b * c.b) * inv_spp;
    }
    out[0] = acc.x; out[1] = acc.y; out[2] = acc.z;
    out2[0] = m2.x; out2[1] = m2.y; out2[2] = m2.z;
}

// Variance of the pixel estimate from the two folded buffers (tinyrt.h trt_variance): S = accum (the mean), M = moment2 (the mean of the
// squares); per channel d = M - S*S, clamped at 0 (NaN -> 0); variance = ((d.r + d.g) + d.b) * inv_nm1, inv_nm1 = 1.0f / float(N - 1) computed
// once on the host; N <= 1: +inf (unknown).  M - S*S cancels in f32: its error is about 2^-23 * M, which is why d can come out below 0.
__global__ __launch_bounds__(256) void variance_kernel(const float* __restrict__ accum, const float* __restrict__ moment2, uint32_t npixels, float inv_nm1,
                                                       uint32_t known, float* __restrict__ variance) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= npixels) return;
    if (!known) { variance[i] = __builtin_inff(); return; }
    const float* s = accum + 3ull * i;
    const float* m = moment2 + 3ull * i;
    float dr = m[0] - s[0] * s[0], dg = m[1] - s[1] * s[1], db = m[2] - s[2] * s[2];
    dr = dr > 0.0f ? dr : 0.0f;
    dg = dg > 0.0f ? dg : 0.0f;
    db = db > 0.0f ? db : 0.0f;
    variance[i] = ((dr + dg) + db) * inv_nm1;
}

hipError_t launch_variance(const float* d_accum, const float* d_moment2, uint32_t npixels, uint32_t samples_per_pixel, float* d_variance, hipStream_t stream) {
    if (npixels == 0u) return hipSuccess;
    const uint32_t known = samples_per_pixel > 1u ? 1u : 0u;
    const float inv_nm1 = known ? 1.0f / (float)(samples_per_pixel - 1u) : 0.0f;
    hipLaunchKernelGGL(variance_kernel, dim3((npixels + 255u) / 256u), dim3(256), 0, stream, d_accum, d_moment2, npixels, inv_nm1, known, d_variance);
    return hipGetLastError();
}

// Samples per pixel per tracing / fold launch pair: as many as keep the radiance buffer within `radiance_gb` GiB (default 16; 16..256 spp).
// Sized for 288 GB of HBM: a launch is a persistent grid that drains a batch queue, and its tail - the last waves finishing their longest
// paths while the rest of the chip idles - is paid once per launch; the Cornell bench frame went from four 64-spp launches per 256-spp
// step (4 GB) to one (+1.2 %), random-spheres 1080p from two to one (+2.6 %; profiles/r03_radiance_budget_sweep.txt).
// Pixels of the 8x8 tiles that cover the image: the radiance buffer holds a record per tile lane (tile-major layout, stream_fold_kernel).
static unsigned long long padded_pixels(uint32_t width, uint32_t rows) { return 64ull * ((width + 7u) / 8u) * ((rows + 7u) / 8u); }

uint32_t streamed_chunk_spp(uint32_t width, uint32_t rows, uint32_t radiance_gb) {
    const unsigned long long px = padded_pixels(width, rows);
    const unsigned long long budget = (unsigned long long)(radiance_gb >= 1u && radiance_gb <= 64u ? radiance_gb : 16u) << 30;
    const unsigned long long fit = px ? budget / (px * 12ull) : 256ull;
    uint32_t c = 16;
    while (c < 256u && 2ull * c <= fit) c *= 2u;                                  // power of two in 16..256
    while (c > 1u && px * c >= (1ull << 32)) c /= 2u;                             // radiance slots are indexed with 32 bits
    return c;
}
// Device scratch of one render: [batch counter, 256 bytes] [radiance records: 12 bytes per pixel and sample of a launch].  A render of fewer
// samples than a full launch holds takes only what it needs.
constexpr size_t kWorkspaceHeader = 256;
size_t streamed_workspace_bytes(uint32_t width, uint32_t rows, uint32_t samples, uint32_t radiance_gb) {
    const uint32_t chunk = streamed_chunk_spp(width, rows, radiance_gb);
    return kWorkspaceHeader + (size_t)padded_pixels(width, rows) * (samples < chunk ? (samples ? samples : 1u) : chunk) * 3 * sizeof(float);
}
// ... and the other way round: the samples per pixel a granted workspace holds (at most 256, and few enough for 32-bit record indices).
// A render that was granted less than it asked for (device memory short: capi.hip halves the request) runs more, shorter launches.
uint32_t streamed_chunk_that_fits(uint32_t width, uint32_t rows, size_t bytes) {
    const unsigned long long px = padded_pixels(width, rows);
    if (px == 0 || bytes <= kWorkspaceHeader) return 0;
    unsigned long long c = (bytes - kWorkspaceHeader) / (px * 12ull);
    if (c > 256ull) c = 256ull;
    while (c > 1ull && px * c >= (1ull << 32)) c--;
    return (uint32_t)c;
}

namespace {

// The kernels' addresses, row for row the shapes of stream_plan.h kStreamKernels: the same two lists, expanded into the instantiations.
// Every instantiation has the same parameter list, so a launch is hipLaunchKernel(fn, ...) with one argument array whichever row is chosen.
#define TRT_FN_POOL(MODE, STATS, MINW, THREADS, WALK, LAZY) reinterpret_cast<const void*>(&stream_pool_kernel<MODE, STATS, MINW, THREADS, WALK, LAZY>),
#define TRT_FN_SAMPLE(MODE, STATS, MINW, THREADS, WALK, LAZY) reinterpret_cast<const void*>(&stream_sample_kernel<MODE, STATS, MINW, THREADS, WALK, LAZY>),
#define TRT_FN_DUAL(MINW) reinterpret_cast<const void*>(&stream_dual_kernel<MINW, 256>),
const void* const kStreamKernelFns[] = {
    TRT_STREAM_SPECIALISED(TRT_FN_POOL, TRT_FN_SAMPLE, TRT_FN_DUAL)
    TRT_STREAM_GENERAL(TRT_FN_POOL, TRT_FN_SAMPLE, TRT_FN_DUAL)
};
#undef TRT_FN_POOL
#undef TRT_FN_SAMPLE
#undef TRT_FN_DUAL
static_assert(sizeof(kStreamKernelFns) / sizeof(kStreamKernelFns[0]) == kStreamKernelCount, "one address per shape row");

// ---- the scene's own kernel (flat_literal.h, literal_kernel.h) ----
// Compilations started (each scene and device: at most one), and why the last one that failed did: a diagnostic, never an error of a
// render - the scene then runs the kernel built ahead of time, which computes the same frame.
std::mutex g_literal_mu;
unsigned long long g_literal_compilations = 0;
std::string g_literal_diagnostic;
uint32_t g_literal_facts_word = 0;          // SceneFacts::word() of the unit compiled and loaded last (trt_flat_literal_facts)
thread_local std::string t_literal_diagnostic_copy;

void literal_unload(void* module) {
    (void)hipModuleUnload(static_cast<hipModule_t>(module));
    (void)hipGetLastError();
}

// Compiles and loads `slot`'s kernel for the current device (called by the one thread that moved the slot to COMPILING).
bool literal_build(LiteralKernel& slot, const LiteralRequest& rq, const FlatReuse& reuse, int minw, std::string& why) {
    {
        std::lock_guard<std::mutex> lock(g_literal_mu);
        g_literal_compilations++;
    }
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) { (void)hipGetLastError(); why = "no device properties"; return false; }
    std::string arch(prop.gcnArchName);
    arch = arch.substr(0, arch.find(':'));                                          // "gfx950:sramecc+:xnack-" -> "gfx950"
    const uint32_t masks[3] = {reuse.x, reuse.y, reuse.z};
    std::string text, source;
    const SceneFacts unit_facts = rq.empty_source ? SceneFacts{} : rq.facts;       // what the source below is written with, and nothing else
    if (!rq.empty_source) {
        FlatCacheStats cache;
        if (!flat_literal_cached_asm(rq.leaf_list, rq.n_leaves, masks, rq.interval_pairs, rq.plane_regs, text, cache)) { why = "leaf list refused"; return false; }
        source = flat_literal_source(text, cache.extra_operands, unit_facts);
    }
    FlatLiteralBuild built;
    if (!flat_literal_compile(source, minw, arch.c_str(), reinterpret_cast<const void*>(&hipModuleLoadData), built)) { why = "hiprtc: " + built.log; return false; }
    hipModule_t mod = nullptr;
    hipFunction_t fn = nullptr;
    hipError_t e = hipModuleLoadData(&mod, built.code.data());
    if (e == hipSuccess) e = hipModuleGetFunction(&fn, mod, built.kernel.c_str());
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (mod) (void)hipModuleUnload(mod);
        why = std::string("module load: ") + hipGetErrorString(e);
        return false;
    }
    slot.module = mod; slot.function = fn; slot.minw = minw; slot.facts = unit_facts; slot.unload = &literal_unload;
    {
        std::lock_guard<std::mutex> lock(g_literal_mu);
        g_literal_facts_word = unit_facts.word();
    }
    return true;
}

// The kernel of this render's scene for the plan `pl`, or null: the kernel built ahead of time runs.  Only the production launch takes it -
// no counters, the lock-step walk on an LDS scene, the plan's own specialised pool instantiation, dynamic LDS within the default limit.
hipFunction_t literal_kernel_for(const StreamLaunchPlan& pl, const RenderArgs& ra, bool stats) {
    const LiteralRequest* rq = t_literal_request;
#ifdef TRT_PHASE_CLOCK
    return nullptr;                          // the diagnostic build measures the kernels built with its clock
#endif
    if (!kAsmBoxLoop) return nullptr;        // the C++-loops build (TRT_ASM_BOX_LOOP=0) exists to run the C++ loops
    if (!rq || !rq->slot || stats || !pl.specialised || !pl.pool || pl.dual || pl.walk != WALK_FLAT || pl.mode != MODE_LDS || ra.ref_tree ||
        pl.kernel_walk != WALK_FLAT || pl.threads != 256 || pl.lds_bytes > 48u * 1024u || rq->n_leaves > kFlatLiteralMaxLeaves) return nullptr;
    LiteralKernel& slot = *rq->slot;
    std::unique_lock<std::mutex> lock(slot.mu);
    while (slot.state == LiteralKernel::COMPILING) slot.cv.wait(lock);
    if (slot.state == LiteralKernel::UNTRIED && rq->wanted) {
        slot.state = LiteralKernel::COMPILING;
        lock.unlock();
        std::string why;
        const bool ok = literal_build(slot, *rq, ra.flat_reuse, pl.kernel_minw, why);
        if (!ok) {
            std::lock_guard<std::mutex> g(g_literal_mu);
            g_literal_diagnostic = "lock-step kernel not compiled for its scene, the built-in kernel runs: " + why;
        }
        lock.lock();
        slot.state = ok ? LiteralKernel::READY : LiteralKernel::FAILED;
        slot.cv.notify_all();
    }
    if (slot.state != LiteralKernel::READY || slot.minw != pl.kernel_minw || slot.facts != rq->facts) return nullptr;
    return static_cast<hipFunction_t>(slot.function);
}

}  // namespace

// d_moment2 == nullptr: the frame only.
static hipError_t launch_streamed_folds(const SceneDev& sc, const CameraDev& cam, const RenderArgs& ra_all, const trt_tuning& tn, void* workspace, size_t workspace_bytes,
                                        float* d_accum, float* d_moment2, unsigned long long* d_counters, bool stats, hipStream_t stream) {
    if (ra_all.rows_local == 0 || cam.width == 0) return hipSuccess;
    uint32_t* batch_counter = static_cast<uint32_t*>(workspace);                                     // layout: streamed_workspace_bytes
    float* colors = reinterpret_cast<float*>(static_cast<char*>(workspace) + kWorkspaceHeader);
    const uint32_t samples_all = ra_all.sample_end - ra_all.sample_begin;
    uint32_t chunk_full = streamed_chunk_spp(cam.width, ra_all.rows_local, tn.radiance_gb);
    const uint32_t granted = streamed_chunk_that_fits(cam.width, ra_all.rows_local, workspace_bytes);      // the scratch in hand decides, not the wish
    if (granted == 0u) return hipErrorInvalidValue;
    if (chunk_full > granted) chunk_full = granted;
    const uint32_t chunk = samples_all < chunk_full ? (samples_all ? samples_all : 1u) : chunk_full;
    uint32_t tiles_x = (cam.width + 7u) / 8u;
    const uint32_t tiles_y = (ra_all.rows_local + 7u) / 8u;
    uint32_t n_tiles = tiles_x * tiles_y;
    int dev = 0, cus = 256;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    const StreamLaunchPlan pl = streamed_launch_plan(sc.L, ra_all, tn, stats);
    if (pl.kernel_index < 0 || (size_t)pl.kernel_index >= kStreamKernelCount) return hipErrorInvalidDeviceFunction;      // no instantiation for this plan: a bug, never a fallback
    const void* const kernel = kStreamKernelFns[pl.kernel_index];
    // the same instantiation compiled for this scene, if the scene has one or is due one now (module API; the same arguments)
    const hipFunction_t literal = literal_kernel_for(pl, ra_all, stats);
    // the kernel's assumptions about its dynamic LDS, checked where the launch is made (scene copy | leaf stack | ray pool)
    const LdsLayout lds = plan_lds_layout(pl);
    if (lds.total() != pl.lds_bytes || !lds.fits(1u) || pl.kernel_threads != pl.threads || (pl.pool && !pl.lds_stack) ||
        (pl.flat && pl.slots < 2u) || (pl.kernel_pool != pl.pool)) return hipErrorInvalidConfiguration;
    SceneDev scd = sc;
    CameraDev camd = cam;
    const float4* leaf_list = (pl.flat || pl.compact) ? sc.blob + sc.L.off_leaf_list : nullptr;
    const uint4* nodes16 = pl.compact ? reinterpret_cast<const uint4*>(sc.blob + sc.L.off_compact) : nullptr;
    const int walk_of_plan = pl.walk;
    const uint32_t resident = (uint32_t)cus * pl.wg_per_cu;
    const uint32_t waves_per_wg = (uint32_t)pl.threads / 64u;
    if (pl.lds_bytes > 48u * 1024u) {
        e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds_bytes);
        if (e != hipSuccess) return e;
    }
    bool first = true;
    for (uint32_t s0 = ra_all.sample_begin; s0 < ra_all.sample_end; s0 += chunk) {
        RenderArgs ra = ra_all;
        ra.lds_leaf_stack = pl.lds_stack ? 1u : 0u;
        if (pl.lds_stack) ra.leaf_slots = pl.slots;
        if (walk_of_plan == WALK_LDS_STACK) {                                   // the LDS tree walk's own straggler threshold
            ra.stragglers = tn.lds_stragglers;
        }
        if (!pl.lds_stack || pl.slots < 2u) ra.stragglers = 0u;                 // a parked walk occupies two slots of the lane's LDS leaf stack (rt_path.h trav_park)
        ra.sample_begin = s0;
        ra.sample_end = s0 + chunk < ra_all.sample_end ? s0 + chunk : ra_all.sample_end;
        uint32_t batch_spp = tn.stream_batch_spp ? tn.stream_batch_spp : kBatchSpp;
        uint32_t n_batches = n_tiles * ((ra.sample_end - ra.sample_begin + batch_spp - 1u) / batch_spp);
        uint32_t grid_x = resident;
        const uint32_t max_useful = (n_batches + waves_per_wg - 1u) / waves_per_wg;   // one batch per wave at least
        if (grid_x > max_useful) grid_x = max_useful ? max_useful : 1u;
        e = hipMemsetAsync(batch_counter, 0, sizeof(uint32_t), stream);
        if (e != hipSuccess) return e;
        void* args[] = {&scd, &camd, &ra, &colors, &batch_counter, &d_counters, &tiles_x, &n_tiles, &n_batches, &batch_spp, &leaf_list, &nodes16};
        timing_mark(stream, true);
        if (literal) e = hipModuleLaunchKernel(literal, grid_x, 1u, 1u, (uint32_t)pl.threads, 1u, 1u, (uint32_t)pl.lds_bytes, stream, args, nullptr);
        else e = hipLaunchKernel(kernel, dim3(grid_x), dim3((uint32_t)pl.threads), args, pl.lds_bytes, stream);
        timing_mark(stream, false);
        if (e != hipSuccess) return e;
        const uint32_t fold_blocks = (n_tiles + 3u) / 4u;                           // four tiles (waves) per workgroup
        if (d_moment2 == nullptr) {
            hipLaunchKernelGGL(stream_fold_kernel, dim3(fold_blocks), dim3(256), 0, stream, colors, d_accum, cam.width, ra_all.rows_local, tiles_x, n_tiles,
                               ra.sample_end - ra.sample_begin, ra_all.inv_spp, (first && !ra_all.accumulate) ? 0u : 1u);
        } else {                                                                    // the frame and its second moments in the one pass over the records
            hipLaunchKernelGGL(stream_fold_moments_kernel, dim3(fold_blocks), dim3(256), 0, stream, colors, d_accum, d_moment2, cam.width, ra_all.rows_local,
                               tiles_x, n_tiles, ra.sample_end - ra.sample_begin, ra_all.inv_spp, (first && !ra_all.accumulate) ? 0u : 1u);
        }
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        first = false;
    }
    return hipSuccess;
}

hipError_t launch_streamed(const SceneDev& sc, const CameraDev& cam, const RenderArgs& ra, const trt_tuning& tn, void* workspace, size_t workspace_bytes,
                           float* d_accum, unsigned long long* d_counters, bool stats, hipStream_t stream) {
    return launch_streamed_folds(sc, cam, ra, tn, workspace, workspace_bytes, d_accum, nullptr, d_counters, stats, stream);
}

hipError_t launch_streamed_moments(const SceneDev& sc, const CameraDev& cam, const RenderArgs& ra, const trt_tuning& tn, void* workspace, size_t workspace_bytes,
                                   float* d_accum, float* d_moment2, unsigned long long* d_counters, bool stats, hipStream_t stream) {
    if (d_moment2 == nullptr) return hipErrorInvalidValue;
    return launch_streamed_folds(sc, cam, ra, tn, workspace, workspace_bytes, d_accum, d_moment2, d_counters, stats, stream);
}

}  // namespace trt

// ---- C ABI of the second moments (tinyrt.h).  The render entry points are trt_render / trt_render_device with one more buffer: capi.hip
// does the work (scene_query.h query_render_moments*) and is handed the launcher above. ----
extern "C" {

int trt_render_moments(trt_scene* s, const trt_camera* cam, const trt_render_params* p, float* accum, float* moment2, trt_stats* stats) {
    return trt::query_render_moments(s, cam, p, accum, moment2, stats, &trt::launch_streamed_moments);
}

int trt_render_moments_device(trt_scene* s, const trt_camera* cam, const trt_render_params* p, float* d_accum, float* d_moment2,
                              uint64_t* d_counters, void* stream) {
    return trt::query_render_moments_device(s, cam, p, d_accum, d_moment2, d_counters, static_cast<hipStream_t>(stream), &trt::launch_streamed_moments);
}

// Variance of the pixel estimate.  Device form: asynchronous on `stream`.
int trt_variance_device(const float* d_accum, const float* d_moment2, uint32_t npixels, uint32_t samples_per_pixel, float* d_variance, void* stream) {
    if (npixels && (!d_accum || !d_moment2 || !d_variance)) return trt::query_fail(TRT_ERR_INVALID_ARG, "null argument");
    if (npixels == 0u) return TRT_OK;
    const int rc = trt::query_require_device();
    if (rc != TRT_OK) return rc;
    const hipError_t e = trt::launch_variance(d_accum, d_moment2, npixels, samples_per_pixel, d_variance, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return trt::query_fail_hip(e, "variance launch");
    return TRT_OK;
}

// Diagnostics of the scenes' own kernels (literal_kernel.h; TRT_FLAT_LITERAL): how many compilations this process has started, and why the
// last one that failed did ("" if none has; the string is the calling thread's until its next call).  A failed compilation is never an
// error of a render.
uint64_t trt_flat_literal_compilations(void) {
    std::lock_guard<std::mutex> lock(trt::g_literal_mu);
    return trt::g_literal_compilations;
}
uint32_t trt_flat_literal_facts(void) {
    std::lock_guard<std::mutex> lock(trt::g_literal_mu);
    return trt::g_literal_facts_word;
}
const char* trt_flat_literal_diagnostic(void) {
    std::lock_guard<std::mutex> lock(trt::g_literal_mu);
    trt::t_literal_diagnostic_copy = trt::g_literal_diagnostic;
    return trt::t_literal_diagnostic_copy.c_str();
}

// Host form: device copies of the call's own, the same kernel, complete when the call returns.  There is no CPU path.
int trt_variance(const float* accum, const float* moment2, uint32_t npixels, uint32_t samples_per_pixel, float* variance) {
    return trt::host_form([&]() -> int {
        if (npixels && (!accum || !moment2 || !variance)) return trt::query_fail(TRT_ERR_INVALID_ARG, "null argument");
        if (npixels == 0u) return TRT_OK;
        const int rc = trt::query_require_device();
        if (rc != TRT_OK) return rc;
        const size_t frame = (size_t)npixels * 12u;
        trt::HostStage st("variance buffers");
        const size_t r_s = st.reserve(frame), r_m = st.reserve(frame), r_v = st.reserve((size_t)npixels * 4u);
        st.alloc();
        st.up(r_s, accum, frame, "hipMemcpy of the inputs");
        st.up(r_m, moment2, frame, "hipMemcpy of the inputs");
        if (st.ok()) st.run(trt::launch_variance(st.ptr<float>(r_s), st.ptr<float>(r_m), npixels, samples_per_pixel, st.ptr<float>(r_v), nullptr), "variance launch");
        st.down(variance, r_v, (size_t)npixels * 4u, "hipMemcpy of the result");
        return st.finish();
    });
}

}  // extern "C"
