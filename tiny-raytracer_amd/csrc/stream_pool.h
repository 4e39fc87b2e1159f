// stream_pool.h - stream_pool_kernel, the streamed backend's kernel for small LDS scenes and scenes in global memory, and what only it
// needs.  DEVICE CODE ONLY: streamed.hip includes it for the instantiations built ahead of time, and the unit that streamed.hip compiles at
// run time for one scene (flat_literal.h: the box phase with the scene's planes as literals) includes it from an embedded copy, so it
// names no host header and makes no host call.
#pragma once

#include "kernels.h"
#include "rt_path.h"
#include "stream_plan.h"
#include "wave_run.h"

namespace trt {

// ------------------------------------------------------------------------------------------------------------------
// Same kernel with the primary rays of a whole wave generated at once.  In the kernel above a lane keeps one primary
// ray in stock (9 VGPRs) and the generation code runs whenever some lane is out of stock: 0.45 times per bounce
// round with 30 % of the lanes busy.  Here an empty per-wave pool in LDS (64 entries x 36 bytes behind the leaf
// stack) is refilled by ALL 64 lanes - the next 64 items of the batch, off-image ones dropped, entries compacted by
// ballot rank - and lanes whose path ended take entries by rank: generation runs once per ~7 rounds with every lane
// busy, and the stock registers are gone.  Which lane traces which sample changes; every sample's radiance does not
// (RNG keyed by pixel and sample, radiance stored per sample, folded in order).  Used where the pool costs no resident
// workgroup (small LDS scene copies, scenes in global memory).
// ------------------------------------------------------------------------------------------------------------------
// The streamed kernels' argument list as the kernel-argument segment lays it out (every argument at its natural alignment, in order).
// stream_pool_kernel reads the arguments that only its refill branch needs - the camera, the band layout, the tile arithmetic: ~40 words,
// used once per ~7 rounds - from that segment INSIDE the branch instead of taking them from the by-value parameters: those are loaded at
// kernel entry and stay live in SGPRs over the whole round loop, where the walk pins s[36:51] besides, and the compiler moved the overflow
// through a VGPR's lanes (v_writelane / v_readlane, a vector instruction each) on the path every round takes.  The empty asm makes the
// pointer opaque, so the loads (scalar loads, wave-uniform) can neither be merged with the entry loads nor hoisted out of the branch.
struct StreamKernargs {
    SceneDev scd; CameraDev cam; RenderArgs ra;
    float* colors; uint32_t* batch_counter; unsigned long long* counters;
    uint32_t tiles_x, n_tiles, n_batches, batch_spp;
    const float4* leaf_list; const uint4* nodes16;
};
struct StreamTileArgs { uint32_t tiles_x, n_tiles, n_batches, batch_spp; };
template <class T>
TRT_DEV T kernarg_reload(size_t offset) {
    static_assert(sizeof(T) % 4 == 0, "whole words");
    typedef const __attribute__((address_space(4))) uint32_t* WordPtr;
    WordPtr w = (WordPtr)__builtin_amdgcn_kernarg_segment_ptr() + offset / 4;
    asm volatile("" : "+s"(w));
    uint32_t words[sizeof(T) / 4];
#pragma unroll
    for (uint32_t i = 0; i < sizeof(T) / 4; i++) words[i] = w[i];
    T v;
    __builtin_memcpy(&v, words, sizeof(T));
    return v;
}

template <int MODE, bool STATS, int MINW = 1, int THREADS = 256, int WALK = WALK_RUNTIME, bool LAZY = false>
__global__ __launch_bounds__(THREADS, MINW) void stream_pool_kernel(SceneDev scd, CameraDev cam_entry, RenderArgs ra,
                                                                           float* __restrict__ colors_entry,
                                                                           uint32_t* __restrict__ batch_counter_entry,
                                                                           unsigned long long* __restrict__ counters,
                                                                           uint32_t tiles_x_entry, uint32_t n_tiles_entry, uint32_t n_batches_entry, uint32_t batch_spp_entry,
                                                                           const float4* __restrict__ leaf_list,
                                                                           const uint4* __restrict__ nodes16) {
    stage_scene_to_lds<MODE>(scd);
    const FlatReuse flat_reuse = axis_quads_to_lds<MODE, STATS, WALK>(scd, ra.flat_reuse);      // axis-exact quads: the LDS copy's records rewritten (rt_path.h)
    const SceneAcc<MODE> sc{scd.blob, scd.L};
    const uint32_t lane = threadIdx.x & 63u;
    const V3 background = v3(ra.background[0], ra.background[1], ra.background[2]);
    char* const lds_tail = lds_behind_scene(sc);
    float2* const leaf_stack = reinterpret_cast<float2*>(lds_tail) + (threadIdx.x >> 6) * (64u * ra.leaf_slots) + lane;
    // the pool: field f of entry e at pool[f * 64 + e]; behind the leaf stack (stream_plan.h LdsLayout::stack_bytes, one stack)
    uint32_t* const pool = reinterpret_cast<uint32_t*>(lds_tail + (size_t)THREADS * ra.leaf_slots * sizeof(float2)) + (threadIdx.x >> 6) * (64u * kPoolDwords);

    uint32_t tile_x0 = 0, tile_row0 = 0, tile_slot0 = 0, ds0 = 0, items_per_batch = 0, cursor = 0;    // wave-uniform work cursor
    uint32_t pool_head = 0, pool_count = 0;                                            // wave-uniform
    bool exhausted = false;

    Path p;
    p.remain = 0u;
    bool has_path = false;
    uint32_t out_idx = 0;
    uint32_t n_samples = 0, n_rays = 0;
    Counters<STATS> ctr;
    // resumable walks (rt_path.h walk_compact, walk_fast_lds): a round's walk phase ends once only a few lanes still walk; they carry
    // their walk into the next round (100 k spheres: 324 trips per round for 222 box steps per ray, +10 %; random-spheres: see DESIGN 13)
    constexpr bool kResumable = !STATS && (WALK == WALK_COMPACT || WALK == WALK_LDS_STACK);
    bool walking = false;                                                         // this lane's walk is parked in its leaf stack (kResumable only)

    TRT_CLK_START(ctr);
    for (;;) {
        // ---- lanes without a path take pool entries; an empty pool is refilled by the whole wave ----
        for (;;) {
            const uint64_t need = __builtin_amdgcn_ballot_w64(!has_path);
            if (need == 0ull) break;
            if (pool_count == 0u) {
                if (exhausted) break;
                // refill-only arguments, read here and not carried through the rounds (kernarg_reload above)
                const CameraDev cam = kernarg_reload<CameraDev>(offsetof(StreamKernargs, cam));
                const RenderArgs rr = kernarg_reload<RenderArgs>(offsetof(StreamKernargs, ra));
                const StreamTileArgs ta = kernarg_reload<StreamTileArgs>(offsetof(StreamKernargs, tiles_x));
                const uint32_t n_spp = rr.sample_end - rr.sample_begin;
                if (cursor >= items_per_batch) {
                    uint32_t* const batch_counter = kernarg_reload<uint32_t*>(offsetof(StreamKernargs, batch_counter));
                    const uint32_t tiles_x = ta.tiles_x, n_tiles = ta.n_tiles, n_batches = ta.n_batches, batch_spp = ta.batch_spp;
                    uint32_t b = 0;
                    if (lane == 0u) b = atomicAdd(batch_counter, 1u);
                    b = __builtin_amdgcn_readfirstlane(b);
                    if (b >= n_batches) { exhausted = true; break; }
                    const uint32_t tile = b % n_tiles;                                    // consecutive batches: neighbouring tiles, same samples
                    ds0 = (b / n_tiles) * batch_spp;
                    tile_x0 = (tile % tiles_x) * 8u;
                    tile_row0 = (tile / tiles_x) * 8u;
                    tile_slot0 = tile * n_spp * 64u;
                    items_per_batch = 64u * (n_spp - ds0 < batch_spp ? n_spp - ds0 : batch_spp);
                    cursor = 0;
                }
                // the next 64 items: one 8x8 tile at one sample index
                const uint32_t item = cursor + lane;
                cursor += 64u;
                const uint32_t ds = ds0 + (item >> 6);
                const uint32_t x = tile_x0 + (lane & 7u), row = tile_row0 + (lane >> 3);
                const bool valid = x < cam.width && row < rr.rows_local;                  // off-image items of an edge tile are dropped
                const uint64_t vmask = __builtin_amdgcn_ballot_w64(valid);
                if (valid) {
                    if constexpr (STATS) { if (first_active_lane()) ctr.w_gen++; }
                    const uint32_t y = image_row(rr, row);
                    Rng rng = rng_seed(rr.seed_key, y * cam.width + x, rr.sample_begin + ds);        // cpu.rs:42-45
                    const Ray ray = primary_ray(cam, x, y, rng);
                    const uint32_t e = wave_rank(vmask);
                    pool[0u * 64u + e] = __float_as_uint(ray.o.x); pool[1u * 64u + e] = __float_as_uint(ray.o.y); pool[2u * 64u + e] = __float_as_uint(ray.o.z);
                    pool[3u * 64u + e] = __float_as_uint(ray.d.x); pool[4u * 64u + e] = __float_as_uint(ray.d.y); pool[5u * 64u + e] = __float_as_uint(ray.d.z);
                    pool[6u * 64u + e] = rng.s0; pool[7u * 64u + e] = rng.s1;
                    pool[8u * 64u + e] = tile_slot0 + ds * 64u + lane;
                }
                pool_head = 0u;
                pool_count = (uint32_t)__builtin_popcountll(vmask);
                if (pool_count == 0u) continue;                                           // a tile row entirely off the image
            }
            const uint32_t rank = wave_rank(need);
            if (!has_path && rank < pool_count) {
                const uint32_t e = pool_head + rank;
                p.ray.o = v3(__uint_as_float(pool[0u * 64u + e]), __uint_as_float(pool[1u * 64u + e]), __uint_as_float(pool[2u * 64u + e]));
                p.ray.d = v3(__uint_as_float(pool[3u * 64u + e]), __uint_as_float(pool[4u * 64u + e]), __uint_as_float(pool[5u * 64u + e]));
                p.rng.s0 = pool[6u * 64u + e]; p.rng.s1 = pool[7u * 64u + e];
                out_idx = pool[8u * 64u + e];
                p.color = v3(0.0f, 0.0f, 0.0f);
                p.atten = v3(1.0f, 1.0f, 1.0f);
                p.remain = ra.max_bounces;
                has_path = true;
                n_samples++;
            }
            const uint32_t wanted = (uint32_t)__builtin_popcountll(need);
            const uint32_t taken = wanted < pool_count ? wanted : pool_count;
            pool_head += taken;
            pool_count -= taken;
        }
        if (__builtin_amdgcn_ballot_w64(has_path) == 0ull) break;                         // nothing left to trace: the batches are used up
        TRT_CLK(ctr, 0);
        if (has_path) {
            if constexpr (STATS) { if (first_active_lane()) ctr.w_rounds++; }
            if constexpr (kResumable) {
                Trav tr = trav_begin<MODE, WALK == WALK_COMPACT>(sc, p.ray, false);                              // see stream_sample_kernel
                if (walking) trav_unpark(leaf_stack, tr); else n_rays++;
                const uint32_t entered = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(true));
                walking = !closest_hit_resume<MODE, STATS, WALK>(sc, p.ray, tr, ctr, ra.leaf_slots, leaf_stack, leaf_list, nodes16, ra.stragglers, entered);
                if (!walking) {
                    if (shade_hit<MODE, STATS, LAZY>(sc, p, tr.prim_best, tr.t_best, background, ctr)) {
                        radiance_store(kernarg_reload<float*>(offsetof(StreamKernargs, colors)), out_idx, p.color);       // the pointer: as the refill arguments
                        has_path = false;
                    }
                }
            } else {
                n_rays++;
                float t;
                const uint32_t prim = closest_hit<MODE, STATS, WALK>(sc, p.ray, STATS && ra.ref_tree != 0u, t, ctr, ra.leaf_slots, leaf_stack, leaf_list, nodes16, flat_reuse);
                bool ended;
                // (the unit compiled for a scene of Lambertian and light quads: one straight-line body, the path updated in place - rt_path.h)
                if constexpr (kFactStraightShade && !STATS && LAZY) ended = shade_straight<MODE>(sc, p, prim, t, background);
                else ended = shade_hit<MODE, STATS, LAZY>(sc, p, prim, t, background, ctr);
                if (ended) {
                    radiance_store(kernarg_reload<float*>(offsetof(StreamKernargs, colors)), out_idx, p.color);       // the pointer: as the refill arguments
                    has_path = false;
                }
            }
        }
        TRT_CLK(ctr, 3);
    }
    flush_counters<STATS>(counters, n_samples, n_rays, ctr);
}

}  // namespace trt
