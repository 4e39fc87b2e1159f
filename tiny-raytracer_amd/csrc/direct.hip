// direct.hip — direct-light queries: the light that reaches a caller-supplied surfel straight from the emitters of a caller-supplied table,
// by shadow rays the device draws (tinyrt.h trt_direct / trt_direct_device), written for gfx950 (CDNA4) only.
//
// The gather queries (radiance.hip) find the lights by chance; these aim at them.  For item i and sample s the draw is gather_draw.h
// direct_draw on RNG stream (seed, first_stream + i * K + s, 1): an emitter of the table, a point y on it, the weight of the sample and the
// normalised ray from the surfel towards y.  The sample is what trt_occluded answers for that ray with t_max = |y - x| * shadow_end:
// BVH::hit over [0.001, t_max), any material.  There is no path and stream (.., 0) is not touched.  A live, unoccluded sample adds
//   radiance.ch = radiance.ch + c.ch * inv_K;   moment2.ch = moment2.ch + (c.ch * c.ch) * inv_K        (c = colour * weight)
// every other sample nothing; in sample order, one IEEE f32 operation per operator, in registers: a lane owns an item for all samples of
// the call, keeps the six sums and writes once per item.
//
// There is no walk code in this file: the kernel is ambient_kernel's two forms (ambient.hip) with a per-lane t_max and a per-lane "walk
// this sample" - a dead sample (facing away, on the point, a weight that is no number) and one whose range [0.001, t_max) is empty stay in
// the wave's rounds and walk nothing.  The dynamic LDS is laid out as the queries lay it out (wave_run.h) and the launch rule is the
// queries' (query_plan.h): a wave owns a contiguous run of the items.
//
// trt_direct_mis / trt_direct_mis_device (tinyrt.h) are a kernel of their own, direct_mis_kernel, in the same six shapes and both forms:
// the shadow sample scaled by wl = 1 / (1 + q(wgt)) (1 for a virtual emitter) and, on stream (seed, j, 0xFFFFFFFF), the gather's cosine
// ray from the surfel, whose hit on a light adds emission * wb (mis_weight.h mis_hit_weight, shared with nee.hip).  Up to two walks per
// sample go through ONE walk call site, nee_kernel's way.  direct_kernel is instruction for instruction what it was; the
// queries' host side - checks, both forms' bodies - is emitter_query.h's, shared with nee.hip.
#include "emitter_pick.h"
#include "emitter_query.h"
#include "gather_draw.h"
#include "host_stage.h"
#include "kernels.h"
#include "mis_weight.h"
#include "query_plan.h"
#include "rt_path.h"
#include "scene_query.h"
#include "wave_run.h"

namespace trt {

static_assert(sizeof(trt_emitter) == 80 && offsetof(trt_emitter, a) == 8 && offsetof(trt_emitter, normal) == 44 && offsetof(trt_emitter, color) == 56 &&
              offsetof(trt_emitter, area) == 68 && offsetof(trt_emitter, reserved) == 72, "trt_emitter layout (tinyrt.h; gather_draw.h direct_draw)");
static_assert(sizeof(trt_direct_params) == 96 && offsetof(trt_direct_params, shadow_end) == 64 && offsetof(trt_direct_params, reserved) == 68,
              "trt_direct_params layout (tinyrt.h)");

struct DirectArgs {
    const float* items;              // n x (point, axis), used as given
    const float* emitters;           // n_emitters x 20 words (trt_emitter)
    float* radiance;                 // n x 3
    float* moment2;                  // n x 3, or nullptr: not wanted
    unsigned long long* counters;    // nullptr, or [CTR_SAMPLES], [CTR_RAYS] are added to
    uint32_t n, rays_per_wave;       // wave w owns items [w * rays_per_wave, ...)
    uint32_t slots, stragglers;      // as in query.hip QueryArgs
    uint32_t samples_per_item;       // K
    uint32_t first_stream;           // first_stream + n * K <= 2^32 (radiance_check): the stream index never wraps
    uint32_t seed_key;               // kernels.h rng_seed_key
    uint32_t sample_begin, sample_end;      // begin < end (launch_direct: an empty range launches query_plan.h batch_zero or nothing)
    uint32_t accumulate;
    uint32_t n_emitters;             // E: 1 .. 2^20
    float inv_k;                     // 1.0f / float(K)
    float shadow_end;                // in (0, 1]
    FlatReuse flat_reuse;
};

// What a PICK kernel is handed besides: the alias table (tinyrt.h trt_emitter_pick, n_emitters x 4 words).  A struct of its own around
// DirectArgs, so that the kernel arguments of the uniform kernels lie where they lay.
struct DirectPickArgs {
    DirectArgs d;
    const float* pick;
};
TRT_DEV const DirectArgs& direct_args(const DirectArgs& a) { return a; }
TRT_DEV const DirectArgs& direct_args(const DirectPickArgs& a) { return a.d; }
TRT_DEV const float* pick_table(const DirectArgs&) { return nullptr; }
TRT_DEV const float* pick_table(const DirectPickArgs& a) { return a.pick; }

// The six sums of one item: read where a call continues them, written once when the item's last sample has folded.
struct DirectSums {
    V3 rad, m2;
};
TRT_DEV DirectSums dir_begin(const DirectArgs& da, uint32_t idx) {
    DirectSums a;
    a.rad = v3(0.0f, 0.0f, 0.0f);
    a.m2 = v3(0.0f, 0.0f, 0.0f);
    if (da.accumulate) {
        const float* const r = da.radiance + 3ull * idx;
        a.rad = v3(r[0], r[1], r[2]);
        if (da.moment2) { const float* const m = da.moment2 + 3ull * idx; a.m2 = v3(m[0], m[1], m[2]); }
    }
    return a;
}
TRT_DEV void dir_store(const DirectArgs& da, uint32_t idx, const DirectSums& a) {
    float* const r = da.radiance + 3ull * idx;
    r[0] = a.rad.x; r[1] = a.rad.y; r[2] = a.rad.z;
    if (da.moment2) { float* const m = da.moment2 + 3ull * idx; m[0] = a.m2.x; m[1] = a.m2.y; m[2] = a.m2.z; }
}
// The fold of one live, unoccluded sample (tinyrt.h); every other sample folds nothing.
TRT_DEV void dir_fold(DirectSums& a, const V3& c, float inv_k) {
    a.rad = a.rad + c * inv_k;
    a.m2 = a.m2 + (c * c) * inv_k;
}

// PICK: the emitter of a sample is chosen through the alias table (trt_direct_pick; gather_draw.h AliasPick), one draw and two loads more.
template <int MODE, int WALK, int THREADS, int MINW, bool PICK = false>
__global__ __launch_bounds__(THREADS, MINW) void direct_kernel(SceneDev scd, std::conditional_t<PICK, DirectPickArgs, DirectArgs> args,
                                                                    const float4* __restrict__ leaf_list, const uint4* __restrict__ nodes16) {
    const DirectArgs& da = direct_args(args);
    const float* __restrict__ const pick = pick_table(args);
    stage_scene_to_lds<MODE>(scd);
    const FlatReuse flat_reuse = axis_quads_to_lds<MODE, false, WALK>(scd, da.flat_reuse);
    const SceneAcc<MODE> sc{scd.blob, scd.L};
    const float* __restrict__ const items = da.items;
    const float* __restrict__ const emitters = da.emitters;
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long begin64 = wave_begin<THREADS>(da.rays_per_wave);
    if (begin64 >= da.n) return;                                            // (after the barriers above)
    const uint32_t begin = (uint32_t)begin64;
    const uint32_t count = wave_count(da.n, da.rays_per_wave, begin);
    // this lane's postponed-leaf stack: behind the scene copy, slots x 64 x 8 bytes per wave
    float2* const stack = WALK != WALK_REGS ? reinterpret_cast<float2*>(lds_behind_scene(sc)) + (threadIdx.x >> 6) * (64u * da.slots) + lane : nullptr;
    Counters<false> ctr;
    constexpr bool kResumable = WALK == WALK_COMPACT || WALK == WALK_LDS_STACK;
    uint32_t n_samples = 0, n_rays = 0;

    if constexpr (kResumable) {
        uint32_t cursor = 0;                                                // wave-uniform
        bool own = false, has_ray = false, walking = false;                 // the lane owns an item; a sample is drawn; its walk is parked
        bool live = false, walks = false;                                   // of the drawn sample: it can fold; it asks the scene
        uint32_t idx = 0, s = 0;
        DirectSums acc;
        acc.rad = v3(0.0f, 0.0f, 0.0f); acc.m2 = v3(0.0f, 0.0f, 0.0f);
        Ray ray;
        ray.o = v3(0.0f, 0.0f, 0.0f); ray.d = v3(0.0f, 0.0f, 0.0f);
        V3 c = v3(0.0f, 0.0f, 0.0f);
        float t_max = 0.0f;
        for (;;) {
            // ---- refill: every lane without an item takes the next one of the run (begin + item < n: item < count <= n - begin) ----
            const uint64_t need = __builtin_amdgcn_ballot_w64(!own);
            if (need != 0ull && cursor < count) {
                const uint32_t item = cursor + wave_rank(need);
                if (!own && item < count) {
                    idx = begin + item;
                    s = da.sample_begin;
                    acc = dir_begin(da, idx);
                    own = true;
                }
                cursor = wave_advance(cursor, need, count);
            }
            if (__builtin_amdgcn_ballot_w64(own) == 0ull) break;            // every lane is free and none could take an item: the run is done
            if (own) {
                // ---- start: the item's next sample draws its emitter point and shadow ray (stream (seed, j, 1)) ----
                if (!has_ray) {
                    Rng g = rng_seed(da.seed_key, da.first_stream + idx * da.samples_per_item + s, 1u);
                    const DirectSample smp = direct_draw_item<PICK, DirectSample>(items, idx, emitters, pick, da.n_emitters, da.shadow_end, g);
                    ray = smp.ray; c = smp.c; t_max = smp.t_max; live = smp.live;
                    walks = live && t_max > kTMin;                          // else dead, or an empty range: nothing is walked
                    has_ray = true;
                    n_samples++;
                }
                // ---- walk; a finished walk folds at once ----
                bool occluded = false;
                if (walks) {
                    Trav tr = trav_begin<MODE, WALK == WALK_COMPACT>(sc, ray, false);      // a new walk, or the frame of a parked one
                    if (walking) trav_unpark(stack, tr); else { tr.t_best = t_max; n_rays++; }
                    const uint32_t entered = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(true));
                    walking = !closest_hit_resume<MODE, false, WALK, true>(sc, ray, tr, ctr, da.slots, stack, leaf_list, nodes16, da.stragglers, entered);
                    occluded = tr.prim_best != PRIM_NONE;
                }
                if (!walking) {
                    if (live && !occluded) dir_fold(acc, c, da.inv_k);
                    has_ray = false;
                    s += 1u;
                    if (s == da.sample_end) {
                        dir_store(da, idx, acc);
                        own = false;
                    }
                }
            }
        }
    } else {
        for (uint32_t base = 0; base < count; base += 64u) {
            if (base + lane < count) {
                const uint32_t idx = begin + base + lane;
                DirectSums acc = dir_begin(da, idx);
                for (uint32_t s = da.sample_begin; s != da.sample_end; s++) {
                    Rng g = rng_seed(da.seed_key, da.first_stream + idx * da.samples_per_item + s, 1u);
                    const DirectSample smp = direct_draw_item<PICK, DirectSample>(items, idx, emitters, pick, da.n_emitters, da.shadow_end, g);
                    n_samples++;
                    uint32_t prim = PRIM_NONE;
                    if (smp.live && smp.t_max > kTMin) {
                        float t = 0.0f;
                        n_rays++;
                        prim = closest_hit<MODE, false, WALK, true>(sc, smp.ray, false, t, ctr, da.slots, stack, leaf_list, nodes16, flat_reuse, smp.t_max);
                    }
                    if (smp.live && prim == PRIM_NONE) dir_fold(acc, smp.c, da.inv_k);
                }
                dir_store(da, idx, acc);
            }
        }
    }
    flush_counters<false>(da.counters, n_samples, n_rays, ctr);
}

// ---- trt_direct_mis: the shadow sample AND a cosine-lobe ray from the surfel, weighted by their densities (tinyrt.h) ----
static_assert(sizeof(trt_direct_mis_params) == 128 && offsetof(trt_direct_mis_params, direct) == 0 && offsetof(trt_direct_mis_params, heuristic) == 96 &&
              offsetof(trt_direct_mis_params, reserved) == 100, "trt_direct_mis_params layout (tinyrt.h)");

struct DirectMisArgs {
    DirectArgs d;                    // direct_kernel's, read the same way
    uint32_t heuristic;              // enum trt_mis_heuristic, wave-uniform
};
// ... of a PICK kernel: the alias table and the table's total power, by which a light hit finds its own choice probability.
struct DirectMisPickArgs {
    DirectMisArgs m;
    const float* pick;
    float total_power;
};
TRT_DEV const DirectMisArgs& direct_mis_args(const DirectMisArgs& a) { return a; }
TRT_DEV const DirectMisArgs& direct_mis_args(const DirectMisPickArgs& a) { return a.m; }
TRT_DEV const float* pick_table(const DirectMisArgs&) { return nullptr; }
TRT_DEV const float* pick_table(const DirectMisPickArgs& a) { return a.pick; }
TRT_DEV float pick_total(const DirectMisArgs&) { return 0.0f; }
TRT_DEV float pick_total(const DirectMisPickArgs& a) { return a.total_power; }

// The shadow sample's share of a drawn sample: 1 / (1 + q(p_bsdf / p_light)); a virtual emitter cannot be hit and counts in full.
TRT_DEV float mis_shadow_weight(const WeightedDirectSample& w, uint32_t heuristic) {
    const float qw = heuristic == TRT_MIS_POWER ? w.wgt * w.wgt : w.wgt;
    return w.geometry != 0xFFFFFFFFu ? 1.0f / (1.0f + qw) : 1.0f;
}
// What the lobe ray of a sample adds, T_b: nothing (false) on a miss or a hit on anything but a light, else emission * wb with csh from the
// item's axis as given (re-read: three registers less per lane while the walks run; a light hit is the rare case).
// PICK: the light's choice probability is its share of total_power (mis_weight.h, the overload), not 1 / E.
template <int MODE, bool PICK>
TRT_DEV bool mis_lobe_term(const SceneAcc<MODE>& sc, const float* __restrict__ items, uint32_t idx, const Ray& ray, uint32_t prim, float t,
                           uint32_t n_emitters, float total_power, uint32_t heuristic, V3& tb) {
    if (prim == PRIM_NONE) return false;
    const uint32_t mat = prim_material<MODE>(sc, prim);
    if (sc.material_kind(mat) != TRT_LIGHT) return false;
    const float* const it = items + 6ull * idx;
    const float csh = dot(v3(it[3], it[4], it[5]), ray.d);
    const V3 normal = hit_unit_normal<MODE>(sc, prim, ray, t);
    if constexpr (PICK) {
        const float4 m = sc.material(mat);
        const V3 emission = v3(m.x, m.y, m.z);
        tb = emission * mis_hit_weight<MODE>(sc, prim, ray, normal, t, csh, emission, total_power, heuristic);
    } else {
        const float wb = mis_hit_weight<MODE>(sc, prim, ray, normal, t, csh, n_emitters, heuristic);
        const float4 m = sc.material(mat);
        tb = v3(m.x, m.y, m.z) * wb;
    }
    return true;
}

// direct_kernel's two forms with up to two walks per sample through ONE walk call site, as nee_kernel has it: a closest-hit walk whose
// first t_best is the shadow ray's t_max ("anything in [0.001, t_max)" is prim_best != PRIM_NONE then) or +inf for the lobe ray.  The
// shadow sample is drawn on stream (seed, j, 1) exactly as direct_kernel draws it, the lobe ray on (seed, j, 0xFFFFFFFF) once the shadow
// walk is over: a lane keeps one ray.  `c` holds T_l while `lit` says it counts; the lobe ray's term joins it or stands alone.
constexpr uint32_t kLobeStreamWord = 0xFFFFFFFFu;
template <int MODE, int WALK, int THREADS, int MINW, bool PICK = false>
__global__ __launch_bounds__(THREADS, MINW) void direct_mis_kernel(SceneDev scd, std::conditional_t<PICK, DirectMisPickArgs, DirectMisArgs> args,
                                                                        const float4* __restrict__ leaf_list, const uint4* __restrict__ nodes16) {
    const DirectMisArgs& ma = direct_mis_args(args);
    const float* __restrict__ const pick = pick_table(args);
    const float total_power = pick_total(args);
    const DirectArgs& da = ma.d;
    stage_scene_to_lds<MODE>(scd);
    const FlatReuse flat_reuse = axis_quads_to_lds<MODE, false, WALK>(scd, da.flat_reuse);
    const SceneAcc<MODE> sc{scd.blob, scd.L};
    const float* __restrict__ const items = da.items;
    const float* __restrict__ const emitters = da.emitters;
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long begin64 = wave_begin<THREADS>(da.rays_per_wave);
    if (begin64 >= da.n) return;                                            // (after the barriers above)
    const uint32_t begin = (uint32_t)begin64;
    const uint32_t count = wave_count(da.n, da.rays_per_wave, begin);
    // this lane's postponed-leaf stack: behind the scene copy, slots x 64 x 8 bytes per wave
    float2* const stack = WALK != WALK_REGS ? reinterpret_cast<float2*>(lds_behind_scene(sc)) + (threadIdx.x >> 6) * (64u * da.slots) + lane : nullptr;
    Counters<false> ctr;
    constexpr bool kResumable = WALK == WALK_COMPACT || WALK == WALK_LDS_STACK;
    uint32_t n_samples = 0, n_rays = 0;

    if constexpr (kResumable) {
        constexpr uint32_t PH_START = 0u, PH_SHADOW = 1u, PH_LOBE_DRAW = 2u, PH_LOBE = 3u;
        uint32_t cursor = 0;                                                // wave-uniform
        bool own = false, walking = false;                                  // the lane owns an item; its walk is parked
        bool lit = false;                                                   // of the sample under way: c counts
        uint32_t phase = PH_START;                                          // draw the shadow sample | its walk | draw the lobe ray | its walk
        uint32_t idx = 0, s = 0;
        DirectSums acc;
        acc.rad = v3(0.0f, 0.0f, 0.0f); acc.m2 = v3(0.0f, 0.0f, 0.0f);
        Ray ray;
        ray.o = v3(0.0f, 0.0f, 0.0f); ray.d = v3(0.0f, 0.0f, 0.0f);
        V3 c = v3(0.0f, 0.0f, 0.0f);
        float t_first = 0.0f;
        for (;;) {
            // ---- refill: every lane without an item takes the next one of the run (begin + item < n: item < count <= n - begin) ----
            const uint64_t need = __builtin_amdgcn_ballot_w64(!own);
            if (need != 0ull && cursor < count) {
                const uint32_t item = cursor + wave_rank(need);
                if (!own && item < count) {
                    idx = begin + item;
                    s = da.sample_begin;
                    acc = dir_begin(da, idx);
                    phase = PH_START;
                    own = true;
                }
                cursor = wave_advance(cursor, need, count);
            }
            if (__builtin_amdgcn_ballot_w64(own) == 0ull) break;            // every lane is free and none could take an item: the run is done
            if (own) {
                const uint32_t stream = da.first_stream + idx * da.samples_per_item + s;
                // ---- start: the item's next sample draws its emitter point and shadow ray (stream (seed, j, 1)) ----
                if (phase == PH_START) {
                    Rng g = rng_seed(da.seed_key, stream, 1u);
                    const WeightedDirectSample w = direct_draw_item<PICK, WeightedDirectSample>(items, idx, emitters, pick, da.n_emitters, da.shadow_end, g);
                    c = w.c * mis_shadow_weight(w, ma.heuristic);
                    lit = w.live;                                           // until its walk finds something
                    n_samples++;
                    phase = PH_LOBE_DRAW;                                   // dead, or an empty range: nothing is walked
                    if (w.live && w.t_max > kTMin) { ray = w.ray; t_first = w.t_max; phase = PH_SHADOW; }
                }
                // ---- the lobe ray (stream (seed, j, 0xFFFFFFFF)): trt_gather's cosine draw about the item ----
                if (phase == PH_LOBE_DRAW) {
                    Rng g = rng_seed(da.seed_key, stream, kLobeStreamWord);
                    ray = gather_ray(items, idx, TRT_LOBE_COSINE, 0.0f, g);
                    t_first = __builtin_inff();
                    phase = PH_LOBE;
                }
                // ---- walk; a finished walk is answered at once ----
                Trav tr = trav_begin<MODE, WALK == WALK_COMPACT>(sc, ray, false);          // a new walk, or the frame of a parked one
                if (walking) trav_unpark(stack, tr); else { tr.t_best = t_first; n_rays++; }
                const uint32_t entered = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(true));
                walking = !closest_hit_resume<MODE, false, WALK, false>(sc, ray, tr, ctr, da.slots, stack, leaf_list, nodes16, da.stragglers, entered);
                if (!walking) {
                    if (phase == PH_SHADOW) {
                        if (tr.prim_best != PRIM_NONE) lit = false;
                        phase = PH_LOBE_DRAW;                               // drawn and walked in the next round
                    } else {
                        V3 tb;
                        if (mis_lobe_term<MODE, PICK>(sc, items, idx, ray, tr.prim_best, tr.t_best, da.n_emitters, total_power, ma.heuristic, tb)) {
                            c = lit ? c + tb : tb;
                            lit = true;
                        }
                        if (lit) dir_fold(acc, c, da.inv_k);
                        phase = PH_START;
                        s += 1u;
                        if (s == da.sample_end) {
                            dir_store(da, idx, acc);
                            own = false;
                        }
                    }
                }
            }
        }
    } else {
        for (uint32_t base = 0; base < count; base += 64u) {
            if (base + lane < count) {
                const uint32_t idx = begin + base + lane;
                DirectSums acc = dir_begin(da, idx);
                for (uint32_t s = da.sample_begin; s != da.sample_end; s++) {
                    const uint32_t stream = da.first_stream + idx * da.samples_per_item + s;
                    Rng g = rng_seed(da.seed_key, stream, 1u);
                    const WeightedDirectSample w = direct_draw_item<PICK, WeightedDirectSample>(items, idx, emitters, pick, da.n_emitters, da.shadow_end, g);
                    n_samples++;
                    V3 c = w.c * mis_shadow_weight(w, ma.heuristic);
                    bool lit = w.live;
                    Ray ray = w.ray;
                    float t_first = w.t_max;
                    bool walks = w.live && w.t_max > kTMin;
                    // the shadow ray, then the lobe ray, through one walk
#pragma unroll 1
                    for (uint32_t lobe = 0; lobe < 2u; lobe++) {
                        if (lobe != 0u) {
                            Rng gl = rng_seed(da.seed_key, stream, kLobeStreamWord);
                            ray = gather_ray(items, idx, TRT_LOBE_COSINE, 0.0f, gl);
                            t_first = __builtin_inff();
                            walks = true;
                        }
                        uint32_t prim = PRIM_NONE;
                        float t = 0.0f;
                        if (walks) {
                            n_rays++;
                            prim = closest_hit<MODE, false, WALK, false>(sc, ray, false, t, ctr, da.slots, stack, leaf_list, nodes16, flat_reuse, t_first);
                        }
                        if (lobe == 0u) {
                            if (prim != PRIM_NONE) lit = false;
                        } else {
                            V3 tb;
                            if (mis_lobe_term<MODE, PICK>(sc, items, idx, ray, prim, t, da.n_emitters, total_power, ma.heuristic, tb)) {
                                c = lit ? c + tb : tb;
                                lit = true;
                            }
                        }
                    }
                    if (lit) dir_fold(acc, c, da.inv_k);
                }
                dir_store(da, idx, acc);
            }
        }
    }
    flush_counters<false>(da.counters, n_samples, n_rays, ctr);
}

namespace {

// The (scene mode, walk, workgroup shape) set of the other batch units, with the register-slot fallback (query_plan.h), so that every
// scene has a kernel: the six shapes, written once.  A table is one kernel template with one PICK over them; its launch bounds, one per
// shape in this order, are all that a table says of its own.  The plan reports the bound (kernel_waves_per_simd).
#define TRT_DIRECT_ROW(KERNEL, PICK, MODE, WALK, THREADS, MINW) \
    BatchKernel{reinterpret_cast<const void*>(&KERNEL<MODE, WALK, THREADS, MINW, PICK>), MODE, WALK, THREADS, MINW}
#define TRT_DIRECT_TABLE(KERNEL, PICK, LDS_FLAT, LDS_STACK_256, LDS_STACK_768, LDS_REGS, GLOBAL_COMPACT, GLOBAL_REGS)                              \
    {TRT_DIRECT_ROW(KERNEL, PICK, MODE_LDS, WALK_FLAT, 256, LDS_FLAT), TRT_DIRECT_ROW(KERNEL, PICK, MODE_LDS, WALK_LDS_STACK, 256, LDS_STACK_256), \
     TRT_DIRECT_ROW(KERNEL, PICK, MODE_LDS, WALK_LDS_STACK, 768, LDS_STACK_768), TRT_DIRECT_ROW(KERNEL, PICK, MODE_LDS, WALK_REGS, 512, LDS_REGS), \
     TRT_DIRECT_ROW(KERNEL, PICK, MODE_GLOBAL, WALK_COMPACT, 256, GLOBAL_COMPACT), TRT_DIRECT_ROW(KERNEL, PICK, MODE_GLOBAL, WALK_REGS, 256, GLOBAL_REGS)}
constexpr size_t kDirectShapes = 6;
// The kernels of a query: [pick][mis].
//  - direct_kernel: a lane carries what a lane of the ambient query carries plus the sample's colour, its t_max and two sums more: the
//    launch bounds are the highest at which the instantiation uses no scratch memory and spills no vector register
//    (profiles/direct_resource_usage.txt).
//  - direct_mis_kernel (trt_direct_mis): a lane carries a whole ray where direct_kernel's any-hit walk carries less, and the light-hit
//    weight besides: bounds by the same rule (profiles/direct_mis_resource_usage.txt).
//  - PICK (trt_direct_pick, trt_direct_mis_pick): the alias draw lives and dies ahead of the emitter record's load.  Bounds by the same
//    rule (profiles/direct_pick_resource_usage.txt).
const BatchKernel kDirectKernels[2][2][kDirectShapes] = {
    {TRT_DIRECT_TABLE(direct_kernel, false, 7, 8, 8, 7, 7, 6), TRT_DIRECT_TABLE(direct_mis_kernel, false, 5, 7, 7, 5, 7, 5)},
    {TRT_DIRECT_TABLE(direct_kernel, true, 7, 8, 8, 7, 7, 6), TRT_DIRECT_TABLE(direct_mis_kernel, true, 5, 7, 7, 5, 7, 5)},
};
#undef TRT_DIRECT_TABLE
#undef TRT_DIRECT_ROW

// What a call asks of the device, after the checks; the variant's fields are emitter_query.h's.
struct DirectCall : EmitterVariant {
    RenderArgs ra;                   // of the path parameters: seed key, 1 / K, sample range, accumulate (radiance_check)
    uint32_t samples_per_item, first_stream;
    uint32_t n_emitters;
    float shadow_end;
    bool nothing() const { return ra.sample_begin == ra.sample_end; }       // an empty sample range: no sample is drawn
};

hipError_t launch_direct(const QueryScene& qs, const DirectCall& c, const float* d_items, uint32_t n, const float* d_emitters, const float* d_pick,
                         float* d_radiance, float* d_moment2, unsigned long long* d_counters, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (c.nothing()) {
        // the sums start at 0, or stay
        if (c.ra.accumulate) return hipSuccess;
        return batch_zero(d_radiance, 3ull * n, d_moment2, 3ull * n, stream);
    }
    SceneDev scd = qs.scene;
    BatchLaunch b;
    const hipError_t e = batch_prepare(scd, n, kDirectKernels[c.pick][c.mis], kDirectShapes, b);
    if (e != hipSuccess) return e;
    const trt_query_plan& q = b.q;
    DirectArgs da{d_items, d_emitters, d_radiance, d_moment2, d_counters, n, q.rays_per_wave, q.leaf_slots, q.stragglers, c.samples_per_item,
                  c.first_stream, c.ra.seed_key, c.ra.sample_begin, c.ra.sample_end, c.ra.accumulate, c.n_emitters, c.ra.inv_spp, c.shadow_end,
                  qs.flat_reuse};
    DirectMisArgs ma{da, c.heuristic};
    DirectPickArgs pa{da, d_pick};
    DirectMisPickArgs mpa{ma, d_pick, c.total_power};
    void* args[] = {&scd, &da, &b.leaf_list, &b.nodes16};
    switch ((c.pick ? 2 : 0) | (c.mis ? 1 : 0)) {                           // the kernel's own argument struct
    case 1: args[1] = &ma; break;
    case 2: args[1] = &pa; break;
    case 3: args[1] = &mpa; break;
    }
    return batch_launch(b, args, stream);
}

// What both forms check before any device work: trt_radiance's rules on p->path (its max_bounces and background are carried along unread),
// then the table's size and this struct's own fields.  The table's entries are the host form's to check: the device form cannot read them.
int direct_check(const trt_scene* s, const trt_ray* items, uint32_t n, const trt_emitter* emitters, uint32_t n_emitters, const trt_direct_params* p,
                 const float* radiance, DirectCall& c) {
    if (!p) return query_fail(TRT_ERR_INVALID_ARG, "null argument");
    int rc = radiance_check(s, items, n, &p->path, radiance, c.ra);
    if (rc != TRT_OK) return rc;
    rc = emitter_table_check(n, emitters, n_emitters, p->shadow_end);
    if (rc != TRT_OK) return rc;
    for (uint32_t r : p->reserved)
        if (r != 0u) return query_fail(TRT_ERR_INVALID_ARG, "reserved words must be zero");
    c.samples_per_item = p->path.samples_per_ray;
    c.first_stream = p->path.first_stream;
    c.n_emitters = n_emitters;
    c.shadow_end = p->shadow_end;
    return TRT_OK;
}
// trt_direct_mis' checks before any device work: trt_direct's on p->direct, then the heuristic and this struct's reserved words.
int direct_check(const trt_scene* s, const trt_ray* items, uint32_t n, const trt_emitter* emitters, uint32_t n_emitters, const trt_direct_mis_params* p,
                 const float* radiance, DirectCall& c) {
    if (!p) return query_fail(TRT_ERR_INVALID_ARG, "null argument");
    const int rc = direct_check(s, items, n, emitters, n_emitters, &p->direct, radiance, c);
    return rc != TRT_OK ? rc : emitter_mis_check(*p, c);
}

constexpr EmitterLabels kDirectLabels{"direct-light query buffers", "direct-light query launch"};

// The two forms of the four queries (emitter_query.h): the family's parameter check, then the query's steps over its tables, then the
// launcher.  `steps` is the query's list below, `t.pick` / `t.total_power` what a PICK query was handed.
template <class Params, size_t K>
int direct_device(const EmitterStep (&steps)[K], trt_scene* s, const trt_ray* d_items, uint32_t n, const EmitterTables& t, const Params* p, float* d_radiance,
                  float* d_moment2, uint64_t* d_counters, void* stream) {
    DirectCall c;
    const int rc = direct_check(s, d_items, n, t.emitters, t.n_emitters, p, d_radiance, c);
    if (rc != TRT_OK) return rc;
    return emitter_query_on_device(s, c, steps, kDirectLabels, launch_direct, d_items, n, t, d_radiance, d_moment2, d_counters, stream);
}
template <class Params, size_t K>
int direct_host(const EmitterStep (&steps)[K], trt_scene* s, const trt_ray* items, uint32_t n, const EmitterTables& t, const Params* p, float* radiance,
                float* moment2, trt_stats* stats) {
    return host_form([&]() -> int {
        DirectCall c;
        const int rc = direct_check(s, items, n, t.emitters, t.n_emitters, p, radiance, c);
        if (rc != TRT_OK) return rc;
        return emitter_query_on_host(s, c, steps, kDirectLabels, launch_direct, items, n, t, radiance, moment2, stats);
    });
}
// How launch_direct would launch n items on this scene with the kernels of a query.
int direct_plan(bool mis, bool pick, const trt_scene* s, uint32_t n, uint32_t compute_units, trt_query_plan* out) {
    return batch_launch_plan(s, n, compute_units, kDirectKernels[pick][mis], kDirectShapes, out);
}

// THE ORDER OF EACH QUERY'S TABLE CHECKS (tinyrt.h), behind trt_direct's / trt_direct_mis' own.  The host form runs every step, the device
// form the pointer's only: it cannot read a table, and the rules are the caller's to keep (the kernel's clamp keeps a wrong pick table's
// reads inside the E records).  An empty batch reads no table either.
constexpr EmitterStep kDirectSteps[] = {STEP_EMITTER_ENTRIES};
constexpr EmitterStep kDirectMisSteps[] = {STEP_EMITTER_ENTRIES, STEP_TABLE_RULE};
constexpr EmitterStep kDirectPickSteps[] = {STEP_PICK_POINTER, STEP_EMITTER_ENTRIES, STEP_PICK_ENTRIES};
// the table rule BEFORE the pick records (trt_nee_mis_pick has them the other way round)
constexpr EmitterStep kDirectMisPickSteps[] = {STEP_PICK_POINTER, STEP_EMITTER_ENTRIES, STEP_TABLE_RULE, STEP_PICK_ENTRIES, STEP_PICK_POWER};

}  // namespace
}  // namespace trt

extern "C" {

void trt_direct_params_default(trt_direct_params* out) {
    if (!out) return;
    *out = trt_direct_params{};
    trt_radiance_params_default(&out->path);
    out->shadow_end = 0.999f;
}

int trt_direct_device(trt_scene* s, const trt_ray* d_items, uint32_t n, const trt_emitter* d_emitters, uint32_t n_emitters, const trt_direct_params* p,
                      float* d_radiance, float* d_moment2, uint64_t* d_counters, void* stream) {
    return trt::direct_device(trt::kDirectSteps, s, d_items, n, {d_emitters, nullptr, n_emitters, 0.0f}, p, d_radiance, d_moment2, d_counters, stream);
}
int trt_direct(trt_scene* s, const trt_ray* items, uint32_t n, const trt_emitter* emitters, uint32_t n_emitters, const trt_direct_params* p,
               float* radiance, float* moment2, trt_stats* stats) {
    return trt::direct_host(trt::kDirectSteps, s, items, n, {emitters, nullptr, n_emitters, 0.0f}, p, radiance, moment2, stats);
}
int trt_direct_launch_plan(const trt_scene* s, uint32_t n, uint32_t compute_units, trt_query_plan* out) {
    return trt::direct_plan(false, false, s, n, compute_units, out);
}

void trt_direct_mis_params_default(trt_direct_mis_params* out) {
    if (!out) return;
    *out = trt_direct_mis_params{};
    trt_direct_params_default(&out->direct);
    out->heuristic = TRT_MIS_BALANCE;
}

int trt_direct_mis_device(trt_scene* s, const trt_ray* d_items, uint32_t n, const trt_emitter* d_emitters, uint32_t n_emitters,
                          const trt_direct_mis_params* p, float* d_radiance, float* d_moment2, uint64_t* d_counters, void* stream) {
    return trt::direct_device(trt::kDirectMisSteps, s, d_items, n, {d_emitters, nullptr, n_emitters, 0.0f}, p, d_radiance, d_moment2, d_counters, stream);
}
int trt_direct_mis(trt_scene* s, const trt_ray* items, uint32_t n, const trt_emitter* emitters, uint32_t n_emitters, const trt_direct_mis_params* p,
                   float* radiance, float* moment2, trt_stats* stats) {
    return trt::direct_host(trt::kDirectMisSteps, s, items, n, {emitters, nullptr, n_emitters, 0.0f}, p, radiance, moment2, stats);
}
int trt_direct_mis_launch_plan(const trt_scene* s, uint32_t n, uint32_t compute_units, trt_query_plan* out) {
    return trt::direct_plan(true, false, s, n, compute_units, out);
}

// ---- the PICK queries: the emitter chosen by power (or the caller's weights) through an alias table ----
int trt_emitter_pick_build(const trt_emitter* emitters, uint32_t n_emitters, const float* weights, trt_emitter_pick* out, float* total) {
    return trt::host_form([&]() -> int { return trt::pick_build(emitters, n_emitters, weights, out, total); });
}

int trt_direct_pick_device(trt_scene* s, const trt_ray* d_items, uint32_t n, const trt_emitter* d_emitters, const trt_emitter_pick* d_pick,
                           uint32_t n_emitters, const trt_direct_params* p, float* d_radiance, float* d_moment2, uint64_t* d_counters, void* stream) {
    return trt::direct_device(trt::kDirectPickSteps, s, d_items, n, {d_emitters, d_pick, n_emitters, 0.0f}, p, d_radiance, d_moment2, d_counters, stream);
}
int trt_direct_pick(trt_scene* s, const trt_ray* items, uint32_t n, const trt_emitter* emitters, const trt_emitter_pick* pick, uint32_t n_emitters,
                    const trt_direct_params* p, float* radiance, float* moment2, trt_stats* stats) {
    return trt::direct_host(trt::kDirectPickSteps, s, items, n, {emitters, pick, n_emitters, 0.0f}, p, radiance, moment2, stats);
}
int trt_direct_pick_launch_plan(const trt_scene* s, uint32_t n, uint32_t compute_units, trt_query_plan* out) {
    return trt::direct_plan(false, true, s, n, compute_units, out);
}

int trt_direct_mis_pick_device(trt_scene* s, const trt_ray* d_items, uint32_t n, const trt_emitter* d_emitters, const trt_emitter_pick* d_pick,
                               uint32_t n_emitters, const trt_direct_mis_params* p, float total_power, float* d_radiance, float* d_moment2,
                               uint64_t* d_counters, void* stream) {
    return trt::direct_device(trt::kDirectMisPickSteps, s, d_items, n, {d_emitters, d_pick, n_emitters, total_power}, p, d_radiance, d_moment2, d_counters,
                              stream);
}
int trt_direct_mis_pick(trt_scene* s, const trt_ray* items, uint32_t n, const trt_emitter* emitters, const trt_emitter_pick* pick, uint32_t n_emitters,
                        const trt_direct_mis_params* p, float total_power, float* radiance, float* moment2, trt_stats* stats) {
    return trt::direct_host(trt::kDirectMisPickSteps, s, items, n, {emitters, pick, n_emitters, total_power}, p, radiance, moment2, stats);
}
int trt_direct_mis_pick_launch_plan(const trt_scene* s, uint32_t n, uint32_t compute_units, trt_query_plan* out) {
    return trt::direct_plan(true, true, s, n, compute_units, out);
}

}  // extern "C"
