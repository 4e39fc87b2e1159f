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
#include "gather_draw.h"
#include "host_stage.h"
#include "kernels.h"
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

template <int MODE, int WALK, int THREADS, int MINW>
__global__ __launch_bounds__(THREADS, MINW) void direct_kernel(SceneDev scd, DirectArgs da, const float4* __restrict__ leaf_list,
                                                                    const uint4* __restrict__ nodes16) {
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
                    const DirectSample smp = direct_draw(items, idx, emitters, da.n_emitters, da.shadow_end, g);
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
                    const DirectSample smp = direct_draw(items, idx, emitters, da.n_emitters, da.shadow_end, g);
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

namespace {

#define TRT_DIRECT(MODE, WALK, THREADS, MINW) \
    BatchKernel{reinterpret_cast<const void*>(&direct_kernel<MODE, WALK, THREADS, MINW>), MODE, WALK, THREADS, MINW}
// the (scene mode, walk, workgroup shape) set of the other batch units, with the register-slot fallback (query_plan.h), so that every
// scene has a kernel.  A lane carries what a lane of the ambient query carries plus the sample's colour, its t_max and two sums more: the
// launch bounds are the highest at which the instantiation uses no scratch memory and spills no vector register
// (profiles/direct_resource_usage.txt).  The plan reports the bound (kernel_waves_per_simd).
const BatchKernel kDirectKernels[] = {
    TRT_DIRECT(MODE_LDS, WALK_FLAT, 256, 7),
    TRT_DIRECT(MODE_LDS, WALK_LDS_STACK, 256, 8),
    TRT_DIRECT(MODE_LDS, WALK_LDS_STACK, 768, 8),
    TRT_DIRECT(MODE_LDS, WALK_REGS, 512, 7),
    TRT_DIRECT(MODE_GLOBAL, WALK_COMPACT, 256, 7),
    TRT_DIRECT(MODE_GLOBAL, WALK_REGS, 256, 6),
};
#undef TRT_DIRECT
constexpr size_t kDirectShapes = sizeof(kDirectKernels) / sizeof(kDirectKernels[0]);

// What a call asks of the device, after the checks.
struct DirectCall {
    RenderArgs ra;                   // of the path parameters: seed key, 1 / K, sample range, accumulate (radiance_check)
    uint32_t samples_per_item, first_stream;
    uint32_t n_emitters;
    float shadow_end;
    bool nothing() const { return ra.sample_begin == ra.sample_end; }       // an empty sample range: no sample is drawn
};

hipError_t launch_direct(const QueryScene& qs, const DirectCall& c, const float* d_items, uint32_t n, const float* d_emitters, float* d_radiance,
                         float* d_moment2, unsigned long long* d_counters, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (c.nothing()) {
        // the sums start at 0, or stay
        if (c.ra.accumulate) return hipSuccess;
        return batch_zero(d_radiance, 3ull * n, d_moment2, 3ull * n, stream);
    }
    SceneDev scd = qs.scene;
    BatchLaunch b;
    const hipError_t e = batch_prepare(scd, n, kDirectKernels, kDirectShapes, b);
    if (e != hipSuccess) return e;
    const trt_query_plan& q = b.q;
    DirectArgs da{d_items, d_emitters, d_radiance, d_moment2, d_counters, n, q.rays_per_wave, q.leaf_slots, q.stragglers, c.samples_per_item,
                  c.first_stream, c.ra.seed_key, c.ra.sample_begin, c.ra.sample_end, c.ra.accumulate, c.n_emitters, c.ra.inv_spp, c.shadow_end,
                  qs.flat_reuse};
    void* args[] = {&scd, &da, &b.leaf_list, &b.nodes16};
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
    trt::DirectCall c;
    const int rc = trt::direct_check(s, d_items, n, d_emitters, n_emitters, p, d_radiance, c);
    if (rc != TRT_OK) return rc;
    return trt::sample_query_on_device(s, n, "direct-light query launch", [&](const trt::QueryScene& qs) {
        return trt::launch_direct(qs, c, reinterpret_cast<const float*>(d_items), n, reinterpret_cast<const float*>(d_emitters), d_radiance, d_moment2,
                                  reinterpret_cast<unsigned long long*>(d_counters), static_cast<hipStream_t>(stream));
    });
}

// Host buffers: staged by host_stage.h sample_query_on_host (items | table | sums | second moments, if wanted | counters).  The table's
// entries are checked where n > 0, ahead of any device work.
int trt_direct(trt_scene* s, const trt_ray* items, uint32_t n, const trt_emitter* emitters, uint32_t n_emitters, const trt_direct_params* p,
               float* radiance, float* moment2, trt_stats* stats) {
    return trt::host_form([&]() -> int {
        trt::DirectCall c;
        int rc = trt::direct_check(s, items, n, emitters, n_emitters, p, radiance, c);
        if (rc != TRT_OK) return rc;
        rc = trt::emitter_entries_check(emitters, n == 0u ? 0u : n_emitters);
        if (rc != TRT_OK) return rc;
        const size_t sums = (size_t)n * 12u;
        const trt::SampleHost h{items, (size_t)n * sizeof(trt_ray), "hipMemcpy of the items", emitters, (size_t)n_emitters * sizeof(trt_emitter),
                                "hipMemcpy of the emitters", radiance, sums, moment2, sums, "hipMemcpy of the second moments"};
        return trt::sample_query_on_host(s, n, h, c.ra.accumulate != 0u, c.nothing(), "direct-light query buffers", "direct-light query launch", stats,
                                         [&](const trt::QueryScene& qs, const trt::SampleDev& d) {
                                             return trt::launch_direct(qs, c, d.items, n, d.table, d.sums, d.sums2, d.counters, nullptr);
                                         });
    });
}

// How launch_direct would launch n items on this scene.
int trt_direct_launch_plan(const trt_scene* s, uint32_t n, uint32_t compute_units, trt_query_plan* out) {
    return trt::batch_launch_plan(s, n, compute_units, trt::kDirectKernels, trt::kDirectShapes, out);
}

}  // extern "C"
