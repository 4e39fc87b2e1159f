// ambient.hip — ambient queries: how much of the lobe about a caller-supplied surfel is open, and in which mean direction (tinyrt.h
// trt_ambient / trt_ambient_device), written for gfx950 (CDNA4) only.
//
// The gather queries (radiance.hip) answer "what light arrives at this surfel"; these answer the question before it: "how much of the
// hemisphere is open" - ambient occlusion, sky visibility, the bent normal.  For item i and sample s the first ray is trt_gather's, bit
// for bit: drawn by gather_draw.h gather_ray from RNG stream (seed, first_stream + i * K + s, 1).  The sample is what trt_occluded answers
// for that ray with t_max = max_distance: BVH::hit over [0.001, max_distance), any material.  There is no path and stream (.., 0) is not
// touched.  An unoccluded sample adds
//   visibility = visibility + inv_K;   bent.ch = bent.ch + d.ch * inv_K
// (d: the unit direction of the first ray), an occluded one nothing; in sample order, one IEEE f32 operation per operator, in registers:
// a lane owns an item for all samples of the call and writes once per item.
//
// There is no walk code in this file: the kernel calls the entry points of rt_path.h with the walks' ANY switch, as query.hip's occlusion
// form does, with the dynamic LDS laid out as the queries lay it out (scene copy | leaf stack: threads x slots x 8 bytes; wave_run.h) and
// is launched by the rule of the queries (query_plan.h): a wave owns a contiguous run of the items.
//
// Work.  With the two resumable walks (LDS tree, 16-byte nodes) the wave runs in radiance_kernel's rounds - refill, start (draw), walk -
// but a finished walk folds at once: there is no shade, no pending hit and no Path.  A walk still under way when at most `stragglers`
// lanes walk is parked in the lane's leaf stack and resumed in the next round beside the fresh draws (query_kernel's ANY form).  The
// other walks (lock-step list, register slots) run to their end: 64 items of the run at a time, every lane its samples in order - all
// lanes of a wave have the same number of samples, so the sample loop is wave-uniform but for the ragged end of the run.
// A max_distance not above 0.001 is an empty range (the ray queries' rule): the same kernel draws and folds and walks nothing.
#include "gather_draw.h"
#include "kernels.h"
#include "query_plan.h"
#include "rt_path.h"
#include "scene_query.h"
#include "wave_run.h"

namespace trt {

static_assert(sizeof(trt_ambient_params) == 128 && offsetof(trt_ambient_params, max_distance) == 96 && offsetof(trt_ambient_params, reserved) == 100,
              "trt_ambient_params layout (tinyrt.h)");

struct AmbientArgs {
    const float* items;              // n x (point, axis), used as given
    float* visibility;               // n
    float* bent;                     // n x 3, or nullptr: not wanted
    unsigned long long* counters;    // nullptr, or [CTR_SAMPLES], [CTR_RAYS] are added to
    uint32_t n, rays_per_wave;       // wave w owns items [w * rays_per_wave, ...)
    uint32_t slots, stragglers;      // as in query.hip QueryArgs
    uint32_t samples_per_item;       // K
    uint32_t first_stream;           // first_stream + n * K <= 2^32 (gather_check): the stream index never wraps
    uint32_t seed_key;               // kernels.h rng_seed_key
    uint32_t sample_begin, sample_end;      // begin < end (launch_ambient: an empty range launches query_plan.h batch_zero or nothing)
    uint32_t accumulate;
    uint32_t lobe;                   // TRT_LOBE_COSINE or TRT_LOBE_CONE: the same for every lane of the launch
    float spread;
    float inv_k;                     // 1.0f / float(K)
    float max_distance;              // not NaN (ambient_check); <= 0.001: nothing is walked
    FlatReuse flat_reuse;
};

// The four sums of one item: read where a call continues them, written once when the item's last sample has folded.
struct AmbientSums {
    float vis;
    V3 bent;
};
TRT_DEV AmbientSums amb_begin(const AmbientArgs& aa, uint32_t idx) {
    AmbientSums a;
    a.vis = 0.0f;
    a.bent = v3(0.0f, 0.0f, 0.0f);
    if (aa.accumulate) {
        a.vis = aa.visibility[idx];
        if (aa.bent) { const float* const b = aa.bent + 3ull * idx; a.bent = v3(b[0], b[1], b[2]); }
    }
    return a;
}
TRT_DEV void amb_store(const AmbientArgs& aa, uint32_t idx, const AmbientSums& a) {
    aa.visibility[idx] = a.vis;
    if (aa.bent) { float* const b = aa.bent + 3ull * idx; b[0] = a.bent.x; b[1] = a.bent.y; b[2] = a.bent.z; }
}
// The fold of one unoccluded sample (tinyrt.h); an occluded sample folds nothing.
TRT_DEV void amb_fold(AmbientSums& a, const V3& d, float inv_k) {
    a.vis = a.vis + inv_k;
    a.bent = a.bent + d * inv_k;
}

template <int MODE, int WALK, int THREADS, int MINW>
__global__ __launch_bounds__(THREADS, MINW) void ambient_kernel(SceneDev scd, AmbientArgs aa, const float4* __restrict__ leaf_list,
                                                                     const uint4* __restrict__ nodes16) {
    stage_scene_to_lds<MODE>(scd);
    const FlatReuse flat_reuse = axis_quads_to_lds<MODE, false, WALK>(scd, aa.flat_reuse);
    const SceneAcc<MODE> sc{scd.blob, scd.L};
    const float* __restrict__ const items = aa.items;
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long begin64 = wave_begin<THREADS>(aa.rays_per_wave);
    if (begin64 >= aa.n) return;                                            // (after the barriers above)
    const uint32_t begin = (uint32_t)begin64;
    const uint32_t count = wave_count(aa.n, aa.rays_per_wave, begin);
    // this lane's postponed-leaf stack: behind the scene copy, slots x 64 x 8 bytes per wave
    float2* const stack = WALK != WALK_REGS ? reinterpret_cast<float2*>(lds_behind_scene(sc)) + (threadIdx.x >> 6) * (64u * aa.slots) + lane : nullptr;
    Counters<false> ctr;
    constexpr bool kResumable = WALK == WALK_COMPACT || WALK == WALK_LDS_STACK;
    const bool walks = aa.max_distance > kTMin;                             // wave-uniform: else an empty range, nothing is occluded
    uint32_t n_samples = 0, n_rays = 0;

    if constexpr (kResumable) {
        uint32_t cursor = 0;                                                // wave-uniform
        bool own = false, has_ray = false, walking = false;                 // the lane owns an item; a sample's ray is drawn; its walk is parked
        uint32_t idx = 0, s = 0;
        AmbientSums acc;
        acc.vis = 0.0f; acc.bent = v3(0.0f, 0.0f, 0.0f);
        Ray ray;
        ray.o = v3(0.0f, 0.0f, 0.0f); ray.d = v3(0.0f, 0.0f, 0.0f);
        for (;;) {
            // ---- refill: every lane without an item takes the next one of the run (begin + item < n: item < count <= n - begin) ----
            const uint64_t need = __builtin_amdgcn_ballot_w64(!own);
            if (need != 0ull && cursor < count) {
                const uint32_t item = cursor + wave_rank(need);
                if (!own && item < count) {
                    idx = begin + item;
                    s = aa.sample_begin;
                    acc = amb_begin(aa, idx);
                    own = true;
                }
                cursor = wave_advance(cursor, need, count);
            }
            if (__builtin_amdgcn_ballot_w64(own) == 0ull) break;            // every lane is free and none could take an item: the run is done
            if (own) {
                // ---- start: the item's next sample draws its first ray (stream (seed, j, 1): trt_gather's) ----
                if (!has_ray) {
                    Rng g = rng_seed(aa.seed_key, aa.first_stream + idx * aa.samples_per_item + s, 1u);
                    ray = gather_ray(items, idx, aa.lobe, aa.spread, g);
                    has_ray = true;
                    n_samples++;
                }
                // ---- walk; a finished walk folds at once ----
                bool occluded = false;
                if (walks) {
                    Trav tr = trav_begin<MODE, WALK == WALK_COMPACT>(sc, ray, false);      // a new walk, or the frame of a parked one
                    if (walking) trav_unpark(stack, tr); else { tr.t_best = aa.max_distance; n_rays++; }
                    const uint32_t entered = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(true));
                    walking = !closest_hit_resume<MODE, false, WALK, true>(sc, ray, tr, ctr, aa.slots, stack, leaf_list, nodes16, aa.stragglers, entered);
                    occluded = tr.prim_best != PRIM_NONE;
                }
                if (!walking) {
                    if (!occluded) amb_fold(acc, ray.d, aa.inv_k);
                    has_ray = false;
                    s += 1u;
                    if (s == aa.sample_end) {
                        amb_store(aa, idx, acc);
                        own = false;
                    }
                }
            }
        }
    } else {
        for (uint32_t base = 0; base < count; base += 64u) {
            if (base + lane < count) {
                const uint32_t idx = begin + base + lane;
                AmbientSums acc = amb_begin(aa, idx);
                for (uint32_t s = aa.sample_begin; s != aa.sample_end; s++) {
                    Rng g = rng_seed(aa.seed_key, aa.first_stream + idx * aa.samples_per_item + s, 1u);
                    const Ray ray = gather_ray(items, idx, aa.lobe, aa.spread, g);
                    n_samples++;
                    uint32_t prim = PRIM_NONE;
                    if (walks) {
                        float t = 0.0f;
                        n_rays++;
                        prim = closest_hit<MODE, false, WALK, true>(sc, ray, false, t, ctr, aa.slots, stack, leaf_list, nodes16, flat_reuse, aa.max_distance);
                    }
                    if (prim == PRIM_NONE) amb_fold(acc, ray.d, aa.inv_k);
                }
                amb_store(aa, idx, acc);
            }
        }
    }
    flush_counters<false>(aa.counters, n_samples, n_rays, ctr);
}

namespace {

#define TRT_AMBIENT(MODE, WALK, THREADS, MINW) \
    BatchKernel{reinterpret_cast<const void*>(&ambient_kernel<MODE, WALK, THREADS, MINW>), MODE, WALK, THREADS, MINW}
// the (scene mode, walk, workgroup shape) set of the other batch units, with the register-slot fallback (query_plan.h), so that every
// scene has a kernel.  A lane carries what a lane of the occlusion query carries plus the draw's ray, the item and sample index and the
// four sums: the launch bounds are the highest at which the instantiation uses no scratch memory and spills no vector register
// (profiles/ambient_resource_usage.txt).  The plan reports the bound (kernel_waves_per_simd).
const BatchKernel kAmbientKernels[] = {
    TRT_AMBIENT(MODE_LDS, WALK_FLAT, 256, 8),
    TRT_AMBIENT(MODE_LDS, WALK_LDS_STACK, 256, 8),
    TRT_AMBIENT(MODE_LDS, WALK_LDS_STACK, 768, 8),
    TRT_AMBIENT(MODE_LDS, WALK_REGS, 512, 7),
    TRT_AMBIENT(MODE_GLOBAL, WALK_COMPACT, 256, 8),
    TRT_AMBIENT(MODE_GLOBAL, WALK_REGS, 256, 7),
};
#undef TRT_AMBIENT
constexpr size_t kAmbientShapes = sizeof(kAmbientKernels) / sizeof(kAmbientKernels[0]);

// What a call asks of the device, after the checks.
struct AmbientCall {
    RenderArgs ra;                   // of the gather parameters: seed key, 1 / K, sample range, accumulate (gather_check)
    Lobe lobe;
    uint32_t samples_per_item, first_stream;
    float max_distance;
    bool nothing() const { return ra.sample_begin == ra.sample_end; }       // an empty sample range: no sample is drawn
};

hipError_t launch_ambient(const QueryScene& qs, const AmbientCall& c, const float* d_items, uint32_t n, float* d_visibility, float* d_bent,
                          unsigned long long* d_counters, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (c.nothing()) {
        // the sums start at 0, or stay
        if (c.ra.accumulate) return hipSuccess;
        return batch_zero(d_visibility, n, d_bent, 3ull * n, stream);
    }
    SceneDev scd = qs.scene;
    BatchLaunch b;
    const hipError_t e = batch_prepare(scd, n, kAmbientKernels, kAmbientShapes, b);
    if (e != hipSuccess) return e;
    const trt_query_plan& q = b.q;
    AmbientArgs aa{d_items, d_visibility, d_bent, d_counters, n, q.rays_per_wave, q.leaf_slots, q.stragglers, c.samples_per_item, c.first_stream,
                   c.ra.seed_key, c.ra.sample_begin, c.ra.sample_end, c.ra.accumulate, c.lobe.lobe, c.lobe.spread, c.ra.inv_spp, c.max_distance,
                   qs.flat_reuse};
    void* args[] = {&scd, &aa, &b.leaf_list, &b.nodes16};
    return batch_launch(b, args, stream);
}

// What both forms check before any device work: trt_gather's rules on p->gather (its max_bounces and background are carried along
// unread), then this struct's own fields.
int ambient_check(const trt_scene* s, const trt_ray* items, uint32_t n, const trt_ambient_params* p, const float* visibility, AmbientCall& c) {
    if (!p) return query_fail(TRT_ERR_INVALID_ARG, "null argument");
    const int rc = gather_check(s, items, n, &p->gather, visibility, c.ra, c.lobe);
    if (rc != TRT_OK) return rc;
    if (p->max_distance != p->max_distance) return query_fail(TRT_ERR_INVALID_ARG, "max_distance must not be NaN");
    for (uint32_t r : p->reserved)
        if (r != 0u) return query_fail(TRT_ERR_INVALID_ARG, "reserved words must be zero");
    c.samples_per_item = p->gather.path.samples_per_ray;
    c.first_stream = p->gather.path.first_stream;
    c.max_distance = p->max_distance;
    return TRT_OK;
}

}  // namespace
}  // namespace trt

extern "C" {

void trt_ambient_params_default(trt_ambient_params* out) {
    if (!out) return;
    *out = trt_ambient_params{};
    trt_gather_params_default(&out->gather);
    out->max_distance = __builtin_inff();
}

int trt_ambient_device(trt_scene* s, const trt_ray* d_items, uint32_t n, const trt_ambient_params* p, float* d_visibility, float* d_bent,
                       uint64_t* d_counters, void* stream) {
    trt::AmbientCall c;
    const int rc = trt::ambient_check(s, d_items, n, p, d_visibility, c);
    if (rc != TRT_OK) return rc;
    return trt::sample_query_on_device(s, n, "ambient query launch", [&](const trt::QueryScene& qs) {
        return trt::launch_ambient(qs, c, reinterpret_cast<const float*>(d_items), n, d_visibility, d_bent,
                                   reinterpret_cast<unsigned long long*>(d_counters), static_cast<hipStream_t>(stream));
    });
}

// Host buffers: staged by host_stage.h sample_query_on_host (items | visibility | bent, if wanted | counters).
int trt_ambient(trt_scene* s, const trt_ray* items, uint32_t n, const trt_ambient_params* p, float* visibility, float* bent, trt_stats* stats) {
    return trt::host_form([&]() -> int {
        trt::AmbientCall c;
        const int rc = trt::ambient_check(s, items, n, p, visibility, c);
        if (rc != TRT_OK) return rc;
        const trt::SampleHost h{items, (size_t)n * sizeof(trt_ray), "hipMemcpy of the items", nullptr, 0u, "", visibility, (size_t)n * 4u, bent,
                                (size_t)n * 12u, "hipMemcpy of the bent sums"};
        return trt::sample_query_on_host(s, n, h, c.ra.accumulate != 0u, c.nothing(), "ambient query buffers", "ambient query launch", stats,
                                         [&](const trt::QueryScene& qs, const trt::SampleDev& d) {
                                             return trt::launch_ambient(qs, c, d.items, n, d.sums, d.sums2, d.counters, nullptr);
                                         });
    });
}

// How launch_ambient would launch n items on this scene.
int trt_ambient_launch_plan(const trt_scene* s, uint32_t n, uint32_t compute_units, trt_query_plan* out) {
    return trt::batch_launch_plan(s, n, compute_units, trt::kAmbientKernels, trt::kAmbientShapes, out);
}

}  // extern "C"
