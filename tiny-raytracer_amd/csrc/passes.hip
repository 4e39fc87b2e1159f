// passes.hip — light-path passes: the radiance a gather or radiance query would return, split by how the path ended and after how many
// scatters (tinyrt.h trt_passes / trt_passes_device), written for gfx950 (CDNA4) only.
//
// A sample's colour comes from exactly one terminal event of CpuSampler::single_point_sampling (cpu.rs:39-65): Light::scatter returns
// None (LIGHT), the ray misses and the background is added (SKY), or the budget runs out and the colour stays 0 (SPENT); every other hit
// adds +0.  shade_hit (rt_path.h) returns true in exactly these three cases and leaves what tells them apart: the primitive it was given
// is PRIM_NONE for SKY, p.remain is 0 for SPENT and unchanged, hence >= 1, for LIGHT, and d = max_bounces - p.remain scatters came
// before.  With b = min(d, B - 1) the sample's slot is b (LIGHT) or B + b (SKY), and the fold is
//   passes[i][slot].ch = passes[i][slot].ch + c.ch * inv_K        spent[i] = spent[i] + inv_K   (SPENT)
// in sample order, one IEEE f32 operation per operator, in registers: a lane owns an item for all samples of the call, keeps the 6 NB sums
// and `spent` and writes them once per item.  A sample touches its own slot only.
//
// The round loop is probe_kernel's - refill, start, SHADE what is pending, WALK what is alive - in a kernel of its own, so that the
// device code of radiance.hip and probe.hip stays what it was by construction.  The first ray is the caller's (TRT_PASSES_RAYS: loaded
// for every sample, as radiance_kernel's lock-step form does) or gather_draw.h gather_ray's, the ONE copy of the gather's draw; the
// source is a wave-uniform word of the arguments, as the probe's hemisphere is.  There is no walk code in this file: the kernel calls
// the entry points of rt_path.h with the dynamic LDS laid out as the queries lay it out (wave_run.h) and is launched by the rule of the
// queries (query_plan.h).
#include "gather_draw.h"
#include "host_stage.h"
#include "kernels.h"
#include "query_plan.h"
#include "rt_path.h"
#include "scene_query.h"
#include "wave_run.h"

namespace trt {

static_assert(sizeof(trt_passes_params) == 128 && offsetof(trt_passes_params, gather) == 0 && offsetof(trt_passes_params, depth_bins) == 96 &&
              offsetof(trt_passes_params, reserved) == 100, "trt_passes_params layout (tinyrt.h)");
static_assert((int)TRT_PASSES_COSINE == (int)TRT_LOBE_COSINE && (int)TRT_PASSES_CONE == (int)TRT_LOBE_CONE, "the drawn sources are the lobes of trt_gather");

struct PassesArgs {
    const float* items;              // n x (origin, direction) or n x (point, axis), used as given
    float* passes;                   // n x 2 bins x 3
    float* spent;                    // n, or nullptr: not wanted
    unsigned long long* counters;    // nullptr, or [CTR_SAMPLES], [CTR_RAYS] are added to
    uint32_t n, rays_per_wave;       // wave w owns items [w * rays_per_wave, ...)
    uint32_t slots, stragglers;      // as in query.hip QueryArgs
    uint32_t samples_per_item;       // K
    uint32_t first_stream;           // first_stream + n * K <= 2^32 (radiance_check): the stream index never wraps
    uint32_t source;                 // enum trt_passes_source; the same for every lane of the launch
    float spread;                    // the cone lobe's sphere radius
    uint32_t bins;                   // B = depth_bins: 1 .. the kernel's NB
};

// The fold of one sample into register slot `slot` of 2 NB (LIGHT at b, SKY at NB + b; >= 2 NB: none).  A compare and a select per
// slot: an index into acc[] would put the sums into scratch memory.
template <int NB>
TRT_DEV void passes_fold(float (&acc)[6 * NB], uint32_t slot, const V3& c, float inv_k) {
    const float tx = c.x * inv_k, ty = c.y * inv_k, tz = c.z * inv_k;
#pragma unroll
    for (int k = 0; k < 2 * NB; k++) {
        const bool mine = slot == (uint32_t)k;
        const float ax = acc[3 * k + 0] + tx, ay = acc[3 * k + 1] + ty, az = acc[3 * k + 2] + tz;
        acc[3 * k + 0] = mine ? ax : acc[3 * k + 0];
        acc[3 * k + 1] = mine ? ay : acc[3 * k + 1];
        acc[3 * k + 2] = mine ? az : acc[3 * k + 2];
    }
}

// ra.sample_begin < ra.sample_end and ra.max_bounces > 0 (launch_passes: nothing to trace launches query_plan.h batch_zero or nothing)
template <int MODE, int WALK, int THREADS, int MINW, int NB>
__global__ __launch_bounds__(THREADS, MINW) void passes_kernel(SceneDev scd, RenderArgs ra, PassesArgs ga, const float4* __restrict__ leaf_list,
                                                                    const uint4* __restrict__ nodes16) {
    stage_scene_to_lds<MODE>(scd);
    const FlatReuse flat_reuse = axis_quads_to_lds<MODE, false, WALK>(scd, ra.flat_reuse);
    const SceneAcc<MODE> sc{scd.blob, scd.L};
    const float* __restrict__ const items = ga.items;
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long begin64 = wave_begin<THREADS>(ga.rays_per_wave);
    if (begin64 >= ga.n) return;                                            // (after the barriers above)
    const uint32_t begin = (uint32_t)begin64;
    const uint32_t count = wave_count(ga.n, ga.rays_per_wave, begin);
    // this lane's postponed-leaf stack: behind the scene copy, slots x 64 x 8 bytes per wave
    float2* const stack = WALK != WALK_REGS ? reinterpret_cast<float2*>(lds_behind_scene(sc)) + (threadIdx.x >> 6) * (64u * ga.slots) + lane : nullptr;
    const V3 background = v3(ra.background[0], ra.background[1], ra.background[2]);
    Counters<false> ctr;
    constexpr bool kResumable = WALK == WALK_COMPACT || WALK == WALK_LDS_STACK;

    uint32_t cursor = 0;                                                    // wave-uniform
    bool own = false, has_path = false, walking = false;                    // the lane owns an item; a path of it is under way; its walk is parked
    bool pending = false;                                                   // a finished walk waits for its shade
    uint32_t idx = 0, s = 0;
    uint32_t hit_prim = PRIM_NONE;
    float hit_t = 0.0f;
    uint32_t n_samples = 0, n_rays = 0;
    float acc[6 * NB];                                                      // LIGHT bins at [0, NB), SKY bins at [NB, 2 NB), 3 channels each
#pragma unroll
    for (int k = 0; k < 6 * NB; k++) acc[k] = 0.0f;
    float sp = 0.0f;
    Path p;
    p.ray.o = v3(0.0f, 0.0f, 0.0f); p.ray.d = v3(0.0f, 0.0f, 0.0f);
    p.color = v3(0.0f, 0.0f, 0.0f); p.atten = v3(0.0f, 0.0f, 0.0f);
    p.remain = 0u;
    p.rng.s0 = 0u; p.rng.s1 = 0u;
    for (;;) {
        // ---- refill: every lane without an item takes the next one of the run (begin + item < n: item < count <= n - begin) ----
        const uint64_t need = __builtin_amdgcn_ballot_w64(!own);
        if (need != 0ull && cursor < count) {
            const uint32_t item = cursor + wave_rank(need);
            if (!own && item < count) {
                idx = begin + item;
                s = ra.sample_begin;
                const float* const a = ga.passes + 6ull * ga.bins * idx;    // idx < n: within [0, 6 * bins * n)
#pragma unroll
                for (int k = 0; k < NB; k++) {
                    const bool read = ra.accumulate && (uint32_t)k < ga.bins;         // wave-uniform
#pragma unroll
                    for (int ch = 0; ch < 3; ch++) {
                        acc[3 * k + ch] = read ? a[3 * k + ch] : 0.0f;
                        acc[3 * (NB + k) + ch] = read ? a[3 * (ga.bins + k) + ch] : 0.0f;
                    }
                }
                sp = ra.accumulate && ga.spent ? ga.spent[idx] : 0.0f;
                own = true;
            }
            cursor = wave_advance(cursor, need, count);
        }
        if (__builtin_amdgcn_ballot_w64(own) == 0ull) break;                // every lane is free and none could take an item: the run is done
        if (own) {
            // ---- start: the item's next sample; a drawn first ray has stream (seed, j, 1), the path starts fresh on (seed, j, 0) ----
            if (!has_path) {
                const uint32_t stream = ga.first_stream + idx * ga.samples_per_item + s;
                if (ga.source == TRT_PASSES_RAYS) {                         // wave-uniform
                    p.ray = rad_load_ray(items, idx);                       // re-read: 24 bytes per sample against six registers per lane
                } else {
                    Rng g = rng_seed(ra.seed_key, stream, 1u);
                    p.ray = gather_ray(items, idx, ga.source, ga.spread, g);
                }
                p.rng = rng_seed(ra.seed_key, stream, 0u);
                p.color = v3(0.0f, 0.0f, 0.0f);
                p.atten = v3(1.0f, 1.0f, 1.0f);
                p.remain = ra.max_bounces;
                has_path = true;
                n_samples++;
            }
            // ---- shade what is pending ----
            if (pending) {
                pending = false;
                if (shade_hit<MODE, false>(sc, p, hit_prim, hit_t, background, ctr)) {
                    // the class of the sample: a miss; else the budget is spent (p.remain == 0); else a light, which left p.remain >= 1
                    const bool sky = hit_prim == PRIM_NONE;
                    const uint32_t depth = ra.max_bounces - p.remain;
                    const uint32_t bin = depth < ga.bins - 1u ? depth : ga.bins - 1u;
                    const bool is_spent = !sky && p.remain == 0u;
                    const uint32_t slot = is_spent ? 2u * NB : (sky ? (uint32_t)NB + bin : bin);
                    passes_fold<NB>(acc, slot, p.color, ra.inv_spp);
                    const float sp1 = sp + ra.inv_spp;
                    sp = is_spent ? sp1 : sp;
                    has_path = false;
                    s += 1u;
                    if (s == ra.sample_end) {
                        float* const a = ga.passes + 6ull * ga.bins * idx;
#pragma unroll
                        for (int k = 0; k < NB; k++) {
                            if ((uint32_t)k < ga.bins) {                    // wave-uniform
#pragma unroll
                                for (int ch = 0; ch < 3; ch++) {
                                    a[3 * k + ch] = acc[3 * k + ch];
                                    a[3 * (ga.bins + k) + ch] = acc[3 * (NB + k) + ch];
                                }
                            }
                        }
                        if (ga.spent) ga.spent[idx] = sp;
                        own = false;
                    }
                }
            }
            // ---- walk what is alive ----
            if (has_path) {
                bool done = true;
                if constexpr (kResumable) {
                    Trav tr = trav_begin<MODE, WALK == WALK_COMPACT>(sc, p.ray, false);      // a new walk, or the frame of a parked one
                    if (walking) trav_unpark(stack, tr); else { tr.t_best = __builtin_inff(); n_rays++; }
                    const uint32_t entered = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(true));
                    walking = !closest_hit_resume<MODE, false, WALK, false>(sc, p.ray, tr, ctr, ga.slots, stack, leaf_list, nodes16, ga.stragglers, entered);
                    done = !walking;
                    hit_prim = tr.prim_best; hit_t = tr.t_best;
                } else {
                    n_rays++;
                    hit_prim = closest_hit<MODE, false, WALK, false>(sc, p.ray, false, hit_t, ctr, ga.slots, stack, leaf_list, nodes16, flat_reuse);
                }
                if (done) pending = true;
            }
        }
    }
    flush_counters<false>(ga.counters, n_samples, n_rays, ctr);
}

namespace {

#define TRT_PASSES(MODE, WALK, THREADS, MINW, NB) \
    BatchKernel{reinterpret_cast<const void*>(&passes_kernel<MODE, WALK, THREADS, MINW, NB>), MODE, WALK, THREADS, MINW}
// The (scene mode, walk, workgroup shape) set of radiance.hip kGatherKernels, once for 2 depth bins (B = 1 and 2) and once for 4 (B = 3
// and 4).  A lane carries what a lane of the gather kernel carries less the second moment, plus the 6 NB sums and `spent`: the launch
// bounds are the highest at which the instantiation uses no scratch memory and spills no vector register
// (profiles/passes_resource_usage.txt).  The plan reports the bound (kernel_waves_per_simd).
const BatchKernel kPassesKernels2[] = {
    TRT_PASSES(MODE_LDS, WALK_FLAT, 256, 5, 2),
    TRT_PASSES(MODE_LDS, WALK_LDS_STACK, 256, 5, 2),
    TRT_PASSES(MODE_LDS, WALK_LDS_STACK, 768, 5, 2),
    TRT_PASSES(MODE_LDS, WALK_REGS, 512, 6, 2),
    TRT_PASSES(MODE_GLOBAL, WALK_COMPACT, 256, 5, 2),
    TRT_PASSES(MODE_GLOBAL, WALK_REGS, 256, 6, 2),
};
const BatchKernel kPassesKernels4[] = {
    TRT_PASSES(MODE_LDS, WALK_FLAT, 256, 5, 4),
    TRT_PASSES(MODE_LDS, WALK_LDS_STACK, 256, 5, 4),
    TRT_PASSES(MODE_LDS, WALK_LDS_STACK, 768, 5, 4),
    TRT_PASSES(MODE_LDS, WALK_REGS, 512, 5, 4),
    TRT_PASSES(MODE_GLOBAL, WALK_COMPACT, 256, 5, 4),
    TRT_PASSES(MODE_GLOBAL, WALK_REGS, 256, 5, 4),
};
#undef TRT_PASSES
constexpr size_t kPassesShapes = sizeof(kPassesKernels4) / sizeof(kPassesKernels4[0]);
static_assert(sizeof(kPassesKernels2) == sizeof(kPassesKernels4), "one instantiation per shape and bin count");
const BatchKernel* passes_table(uint32_t bins) { return bins > 2u ? kPassesKernels4 : kPassesKernels2; }

// What a call asks of the device, after the checks.
struct PassesCall {
    RenderArgs ra;                   // of the path parameters (radiance_check)
    uint32_t samples_per_item, first_stream;
    uint32_t source, bins;
    float spread;
    bool nothing() const { return ra.sample_begin == ra.sample_end || ra.max_bounces == 0u; }
};

hipError_t launch_passes(const QueryScene& qs, const PassesCall& c, const float* d_items, uint32_t n, float* d_passes, float* d_spent,
                         unsigned long long* d_counters, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (c.nothing()) {
        // nothing to trace: a path with no bounce budget returns colour 0 (cpu.rs:43-47,64) and is no sample of the call; the sums start at 0, or stay
        if (c.ra.accumulate) return hipSuccess;
        return batch_zero(d_passes, 6ull * c.bins * n, d_spent, n, stream);
    }
    SceneDev scd = qs.scene;
    BatchLaunch b;
    const hipError_t e = batch_prepare(scd, n, passes_table(c.bins), kPassesShapes, b);
    if (e != hipSuccess) return e;
    const trt_query_plan& q = b.q;
    RenderArgs ra = c.ra;
    ra.flat_reuse = qs.flat_reuse;
    PassesArgs ga{d_items, d_passes, d_spent, d_counters, n, q.rays_per_wave, q.leaf_slots, q.stragglers, c.samples_per_item, c.first_stream,
                  c.source, c.spread, c.bins};
    void* args[] = {&scd, &ra, &ga, &b.leaf_list, &b.nodes16};
    return batch_launch(b, args, stream);
}

// What both forms check before any device work: trt_radiance's rules on p->gather.path (radiance_check), trt_gather's on the source where
// it is a lobe, then this struct's fields.
int passes_check(const trt_scene* s, const trt_ray* items, uint32_t n, const trt_passes_params* p, const float* passes, PassesCall& c) {
    if (!p) return query_fail(TRT_ERR_INVALID_ARG, "null argument");
    const trt_gather_params& g = p->gather;
    int rc = radiance_check(s, items, n, &g.path, passes, c.ra);
    if (rc != TRT_OK) return rc;
    rc = gather_source_check(g);
    if (rc != TRT_OK) return rc;
    if (p->depth_bins < 1u || p->depth_bins > 4u) return query_fail(TRT_ERR_INVALID_ARG, "depth_bins must be 1, 2, 3 or 4");
    for (uint32_t r : p->reserved)
        if (r != 0u) return query_fail(TRT_ERR_INVALID_ARG, "reserved words must be zero");
    c.samples_per_item = g.path.samples_per_ray;
    c.first_stream = g.path.first_stream;
    c.source = g.lobe;
    c.spread = g.lobe == TRT_PASSES_RAYS ? 0.0f : g.spread;
    c.bins = p->depth_bins;
    return TRT_OK;
}

}  // namespace
}  // namespace trt

extern "C" {

void trt_passes_params_default(trt_passes_params* out) {
    if (!out) return;
    *out = trt_passes_params{};
    trt_gather_params_default(&out->gather);
    out->gather.lobe = TRT_PASSES_COSINE;
    out->depth_bins = 3u;
}

int trt_passes_device(trt_scene* s, const trt_ray* d_items, uint32_t n, const trt_passes_params* p, float* d_passes, float* d_spent,
                      uint64_t* d_counters, void* stream) {
    trt::PassesCall c;
    const int rc = trt::passes_check(s, d_items, n, p, d_passes, c);
    if (rc != TRT_OK) return rc;
    return trt::sample_query_on_device(s, n, "passes query launch", [&](const trt::QueryScene& qs) {
        return trt::launch_passes(qs, c, reinterpret_cast<const float*>(d_items), n, d_passes, d_spent, reinterpret_cast<unsigned long long*>(d_counters),
                                  static_cast<hipStream_t>(stream));
    });
}

// Host buffers: staged by host_stage.h sample_query_on_host (items | passes | spent, if wanted | counters).
int trt_passes(trt_scene* s, const trt_ray* items, uint32_t n, const trt_passes_params* p, float* passes, float* spent, trt_stats* stats) {
    return trt::host_form([&]() -> int {
        trt::PassesCall c;
        const int rc = trt::passes_check(s, items, n, p, passes, c);
        if (rc != TRT_OK) return rc;
        const trt::SampleHost h{items, (size_t)n * sizeof(trt_ray), "hipMemcpy of the items", nullptr, 0u, "", passes, (size_t)n * 24u * c.bins, spent,
                                (size_t)n * 4u, "hipMemcpy of the spent shares"};
        return trt::sample_query_on_host(s, n, h, c.ra.accumulate != 0u, c.nothing(), "passes query buffers", "passes query launch", stats,
                                         [&](const trt::QueryScene& qs, const trt::SampleDev& d) {
                                             return trt::launch_passes(qs, c, d.items, n, d.sums, d.sums2, d.counters, nullptr);
                                         });
    });
}

// How launch_passes would launch n items on this scene with this many depth bins.
int trt_passes_launch_plan(const trt_scene* s, uint32_t n, uint32_t depth_bins, uint32_t compute_units, trt_query_plan* out) {
    if (depth_bins < 1u || depth_bins > 4u) return trt::query_fail(TRT_ERR_INVALID_ARG, "depth_bins must be 1, 2, 3 or 4");
    return trt::batch_launch_plan(s, n, compute_units, trt::passes_table(depth_bins), trt::kPassesShapes, out);
}

}  // extern "C"
