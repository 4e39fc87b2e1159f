// radiance.hip — radiance queries: path tracing of caller-supplied rays (tinyrt.h trt_radiance / trt_radiance_device), and gather
// queries: the same from device-drawn rays about caller-supplied surfels (trt_gather / trt_gather_device), written for gfx950 (CDNA4) only.
//
// The ray queries (query.hip) answer "what does this ray hit" for any ray; this unit answers "what light arrives along it": for ray i and
// sample s the colour of CpuSampler::single_point_sampling (cpu.rs:39-65) for the ray as given, with RNG stream
// (seed, first_stream + i * K + s, 0) - trt_sample_batch's numbering opened by an offset, so that every sample can be checked against the
// oracle's restatement of that entry point on a list with each ray repeated K times - folded per ray with the imager's rule
//   radiance.ch = radiance.ch + c.ch * inv_K;   moment2.ch = moment2.ch + (c.ch * c.ch) * inv_K
// in sample order, one IEEE f32 operation per operator, in registers: a lane owns a ray for all samples of the call (pixels.hip's loop).
//
// There is no walk code in this file and no render kernel is touched: the kernel calls the entry points of rt_path.h with the dynamic LDS
// laid out as the queries lay it out (scene copy | leaf stack: threads x slots x 8 bytes; the run, the place of the stack and the refill's
// cursor step are wave_run.h's) and is launched by the rule of the queries (query_plan.h): a wave owns a contiguous run of the rays.
//
// Work: the wave runs in rounds - refill, start, SHADE what is pending, WALK what is alive.  A walk that ended in a round leaves its
// (primitive, t) pending and is shaded at the top of the next, so shade_hit stays one call site.  The first segment of a ray is walked
// once per ray and call, not once per sample (every walk but the lock-step list, where the two registers cost an occupancy step and
// each sample walks): the closest hit of the caller's ray depends on nothing a sample draws, so when a ray's
// first walk ends its (primitive, t) is kept in two registers and every later sample of that ray starts with it pending.  shade_hit
// then receives the arguments a walk of its own would have given it, hence the same bits; the reference's world.hit call for that
// segment (cpu.rs:48) is still counted once per sample.  TRT_RADIANCE_PLAIN_WALK = 1 builds the form in which every sample walks its
// first segment (the A/B of tools/radiance_bench.py).
//
// Gather queries (tinyrt.h trt_gather / trt_gather_device) are the same kernel with LOBE != 0: an item is a surfel (point, axis), and the
// start step DRAWS the sample's first ray about the axis - Lambertian::scatter's rule (cosine lobe) or Metal::scatter's with the axis as
// the mirror direction (cone lobe), from stream (seed, j, 1) - where a radiance query loads it; the path then runs on stream (seed, j, 0)
// as above.  The first segment differs per sample, so nothing of it is shared.
#include "gather_draw.h"
#include "kernels.h"
#include "query_plan.h"
#include "rt_path.h"
#include "scene_query.h"
#include "wave_run.h"

#ifndef TRT_RADIANCE_PLAIN_WALK
#define TRT_RADIANCE_PLAIN_WALK 0
#endif

namespace trt {

static_assert(sizeof(trt_radiance_params) == 64, "trt_radiance_params layout (tinyrt.h)");
static_assert(sizeof(trt_gather_params) == 96, "trt_gather_params layout (tinyrt.h)");

struct RadianceArgs {
    const float* rays;               // n x (origin, direction), used as given
    float* radiance;                 // n x 3
    float* moment2;                  // n x 3, or nullptr: not wanted
    unsigned long long* counters;    // nullptr, or [CTR_SAMPLES], [CTR_RAYS] are added to
    uint32_t n, rays_per_wave;       // wave w owns rays [w * rays_per_wave, ...)
    uint32_t slots, stragglers;      // as in query.hip QueryArgs
    uint32_t samples_per_ray;        // K
    uint32_t first_stream;           // first_stream + n * K <= 2^32 (radiance_check): the stream index never wraps
};
// The gather kernels' arguments: RadianceArgs and the lobe.  A derived struct, not two more fields above: a longer RadianceArgs moves the
// kernel arguments behind it, and with them the scalar loads of every LOBE == 0 instantiation.
struct GatherArgs : RadianceArgs {
    uint32_t lobe;                   // TRT_LOBE_COSINE or TRT_LOBE_CONE (gather_check): the same for every lane of the launch
    float spread;                    // the cone lobe's sphere radius
};
constexpr int LOBE_NONE = 0, LOBE_GATHER = 1;   // radiance_kernel's LOBE: the items are rays | surfels, the lobe is GatherArgs::lobe
template <int LOBE> struct RadianceArgsOf { using type = RadianceArgs; };
template <> struct RadianceArgsOf<LOBE_GATHER> { using type = GatherArgs; };

// (rad_load_ray and gather_ray, the item load and the draw of a gather sample: gather_draw.h, shared with ambient.hip)

// ra.sample_begin < ra.sample_end and ra.max_bounces > 0 (launch_radiance: nothing to trace launches the zero kernel or nothing)
template <int MODE, int WALK, int THREADS, int MINW, int LOBE>
__global__ __launch_bounds__(THREADS, MINW) void radiance_kernel(SceneDev scd, RenderArgs ra, typename RadianceArgsOf<LOBE>::type ga,
                                                                      const float4* __restrict__ leaf_list, const uint4* __restrict__ nodes16) {
    stage_scene_to_lds<MODE>(scd);
    const FlatReuse flat_reuse = axis_quads_to_lds<MODE, false, WALK>(scd, ra.flat_reuse);
    const SceneAcc<MODE> sc{scd.blob, scd.L};
    const float* __restrict__ const rays = ga.rays;
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
    // the first segment is walked once per ray where keeping its (primitive, t) costs no occupancy: every walk but the lock-step list;
    // a gather sample draws its own first segment
    constexpr bool kShareFirst = !TRT_RADIANCE_PLAIN_WALK && WALK != WALK_FLAT && LOBE == LOBE_NONE;

    uint32_t cursor = 0;                                                    // wave-uniform
    bool own = false, has_path = false, walking = false;                    // the lane owns a ray; a path of it is under way; its walk is parked
    bool pending = false, have_first = false;                               // a finished walk waits for its shade; the ray's first hit is known
    uint32_t idx = 0, s = 0;
    uint32_t hit_prim = PRIM_NONE, first_prim = PRIM_NONE;
    float hit_t = 0.0f, first_t = 0.0f;
    uint32_t n_samples = 0, n_rays = 0;
    V3 acc = v3(0.0f, 0.0f, 0.0f), m2 = v3(0.0f, 0.0f, 0.0f);
    Path p;
    p.ray.o = v3(0.0f, 0.0f, 0.0f); p.ray.d = v3(0.0f, 0.0f, 0.0f);
    p.color = v3(0.0f, 0.0f, 0.0f); p.atten = v3(0.0f, 0.0f, 0.0f);
    p.remain = 0u;
    p.rng.s0 = 0u; p.rng.s1 = 0u;
    for (;;) {
        // ---- refill: every lane without a ray takes the next one of the run (begin + item < n: item < count <= n - begin) ----
        const uint64_t need = __builtin_amdgcn_ballot_w64(!own);
        if (need != 0ull && cursor < count) {
            const uint32_t item = cursor + wave_rank(need);
            if (!own && item < count) {
                idx = begin + item;
                s = ra.sample_begin;
                if (ra.accumulate) {
                    const float* const a = ga.radiance + 3ull * idx;
                    acc = v3(a[0], a[1], a[2]);
                    if (ga.moment2) { const float* const m = ga.moment2 + 3ull * idx; m2 = v3(m[0], m[1], m[2]); }
                } else {
                    acc = v3(0.0f, 0.0f, 0.0f);
                    m2 = v3(0.0f, 0.0f, 0.0f);
                }
                have_first = false;
                own = true;
            }
            cursor = wave_advance(cursor, need, count);
        }
        if (__builtin_amdgcn_ballot_w64(own) == 0ull) break;                // every lane is free and none could take a ray: the run is done
        if (own) {
            // ---- start: the ray's next sample (cpu.rs:42-45 with the caller's ray; no primary-ray draws) ----
            if (!has_path) {
                const uint32_t stream = ga.first_stream + idx * ga.samples_per_ray + s;
                if constexpr (LOBE == LOBE_NONE) {
                    p.rng = rng_seed(ra.seed_key, stream, 0u);
                    p.ray = rad_load_ray(rays, idx);                        // re-read: 24 bytes per sample against six registers per lane
                } else {
                    // the surfel is re-read like a ray; its draw has a stream of its own (sample index 1), the path starts fresh at 0
                    Rng g = rng_seed(ra.seed_key, stream, 1u);
                    p.ray = gather_ray(rays, idx, ga.lobe, ga.spread, g);
                    p.rng = rng_seed(ra.seed_key, stream, 0u);
                }
                p.color = v3(0.0f, 0.0f, 0.0f);
                p.atten = v3(1.0f, 1.0f, 1.0f);
                p.remain = ra.max_bounces;
                has_path = true;
                n_samples++;
                if (have_first) {                                           // the first segment's walk, done once for the ray
                    hit_prim = first_prim; hit_t = first_t;
                    pending = true;
                    n_rays++;                                               // the reference's world.hit of this sample (cpu.rs:48)
                }
            }
            // ---- shade what is pending ----
            if (pending) {
                pending = false;
                if (shade_hit<MODE, false>(sc, p, hit_prim, hit_t, background, ctr)) {
                    // imager.rs:35,50 and the second moment beside it, in the operation order of pixels_kernel
                    acc = acc + p.color * ra.inv_spp;
                    m2.x = m2.x + (p.color.x * p.color.x) * ra.inv_spp;
                    m2.y = m2.y + (p.color.y * p.color.y) * ra.inv_spp;
                    m2.z = m2.z + (p.color.z * p.color.z) * ra.inv_spp;
                    has_path = false;
                    s += 1u;
                    if (s == ra.sample_end) {
                        float* const a = ga.radiance + 3ull * idx;
                        a[0] = acc.x; a[1] = acc.y; a[2] = acc.z;
                        if (ga.moment2) { float* const m = ga.moment2 + 3ull * idx; m[0] = m2.x; m[1] = m2.y; m[2] = m2.z; }
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
                if (done) {
                    pending = true;
                    if constexpr (kShareFirst) {
                        if (p.remain == ra.max_bounces) { first_prim = hit_prim; first_t = hit_t; have_first = true; }  // the caller's ray itself
                    }
                }
            }
        }
    }
    flush_counters<false>(ga.counters, n_samples, n_rays, ctr);
}

// Nothing to trace (an empty sample range, max_bounces == 0) without accumulate: the sums become 0.  The ONE zero kernel of the sample
// queries (query_plan.h batch_zero): n_a floats of a, and n_b floats of b where b is wanted.
__global__ __launch_bounds__(256) void sums_zero_kernel(float* __restrict__ a, unsigned long long n_a, float* __restrict__ b, unsigned long long n_b) {
    const unsigned long long i = blockIdx.x * 256ull + threadIdx.x;
    if (i < n_a) a[i] = 0.0f;
    if (b && i < n_b) b[i] = 0.0f;
}
hipError_t batch_zero(float* d_a, unsigned long long n_a, float* d_b, unsigned long long n_b, hipStream_t stream) {
    const unsigned long long floats = d_b && n_b > n_a ? n_b : n_a;
    if (floats == 0ull) return hipSuccess;
    hipLaunchKernelGGL(sums_zero_kernel, dim3((uint32_t)((floats + 255ull) / 256ull)), dim3(256), 0, stream, d_a, n_a, d_b, n_b);
    return hipGetLastError();
}

namespace {

#define TRT_RADIANCE(MODE, WALK, THREADS, MINW, LOBE) \
    BatchKernel{reinterpret_cast<const void*>(&radiance_kernel<MODE, WALK, THREADS, MINW, LOBE>), MODE, WALK, THREADS, MINW}
// the (scene mode, walk, workgroup shape) set of the sparse render's table, with the register-slot fallback (query_plan.h), so that every
// scene has a kernel.  A lane carries what a lane of pixels_kernel carries plus the pending and the first (primitive, t): the launch
// bounds are the highest at which the instantiation uses no scratch memory (profiles/radiance_resource_usage.txt).  The plan reports
// the bound (kernel_waves_per_simd).  The lock-step list keeps no first (primitive, t) (kShareFirst): with it that instantiation needs 76
// registers and drops from 7 waves per SIMD to 6; without it all six shapes run at 7.
const BatchKernel kRadianceKernels[] = {
    TRT_RADIANCE(MODE_LDS, WALK_FLAT, 256, 7, LOBE_NONE),
    TRT_RADIANCE(MODE_LDS, WALK_LDS_STACK, 256, 7, LOBE_NONE),
    TRT_RADIANCE(MODE_LDS, WALK_LDS_STACK, 768, 7, LOBE_NONE),
    TRT_RADIANCE(MODE_LDS, WALK_REGS, 512, 7, LOBE_NONE),
    TRT_RADIANCE(MODE_GLOBAL, WALK_COMPACT, 256, 7, LOBE_NONE),
    TRT_RADIANCE(MODE_GLOBAL, WALK_REGS, 256, 7, LOBE_NONE),
};
// The gather queries' table: the same six shapes, one instantiation each.  The lobe is a kernel argument, not a template parameter: it is
// the same for every lane of a launch, so the choice is a scalar branch around a few vector instructions of the start step, the draw
// itself is shared by both lobes as it is in shade_hit, and six more instantiations would buy nothing the register report shows - a lane
// carries what a lane of the LOBE_NONE kernel carries less the first (primitive, t), and the draw's temporaries die before the walk; with
// the lobe fixed at compile time every shape reports the registers it reports here.  Five shapes run at 7 waves per SIMD without scratch.
// The lock-step list needs 74 registers, two more than 7 waves allow (the LOBE_NONE one needs exactly 72): at 7 the compiler spills two
// in the leaf loop, so its bound is 6 (profiles/gather_resource_usage.txt; the render's lock-step kernel measured no slower at 6 than at 7,
// profiles/r02_cornell_waves_sweep.txt).
const BatchKernel kGatherKernels[] = {
    TRT_RADIANCE(MODE_LDS, WALK_FLAT, 256, 6, LOBE_GATHER),
    TRT_RADIANCE(MODE_LDS, WALK_LDS_STACK, 256, 7, LOBE_GATHER),
    TRT_RADIANCE(MODE_LDS, WALK_LDS_STACK, 768, 7, LOBE_GATHER),
    TRT_RADIANCE(MODE_LDS, WALK_REGS, 512, 7, LOBE_GATHER),
    TRT_RADIANCE(MODE_GLOBAL, WALK_COMPACT, 256, 7, LOBE_GATHER),
    TRT_RADIANCE(MODE_GLOBAL, WALK_REGS, 256, 7, LOBE_GATHER),
};
#undef TRT_RADIANCE
constexpr size_t kRadianceShapes = sizeof(kRadianceKernels) / sizeof(kRadianceKernels[0]);
static_assert(sizeof(kGatherKernels) == sizeof(kRadianceKernels), "one gather instantiation per radiance shape");

hipError_t launch_radiance(const QueryScene& qs, RenderArgs ra, const float* d_rays, uint32_t n, uint32_t samples_per_ray, uint32_t first_stream,
                           float* d_radiance, float* d_moment2, unsigned long long* d_counters, hipStream_t stream, Lobe lobe = Lobe{0u, 0.0f}) {
    if (n == 0) return hipSuccess;
    if (ra.sample_begin == ra.sample_end || ra.max_bounces == 0) {
        // nothing to trace: a path with no bounce budget returns colour 0 (cpu.rs:43-47,64); the sums start at 0, or stay
        if (ra.accumulate) return hipSuccess;
        return batch_zero(d_radiance, 3ull * n, d_moment2, 3ull * n, stream);
    }
    SceneDev scd = qs.scene;
    BatchLaunch b;
    const hipError_t e = batch_prepare(scd, n, lobe.lobe ? kGatherKernels : kRadianceKernels, kRadianceShapes, b);
    if (e != hipSuccess) return e;
    const trt_query_plan& q = b.q;
    ra.flat_reuse = qs.flat_reuse;
    // a radiance kernel reads the RadianceArgs in front, a gather kernel all of it
    GatherArgs ga{{d_rays, d_radiance, d_moment2, d_counters, n, q.rays_per_wave, q.leaf_slots, q.stragglers, samples_per_ray, first_stream},
                  lobe.lobe, lobe.spread};
    void* args[] = {&scd, &ra, &ga, &b.leaf_list, &b.nodes16};
    return batch_launch(b, args, stream);
}

// The device form of both queries, after the checks (host_stage.h sample_query_on_device).
int radiance_on_device(trt_scene* s, const RenderArgs& ra, const trt_radiance_params& p, Lobe lobe, const trt_ray* d_rays, uint32_t n, float* d_radiance,
                       float* d_moment2, uint64_t* d_counters, void* stream, const char* what) {
    return sample_query_on_device(s, n, what, [&](const QueryScene& qs) {
        return launch_radiance(qs, ra, reinterpret_cast<const float*>(d_rays), n, p.samples_per_ray, p.first_stream, d_radiance, d_moment2,
                               reinterpret_cast<unsigned long long*>(d_counters), static_cast<hipStream_t>(stream), lobe);
    });
}

// The host form of both queries, after the checks (inside host_form; host_stage.h sample_query_on_host).
int radiance_on_host(trt_scene* s, const RenderArgs& ra, const trt_radiance_params& p, Lobe lobe, const trt_ray* rays, uint32_t n, float* radiance,
                     float* moment2, trt_stats* stats, const char* buffers, const char* launch) {
    const size_t sums = (size_t)n * 12u;
    const SampleHost h{rays, (size_t)n * sizeof(trt_ray), "hipMemcpy of the rays", nullptr, 0u, "", radiance, sums, moment2, sums,
                       "hipMemcpy of the second moments"};
    const bool nothing = ra.sample_begin == ra.sample_end || ra.max_bounces == 0u;
    return sample_query_on_host(s, n, h, ra.accumulate != 0u, nothing, buffers, launch, stats, [&](const QueryScene& qs, const SampleDev& d) {
        return launch_radiance(qs, ra, d.items, n, p.samples_per_ray, p.first_stream, d.sums, d.sums2, d.counters, nullptr, lobe);
    });
}

}  // namespace

// The rules that more than one unit applies to its parameters (declared in gather_draw.h).  The source, spread and reserved words of a
// trt_gather_params whose lobe word is an enum trt_passes_source (passes.hip, nee.hip):
int gather_source_check(const trt_gather_params& g) {
    if (g.lobe != TRT_PASSES_RAYS && g.lobe != TRT_PASSES_COSINE && g.lobe != TRT_PASSES_CONE)
        return query_fail(TRT_ERR_INVALID_ARG, "source must be TRT_PASSES_RAYS, TRT_PASSES_COSINE or TRT_PASSES_CONE");
    if (g.lobe == TRT_PASSES_CONE && !(g.spread >= 0.0f && g.spread < __builtin_inff()))
        return query_fail(TRT_ERR_INVALID_ARG, "spread of the cone lobe must be finite and not negative");
    for (uint32_t r : g.reserved)
        if (r != 0u) return query_fail(TRT_ERR_INVALID_ARG, "reserved words must be zero");
    return TRT_OK;
}
// the emitter table's pointer and size and the shadow ray's end (direct.hip, nee.hip), for both forms
int emitter_table_check(uint32_t n, const trt_emitter* emitters, uint32_t n_emitters, float shadow_end) {
    constexpr uint32_t kMaxEmitters = 1u << 20;
    if (n > 0u && !emitters) return query_fail(TRT_ERR_INVALID_ARG, "null emitter table");
    if (n > 0u && (n_emitters < 1u || n_emitters > kMaxEmitters)) return query_fail(TRT_ERR_INVALID_ARG, "n_emitters must be in 1 .. 2^20");
    if (!(shadow_end > 0.0f && shadow_end <= 1.0f)) return query_fail(TRT_ERR_INVALID_ARG, "shadow_end must be in (0, 1]");
    return TRT_OK;
}
// and the table's entries, which are the host form's to check: the device form cannot read them
int emitter_entries_check(const trt_emitter* emitters, uint32_t n_emitters) {
    for (uint32_t k = 0; k < n_emitters; k++) {
        if (emitters[k].kind > 1u) return query_fail(TRT_ERR_INVALID_ARG, "emitter kind must be 0 (sphere) or 1 (quad)");
        if (emitters[k].reserved[0] != 0u || emitters[k].reserved[1] != 0u)
            return query_fail(TRT_ERR_INVALID_ARG, "reserved words of an emitter must be zero");
    }
    return TRT_OK;
}

// What both forms check before any device work, and the kernel arguments of the parameters (declared in gather_draw.h: the probe queries
// apply the same rules to their path).
int radiance_check(const trt_scene* s, const trt_ray* rays, uint32_t n, const trt_radiance_params* p, const float* radiance, RenderArgs& ra) {
    if (!s || !p) return query_fail(TRT_ERR_INVALID_ARG, "null argument");
    if (n > 0u && (!rays || !radiance)) return query_fail(TRT_ERR_INVALID_ARG, "null buffer");
    const uint32_t K = p->samples_per_ray;
    if (K == 0u) return query_fail(TRT_ERR_INVALID_ARG, "samples_per_ray must be positive");
    const uint32_t s1 = p->sample_end == 0u ? K : p->sample_end;
    if (p->sample_begin > s1 || s1 > K) return query_fail(TRT_ERR_INVALID_ARG, "sample range must satisfy begin <= end <= samples_per_ray");
    for (uint32_t r : p->reserved)
        if (r != 0u) return query_fail(TRT_ERR_INVALID_ARG, "reserved words must be zero");
    // the last stream index, first_stream + n * K - 1, must fit 32 bits (n * K < 2^64: both are below 2^32)
    if ((unsigned long long)p->first_stream + (unsigned long long)n * K > 0x100000000ull)
        return query_fail(TRT_ERR_INVALID_ARG, "first_stream + n * samples_per_ray exceeds 2^32 RNG streams");
    ra = RenderArgs{};
    ra.background[0] = p->background.x; ra.background[1] = p->background.y; ra.background[2] = p->background.z;
    ra.inv_spp = 1.0f / (float)K;
    ra.max_bounces = p->max_bounces;
    ra.seed_key = rng_seed_key(p->seed);
    ra.sample_begin = p->sample_begin;
    ra.sample_end = s1;
    ra.accumulate = p->accumulate ? 1u : 0u;
    return TRT_OK;
}

// What the gather forms check before any device work: trt_radiance's rules on p->path, then the lobe (gather_draw.h: ambient.hip
// applies the same rules to its own trt_gather_params).
int gather_check(const trt_scene* s, const trt_ray* items, uint32_t n, const trt_gather_params* p, const float* radiance, RenderArgs& ra, Lobe& lobe) {
    if (!p) return query_fail(TRT_ERR_INVALID_ARG, "null argument");
    const int rc = radiance_check(s, items, n, &p->path, radiance, ra);
    if (rc != TRT_OK) return rc;
    if (p->lobe != TRT_LOBE_COSINE && p->lobe != TRT_LOBE_CONE) return query_fail(TRT_ERR_INVALID_ARG, "lobe must be TRT_LOBE_COSINE or TRT_LOBE_CONE");
    if (p->lobe == TRT_LOBE_CONE && !(p->spread >= 0.0f && p->spread < __builtin_inff()))
        return query_fail(TRT_ERR_INVALID_ARG, "spread of the cone lobe must be finite and not negative");
    for (uint32_t r : p->reserved)
        if (r != 0u) return query_fail(TRT_ERR_INVALID_ARG, "reserved words must be zero");
    lobe = Lobe{p->lobe, p->spread};
    return TRT_OK;
}

}  // namespace trt

extern "C" {

void trt_radiance_params_default(trt_radiance_params* out) {
    if (!out) return;
    *out = trt_radiance_params{};
    out->samples_per_ray = 1u;
    out->max_bounces = 50u;
    out->seed = 1u;
}

int trt_radiance_device(trt_scene* s, const trt_ray* d_rays, uint32_t n, const trt_radiance_params* p, float* d_radiance, float* d_moment2,
                        uint64_t* d_counters, void* stream) {
    trt::RenderArgs ra;
    const int rc = trt::radiance_check(s, d_rays, n, p, d_radiance, ra);
    if (rc != TRT_OK) return rc;
    return trt::radiance_on_device(s, ra, *p, trt::Lobe{0u, 0.0f}, d_rays, n, d_radiance, d_moment2, d_counters, stream, "radiance query launch");
}

int trt_radiance(trt_scene* s, const trt_ray* rays, uint32_t n, const trt_radiance_params* p, float* radiance, float* moment2, trt_stats* stats) {
    return trt::host_form([&]() -> int {
        trt::RenderArgs ra;
        const int rc = trt::radiance_check(s, rays, n, p, radiance, ra);
        if (rc != TRT_OK) return rc;
        return trt::radiance_on_host(s, ra, *p, trt::Lobe{0u, 0.0f}, rays, n, radiance, moment2, stats, "radiance query buffers", "radiance query launch");
    });
}

// How launch_radiance would launch n rays on this scene.
int trt_radiance_launch_plan(const trt_scene* s, uint32_t n, uint32_t compute_units, trt_query_plan* out) {
    return trt::batch_launch_plan(s, n, compute_units, trt::kRadianceKernels, trt::kRadianceShapes, out);
}

void trt_gather_params_default(trt_gather_params* out) {
    if (!out) return;
    *out = trt_gather_params{};
    trt_radiance_params_default(&out->path);
    out->lobe = TRT_LOBE_COSINE;
}

int trt_gather_device(trt_scene* s, const trt_ray* d_items, uint32_t n, const trt_gather_params* p, float* d_radiance, float* d_moment2,
                      uint64_t* d_counters, void* stream) {
    trt::RenderArgs ra;
    trt::Lobe lobe;
    const int rc = trt::gather_check(s, d_items, n, p, d_radiance, ra, lobe);
    if (rc != TRT_OK) return rc;
    return trt::radiance_on_device(s, ra, p->path, lobe, d_items, n, d_radiance, d_moment2, d_counters, stream, "gather query launch");
}

int trt_gather(trt_scene* s, const trt_ray* items, uint32_t n, const trt_gather_params* p, float* radiance, float* moment2, trt_stats* stats) {
    return trt::host_form([&]() -> int {
        trt::RenderArgs ra;
        trt::Lobe lobe;
        const int rc = trt::gather_check(s, items, n, p, radiance, ra, lobe);
        if (rc != TRT_OK) return rc;
        return trt::radiance_on_host(s, ra, p->path, lobe, items, n, radiance, moment2, stats, "gather query buffers", "gather query launch");
    });
}

// How launch_radiance would launch n surfels on this scene.
int trt_gather_launch_plan(const trt_scene* s, uint32_t n, uint32_t compute_units, trt_query_plan* out) {
    return trt::batch_launch_plan(s, n, compute_units, trt::kGatherKernels, trt::kRadianceShapes, out);
}

}  // extern "C"
