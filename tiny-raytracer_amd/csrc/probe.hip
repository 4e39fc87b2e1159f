// probe.hip — probe queries: the radiance that arrives at caller-supplied points as a function of direction, projected onto real spherical
// harmonics (tinyrt.h trt_probe / trt_probe_device), written for gfx950 (CDNA4) only.
//
// A gather query (radiance.hip) folds the colours of an item's K device-drawn paths into ONE colour; a light probe or a directional
// lightmap texel keeps the directions: for item i and sample s the first ray is drawn uniformly over the sphere or over the hemisphere
// about the item's axis (gather_draw.h probe_ray, RNG stream (seed, first_stream + i * K + s, 1)), its path runs on stream (.., 0) exactly
// as a gather sample's does, and the colour c is folded against the basis at the ray's STORED direction d (Ray::new's second normalisation
// included):
//   t = b_k(d) * inv_K;   sh[k].ch = sh[k].ch + c.ch * t        for k < C = bands^2
// in sample order, one IEEE f32 operation per operator, in registers: a lane owns an item for all samples of the call, keeps d from the
// start step to the fold and writes the C x 3 sums once per item.  A sample whose first ray has a NaN component is traced and counted and
// folds nothing.
//
// The round loop is radiance_kernel's for LOBE_GATHER - refill, start, SHADE what is pending, WALK what is alive - in a kernel of its own:
// with the 3 C sums and d as further template-dependent state in radiance_kernel the twelve existing instantiations would have had to be
// shown unchanged instruction for instruction; a second kernel leaves radiance.hip's device code untouched by construction.  There is no
// walk code in this file: the kernel calls the entry points of rt_path.h with the dynamic LDS laid out as the queries lay it out (scene
// copy | leaf stack: threads x slots x 8 bytes; wave_run.h) and is launched by the rule of the queries (query_plan.h).
#include "gather_draw.h"
#include "host_stage.h"
#include "kernels.h"
#include "probe_call.h"
#include "query_plan.h"
#include "rt_path.h"
#include "scene_query.h"
#include "sh_basis.h"
#include "wave_run.h"

namespace trt {

static_assert(sizeof(trt_probe_params) == 96 && offsetof(trt_probe_params, domain) == 64 && offsetof(trt_probe_params, bands) == 68 &&
              offsetof(trt_probe_params, reserved) == 72, "trt_probe_params layout (tinyrt.h)");

struct ProbeArgs {
    const float* items;              // n x (point, axis), used as given
    float* sh;                       // n x coeffs x 3
    unsigned long long* counters;    // nullptr, or [CTR_SAMPLES], [CTR_RAYS] are added to
    uint32_t n, rays_per_wave;       // wave w owns items [w * rays_per_wave, ...)
    uint32_t slots, stragglers;      // as in query.hip QueryArgs
    uint32_t samples_per_item;       // K
    uint32_t first_stream;           // first_stream + n * K <= 2^32 (radiance_check): the stream index never wraps
    uint32_t hemisphere;             // 0: TRT_PROBE_SPHERE, 1: TRT_PROBE_HEMISPHERE; the same for every lane of the launch
    uint32_t coeffs;                 // coefficients stored per item, bands^2: 1, 4 or 9, at most the kernel's NC
};

// The fold of one sample (tinyrt.h): the real SH basis in the graphics convention at d (sh_basis.h, the one copy), each product and sum
// one f32 operation in the header's parenthesisation.  NC = 4 evaluates bands 0 and 1 only.
template <int NC>
TRT_DEV void probe_fold(float (&acc)[3 * NC], const V3& d, const V3& c, float inv_k) {
    float b[NC];
    sh_basis<NC>(b, d);
#pragma unroll
    for (int k = 0; k < NC; k++) {
        const float t = b[k] * inv_k;
        acc[3 * k + 0] = acc[3 * k + 0] + c.x * t;
        acc[3 * k + 1] = acc[3 * k + 1] + c.y * t;
        acc[3 * k + 2] = acc[3 * k + 2] + c.z * t;
    }
}

// ra.sample_begin < ra.sample_end and ra.max_bounces > 0 (launch_probe: nothing to trace launches query_plan.h batch_zero or nothing)
template <int MODE, int WALK, int THREADS, int MINW, int NC>
__global__ __launch_bounds__(THREADS, MINW) void probe_kernel(SceneDev scd, RenderArgs ra, ProbeArgs ga, const float4* __restrict__ leaf_list,
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
    float acc[3 * NC];
#pragma unroll
    for (int k = 0; k < 3 * NC; k++) acc[k] = 0.0f;
    V3 d = v3(0.0f, 0.0f, 0.0f);                                            // the first ray's stored direction; d.x is NaN where the sample folds nothing
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
                const float* const a = ga.sh + 3ull * ga.coeffs * idx;      // idx < n: within [0, 3 * coeffs * n)
#pragma unroll
                for (int k = 0; k < NC; k++) {
                    const bool read = ra.accumulate && (uint32_t)k < ga.coeffs;       // wave-uniform
                    acc[3 * k + 0] = read ? a[3 * k + 0] : 0.0f;
                    acc[3 * k + 1] = read ? a[3 * k + 1] : 0.0f;
                    acc[3 * k + 2] = read ? a[3 * k + 2] : 0.0f;
                }
                own = true;
            }
            cursor = wave_advance(cursor, need, count);
        }
        if (__builtin_amdgcn_ballot_w64(own) == 0ull) break;                // every lane is free and none could take an item: the run is done
        if (own) {
            // ---- start: the item's next sample draws its first ray (stream (seed, j, 1)); the path starts fresh on (seed, j, 0) ----
            if (!has_path) {
                const uint32_t stream = ga.first_stream + idx * ga.samples_per_item + s;
                Rng g = rng_seed(ra.seed_key, stream, 1u);
                p.ray = probe_ray(items, idx, ga.hemisphere != 0u, g);
                p.rng = rng_seed(ra.seed_key, stream, 0u);
                d = p.ray.d;
                // a NaN point: the sample is traced and counted and must fold nothing (a NaN direction says so by itself)
                if (p.ray.o.x != p.ray.o.x || p.ray.o.y != p.ray.o.y || p.ray.o.z != p.ray.o.z) d.x = __builtin_nanf("");
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
                    if (d.x == d.x && d.y == d.y && d.z == d.z) probe_fold<NC>(acc, d, p.color, ra.inv_spp);
                    has_path = false;
                    s += 1u;
                    if (s == ra.sample_end) {
                        float* const a = ga.sh + 3ull * ga.coeffs * idx;
#pragma unroll
                        for (int k = 0; k < NC; k++) {
                            if ((uint32_t)k < ga.coeffs) {                  // wave-uniform
                                a[3 * k + 0] = acc[3 * k + 0]; a[3 * k + 1] = acc[3 * k + 1]; a[3 * k + 2] = acc[3 * k + 2];
                            }
                        }
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

#define TRT_PROBE(MODE, WALK, THREADS, MINW, NC) \
    BatchKernel{reinterpret_cast<const void*>(&probe_kernel<MODE, WALK, THREADS, MINW, NC>), MODE, WALK, THREADS, MINW}
// The (scene mode, walk, workgroup shape) set of radiance.hip kGatherKernels, once for 4 coefficients (bands 1 and 2) and once for 9
// (bands 3).  A lane carries what a lane of the gather kernel carries plus d and the 3 NC sums: the launch bounds are the highest at which
// the instantiation uses no scratch memory and spills no vector register (profiles/probe_resource_usage.txt).  The plan reports the bound
// (kernel_waves_per_simd).
const BatchKernel kProbeKernels4[] = {
    TRT_PROBE(MODE_LDS, WALK_FLAT, 256, 5, 4),
    TRT_PROBE(MODE_LDS, WALK_LDS_STACK, 256, 5, 4),
    TRT_PROBE(MODE_LDS, WALK_LDS_STACK, 768, 5, 4),
    TRT_PROBE(MODE_LDS, WALK_REGS, 512, 6, 4),
    TRT_PROBE(MODE_GLOBAL, WALK_COMPACT, 256, 5, 4),
    TRT_PROBE(MODE_GLOBAL, WALK_REGS, 256, 6, 4),
};
const BatchKernel kProbeKernels9[] = {
    TRT_PROBE(MODE_LDS, WALK_FLAT, 256, 4, 9),
    TRT_PROBE(MODE_LDS, WALK_LDS_STACK, 256, 5, 9),
    TRT_PROBE(MODE_LDS, WALK_LDS_STACK, 768, 5, 9),
    TRT_PROBE(MODE_LDS, WALK_REGS, 512, 4, 9),
    TRT_PROBE(MODE_GLOBAL, WALK_COMPACT, 256, 4, 9),
    TRT_PROBE(MODE_GLOBAL, WALK_REGS, 256, 4, 9),
};
#undef TRT_PROBE
constexpr size_t kProbeShapes = sizeof(kProbeKernels9) / sizeof(kProbeKernels9[0]);
static_assert(sizeof(kProbeKernels4) == sizeof(kProbeKernels9), "one instantiation per shape and coefficient count");
const BatchKernel* probe_table(uint32_t bands) { return bands == 3u ? kProbeKernels9 : kProbeKernels4; }

hipError_t launch_probe(const QueryScene& qs, const ProbeCall& c, const float* d_items, uint32_t n, float* d_sh, unsigned long long* d_counters,
                        hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (c.nothing()) {
        // nothing to trace: a path with no bounce budget returns colour 0 (cpu.rs:43-47,64); the sums start at 0, or stay
        if (c.ra.accumulate) return hipSuccess;
        return batch_zero(d_sh, 3ull * c.coeffs() * n, nullptr, 0ull, stream);
    }
    SceneDev scd = qs.scene;
    BatchLaunch b;
    const hipError_t e = batch_prepare(scd, n, probe_table(c.bands), kProbeShapes, b);
    if (e != hipSuccess) return e;
    const trt_query_plan& q = b.q;
    RenderArgs ra = c.ra;
    ra.flat_reuse = qs.flat_reuse;
    ProbeArgs ga{d_items, d_sh, d_counters, n, q.rays_per_wave, q.leaf_slots, q.stragglers, c.samples_per_item, c.first_stream, c.hemisphere, c.coeffs()};
    void* args[] = {&scd, &ra, &ga, &b.leaf_list, &b.nodes16};
    return batch_launch(b, args, stream);
}

}  // namespace

// What both forms check before any device work (probe_call.h: project.hip's trt_probe_parallel applies the same): trt_radiance's rules
// on p->path (radiance.hip radiance_check), then this struct's fields.
int probe_check(const trt_scene* s, const trt_ray* items, uint32_t n, const trt_probe_params* p, const float* sh, ProbeCall& c) {
    if (!p) return query_fail(TRT_ERR_INVALID_ARG, "null argument");
    const int rc = radiance_check(s, items, n, &p->path, sh, c.ra);
    if (rc != TRT_OK) return rc;
    if (p->domain != TRT_PROBE_SPHERE && p->domain != TRT_PROBE_HEMISPHERE)
        return query_fail(TRT_ERR_INVALID_ARG, "domain must be TRT_PROBE_SPHERE or TRT_PROBE_HEMISPHERE");
    if (p->bands < 1u || p->bands > 3u) return query_fail(TRT_ERR_INVALID_ARG, "bands must be 1, 2 or 3");
    for (uint32_t r : p->reserved)
        if (r != 0u) return query_fail(TRT_ERR_INVALID_ARG, "reserved words must be zero");
    c.samples_per_item = p->path.samples_per_ray;
    c.first_stream = p->path.first_stream;
    c.hemisphere = p->domain == TRT_PROBE_HEMISPHERE ? 1u : 0u;
    c.bands = p->bands;
    return TRT_OK;
}

}  // namespace trt

extern "C" {

void trt_probe_params_default(trt_probe_params* out) {
    if (!out) return;
    *out = trt_probe_params{};
    trt_radiance_params_default(&out->path);
    out->domain = TRT_PROBE_SPHERE;
    out->bands = 3u;
}

int trt_probe_device(trt_scene* s, const trt_ray* d_items, uint32_t n, const trt_probe_params* p, float* d_sh, uint64_t* d_counters, void* stream) {
    trt::ProbeCall c;
    const int rc = trt::probe_check(s, d_items, n, p, d_sh, c);
    if (rc != TRT_OK) return rc;
    return trt::sample_query_on_device(s, n, "probe query launch", [&](const trt::QueryScene& qs) {
        return trt::launch_probe(qs, c, reinterpret_cast<const float*>(d_items), n, d_sh, reinterpret_cast<unsigned long long*>(d_counters),
                                 static_cast<hipStream_t>(stream));
    });
}

// Host buffers: staged by host_stage.h sample_query_on_host (items | sums | counters; there is no second output).
int trt_probe(trt_scene* s, const trt_ray* items, uint32_t n, const trt_probe_params* p, float* sh, trt_stats* stats) {
    return trt::host_form([&]() -> int {
        trt::ProbeCall c;
        const int rc = trt::probe_check(s, items, n, p, sh, c);
        if (rc != TRT_OK) return rc;
        const trt::SampleHost h{items, (size_t)n * sizeof(trt_ray), "hipMemcpy of the items", nullptr, 0u, "", sh, (size_t)n * 12u * c.coeffs(), nullptr, 0u, ""};
        return trt::sample_query_on_host(s, n, h, c.ra.accumulate != 0u, c.nothing(), "probe query buffers", "probe query launch", stats,
                                         [&](const trt::QueryScene& qs, const trt::SampleDev& d) {
                                             return trt::launch_probe(qs, c, d.items, n, d.sums, d.counters, nullptr);
                                         });
    });
}

// How launch_probe would launch n items on this scene with this many bands.
int trt_probe_launch_plan(const trt_scene* s, uint32_t n, uint32_t bands, uint32_t compute_units, trt_query_plan* out) {
    if (bands < 1u || bands > 3u) return trt::query_fail(TRT_ERR_INVALID_ARG, "bands must be 1, 2 or 3");
    return trt::batch_launch_plan(s, n, compute_units, trt::probe_table(bands), trt::kProbeShapes, out);
}

}  // extern "C"
