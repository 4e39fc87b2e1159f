// nee_samples.hip — sample-parallel next-event queries: every sample's colour and first direction for the four next-event queries
// (tinyrt.h trt_nee_samples / trt_nee_samples_device), written for gfx950 (CDNA4) only.
//
// nee.hip's kernels let a lane own an ITEM for all K samples of the call, so the launch rule gives a wave 256 items whatever K is, and a
// caller never sees a sample.  Here a lane owns one SAMPLE, as in samples.hip: the call's work is the n x R samples of the range, work
// index q = (item, sample) by sample_index.h, a wave owns a contiguous run of q (query_plan.h's rule with n x R in the place of n), and a
// finished path stores its colour at record i * K + s and frees the lane.  trt_fold_samples (samples.hip) turns the records into the
// bytes of trt_nee / trt_nee_mis / trt_nee_pick / trt_nee_mis_pick: nee_kernel's fold is trt_radiance's, operator for operator.
//
// The kernel is samples_kernel's round loop with nee_kernel's shade and next-event block in the place of shade_hit.  Of nee_kernel's lane
// the sums, the sample counter and the item index are gone (acc, m2, s, idx: eight registers); what a shadow ray needs stays (sh_d, sh_t,
// sh_c, shadow, after_diffuse, csh for MIS).  There is ONE walk call site, as in nee_kernel: a round walks the lane's shadow ray if one
// is outstanding, else its path ray, through the same closest_hit / closest_hit_resume call with a per-lane first t_best.  The colour is
// stored where the shade ends the path, after the weighted light term; the lane is freed at the END of the round (samples.hip says why).
// The source is a kernel argument, as in samples_kernel: 2 (MIS) x 2 (PICK) x 6 shapes = 24 instantiations.
//
// The next-event block ("draw at a vertex, weigh, park the shadow ray") and the weighted light hit are RESTATED here, line for line from
// nee_kernel, and nee_kernel is left as it was: nee.hip's device assembly is the parent's.  The draws themselves
// (gather_draw.h direct_draw_at), the weights (mis_weight.h), the shade body and the walks (rt_path.h) are the one copy both call.  The
// host side - NeeCall, nee_check, the step lists - is nee_call.h's, shared with nee.hip.
#include "emitter_pick.h"
#include "emitter_query.h"
#include "gather_draw.h"
#include "host_stage.h"
#include "kernels.h"
#include "mis_weight.h"
#include "nee_call.h"
#include "query_plan.h"
#include "rt_path.h"
#include "sample_index.h"
#include "scene_query.h"
#include "wave_run.h"

namespace trt {

static_assert(sizeof(trt_nee_samples_params) == 192 && offsetof(trt_nee_samples_params, query) == 0 && offsetof(trt_nee_samples_params, weighted) == 160 &&
              offsetof(trt_nee_samples_params, total_power) == 164 && offsetof(trt_nee_samples_params, reserved) == 168,
              "trt_nee_samples_params layout (tinyrt.h)");

struct NeeSamplesArgs {
    const float* items;              // n x (origin, direction) or n x (point, axis), used as given
    const float* emitters;           // n_emitters x 20 words (trt_emitter)
    float* colors;                   // n x K x 3
    float* directions;               // n x K x 3, or nullptr: not wanted
    unsigned long long* counters;    // nullptr, or [CTR_SAMPLES], [CTR_RAYS] are added to
    uint32_t work, per_wave;         // n x R work indices (nee_samples_check: below 2^32); wave w owns [w * per_wave, ...)
    uint32_t slots, stragglers;      // as in query.hip QueryArgs
    uint32_t samples_per_item;       // K
    uint32_t first_stream;           // first_stream + n * K <= 2^32 (radiance_check): neither the record nor the stream index wraps
    uint32_t range_length;           // R = sample_end - sample_begin >= 1
    uint32_t source;                 // enum trt_passes_source: the same for every lane of the launch
    float spread;                    // the cone lobe's sphere radius
    uint32_t n_emitters;             // E: 1 .. 2^20
    float shadow_end;                // in (0, 1]
    uint32_t source_is_diffuse;      // after_diffuse at the first hit
    uint32_t heuristic;              // enum trt_mis_heuristic, wave-uniform (the MIS kernels; the others do not read it)
};
// What a PICK kernel is handed besides, in nee.hip NeePickArgs' shape: the alias table and the table's total power (the weighted
// kernels; the others do not read it).  A struct of its own, so that the uniform kernels' arguments lie where they lie without it.
struct NeeSamplesPickArgs {
    NeeSamplesArgs g;
    const float* pick;
    float total_power;
};
TRT_DEV const NeeSamplesArgs& nee_samples_args(const NeeSamplesArgs& a) { return a; }
TRT_DEV const NeeSamplesArgs& nee_samples_args(const NeeSamplesPickArgs& a) { return a.g; }
TRT_DEV const float* nee_samples_pick_table(const NeeSamplesArgs&) { return nullptr; }
TRT_DEV const float* nee_samples_pick_table(const NeeSamplesPickArgs& a) { return a.pick; }
TRT_DEV float nee_samples_pick_total(const NeeSamplesArgs&) { return 0.0f; }
TRT_DEV float nee_samples_pick_total(const NeeSamplesPickArgs& a) { return a.total_power; }

// ra.sample_begin < ra.sample_end and ra.max_bounces > 0 (launch_nee_samples: nothing to trace launches the range's zero kernel or nothing)
template <int MODE, int WALK, int THREADS, int MINW, bool MIS, bool PICK>
__global__ __launch_bounds__(THREADS, MINW) void nee_samples_kernel(SceneDev scd, RenderArgs ra,
                                                                         std::conditional_t<PICK, NeeSamplesPickArgs, NeeSamplesArgs> args,
                                                                         const float4* __restrict__ leaf_list, const uint4* __restrict__ nodes16) {
    const NeeSamplesArgs& ga = nee_samples_args(args);
    [[maybe_unused]] const float* __restrict__ const pick = nee_samples_pick_table(args);
    [[maybe_unused]] const float total_power = nee_samples_pick_total(args);
    stage_scene_to_lds<MODE>(scd);
    const FlatReuse flat_reuse = axis_quads_to_lds<MODE, false, WALK>(scd, ra.flat_reuse);
    const SceneAcc<MODE> sc{scd.blob, scd.L};
    const float* __restrict__ const items = ga.items;
    const float* __restrict__ const emitters = ga.emitters;
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long begin64 = wave_begin<THREADS>(ga.per_wave);
    if (begin64 >= ga.work) return;                                         // (after the barriers above)
    const uint32_t begin = (uint32_t)begin64;
    const uint32_t count = wave_count(ga.work, ga.per_wave, begin);
    // this lane's postponed-leaf stack: behind the scene copy, slots x 64 x 8 bytes per wave
    float2* const stack = WALK != WALK_REGS ? reinterpret_cast<float2*>(lds_behind_scene(sc)) + (threadIdx.x >> 6) * (64u * ga.slots) + lane : nullptr;
    const V3 background = v3(ra.background[0], ra.background[1], ra.background[2]);
    Counters<false> ctr;
    constexpr bool kResumable = WALK == WALK_COMPACT || WALK == WALK_LDS_STACK;

    uint32_t cursor = 0;                                                    // wave-uniform
    bool own = false, has_path = false, walking = false;                    // the lane owns a sample; its path is under way; its walk is parked
    bool pending = false, shadow = false;                                   // a finished path walk waits for its shade; a shadow ray is outstanding
    bool after_diffuse = false;                                             // the path's last scatter was Lambertian (or the source counts as one)
    uint32_t rec = 0;                                                       // the work index until the start step, then the record i * K + s
    uint32_t hit_prim = PRIM_NONE;
    float hit_t = 0.0f;
    uint32_t n_samples = 0, n_rays = 0;
    V3 sh_d = v3(0.0f, 0.0f, 0.0f), sh_c = v3(0.0f, 0.0f, 0.0f);            // of the outstanding shadow ray: direction, atten * c
    float sh_t = 0.0f;                                                      // and its t_max
    [[maybe_unused]] float csh = 0.0f;                                      // MIS: the cosine of the last Lambertian scatter, kept until the next hit
    Path p;
    p.ray.o = v3(0.0f, 0.0f, 0.0f); p.ray.d = v3(0.0f, 0.0f, 0.0f);
    p.color = v3(0.0f, 0.0f, 0.0f); p.atten = v3(0.0f, 0.0f, 0.0f);
    p.remain = 0u;
    p.rng.s0 = 0u; p.rng.s1 = 0u;
    for (;;) {
        // ---- refill: every lane without a sample takes the next work index of the run (begin + item < work: item < count <= work - begin) ----
        const uint64_t need = __builtin_amdgcn_ballot_w64(!own);
        if (need != 0ull && cursor < count) {
            const uint32_t item = cursor + wave_rank(need);
            if (!own && item < count) {
                rec = begin + item;
                own = true;
            }
            cursor = wave_advance(cursor, need, count);
        }
        if (__builtin_amdgcn_ballot_w64(own) == 0ull) break;                // every lane is free and none could take a sample: the run is done
        if (own) {
            // ---- start: the sample's path; a drawn first ray has stream (seed, j, 1), the path starts fresh on (seed, j, 0) ----
            if (!has_path) {
                const SampleIndex q = sample_index(rec, ga.range_length, ra.sample_begin);
                rec = q.item * ga.samples_per_item + q.sample;              // < n * K <= 2^32 - first_stream
                const uint32_t stream = ga.first_stream + rec;
                if (ga.source == TRT_PASSES_RAYS) {
                    p.ray = rad_load_ray(items, q.item);
                } else {
                    Rng g = rng_seed(ra.seed_key, stream, 1u);
                    p.ray = gather_ray(items, q.item, ga.source, ga.spread, g);
                }
                p.rng = rng_seed(ra.seed_key, stream, 0u);
                if (ga.directions) {                                        // the traced ray's stored direction (rec < n * K: within the buffer)
                    float* const d = ga.directions + 3ull * rec;
                    d[0] = p.ray.d.x; d[1] = p.ray.d.y; d[2] = p.ray.d.z;
                }
                p.color = v3(0.0f, 0.0f, 0.0f);
                p.atten = v3(1.0f, 1.0f, 1.0f);
                p.remain = ra.max_bounces;
                after_diffuse = ga.source_is_diffuse != 0u;
                has_path = true;
                n_samples++;
            }
            // ---- shade what is pending ----
            if (pending) {
                pending = false;
                ShadeInfo info;
                info.hide_light = after_diffuse;
                info.kind = SHADE_KIND_MISS;
                info.normal = v3(0.0f, 0.0f, 0.0f);
                if (shade_hit_info<MODE, false>(sc, p, hit_prim, hit_t, background, ctr, info)) {
                    if constexpr (MIS) {
                        // a light reached by a diffuse scatter at hit >= 2 (a light leaves remain and the ray as they were): the shadow ray of
                        // the vertex before has counted it with wl, the hit counts with wb.  Cold: the path has ended.
                        if (info.kind == TRT_LIGHT && after_diffuse && p.remain != ra.max_bounces) {
                            if constexpr (PICK) {
                                const float4 m = sc.material(prim_material<MODE>(sc, hit_prim));
                                const V3 emission = v3(m.x, m.y, m.z);
                                const float wb = mis_hit_weight<MODE>(sc, hit_prim, p.ray, info.normal, hit_t, csh, emission, total_power, ga.heuristic);
                                p.color = p.color + p.atten * (emission * wb);
                            } else {
                                const float wb = mis_hit_weight<MODE>(sc, hit_prim, p.ray, info.normal, hit_t, csh, ga.n_emitters, ga.heuristic);
                                const float4 m = sc.material(prim_material<MODE>(sc, hit_prim));
                                p.color = p.color + p.atten * (v3(m.x, m.y, m.z) * wb);
                            }
                        }
                    }
                    float* const c = ga.colors + 3ull * rec;                // the sample's colour (rec < n * K: within the buffer)
                    c[0] = p.color.x; c[1] = p.color.y; c[2] = p.color.z;
                    has_path = false;
                } else {
                    // the path goes on (p.remain > 0 after the decrement): metal and glass are specular, a light they lead to is the path's own
                    after_diffuse = info.kind == TRT_LAMBERTIAN;
                    if (after_diffuse) {
                        // ---- next event: the surfel is (the new ray's origin, the record's normal); d = max_bounces - remain - 1 scatters before ----
                        Rng g = rng_seed(ra.seed_key, ga.first_stream + rec, 1u + (ra.max_bounces - p.remain));
                        DirectSample smp;
                        [[maybe_unused]] float wl = 1.0f;
                        if constexpr (MIS) {
                            const WeightedDirectSample w = direct_draw_at<PICK, WeightedDirectSample>(p.ray.o, info.normal, emitters, pick, ga.n_emitters, ga.shadow_end, g);
                            smp = w;
                            csh = dot(info.normal, p.ray.d);
                            // the shadow sample's share: 1 / (1 + q(p_bsdf / p_light)); a virtual emitter cannot be hit and counts in full
                            const float qw = ga.heuristic == TRT_MIS_POWER ? w.wgt * w.wgt : w.wgt;
                            if (w.geometry != 0xFFFFFFFFu) wl = 1.0f / (1.0f + qw);
                        } else {
                            smp = direct_draw_at<PICK, DirectSample>(p.ray.o, info.normal, emitters, pick, ga.n_emitters, ga.shadow_end, g);
                        }
                        V3 c = smp.c;
                        if constexpr (MIS) c = c * wl;
                        const V3 term = p.atten * c;
                        if (smp.live) {
                            if (smp.t_max > kTMin) {
                                shadow = true;
                                sh_d = smp.ray.d; sh_t = smp.t_max; sh_c = term;
                            } else {
                                p.color = p.color + term;                   // an empty range: nothing is walked, the sample is unoccluded
                            }
                        }
                    }
                }
            }
            // ---- walk what is alive: the shadow ray first, the path ray in a round after it ----
            if (has_path) {
                Ray ray = p.ray;
                if (shadow) ray.d = sh_d;
                const float t_first = shadow ? sh_t : __builtin_inff();
                bool done = true;
                uint32_t prim;
                float t;
                if constexpr (kResumable) {
                    Trav tr = trav_begin<MODE, WALK == WALK_COMPACT>(sc, ray, false);        // a new walk, or the frame of a parked one
                    if (walking) trav_unpark(stack, tr); else { tr.t_best = t_first; n_rays++; }
                    const uint32_t entered = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(true));
                    walking = !closest_hit_resume<MODE, false, WALK, false>(sc, ray, tr, ctr, ga.slots, stack, leaf_list, nodes16, ga.stragglers, entered);
                    done = !walking;
                    prim = tr.prim_best; t = tr.t_best;
                } else {
                    n_rays++;
                    prim = closest_hit<MODE, false, WALK, false>(sc, ray, false, t, ctr, ga.slots, stack, leaf_list, nodes16, flat_reuse, t_first);
                }
                if (done) {
                    if (shadow) {
                        if (prim == PRIM_NONE) p.color = p.color + sh_c;
                        shadow = false;
                    } else {
                        hit_prim = prim; hit_t = t;
                        pending = true;
                    }
                }
            }
            if (!has_path) own = false;
        }
    }
    flush_counters<false>(ga.counters, n_samples, n_rays, ctr);
}

// max_bounces == 0 over a range that is not empty: the colours of the range become +0 (cpu.rs:43-47,64), nothing else is touched.  The
// eight lines of samples.hip samples_zero_kernel again: sharing that kernel through a header would make it a symbol of two units.
__global__ __launch_bounds__(256) void nee_samples_zero_kernel(float* __restrict__ colors, uint32_t work, uint32_t range_length, uint32_t sample_begin,
                                                               uint32_t samples_per_item) {
    const unsigned long long q = blockIdx.x * 256ull + threadIdx.x;
    if (q >= work) return;
    const SampleIndex x = sample_index((uint32_t)q, range_length, sample_begin);
    float* const c = colors + 3ull * (x.item * samples_per_item + x.sample);
    c[0] = 0.0f; c[1] = 0.0f; c[2] = 0.0f;
}

namespace {

// The six shapes of nee.hip kNeeKernels, [pick][mis]: the source is a kernel argument, so a table is one (MIS, PICK) over them.  A lane
// carries eight registers fewer than its nee_kernel sibling; the launch bounds are the highest at which the instantiation uses no
// scratch memory and spills no vector register (profiles/nee_samples_resource_usage.txt).  The plan reports the bound
// (kernel_waves_per_simd).
#define TRT_NEE_SAMPLES_ROW(MIS, PICK, MODE, WALK, THREADS, MINW) \
    BatchKernel{reinterpret_cast<const void*>(&nee_samples_kernel<MODE, WALK, THREADS, MINW, MIS, PICK>), MODE, WALK, THREADS, MINW}
#define TRT_NEE_SAMPLES_TABLE(MIS, PICK, LDS_FLAT, LDS_STACK_256, LDS_STACK_768, LDS_REGS, GLOBAL_COMPACT, GLOBAL_REGS)                                  \
    {TRT_NEE_SAMPLES_ROW(MIS, PICK, MODE_LDS, WALK_FLAT, 256, LDS_FLAT), TRT_NEE_SAMPLES_ROW(MIS, PICK, MODE_LDS, WALK_LDS_STACK, 256, LDS_STACK_256),    \
     TRT_NEE_SAMPLES_ROW(MIS, PICK, MODE_LDS, WALK_LDS_STACK, 768, LDS_STACK_768), TRT_NEE_SAMPLES_ROW(MIS, PICK, MODE_LDS, WALK_REGS, 512, LDS_REGS),    \
     TRT_NEE_SAMPLES_ROW(MIS, PICK, MODE_GLOBAL, WALK_COMPACT, 256, GLOBAL_COMPACT), TRT_NEE_SAMPLES_ROW(MIS, PICK, MODE_GLOBAL, WALK_REGS, 256, GLOBAL_REGS)}
constexpr size_t kNeeSamplesShapes = 6;
const BatchKernel kNeeSamplesKernels[2][2][kNeeSamplesShapes] = {
    {TRT_NEE_SAMPLES_TABLE(false, false, 6, 6, 6, 6, 6, 6), TRT_NEE_SAMPLES_TABLE(true, false, 5, 6, 6, 6, 6, 6)},
    {TRT_NEE_SAMPLES_TABLE(false, true, 6, 6, 6, 6, 6, 6), TRT_NEE_SAMPLES_TABLE(true, true, 5, 6, 6, 6, 6, 6)},
};
#undef TRT_NEE_SAMPLES_TABLE
#undef TRT_NEE_SAMPLES_ROW

uint32_t range_of(const NeeCall& c) { return c.ra.sample_end - c.ra.sample_begin; }

hipError_t launch_nee_samples(const QueryScene& qs, const NeeCall& c, const float* d_items, uint32_t n, const float* d_emitters, const float* d_pick,
                              float* d_colors, float* d_directions, unsigned long long* d_counters, hipStream_t stream) {
    const uint32_t R = range_of(c);
    if (n == 0 || R == 0u) return hipSuccess;                               // an empty range touches nothing
    const uint32_t work = n * R;                                            // nee_samples_check: n * R <= 2^32 - 1
    if (c.ra.max_bounces == 0u) {
        hipLaunchKernelGGL(nee_samples_zero_kernel, dim3((uint32_t)(((unsigned long long)work + 255ull) / 256ull)), dim3(256), 0, stream, d_colors, work,
                           R, c.ra.sample_begin, c.samples_per_item);
        return hipGetLastError();
    }
    SceneDev scd = qs.scene;
    BatchLaunch b;
    const hipError_t e = batch_prepare(scd, work, kNeeSamplesKernels[c.pick][c.mis], kNeeSamplesShapes, b);
    if (e != hipSuccess) return e;
    const trt_query_plan& q = b.q;
    RenderArgs ra = c.ra;
    ra.flat_reuse = qs.flat_reuse;
    NeeSamplesArgs ga{d_items, d_emitters, d_colors, d_directions, d_counters, work, q.rays_per_wave, q.leaf_slots, q.stragglers, c.samples_per_item,
                      c.first_stream, R, c.source, c.spread, c.n_emitters, c.shadow_end, c.source_is_diffuse, c.heuristic};
    NeeSamplesPickArgs pa{ga, d_pick, c.total_power};
    void* args[] = {&scd, &ra, &ga, &b.leaf_list, &b.nodes16};
    if (c.pick) args[2] = &pa;                                              // the PICK kernels' own argument struct
    return batch_launch(b, args, stream);
}

// What both forms check before any device work, in the header's order: trt_nee's checks on p->query.nee with `colors` where the sums
// stand, accumulate, weighted, trt_nee_mis' own fields when weighted, this struct's reserved words, the n x R bound.
int nee_samples_check(const trt_scene* s, const trt_ray* items, uint32_t n, const trt_emitter* emitters, uint32_t n_emitters,
                      const trt_nee_samples_params* p, const float* colors, NeeCall& c) {
    if (!p) return query_fail(TRT_ERR_INVALID_ARG, "null argument");
    int rc = nee_check(s, items, n, emitters, n_emitters, &p->query.nee, colors, c);
    if (rc != TRT_OK) return rc;
    if (p->query.nee.gather.path.accumulate != 0u)
        return query_fail(TRT_ERR_INVALID_ARG, "accumulate must be 0: a sample's record is written, never added to");
    if (p->weighted > 1u) return query_fail(TRT_ERR_INVALID_ARG, "weighted must be 0 or 1");
    if (p->weighted) {
        rc = emitter_mis_check(p->query, c);
        if (rc != TRT_OK) return rc;
    }
    for (uint32_t r : p->reserved)
        if (r != 0u) return query_fail(TRT_ERR_INVALID_ARG, "reserved words must be zero");
    if ((unsigned long long)n * range_of(c) > 0xFFFFFFFFull)
        return query_fail(TRT_ERR_INVALID_ARG, "more than 2^32 - 1 samples in the range of one call");
    return TRT_OK;
}

// The sibling's step list by (weighted, pick != NULL), unchanged and in the sibling's order (nee_call.h).
int nee_samples_steps(const trt_scene* s, uint32_t n, const EmitterTables& t, EmitterForm form, NeeCall& c) {
    if (t.pick) return c.mis ? emitter_steps_run(s, n, t, form, kNeeMisPickSteps, c) : emitter_steps_run(s, n, t, form, kNeePickSteps, c);
    return c.mis ? emitter_steps_run(s, n, t, form, kNeeMisSteps, c) : emitter_steps_run(s, n, t, form, kNeeSteps, c);
}

}  // namespace
}  // namespace trt

extern "C" {

void trt_nee_samples_params_default(trt_nee_samples_params* out) {
    if (!out) return;
    *out = trt_nee_samples_params{};
    trt_nee_mis_params_default(&out->query);
}

int trt_nee_samples_device(trt_scene* s, const trt_ray* d_items, uint32_t n, const trt_emitter* d_emitters, const trt_emitter_pick* d_pick,
                           uint32_t n_emitters, const trt_nee_samples_params* p, float* d_colors, float* d_directions, uint64_t* d_counters,
                           void* stream) {
    trt::NeeCall c;
    int rc = trt::nee_samples_check(s, d_items, n, d_emitters, n_emitters, p, d_colors, c);
    if (rc != TRT_OK) return rc;
    const trt::EmitterTables t{d_emitters, d_pick, n_emitters, p->total_power};
    rc = trt::nee_samples_steps(s, n, t, trt::FORM_DEVICE, c);
    if (rc != TRT_OK) return rc;
    return trt::sample_query_on_device(s, n, trt::kNeeLabels.launch, [&](const trt::QueryScene& qs) {
        return trt::launch_nee_samples(qs, c, reinterpret_cast<const float*>(d_items), n, reinterpret_cast<const float*>(d_emitters),
                                       reinterpret_cast<const float*>(d_pick), d_colors, d_directions,
                                       reinterpret_cast<unsigned long long*>(d_counters), static_cast<hipStream_t>(stream));
    });
}

// Host buffers: staged by host_stage.h sample_query_on_host (items | emitter table | colours | directions | counters | pick table).  The
// call writes the records of its range only, so a call that leaves records of the buffers alone - a part of the range, or
// max_bounces == 0, which leaves the directions - sends the caller's buffers up first; an empty range brings nothing down.
int trt_nee_samples(trt_scene* s, const trt_ray* items, uint32_t n, const trt_emitter* emitters, const trt_emitter_pick* pick, uint32_t n_emitters,
                    const trt_nee_samples_params* p, float* colors, float* directions, trt_stats* stats) {
    return trt::host_form([&]() -> int {
        trt::NeeCall c;
        int rc = trt::nee_samples_check(s, items, n, emitters, n_emitters, p, colors, c);
        if (rc != TRT_OK) return rc;
        const trt::EmitterTables t{emitters, pick, n_emitters, p->total_power};
        rc = trt::nee_samples_steps(s, n, t, trt::FORM_HOST, c);
        if (rc != TRT_OK) return rc;
        const size_t records = (size_t)n * c.samples_per_item * 12u;
        trt::SampleHost h{items, (size_t)n * sizeof(trt_ray), "hipMemcpy of the items", emitters, (size_t)n_emitters * sizeof(trt_emitter),
                          "hipMemcpy of the emitters", colors, records, directions, records, "hipMemcpy of the directions"};
        if (c.pick) { h.table2 = pick; h.table2_b = (size_t)n_emitters * sizeof(trt_emitter_pick); h.table2_what = "hipMemcpy of the pick table"; }
        const bool keeps = trt::range_of(c) < c.samples_per_item || c.ra.max_bounces == 0u;
        return trt::sample_query_on_host(s, n, h, keeps, trt::range_of(c) == 0u, trt::kNeeLabels.buffers, trt::kNeeLabels.launch, stats,
                                         [&](const trt::QueryScene& qs, const trt::SampleDev& d) {
                                             return trt::launch_nee_samples(qs, c, d.items, n, d.table, d.table2, d.sums, d.sums2, d.counters, nullptr);
                                         });
    });
}

// How launch_nee_samples would launch n items with a range of range_length samples on this scene with the kernels of (weighted, pick).
int trt_nee_samples_launch_plan(const trt_scene* s, uint32_t n, uint32_t range_length, uint32_t weighted, uint32_t pick, uint32_t compute_units,
                                trt_query_plan* out) {
    if ((unsigned long long)n * range_length > 0xFFFFFFFFull) return trt::query_fail(TRT_ERR_INVALID_ARG, "more than 2^32 - 1 samples in the range of one call");
    return trt::batch_launch_plan(s, n * range_length, compute_units, trt::kNeeSamplesKernels[pick != 0u][weighted != 0u], trt::kNeeSamplesShapes, out);
}

}  // extern "C"
