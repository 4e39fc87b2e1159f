// nee.hip — next-event queries: the paths of the radiance and gather queries with a device-drawn shadow ray to a caller-supplied emitter
// table at every diffuse vertex (tinyrt.h trt_nee / trt_nee_device), written for gfx950 (CDNA4) only.
//
// The gather queries (radiance.hip) find the lights by chance at every bounce; the direct-light queries (direct.hip) aim at them, for the
// surfel itself only.  This unit puts the two together.  Sample j of an item runs the path of CpuSampler::single_point_sampling
// (cpu.rs:39-65) on RNG stream (seed, j, 0) with exactly the reference's draws, so its vertices are trt_radiance's / trt_gather's bit for
// bit, and changes the loop body in two places:
//   * at a hit a light's emission is Vec3::zero() when the path came there by a Lambertian scatter (after_diffuse);
//   * after a Lambertian scatter that leaves bounce budget, gather_draw.h direct_draw_at (direct_draw's body, given the vertex in place
//     of an item) on stream (seed, j, 2 + d) - d scatters before
//     this vertex - draws an emitter point for the surfel (rec.p, rec.normal); a live sample whose shadow ray finds nothing in
//     [0.001, t_max) adds  color = color + atten * c,  atten being the attenuation after the vertex's albedo.
// The shadow ray stands for the emission the reference would find one hit later, which is why a light reached diffusely is hidden and why
// the last vertex of the budget draws none: the expectation is the reference's at the same max_bounces.  The fold per item is
// trt_radiance's, in registers: a lane owns an item for all samples of the call.
//
// The round loop is radiance_kernel's - refill, start, SHADE what is pending, WALK what is alive - with one more lane state: a shadow
// ray is outstanding.  Its origin is the continuation ray's, so the lane keeps its direction, its t_max and what it would add.  There
// is ONE walk call site: a round walks the lane's shadow ray if one is outstanding, else its path ray, through the same closest_hit /
// closest_hit_resume call with a per-lane first t_best of t_max or +inf; "anything in [0.001, t_max)" is prim_best != PRIM_NONE after a
// closest-hit walk that starts at t_max (rt_path.h: up to the first acceptance t_best is the caller's t_max).  A lane with a shadow ray
// walks its continuation ray in the next round.  Every sample walks its own first segment (no kShareFirst): the two registers are
// needed elsewhere.  There is no walk code in this file; the dynamic LDS is the queries' (wave_run.h), the launch rule too (query_plan.h).
// Nor is there shading code: shade_hit_info is rt_path.h's one shade body with the lines that read and fill ShadeInfo switched on.  The
// two forms' scaffold is host_stage.h's, the checks of the source and of the emitter table are gather_draw.h's, shared with passes.hip
// and direct.hip.
//
// trt_nee_mis / trt_nee_mis_device (tinyrt.h) are the same kernel with MIS = true: the same rounds, walks and draws, and two weights on
// what a sample adds.  The shadow term is scaled by wl = 1 / (1 + q(wgt)) where the draw's result becomes sh_c (1 for a virtual
// emitter), and a light the path reaches after a diffuse scatter at hit >= 2, which the plain kernel hides, adds its emission scaled by
// wb = q(g) / (1 + q(g)) (mis_weight.h mis_hit_weight) in the branch where shade has ended the path: cold, since a light always ends it.  A lane
// carries csh, the cosine of its last Lambertian scatter, besides.  The MIS = false instantiations are instruction for instruction what
// they were without the parameter; the host side of all four queries is emitter_query.h's, shared with direct.hip.
//
// trt_nee_pick / trt_nee_mis_pick (tinyrt.h) are the same kernel with PICK = true: every vertex draw goes through the alias table of
// direct.hip's PICK queries (gather_draw.h AliasPick: one draw and two loads more), and the weighted hit takes the light's choice
// probability from the hit itself (mis_weight.h, the overload with total_power).  The table's checks are emitter_pick.h's, in the order
// of this unit's step lists (emitter_query.h).  The PICK = false instantiations are instruction for instruction what they were.
#include "emitter_pick.h"
#include "emitter_query.h"
#include "gather_draw.h"
#include "host_stage.h"
#include "kernels.h"
#include "mis_weight.h"
#include "nee_call.h"
#include "query_plan.h"
#include "rt_path.h"
#include "scene_query.h"
#include "wave_run.h"

namespace trt {

static_assert(sizeof(trt_nee_params) == 128 && offsetof(trt_nee_params, gather) == 0 && offsetof(trt_nee_params, shadow_end) == 96 &&
              offsetof(trt_nee_params, source_is_diffuse) == 100 && offsetof(trt_nee_params, reserved) == 104, "trt_nee_params layout (tinyrt.h)");
static_assert(sizeof(trt_nee_mis_params) == 160 && offsetof(trt_nee_mis_params, nee) == 0 && offsetof(trt_nee_mis_params, heuristic) == 128 &&
              offsetof(trt_nee_mis_params, reserved) == 132, "trt_nee_mis_params layout (tinyrt.h)");

struct NeeArgs {
    const float* items;              // n x (origin, direction) or n x (point, axis), used as given
    const float* emitters;           // n_emitters x 20 words (trt_emitter)
    float* radiance;                 // n x 3
    float* moment2;                  // n x 3, or nullptr: not wanted
    unsigned long long* counters;    // nullptr, or [CTR_SAMPLES], [CTR_RAYS] are added to
    uint32_t n, rays_per_wave;       // wave w owns items [w * rays_per_wave, ...)
    uint32_t slots, stragglers;      // as in query.hip QueryArgs
    uint32_t samples_per_item;       // K
    uint32_t first_stream;           // first_stream + n * K <= 2^32 (radiance_check): the stream index never wraps
    uint32_t source;                 // enum trt_passes_source of the lobe kernels (the RAYS kernels do not read it)
    float spread;                    // the cone lobe's sphere radius
    uint32_t n_emitters;             // E: 1 .. 2^20
    float shadow_end;                // in (0, 1]
    uint32_t source_is_diffuse;      // after_diffuse at the first hit
    uint32_t heuristic;              // enum trt_mis_heuristic, wave-uniform (the MIS kernels; the others do not read it)
};
// What a PICK kernel is handed besides (trt_nee_pick, trt_nee_mis_pick): the alias table (tinyrt.h trt_emitter_pick, n_emitters x 4 words)
// and the table's total power, by which a light hit finds its own choice probability (the weighted kernels; the others do not read it).
// A struct of its own around NeeArgs, as direct.hip DirectPickArgs is: the kernel arguments of the uniform kernels lie where they lay.
struct NeePickArgs {
    NeeArgs g;
    const float* pick;
    float total_power;
};
TRT_DEV const NeeArgs& nee_args(const NeeArgs& a) { return a; }
TRT_DEV const NeeArgs& nee_args(const NeePickArgs& a) { return a.g; }
TRT_DEV const float* nee_pick_table(const NeeArgs&) { return nullptr; }
TRT_DEV const float* nee_pick_table(const NeePickArgs& a) { return a.pick; }
TRT_DEV float nee_pick_total(const NeeArgs&) { return 0.0f; }
TRT_DEV float nee_pick_total(const NeePickArgs& a) { return a.total_power; }
constexpr int NEE_RAYS = 0, NEE_LOBE = 1;      // nee_kernel's SOURCE: the items are rays | surfels whose lobe is NeeArgs::source

// ra.sample_begin < ra.sample_end and ra.max_bounces > 0 (launch_nee: nothing to trace launches query_plan.h batch_zero or nothing)
// MIS (tinyrt.h trt_nee_mis): the same rounds, walks and draws; a shadow sample is scaled by wl, and a light the path reaches after a
// diffuse scatter at hit >= 2 adds its emission scaled by wb where the plain kernel adds nothing.  A lane carries csh, one register more.
// PICK (trt_nee_pick, trt_nee_mis_pick): the emitter of a vertex's shadow ray is chosen through the alias table (gather_draw.h AliasPick),
// one draw and two loads more per vertex; the weighted light hit takes its choice probability from the hit material and total_power.
template <int MODE, int WALK, int THREADS, int MINW, int SOURCE, bool MIS, bool PICK = false>
__global__ __launch_bounds__(THREADS, MINW) void nee_kernel(SceneDev scd, RenderArgs ra, std::conditional_t<PICK, NeePickArgs, NeeArgs> args,
                                                                 const float4* __restrict__ leaf_list, const uint4* __restrict__ nodes16) {
    const NeeArgs& ga = nee_args(args);
    [[maybe_unused]] const float* __restrict__ const pick = nee_pick_table(args);
    [[maybe_unused]] const float total_power = nee_pick_total(args);
    stage_scene_to_lds<MODE>(scd);
    const FlatReuse flat_reuse = axis_quads_to_lds<MODE, false, WALK>(scd, ra.flat_reuse);
    const SceneAcc<MODE> sc{scd.blob, scd.L};
    const float* __restrict__ const items = ga.items;
    const float* __restrict__ const emitters = ga.emitters;
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
    bool pending = false, shadow = false;                                   // a finished path walk waits for its shade; a shadow ray is outstanding
    bool after_diffuse = false;                                             // the path's last scatter was Lambertian (or the source counts as one)
    uint32_t idx = 0, s = 0;
    uint32_t hit_prim = PRIM_NONE;
    float hit_t = 0.0f;
    uint32_t n_samples = 0, n_rays = 0;
    V3 acc = v3(0.0f, 0.0f, 0.0f), m2 = v3(0.0f, 0.0f, 0.0f);
    V3 sh_d = v3(0.0f, 0.0f, 0.0f), sh_c = v3(0.0f, 0.0f, 0.0f);            // of the outstanding shadow ray: direction, atten * c
    float sh_t = 0.0f;                                                      // and its t_max
    [[maybe_unused]] float csh = 0.0f;                                      // MIS: the cosine of the last Lambertian scatter, kept until the next hit
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
                if (ra.accumulate) {
                    const float* const a = ga.radiance + 3ull * idx;
                    acc = v3(a[0], a[1], a[2]);
                    if (ga.moment2) { const float* const m = ga.moment2 + 3ull * idx; m2 = v3(m[0], m[1], m[2]); }
                } else {
                    acc = v3(0.0f, 0.0f, 0.0f);
                    m2 = v3(0.0f, 0.0f, 0.0f);
                }
                own = true;
            }
            cursor = wave_advance(cursor, need, count);
        }
        if (__builtin_amdgcn_ballot_w64(own) == 0ull) break;                // every lane is free and none could take an item: the run is done
        if (own) {
            // ---- start: the item's next sample; a drawn first ray has stream (seed, j, 1), the path starts fresh on (seed, j, 0) ----
            if (!has_path) {
                const uint32_t stream = ga.first_stream + idx * ga.samples_per_item + s;
                if constexpr (SOURCE == NEE_RAYS) {
                    p.ray = rad_load_ray(items, idx);                       // re-read: 24 bytes per sample against six registers per lane
                } else {
                    Rng g = rng_seed(ra.seed_key, stream, 1u);
                    p.ray = gather_ray(items, idx, ga.source, ga.spread, g);
                }
                p.rng = rng_seed(ra.seed_key, stream, 0u);
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
                } else {
                    // the path goes on (p.remain > 0 after the decrement): metal and glass are specular, a light they lead to is the path's own
                    after_diffuse = info.kind == TRT_LAMBERTIAN;
                    if (after_diffuse) {
                        // ---- next event: the surfel is (the new ray's origin, the record's normal); d = max_bounces - remain - 1 scatters before ----
                        const uint32_t stream = ga.first_stream + idx * ga.samples_per_item + s;
                        Rng g = rng_seed(ra.seed_key, stream, 1u + (ra.max_bounces - p.remain));
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
        }
    }
    flush_counters<false>(ga.counters, n_samples, n_rays, ctr);
}

namespace {

// The (scene mode, walk, workgroup shape) set of the other batch units, with the register-slot fallback (query_plan.h), so that every
// scene has a kernel: the six shapes, written once.  A table is nee_kernel with one (SOURCE, MIS, PICK) over them; its launch bounds, one
// per shape in this order, are all that a table says of its own, and the tables for rays as given and for the drawn lobes (as
// radiance.hip has them) share theirs.  The plan reports the bound (kernel_waves_per_simd).
#define TRT_NEE_ROW(SOURCE, MIS, PICK, MODE, WALK, THREADS, MINW) \
    BatchKernel{reinterpret_cast<const void*>(&nee_kernel<MODE, WALK, THREADS, MINW, SOURCE, MIS, PICK>), MODE, WALK, THREADS, MINW}
#define TRT_NEE_TABLE(SOURCE, MIS, PICK, LDS_FLAT, LDS_STACK_256, LDS_STACK_768, LDS_REGS, GLOBAL_COMPACT, GLOBAL_REGS)                                       \
    {TRT_NEE_ROW(SOURCE, MIS, PICK, MODE_LDS, WALK_FLAT, 256, LDS_FLAT), TRT_NEE_ROW(SOURCE, MIS, PICK, MODE_LDS, WALK_LDS_STACK, 256, LDS_STACK_256),         \
     TRT_NEE_ROW(SOURCE, MIS, PICK, MODE_LDS, WALK_LDS_STACK, 768, LDS_STACK_768), TRT_NEE_ROW(SOURCE, MIS, PICK, MODE_LDS, WALK_REGS, 512, LDS_REGS),         \
     TRT_NEE_ROW(SOURCE, MIS, PICK, MODE_GLOBAL, WALK_COMPACT, 256, GLOBAL_COMPACT), TRT_NEE_ROW(SOURCE, MIS, PICK, MODE_GLOBAL, WALK_REGS, 256, GLOBAL_REGS)}
#define TRT_NEE_TABLES(MIS, PICK, ...) {TRT_NEE_TABLE(NEE_RAYS, MIS, PICK, __VA_ARGS__), TRT_NEE_TABLE(NEE_LOBE, MIS, PICK, __VA_ARGS__)}
constexpr size_t kNeeShapes = 6;
// The kernels of a query: [pick][mis][SOURCE].
//  - plain: a lane carries what a lane of the gather kernel carries plus the outstanding shadow ray (direction, t_max, colour) and two
//    flags: the launch bounds are the highest at which the instantiation uses no scratch memory and spills no vector register
//    (profiles/nee_resource_usage.txt).
//  - weighted (trt_nee_mis): a lane carries csh besides.  Bounds by the same rule, read per shape off both sources
//    (profiles/nee_mis_resource_usage.txt).
//  - PICK (trt_nee_pick, trt_nee_mis_pick): u1, q and the alias die before the emitter record is loaded, the table pointer is
//    wave-uniform; bounds by the same rule, read per shape off both sources (profiles/nee_pick_resource_usage.txt).
const BatchKernel kNeeKernels[2][2][2][kNeeShapes] = {
    {TRT_NEE_TABLES(false, false, 5, 6, 6, 5, 5, 5), TRT_NEE_TABLES(true, false, 5, 5, 5, 5, 5, 5)},
    {TRT_NEE_TABLES(false, true, 5, 6, 6, 5, 5, 5), TRT_NEE_TABLES(true, true, 5, 5, 5, 5, 5, 5)},
};
#undef TRT_NEE_TABLES
#undef TRT_NEE_TABLE
#undef TRT_NEE_ROW

hipError_t launch_nee(const QueryScene& qs, const NeeCall& c, const float* d_items, uint32_t n, const float* d_emitters, const float* d_pick,
                      float* d_radiance, float* d_moment2, unsigned long long* d_counters, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (c.nothing()) {
        // nothing to trace: a path with no bounce budget returns colour 0 (cpu.rs:43-47,64); the sums start at 0, or stay
        if (c.ra.accumulate) return hipSuccess;
        return batch_zero(d_radiance, 3ull * n, d_moment2, 3ull * n, stream);
    }
    SceneDev scd = qs.scene;
    BatchLaunch b;
    const hipError_t e = batch_prepare(scd, n, kNeeKernels[c.pick][c.mis][c.source == TRT_PASSES_RAYS ? NEE_RAYS : NEE_LOBE], kNeeShapes, b);
    if (e != hipSuccess) return e;
    const trt_query_plan& q = b.q;
    RenderArgs ra = c.ra;
    ra.flat_reuse = qs.flat_reuse;
    NeeArgs ga{d_items, d_emitters, d_radiance, d_moment2, d_counters, n, q.rays_per_wave, q.leaf_slots, q.stragglers, c.samples_per_item,
               c.first_stream, c.source, c.spread, c.n_emitters, c.shadow_end, c.source_is_diffuse, c.heuristic};
    NeePickArgs pa{ga, d_pick, c.total_power};
    void* args[] = {&scd, &ra, &ga, &b.leaf_list, &b.nodes16};
    if (c.pick) args[2] = &pa;                                              // the PICK kernels' own argument struct
    return batch_launch(b, args, stream);
}

// NeeCall, nee_check, the labels and the four step lists are nee_call.h's, shared with nee_samples.hip.

// The two forms of the four queries (emitter_query.h): the family's parameter check, then the query's steps over its tables, then the
// launcher.  `steps` is the query's list below, `t.pick` / `t.total_power` what a PICK query was handed.
template <class Params, size_t K>
int nee_device(const EmitterStep (&steps)[K], trt_scene* s, const trt_ray* d_items, uint32_t n, const EmitterTables& t, const Params* p, float* d_radiance,
               float* d_moment2, uint64_t* d_counters, void* stream) {
    NeeCall c;
    const int rc = nee_check(s, d_items, n, t.emitters, t.n_emitters, p, d_radiance, c);
    if (rc != TRT_OK) return rc;
    return emitter_query_on_device(s, c, steps, kNeeLabels, launch_nee, d_items, n, t, d_radiance, d_moment2, d_counters, stream);
}
template <class Params, size_t K>
int nee_host(const EmitterStep (&steps)[K], trt_scene* s, const trt_ray* items, uint32_t n, const EmitterTables& t, const Params* p, float* radiance,
             float* moment2, trt_stats* stats) {
    return host_form([&]() -> int {
        NeeCall c;
        const int rc = nee_check(s, items, n, t.emitters, t.n_emitters, p, radiance, c);
        if (rc != TRT_OK) return rc;
        return emitter_query_on_host(s, c, steps, kNeeLabels, launch_nee, items, n, t, radiance, moment2, stats);
    });
}
// How launch_nee would launch n items on this scene with the kernels of a query: the two sources' tables share their shapes and bounds,
// so the source does not enter.
int nee_plan(bool mis, bool pick, const trt_scene* s, uint32_t n, uint32_t compute_units, trt_query_plan* out) {
    return batch_launch_plan(s, n, compute_units, kNeeKernels[pick][mis][NEE_LOBE], kNeeShapes, out);
}

}  // namespace
}  // namespace trt

extern "C" {

void trt_nee_params_default(trt_nee_params* out) {
    if (!out) return;
    *out = trt_nee_params{};
    trt_gather_params_default(&out->gather);
    out->gather.lobe = TRT_PASSES_COSINE;
    out->shadow_end = 0.999f;
}

int trt_nee_device(trt_scene* s, const trt_ray* d_items, uint32_t n, const trt_emitter* d_emitters, uint32_t n_emitters, const trt_nee_params* p,
                   float* d_radiance, float* d_moment2, uint64_t* d_counters, void* stream) {
    return trt::nee_device(trt::kNeeSteps, s, d_items, n, {d_emitters, nullptr, n_emitters, 0.0f}, p, d_radiance, d_moment2, d_counters, stream);
}
int trt_nee(trt_scene* s, const trt_ray* items, uint32_t n, const trt_emitter* emitters, uint32_t n_emitters, const trt_nee_params* p, float* radiance,
            float* moment2, trt_stats* stats) {
    return trt::nee_host(trt::kNeeSteps, s, items, n, {emitters, nullptr, n_emitters, 0.0f}, p, radiance, moment2, stats);
}
int trt_nee_launch_plan(const trt_scene* s, uint32_t n, uint32_t compute_units, trt_query_plan* out) {
    return trt::nee_plan(false, false, s, n, compute_units, out);
}

void trt_nee_mis_params_default(trt_nee_mis_params* out) {
    if (!out) return;
    *out = trt_nee_mis_params{};
    trt_nee_params_default(&out->nee);
    out->heuristic = TRT_MIS_BALANCE;
}

int trt_nee_mis_device(trt_scene* s, const trt_ray* d_items, uint32_t n, const trt_emitter* d_emitters, uint32_t n_emitters,
                       const trt_nee_mis_params* p, float* d_radiance, float* d_moment2, uint64_t* d_counters, void* stream) {
    return trt::nee_device(trt::kNeeMisSteps, s, d_items, n, {d_emitters, nullptr, n_emitters, 0.0f}, p, d_radiance, d_moment2, d_counters, stream);
}
int trt_nee_mis(trt_scene* s, const trt_ray* items, uint32_t n, const trt_emitter* emitters, uint32_t n_emitters, const trt_nee_mis_params* p,
                float* radiance, float* moment2, trt_stats* stats) {
    return trt::nee_host(trt::kNeeMisSteps, s, items, n, {emitters, nullptr, n_emitters, 0.0f}, p, radiance, moment2, stats);
}
int trt_nee_mis_launch_plan(const trt_scene* s, uint32_t n, uint32_t compute_units, trt_query_plan* out) {
    return trt::nee_plan(true, false, s, n, compute_units, out);
}

// ---- the PICK queries: the emitter of every vertex's shadow ray chosen by power (or the caller's weights) through an alias table ----
int trt_nee_pick_device(trt_scene* s, const trt_ray* d_items, uint32_t n, const trt_emitter* d_emitters, const trt_emitter_pick* d_pick,
                        uint32_t n_emitters, const trt_nee_params* p, float* d_radiance, float* d_moment2, uint64_t* d_counters, void* stream) {
    return trt::nee_device(trt::kNeePickSteps, s, d_items, n, {d_emitters, d_pick, n_emitters, 0.0f}, p, d_radiance, d_moment2, d_counters, stream);
}
int trt_nee_pick(trt_scene* s, const trt_ray* items, uint32_t n, const trt_emitter* emitters, const trt_emitter_pick* pick, uint32_t n_emitters,
                 const trt_nee_params* p, float* radiance, float* moment2, trt_stats* stats) {
    return trt::nee_host(trt::kNeePickSteps, s, items, n, {emitters, pick, n_emitters, 0.0f}, p, radiance, moment2, stats);
}
int trt_nee_pick_launch_plan(const trt_scene* s, uint32_t n, uint32_t compute_units, trt_query_plan* out) {
    return trt::nee_plan(false, true, s, n, compute_units, out);
}

int trt_nee_mis_pick_device(trt_scene* s, const trt_ray* d_items, uint32_t n, const trt_emitter* d_emitters, const trt_emitter_pick* d_pick,
                            uint32_t n_emitters, const trt_nee_mis_params* p, float total_power, float* d_radiance, float* d_moment2,
                            uint64_t* d_counters, void* stream) {
    return trt::nee_device(trt::kNeeMisPickSteps, s, d_items, n, {d_emitters, d_pick, n_emitters, total_power}, p, d_radiance, d_moment2, d_counters, stream);
}
int trt_nee_mis_pick(trt_scene* s, const trt_ray* items, uint32_t n, const trt_emitter* emitters, const trt_emitter_pick* pick, uint32_t n_emitters,
                     const trt_nee_mis_params* p, float total_power, float* radiance, float* moment2, trt_stats* stats) {
    return trt::nee_host(trt::kNeeMisPickSteps, s, items, n, {emitters, pick, n_emitters, total_power}, p, radiance, moment2, stats);
}
int trt_nee_mis_pick_launch_plan(const trt_scene* s, uint32_t n, uint32_t compute_units, trt_query_plan* out) {
    return trt::nee_plan(true, true, s, n, compute_units, out);
}

}  // extern "C"
