// samples.hip — sample queries: every sample's colour and first direction (tinyrt.h trt_samples / trt_samples_device), and the device fold
// that turns those records into the sums of a radiance or gather query (trt_fold_samples / trt_fold_samples_device), written for gfx950
// (CDNA4) only.
//
// The folding queries (radiance.hip, probe.hip, ...) trace K samples per item and return only their fold: a lane owns an ITEM for all
// samples of the call, and the launch rule gives a wave 256 items whatever K is.  Here a lane owns one SAMPLE: the call's work is the
// n x R samples of the range, work index q = (item, sample) by sample_index.h, a wave owns a contiguous run of q (query_plan.h's rule with
// n x R in the place of n), and a finished path stores its colour at record i * K + s and frees the lane.  64 probes of 16 384 samples
// are 4 096 waves, not one.
//
// The sample kernel is radiance_kernel's round loop - refill, start, SHADE what is pending, WALK what is alive - with the sums, the
// per-lane sample counter and the shared first segment taken out; refill and start are one step, because a lane that takes a work index
// starts its path at once.  The first ray is the item itself (rad_load_ray) or the draw of a gather or a probe query (gather_ray,
// probe_ray: gather_draw.h, the one copy), chosen by a kernel argument: a scalar branch in the start step.  Its stored direction goes out
// in the start step, so nothing is carried for it.  There is no walk code in this file: the walks and shade_hit are rt_path.h's, the run,
// the leaf stacks and the refill step wave_run.h's, the launch query_plan.h's, the two forms host_stage.h's.
//
// The fold kernels read the records of an item in sample order and apply the imager's rule,
//   radiance.ch = radiance.ch + c.ch * inv_K;   moment2.ch = moment2.ch + (c.ch * c.ch) * inv_K
// one IEEE f32 operation per operator: a serial chain per item and channel, as the contract demands.  Two regimes, one host rule
// (fold_by_wave), the same bytes:
//   tile  a lane owns an item; a wave loads the records of its 64 items coalesced, 16 samples of each at a time, into LDS and every lane
//         reads its own row back (a transposition: the rows are 12 K bytes apart in memory);
//   wave  a wave owns an item: 64 consecutive records are loaded coalesced, their products formed in parallel and added in sample order
//         through cross-lane reads.
#include "gather_draw.h"
#include "host_stage.h"
#include "kernels.h"
#include "query_plan.h"
#include "rt_path.h"
#include "sample_index.h"
#include "samples_call.h"
#include "scene_query.h"
#include "wave_run.h"

namespace trt {

static_assert(sizeof(trt_samples_params) == 96 && offsetof(trt_samples_params, source) == 64 && offsetof(trt_samples_params, spread) == 68 &&
              offsetof(trt_samples_params, reserved) == 72, "trt_samples_params layout (tinyrt.h)");
static_assert((uint32_t)TRT_SAMPLE_RAYS == (uint32_t)TRT_PASSES_RAYS && (uint32_t)TRT_SAMPLE_COSINE == (uint32_t)TRT_LOBE_COSINE &&
                  (uint32_t)TRT_SAMPLE_CONE == (uint32_t)TRT_LOBE_CONE,
              "the first three sources are enum trt_passes_source: gather_ray takes the word as its lobe");

struct SamplesArgs {
    const float* items;              // n x (origin, direction) or (point, axis), used as given
    float* colors;                   // n x K x 3
    float* directions;               // n x K x 3, or nullptr: not wanted
    unsigned long long* counters;    // nullptr, or [CTR_SAMPLES], [CTR_RAYS] are added to
    uint32_t work, per_wave;         // n x R work indices (samples_check: below 2^32); wave w owns [w * per_wave, ...)
    uint32_t slots, stragglers;      // as in query.hip QueryArgs
    uint32_t samples_per_item;       // K
    uint32_t first_stream;           // first_stream + n * K <= 2^32 (radiance_check): neither the record nor the stream index wraps
    uint32_t range_length;           // R = sample_end - sample_begin >= 1
    uint32_t source;                 // enum trt_sample_source: the same for every lane of the launch
    float spread;                    // the cone lobe's sphere radius
};

// ra.sample_begin < ra.sample_end and ra.max_bounces > 0 (launch_samples: nothing to trace launches the range's zero kernel or nothing)
template <int MODE, int WALK, int THREADS, int MINW>
__global__ __launch_bounds__(THREADS, MINW) void samples_kernel(SceneDev scd, RenderArgs ra, SamplesArgs ga, const float4* __restrict__ leaf_list,
                                                                     const uint4* __restrict__ nodes16) {
    stage_scene_to_lds<MODE>(scd);
    const FlatReuse flat_reuse = axis_quads_to_lds<MODE, false, WALK>(scd, ra.flat_reuse);
    const SceneAcc<MODE> sc{scd.blob, scd.L};
    const float* __restrict__ const items = ga.items;
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
    bool pending = false;                                                   // a finished walk waits for its shade
    uint32_t rec = 0;                                                       // the work index until the start step, then the record i * K + s
    uint32_t hit_prim = PRIM_NONE;
    float hit_t = 0.0f;
    uint32_t n_samples = 0, n_rays = 0;
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
            // ---- start: the sample's path (cpu.rs:42-45); its first ray by the source ----
            if (!has_path) {
                const SampleIndex q = sample_index(rec, ga.range_length, ra.sample_begin);
                rec = q.item * ga.samples_per_item + q.sample;              // < n * K <= 2^32 - first_stream
                const uint32_t stream = ga.first_stream + rec;
                if (ga.source == TRT_SAMPLE_RAYS) {
                    p.ray = rad_load_ray(items, q.item);
                } else {
                    // the draw has a stream of its own (sample index 1), the path starts fresh at 0: as the gather and probe kernels draw
                    Rng g = rng_seed(ra.seed_key, stream, 1u);
                    if (ga.source <= TRT_SAMPLE_CONE) p.ray = gather_ray(items, q.item, ga.source, ga.spread, g);
                    else p.ray = probe_ray(items, q.item, ga.source == TRT_SAMPLE_HEMISPHERE, g);
                }
                p.rng = rng_seed(ra.seed_key, stream, 0u);
                if (ga.directions) {                                        // the traced ray's stored direction (rec < n * K: within the buffer)
                    float* const d = ga.directions + 3ull * rec;
                    d[0] = p.ray.d.x; d[1] = p.ray.d.y; d[2] = p.ray.d.z;
                }
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
                    float* const c = ga.colors + 3ull * rec;                // the sample's colour: the lane is free again
                    c[0] = p.color.x; c[1] = p.color.y; c[2] = p.color.z;
                    has_path = false;
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
            if (!has_path) own = false;
        }
    }
    flush_counters<false>(ga.counters, n_samples, n_rays, ctr);
}

// max_bounces == 0 over a range that is not empty: the colours of the range become +0 (cpu.rs:43-47,64), nothing else is touched.
__global__ __launch_bounds__(256) void samples_zero_kernel(float* __restrict__ colors, uint32_t work, uint32_t range_length, uint32_t sample_begin,
                                                           uint32_t samples_per_item) {
    const unsigned long long q = blockIdx.x * 256ull + threadIdx.x;
    if (q >= work) return;
    const SampleIndex x = sample_index((uint32_t)q, range_length, sample_begin);
    float* const c = colors + 3ull * (x.item * samples_per_item + x.sample);
    c[0] = 0.0f; c[1] = 0.0f; c[2] = 0.0f;
}

// ---- the fold ----

struct FoldArgs {
    const float* colors;             // n x K x 3
    float* radiance;                 // n x 3
    float* moment2;                  // n x 3, or nullptr: not wanted
    uint32_t n, samples_per_item;    // K
    uint32_t sample_begin, range_length;     // [b, b + R), R >= 1
    uint32_t accumulate;
    float inv_k;                     // 1.0f / float(K)
};

constexpr uint32_t kFoldChunk = 16u;                                       // samples of an item in LDS at a time
constexpr uint32_t kFoldRow = 3u * kFoldChunk + 1u;                        // floats between two rows: odd, so that 64 rows meet 64 banks

// Tile regime: lane l of wave w owns item (blockIdx.x * 4 + w) * 64 + l.  The four waves of a workgroup work on their own quarter of the
// LDS; the barriers only order a wave's own writes and reads, and every wave passes the same number of them (R is uniform).
__global__ __launch_bounds__(256) void fold_tile_kernel(FoldArgs fa) {
    __shared__ float tile[4u * 64u * kFoldRow];
    const uint32_t lane = threadIdx.x & 63u;
    float* const rows = tile + (threadIdx.x >> 6) * (64u * kFoldRow);
    const unsigned long long first = (blockIdx.x * 4ull + (threadIdx.x >> 6)) * 64ull;      // the wave's first item, in 64 bits
    const unsigned long long mine = first + lane;
    const bool own = mine < fa.n;
    V3 acc = v3(0.0f, 0.0f, 0.0f), m2 = v3(0.0f, 0.0f, 0.0f);
    if (own && fa.accumulate) {
        const float* const a = fa.radiance + 3ull * mine;
        acc = v3(a[0], a[1], a[2]);
        if (fa.moment2) { const float* const m = fa.moment2 + 3ull * mine; m2 = v3(m[0], m[1], m[2]); }
    }
    for (uint32_t c0 = 0; c0 < fa.range_length; c0 += kFoldChunk) {
        const uint32_t cs = fa.range_length - c0 < kFoldChunk ? fa.range_length - c0 : kFoldChunk;
        const uint32_t len = 3u * cs, magic = fold_row_magic(len);         // floats of a row's part in this chunk: 3 .. 48
        for (uint32_t e = lane; e < 64u * len; e += 64u) {
            const uint32_t row = fold_row(e, magic), col = e - row * len;
            const unsigned long long item = first + row;
            // item < n, sample_begin + c0 + col / 3 < sample_begin + R <= K: within [0, 3 n K)
            if (item < fa.n) rows[row * kFoldRow + col] = fa.colors[3ull * (item * fa.samples_per_item + fa.sample_begin + c0) + col];
        }
        __syncthreads();
        if (own) {
            const float* const r = rows + lane * kFoldRow;
            for (uint32_t k = 0; k < cs; k++) {
                const V3 c = v3(r[3u * k], r[3u * k + 1u], r[3u * k + 2u]);
                acc = acc + c * fa.inv_k;
                m2.x = m2.x + (c.x * c.x) * fa.inv_k;
                m2.y = m2.y + (c.y * c.y) * fa.inv_k;
                m2.z = m2.z + (c.z * c.z) * fa.inv_k;
            }
        }
        __syncthreads();
    }
    if (own) {
        float* const a = fa.radiance + 3ull * mine;
        a[0] = acc.x; a[1] = acc.y; a[2] = acc.z;
        if (fa.moment2) { float* const m = fa.moment2 + 3ull * mine; m[0] = m2.x; m[1] = m2.y; m[2] = m2.z; }
    }
}

// v of lane l, l wave-uniform: a scalar read, the same value in every lane.
TRT_DEV float lane_value(float v, uint32_t l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), (int)l)); }

// Wave regime: wave w of the grid owns item w.  Lane l loads record b + c0 + l of the item and forms its six terms; the sums, the same in
// every lane, take the terms of lanes 0 .. cs - 1 in order.  Lane 0 writes.
__global__ __launch_bounds__(256) void fold_wave_kernel(FoldArgs fa) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long item = blockIdx.x * 4ull + (threadIdx.x >> 6);
    if (item >= fa.n) return;
    V3 acc = v3(0.0f, 0.0f, 0.0f), m2 = v3(0.0f, 0.0f, 0.0f);
    if (fa.accumulate) {
        const float* const a = fa.radiance + 3ull * item;
        acc = v3(a[0], a[1], a[2]);
        if (fa.moment2) { const float* const m = fa.moment2 + 3ull * item; m2 = v3(m[0], m[1], m[2]); }
    }
    const float* const recs = fa.colors + 3ull * (item * fa.samples_per_item + fa.sample_begin);
    for (uint32_t c0 = 0; c0 < fa.range_length; c0 += 64u) {
        const uint32_t cs = fa.range_length - c0 < 64u ? fa.range_length - c0 : 64u;    // wave-uniform
        V3 t = v3(0.0f, 0.0f, 0.0f), t2 = v3(0.0f, 0.0f, 0.0f);
        if (lane < cs) {                                                    // c0 + lane < R: within the item's records
            const float* const r = recs + 3ull * (c0 + lane);
            const V3 c = v3(r[0], r[1], r[2]);
            t = c * fa.inv_k;
            t2 = v3((c.x * c.x) * fa.inv_k, (c.y * c.y) * fa.inv_k, (c.z * c.z) * fa.inv_k);
        }
        if (cs == 64u) {
            // a full load: the lane numbers are literals, so the scalar reads run ahead of the six chains of additions
#pragma unroll
            for (uint32_t l = 0; l < 64u; l++) {
                acc.x = acc.x + lane_value(t.x, l); acc.y = acc.y + lane_value(t.y, l); acc.z = acc.z + lane_value(t.z, l);
                m2.x = m2.x + lane_value(t2.x, l); m2.y = m2.y + lane_value(t2.y, l); m2.z = m2.z + lane_value(t2.z, l);
            }
        } else {
            for (uint32_t l = 0; l < cs; l++) {
                acc.x = acc.x + lane_value(t.x, l); acc.y = acc.y + lane_value(t.y, l); acc.z = acc.z + lane_value(t.z, l);
                m2.x = m2.x + lane_value(t2.x, l); m2.y = m2.y + lane_value(t2.y, l); m2.z = m2.z + lane_value(t2.z, l);
            }
        }
    }
    if (lane == 0u) {
        float* const a = fa.radiance + 3ull * item;
        a[0] = acc.x; a[1] = acc.y; a[2] = acc.z;
        if (fa.moment2) { float* const m = fa.moment2 + 3ull * item; m[0] = m2.x; m[1] = m2.y; m[2] = m2.z; }
    }
}

namespace {

#define TRT_SAMPLES(MODE, WALK, THREADS, MINW) \
    BatchKernel{reinterpret_cast<const void*>(&samples_kernel<MODE, WALK, THREADS, MINW>), MODE, WALK, THREADS, MINW}
// The (scene mode, walk, workgroup shape) set of radiance.hip kRadianceKernels, so that every scene has a kernel, one instantiation each:
// the source is a kernel argument, as the lobe of the gather kernels is.  A lane carries what a lane of the gather kernel carries less
// the sums, the item index and the sample counter; the launch bounds are the highest at which the instantiation uses no scratch memory
// (profiles/samples_resource_usage.txt): 8 waves per SIMD for four shapes, 7 for the lock-step list and the 16-byte nodes, each at or
// above its sibling in kGatherKernels.  The plan reports the bound (kernel_waves_per_simd).  The report also says why the round loop
// frees a lane at the END of the round (`if (!has_path) own = false`) and not where the colour is stored: with `own` cleared beside
// `has_path` the compiler threads the loop's back edge through the shade and every shape spills 3 to 16 vector registers at 7.
const BatchKernel kSamplesKernels[] = {
    TRT_SAMPLES(MODE_LDS, WALK_FLAT, 256, 7),
    TRT_SAMPLES(MODE_LDS, WALK_LDS_STACK, 256, 8),
    TRT_SAMPLES(MODE_LDS, WALK_LDS_STACK, 768, 8),
    TRT_SAMPLES(MODE_LDS, WALK_REGS, 512, 8),
    TRT_SAMPLES(MODE_GLOBAL, WALK_COMPACT, 256, 7),
    TRT_SAMPLES(MODE_GLOBAL, WALK_REGS, 256, 8),
};
#undef TRT_SAMPLES
constexpr size_t kSamplesShapes = sizeof(kSamplesKernels) / sizeof(kSamplesKernels[0]);

}  // namespace

// The launch of a call after the checks (samples_call.h: project.hip's trt_probe_parallel launches its chunks through it).
hipError_t launch_samples(const QueryScene& qs, const SamplesCall& c, const float* d_items, uint32_t n, float* d_colors, float* d_directions,
                          unsigned long long* d_counters, hipStream_t stream) {
    const uint32_t R = c.range();
    if (n == 0 || R == 0u) return hipSuccess;                               // an empty range touches nothing
    const uint32_t work = n * R;                                            // samples_check: n * R <= 2^32 - 1
    if (c.ra.max_bounces == 0u) {
        hipLaunchKernelGGL(samples_zero_kernel, dim3((uint32_t)(((unsigned long long)work + 255ull) / 256ull)), dim3(256), 0, stream, d_colors, work, R,
                           c.ra.sample_begin, c.samples_per_item);
        return hipGetLastError();
    }
    SceneDev scd = qs.scene;
    BatchLaunch b;
    const hipError_t e = batch_prepare(scd, work, kSamplesKernels, kSamplesShapes, b);
    if (e != hipSuccess) return e;
    const trt_query_plan& q = b.q;
    RenderArgs ra = c.ra;
    ra.flat_reuse = qs.flat_reuse;
    SamplesArgs ga{d_items, d_colors, d_directions, d_counters, work, q.rays_per_wave, q.leaf_slots, q.stragglers, c.samples_per_item, c.first_stream,
                   R, c.source, c.spread};
    void* args[] = {&scd, &ra, &ga, &b.leaf_list, &b.nodes16};
    return batch_launch(b, args, stream);
}

namespace {

// What both forms check before any device work: trt_radiance's rules on p->path (radiance.hip radiance_check), then this struct's fields.
int samples_check(const trt_scene* s, const trt_ray* items, uint32_t n, const trt_samples_params* p, const float* colors, SamplesCall& c) {
    if (!p) return query_fail(TRT_ERR_INVALID_ARG, "null argument");
    const int rc = radiance_check(s, items, n, &p->path, colors, c.ra);
    if (rc != TRT_OK) return rc;
    if (p->path.accumulate != 0u) return query_fail(TRT_ERR_INVALID_ARG, "accumulate must be 0: a sample's record is written, never added to");
    if (p->source > TRT_SAMPLE_HEMISPHERE)
        return query_fail(TRT_ERR_INVALID_ARG, "source must be TRT_SAMPLE_RAYS, _COSINE, _CONE, _SPHERE or _HEMISPHERE");
    if (p->source == TRT_SAMPLE_CONE && !(p->spread >= 0.0f && p->spread < __builtin_inff()))
        return query_fail(TRT_ERR_INVALID_ARG, "spread of the cone lobe must be finite and not negative");
    for (uint32_t r : p->reserved)
        if (r != 0u) return query_fail(TRT_ERR_INVALID_ARG, "reserved words must be zero");
    if ((unsigned long long)n * (c.ra.sample_end - c.ra.sample_begin) > 0xFFFFFFFFull)
        return query_fail(TRT_ERR_INVALID_ARG, "more than 2^32 - 1 samples in the range of one call");
    c.samples_per_item = p->path.samples_per_ray;
    c.first_stream = p->path.first_stream;
    c.source = p->source;
    c.spread = p->spread;
    return TRT_OK;
}

// The one host rule of the fold's two regimes: a wave per item where an item has at least one full load of 64 records
// and the items are too few to fill the device with a lane each.
constexpr uint32_t kFoldWaveMinRange = 64u, kFoldWaveMaxItems = 4096u;
bool fold_by_wave(uint32_t n, uint32_t range_length) { return range_length >= kFoldWaveMinRange && n <= kFoldWaveMaxItems; }

// The fold's own parameters, as both forms read them.
struct FoldCall {
    uint32_t samples_per_item, sample_begin, sample_end, accumulate;
    uint32_t range() const { return sample_end - sample_begin; }
};
int fold_check(const float* colors, uint32_t n, const trt_radiance_params* p, const float* radiance, FoldCall& c) {
    if (!p) return query_fail(TRT_ERR_INVALID_ARG, "null argument");
    const uint32_t K = p->samples_per_ray;
    if (K == 0u) return query_fail(TRT_ERR_INVALID_ARG, "samples_per_ray must be positive");
    const uint32_t s1 = p->sample_end == 0u ? K : p->sample_end;
    if (p->sample_begin > s1 || s1 > K) return query_fail(TRT_ERR_INVALID_ARG, "sample range must satisfy begin <= end <= samples_per_ray");
    if (n > 0u && (!colors || !radiance)) return query_fail(TRT_ERR_INVALID_ARG, "null buffer");
    for (uint32_t r : p->reserved)
        if (r != 0u) return query_fail(TRT_ERR_INVALID_ARG, "reserved words must be zero");
    c = FoldCall{K, p->sample_begin, s1, p->accumulate ? 1u : 0u};
    return TRT_OK;
}

hipError_t launch_fold(const FoldCall& c, const float* d_colors, uint32_t n, float* d_radiance, float* d_moment2, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint32_t R = c.range();
    if (R == 0u) {
        // an empty range: the sums start at 0, or stay
        if (c.accumulate) return hipSuccess;
        return batch_zero(d_radiance, 3ull * n, d_moment2, 3ull * n, stream);
    }
    const FoldArgs fa{d_colors, d_radiance, d_moment2, n, c.samples_per_item, c.sample_begin, R, c.accumulate, 1.0f / (float)c.samples_per_item};
    if (fold_by_wave(n, R)) hipLaunchKernelGGL(fold_wave_kernel, dim3((n + 3u) / 4u), dim3(256), 0, stream, fa);
    else hipLaunchKernelGGL(fold_tile_kernel, dim3((uint32_t)(((unsigned long long)n + 255ull) / 256ull)), dim3(256), 0, stream, fa);
    return hipGetLastError();
}

}  // namespace
}  // namespace trt

extern "C" {

void trt_samples_params_default(trt_samples_params* out) {
    if (!out) return;
    *out = trt_samples_params{};
    trt_radiance_params_default(&out->path);
    out->source = TRT_SAMPLE_COSINE;
}

int trt_samples_device(trt_scene* s, const trt_ray* d_items, uint32_t n, const trt_samples_params* p, float* d_colors, float* d_directions,
                       uint64_t* d_counters, void* stream) {
    trt::SamplesCall c;
    const int rc = trt::samples_check(s, d_items, n, p, d_colors, c);
    if (rc != TRT_OK) return rc;
    return trt::sample_query_on_device(s, n, "sample query launch", [&](const trt::QueryScene& qs) {
        return trt::launch_samples(qs, c, reinterpret_cast<const float*>(d_items), n, d_colors, d_directions,
                                   reinterpret_cast<unsigned long long*>(d_counters), static_cast<hipStream_t>(stream));
    });
}

// Host buffers: staged by host_stage.h sample_query_on_host (items | colours | directions | counters).  The call writes the records of its
// range only, so a call that leaves records of the buffers alone - a part of the range, or max_bounces == 0, which leaves the directions -
// sends the caller's buffers up first, as a pass that continues sums does; an empty range brings nothing down.
int trt_samples(trt_scene* s, const trt_ray* items, uint32_t n, const trt_samples_params* p, float* colors, float* directions, trt_stats* stats) {
    return trt::host_form([&]() -> int {
        trt::SamplesCall c;
        const int rc = trt::samples_check(s, items, n, p, colors, c);
        if (rc != TRT_OK) return rc;
        const size_t records = (size_t)n * c.samples_per_item * 12u;
        const trt::SampleHost h{items, (size_t)n * sizeof(trt_ray), "hipMemcpy of the items", nullptr, 0u, "", colors, records, directions, records,
                                "hipMemcpy of the directions"};
        const bool keeps = c.range() < c.samples_per_item || c.ra.max_bounces == 0u;
        return trt::sample_query_on_host(s, n, h, keeps, c.range() == 0u, "sample query buffers", "sample query launch", stats,
                                         [&](const trt::QueryScene& qs, const trt::SampleDev& d) {
                                             return trt::launch_samples(qs, c, d.items, n, d.sums, d.sums2, d.counters, nullptr);
                                         });
    });
}

// How launch_samples would launch n items with a range of range_length samples on this scene.
int trt_samples_launch_plan(const trt_scene* s, uint32_t n, uint32_t range_length, uint32_t compute_units, trt_query_plan* out) {
    if ((unsigned long long)n * range_length > 0xFFFFFFFFull) return trt::query_fail(TRT_ERR_INVALID_ARG, "more than 2^32 - 1 samples in the range of one call");
    return trt::batch_launch_plan(s, n * range_length, compute_units, trt::kSamplesKernels, trt::kSamplesShapes, out);
}

int trt_fold_samples_device(const float* d_colors, uint32_t n, const trt_radiance_params* p, float* d_radiance, float* d_moment2, void* stream) {
    trt::FoldCall c;
    const int rc = trt::fold_check(d_colors, n, p, d_radiance, c);
    if (rc != TRT_OK) return rc;
    const unsigned long long records = 12ull * n * c.samples_per_item, sums = 12ull * n;
    if (trt::ranges_overlap(d_radiance, sums, d_colors, records) || trt::ranges_overlap(d_moment2, sums, d_colors, records))
        return trt::query_fail(TRT_ERR_INVALID_ARG, "the sums must not overlap the colours");
    if (n == 0u) return TRT_OK;
    const int rd = trt::query_require_device();
    if (rd != TRT_OK) return rd;
    const hipError_t e = trt::launch_fold(c, d_colors, n, d_radiance, d_moment2, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return trt::query_fail_hip(e, "sample fold launch");
    return TRT_OK;
}

// Host form: device copies of the call's own, the same kernels, complete when the call returns.  There is no CPU path.
int trt_fold_samples(const float* colors, uint32_t n, const trt_radiance_params* p, float* radiance, float* moment2) {
    return trt::host_form([&]() -> int {
        trt::FoldCall c;
        const int rc = trt::fold_check(colors, n, p, radiance, c);
        if (rc != TRT_OK) return rc;
        if (n == 0u) return TRT_OK;
        const int rd = trt::query_require_device();
        if (rd != TRT_OK) return rd;
        const size_t records = (size_t)n * c.samples_per_item * 12u, sums = (size_t)n * 12u;
        trt::HostStage st("sample fold buffers");
        const size_t r_c = st.reserve(records), r_s = st.reserve(sums), r_m = st.reserve(sums, moment2 != nullptr);
        st.alloc();
        st.up(r_c, colors, records, "hipMemcpy of the colours");
        if (c.accumulate) st.up(r_s, radiance, sums, "hipMemcpy of the sums");
        if (c.accumulate) st.up(r_m, moment2, sums, "hipMemcpy of the second moments");
        if (st.ok()) st.run(trt::launch_fold(c, st.ptr<float>(r_c), n, st.ptr<float>(r_s), st.ptr<float>(r_m), nullptr), "sample fold launch");
        if (!(c.accumulate && c.range() == 0u)) {
            st.down(radiance, r_s, sums, "hipMemcpy of the results");
            st.down(moment2, r_m, sums, "hipMemcpy of the results");
        }
        return st.finish();
    });
}

}  // extern "C"
