// query.hip — ray queries (tinyrt.h trt_intersect / trt_occluded and their device forms), written for gfx950 (CDNA4) only.
//
// The question a BVH is built to answer, for caller-supplied rays: what does ray i hit in [0.001, t_max[i]) - BVH::hit
// (hittable/bvh.rs:24-27,88-107), bit for bit - or, for the occlusion form, whether it hits anything there at all.  There is no walk code
// in this file: the kernels call the entry points of rt_path.h the way streamed.hip does (stage_scene_to_lds, axis_quads_to_lds,
// trav_begin, closest_hit, closest_hit_resume, trav_unpark) with the dynamic LDS laid out as streamed.hip lays it out (scene copy | leaf
// stack: threads x slots x 8 bytes), and run the walk the streamed launch plan picks for the scene (query_plan below).
//
// Work: a wave owns a contiguous run of the caller's rays, in the caller's order - nothing is sorted or compacted, coherence is the
// caller's business (the run, the place of the leaf stack and the refill's cursor step are wave_run.h's, shared with aov.hip and pixels.hip; the launch is
// query_plan.h's).  With the two resumable walks (LDS tree, 16-byte nodes) the wave works in the rounds of stream_sample_kernel: a lane
// whose walk completed writes its answer and takes the next ray of the run, a lane whose walk is still under way when at most
// `stragglers` lanes walk parks it in its leaf stack and resumes beside the fresh rays, so one long walk does not hold 63 lanes.  The
// other walks (lock-step list, register slots) run to their end, 64 rays of the run at a time.
//
// The occlusion kernels are the same template with the walks' ANY switch (rt_path.h closest_hit_ref): the walk ends after the leaf phase in
// which a primitive was first accepted, and one byte is written per ray instead of a 28-byte record.
#include "kernels.h"
#include "query_plan.h"
#include "rt_path.h"
#include "scene_query.h"
#include "wave_run.h"

namespace trt {

static_assert(sizeof(trt_hit) == 28 && offsetof(trt_hit, normal) == 16, "trt_hit layout (tinyrt.h)");

TRT_DEV Ray q_load_ray(const float* __restrict__ rays, uint32_t idx) {
    const float* r = rays + 6ull * idx;
    Ray ray;
    ray.o = v3(r[0], r[1], r[2]);
    ray.d = v3(r[3], r[4], r[5]);
    return ray;
}

// The answer of one ray.  ANY: one byte.  Else the record of HitRecord::new (hittable/mod.rs:28-48) for the winning primitive
// (wave_run.h hit_surface).  A miss: t = +inf, geometry = material = 0xFFFFFFFF, everything else 0.
template <int MODE, bool ANY>
TRT_DEV void q_store(const SceneAcc<MODE>& sc, const uint32_t* __restrict__ geo_index, void* __restrict__ out, uint32_t idx, const Ray& ray,
                     uint32_t prim, float t) {
    if constexpr (ANY) {
        static_cast<uint8_t*>(out)[idx] = prim != PRIM_NONE ? 1u : 0u;
    } else {
        uint32_t* const rec = reinterpret_cast<uint32_t*>(static_cast<trt_hit*>(out) + idx);
        if (prim == PRIM_NONE) {
            rec[0] = __float_as_uint(__builtin_inff()); rec[1] = 0xFFFFFFFFu; rec[2] = 0xFFFFFFFFu; rec[3] = 0u;
            rec[4] = 0u; rec[5] = 0u; rec[6] = 0u;
            return;
        }
        const HitSurface h = hit_surface<MODE>(sc, geo_index, ray, prim, t);
        rec[0] = __float_as_uint(t);
        rec[1] = h.geometry;
        rec[2] = h.material;
        rec[3] = h.front_face ? 1u : 0u;
        rec[4] = __float_as_uint(h.normal.x); rec[5] = __float_as_uint(h.normal.y); rec[6] = __float_as_uint(h.normal.z);
    }
}

struct QueryArgs {
    const float* rays;               // n x (origin, direction), used as given
    const float* t_max;              // n, or nullptr = +inf for every ray
    void* out;                       // n x trt_hit, or n bytes (ANY)
    const uint32_t* geo_index;
    uint32_t n, rays_per_wave;       // wave w owns rays [w * rays_per_wave, ...)
    uint32_t slots, stragglers;      // leaf stack depth per lane; resumable walks: lanes that may carry a walk into the next round
    FlatReuse flat_reuse;
};

template <int MODE, int WALK, bool ANY, int THREADS, int MINW>
__global__ __launch_bounds__(THREADS, MINW) void query_kernel(SceneDev scd, QueryArgs qa, const float4* __restrict__ leaf_list,
                                                                   const uint4* __restrict__ nodes16) {
    stage_scene_to_lds<MODE>(scd);
    const FlatReuse flat_reuse = axis_quads_to_lds<MODE, false, WALK>(scd, qa.flat_reuse);
    const SceneAcc<MODE> sc{scd.blob, scd.L};
    const float* __restrict__ const rays = qa.rays;
    const float* __restrict__ const t_max = qa.t_max;
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long begin64 = wave_begin<THREADS>(qa.rays_per_wave);
    if (begin64 >= qa.n) return;                                            // (after the barriers above)
    const uint32_t begin = (uint32_t)begin64;
    const uint32_t count = wave_count(qa.n, qa.rays_per_wave, begin);
    // this lane's postponed-leaf stack: behind the scene copy, slots x 64 x 8 bytes per wave
    float2* const stack = WALK != WALK_REGS ? reinterpret_cast<float2*>(lds_behind_scene(sc)) + (threadIdx.x >> 6) * (64u * qa.slots) + lane : nullptr;
    Counters<false> ctr;
    constexpr bool kResumable = WALK == WALK_COMPACT || WALK == WALK_LDS_STACK;

    if constexpr (kResumable) {
        uint32_t cursor = 0;                                                // wave-uniform
        bool has = false, walking = false;
        uint32_t idx = 0;
        float tm = 0.0f;
        Ray ray;
        ray.o = v3(0.0f, 0.0f, 0.0f); ray.d = v3(0.0f, 0.0f, 0.0f);
        for (;;) {
            const uint64_t need = __builtin_amdgcn_ballot_w64(!has);
            if (need != 0ull && cursor < count) {
                const uint32_t item = cursor + wave_rank(need);
                if (!has && item < count) {
                    idx = begin + item;
                    ray = q_load_ray(rays, idx);
                    tm = t_max ? t_max[idx] : __builtin_inff();
                    if (tm > kTMin) has = true;
                    else q_store<MODE, ANY>(sc, qa.geo_index, qa.out, idx, ray, PRIM_NONE, 0.0f);      // an empty or NaN range: a miss, not walked
                }
                cursor = wave_advance(cursor, need, count);
            }
            if (__builtin_amdgcn_ballot_w64(has) == 0ull) {
                if (cursor >= count) break;
                continue;                                                   // every ray taken in this round had an empty range
            }
            if (has) {
                Trav tr = trav_begin<MODE, WALK == WALK_COMPACT>(sc, ray, false);      // a new walk, or the frame of a parked one
                if (walking) trav_unpark(stack, tr); else tr.t_best = tm;
                const uint32_t entered = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(true));
                walking = !closest_hit_resume<MODE, false, WALK, ANY>(sc, ray, tr, ctr, qa.slots, stack, leaf_list, nodes16, qa.stragglers, entered);
                if (!walking) {
                    q_store<MODE, ANY>(sc, qa.geo_index, qa.out, idx, ray, tr.prim_best, tr.t_best);
                    has = false;
                }
            }
        }
    } else {
        for (uint32_t base = 0; base < count; base += 64u) {
            if (base + lane < count) {
                const uint32_t idx = begin + base + lane;
                const Ray ray = q_load_ray(rays, idx);
                const float tm = t_max ? t_max[idx] : __builtin_inff();
                float t = 0.0f;
                uint32_t prim = PRIM_NONE;
                if (tm > kTMin) prim = closest_hit<MODE, false, WALK, ANY>(sc, ray, false, t, ctr, qa.slots, stack, leaf_list, nodes16, flat_reuse, tm);
                q_store<MODE, ANY>(sc, qa.geo_index, qa.out, idx, ray, prim, t);
            }
        }
    }
}

namespace {

#define TRT_QUERY(ANY, MODE, WALK, THREADS, MINW) \
    BatchKernel{reinterpret_cast<const void*>(&query_kernel<MODE, WALK, ANY, THREADS, MINW>), MODE, WALK, THREADS, MINW}
// one instantiation per (scene mode, walk, workgroup shape) the streamed launch plan produces for the scenes the tuning was measured on:
// lock-step list in LDS / 256 lanes (up to 32 primitives), LDS tree with the leaf stack in LDS at 256 and at 768 lanes, 16-byte nodes from
// global memory; and the register-slot walk for LDS scenes (512 lanes) and for scenes in global memory (256 lanes).  The table does NOT
// hold every plan the default tuning produces: an LDS scene too large for two 768-lane workgroups per CU but whose leaf stack still costs
// no resident 512-lane workgroup (scene copies of roughly 56 to 64 KB) is planned as LDS tree / 512 lanes, which is not here, and
// neither are the plans only scene options reach (a tree walk from global memory with the 16-byte nodes switched off; the lock-step
// list forced on a scene of more than 32 primitives that is in LDS at 768 lanes or in global memory).  Those run the register-slot
// instantiation of their scene mode (stream_plan.h plan_batch: fallback), which walks the culling tree every compiled scene carries and
// needs neither the leaf list nor the 16-byte nodes.  Row 0: the closest-hit form, row 1: the occlusion form of the same shapes.
#define TRT_QUERY_TABLE(ANY)                                \
    {                                                       \
        TRT_QUERY(ANY, MODE_LDS, WALK_FLAT, 256, 8),        \
        TRT_QUERY(ANY, MODE_LDS, WALK_LDS_STACK, 256, 8),   \
        TRT_QUERY(ANY, MODE_LDS, WALK_LDS_STACK, 768, 6),   \
        TRT_QUERY(ANY, MODE_LDS, WALK_REGS, 512, 6),        \
        TRT_QUERY(ANY, MODE_GLOBAL, WALK_COMPACT, 256, 8),  \
        TRT_QUERY(ANY, MODE_GLOBAL, WALK_REGS, 256, 8),     \
    }
constexpr size_t kQueryShapes = 6;
const BatchKernel kQueryKernels[2][kQueryShapes] = {TRT_QUERY_TABLE(false), TRT_QUERY_TABLE(true)};
#undef TRT_QUERY_TABLE
#undef TRT_QUERY

// launches exactly what trt_query_launch_plan reports (query_plan.h: one rule)
hipError_t launch_query(const QueryScene& qs, const float* d_rays, const float* d_t_max, uint32_t n, void* d_out, bool any, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    SceneDev scd = qs.scene;
    BatchLaunch b;
    const hipError_t e = batch_prepare(scd, n, kQueryKernels[any ? 1 : 0], kQueryShapes, b);
    if (e != hipSuccess) return e;
    const trt_query_plan& q = b.q;
    QueryArgs qa{d_rays, d_t_max, d_out, qs.geo_index, n, q.rays_per_wave, q.leaf_slots, q.stragglers, qs.flat_reuse};
    void* args[] = {&scd, &qa, &b.leaf_list, &b.nodes16};
    return hipLaunchKernel(b.fn, dim3(q.workgroups), dim3(q.threads_per_workgroup), args, q.lds_bytes, stream);
}

// Argument checks shared by the four entry points: TRT_ERR_INVALID_ARG before any device work, then TRT_ERR_NO_DEVICE (trt_sample_batch's order).
int query_check(const trt_scene* s, const void* rays, uint32_t n, const void* out) {
    if (!s) return query_fail(TRT_ERR_INVALID_ARG, "scene is null");
    if (n && (!rays || !out)) return query_fail(TRT_ERR_INVALID_ARG, "null buffer");
    return query_require_device();
}

int query_device(trt_scene* s, const trt_ray* d_rays, const float* d_t_max, uint32_t n, void* d_out, bool any, void* stream) {
    int rc = query_check(s, d_rays, n, d_out);
    if (rc != TRT_OK || n == 0) return rc;
    QueryScene qs;
    rc = query_scene_on_device(s, qs);
    if (rc != TRT_OK) return rc;
    const hipError_t e = launch_query(qs, reinterpret_cast<const float*>(d_rays), d_t_max, n, d_out, any, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return query_fail_hip(e, "ray query launch");
    return TRT_OK;
}

// Host buffers: device copies of the call's own, one stream-ordered sequence on the default stream, complete when the call returns.
// (Runs inside host_form: the two entry points below.)
int query_host(trt_scene* s, const trt_ray* rays, const float* t_max, uint32_t n, void* out, size_t out_stride, bool any) {
    int rc = query_check(s, rays, n, out);
    if (rc != TRT_OK || n == 0) return rc;
    QueryScene qs;
    rc = query_scene_on_device(s, qs);
    if (rc != TRT_OK) return rc;
    const size_t rays_b = (size_t)n * sizeof(trt_ray), tmax_b = (size_t)n * sizeof(float), out_b = (size_t)n * out_stride;
    HostStage st("ray query buffers");
    const size_t r_rays = st.reserve(rays_b), r_tmax = st.reserve(tmax_b, t_max != nullptr), r_out = st.reserve(out_b);
    st.alloc();
    st.up(r_rays, rays, rays_b, "hipMemcpy of the rays");
    st.up(r_tmax, t_max, tmax_b, "hipMemcpy of t_max");
    if (st.ok()) st.run(launch_query(qs, st.ptr<float>(r_rays), st.ptr<float>(r_tmax), n, st.ptr<void>(r_out), any, nullptr), "ray query launch");
    st.down(out, r_out, out_b, "hipMemcpy of the answers");
    return st.finish();
}

}  // namespace
}  // namespace trt

extern "C" {

int trt_intersect(trt_scene* s, const trt_ray* rays, const float* t_max, uint32_t n, trt_hit* hits) {
    return trt::host_form([&] { return trt::query_host(s, rays, t_max, n, hits, sizeof(trt_hit), false); });
}
int trt_occluded(trt_scene* s, const trt_ray* rays, const float* t_max, uint32_t n, uint8_t* occluded) {
    return trt::host_form([&] { return trt::query_host(s, rays, t_max, n, occluded, 1u, true); });
}
int trt_intersect_device(trt_scene* s, const trt_ray* d_rays, const float* d_t_max, uint32_t n, trt_hit* d_hits, void* stream) {
    return trt::query_device(s, d_rays, d_t_max, n, d_hits, false, stream);
}
int trt_occluded_device(trt_scene* s, const trt_ray* d_rays, const float* d_t_max, uint32_t n, uint8_t* d_occluded, void* stream) {
    return trt::query_device(s, d_rays, d_t_max, n, d_occluded, true, stream);
}
// How launch_query would launch n rays on this scene.
int trt_query_launch_plan(const trt_scene* s, uint32_t n, uint32_t compute_units, trt_query_plan* out) {
    return trt::batch_launch_plan(s, n, compute_units, trt::kQueryKernels[0], trt::kQueryShapes, out);
}

}  // extern "C"
