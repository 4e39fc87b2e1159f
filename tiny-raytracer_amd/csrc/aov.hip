// aov.hip — first-hit feature buffers of a frame (tinyrt.h trt_render_aov / trt_render_aov_device) and the primary rays the render traces
// (trt_primary_rays / trt_primary_rays_device), written for gfx950 (CDNA4) only.
//
// What a denoiser, a matte or a picking buffer needs of a frame: per pixel the albedo, normal, depth and coverage of the camera rays'
// first hits, folded over the samples as the imager folds radiance (acc = acc + value * (1/spp), in sample order, imager.rs:35,50), and
// the geometry / material index of sample 0.  The rays are the render's own: rng_seed(seed, y * W + x, s) followed by primary_ray
// (rt_path.h), the first hit is BVH::hit over [0.001, +inf) - the record trt_intersect gives for that ray (wave_run.h hit_surface).
//
// One kernel generates the ray, walks and folds: no ray and no record goes through memory.  There is no walk code in this file: the
// kernel calls the entry points of rt_path.h with the dynamic LDS laid out as the queries lay it out (scene copy | leaf stack: threads x
// slots x 8 bytes; the run, the place of the stack and the refill's cursor step are wave_run.h's), and is launched by the rule of the queries (query_plan.h)
// with pixels in place of rays.
//
// Work: a wave owns a contiguous run of the local image's pixels, and a lane owns a pixel for all of its samples, so the sums run in
// sample order without atomics and without a second kernel.  With the two resumable walks (LDS tree, 16-byte nodes) the wave works in the
// rounds of query_kernel: a lane whose walk completed folds the hit into its pixel and starts that pixel's next sample, or writes the
// pixel and takes the next pixel of the run; a lane whose walk is still under way when at most `stragglers` lanes walk parks it in its
// leaf stack and resumes beside the fresh rays.  The other walks (lock-step list, register slots) run to their end, 64 pixels of the run
// at a time, sample after sample.
#include "kernels.h"
#include "query_plan.h"
#include "rt_path.h"
#include "scene_query.h"
#include "wave_run.h"

namespace trt {

static_assert(sizeof(trt_aov_buffers) == 48, "trt_aov_buffers layout (tinyrt.h)");
static_assert(sizeof(trt_ray) == 24, "trt_ray layout (tinyrt.h)");

// The ray the render traces for sample s of local pixel `pix` (row-major over the rows this call owns): path_begin's first two lines.
TRT_DEV Ray aov_primary_ray(const CameraDev& cam, const RenderArgs& ra, uint32_t pix, uint32_t s) {
    const uint32_t row = pix / cam.width, x = pix - row * cam.width;
    const uint32_t y = image_row(ra, row);
    Rng rng = rng_seed(ra.seed_key, y * cam.width + x, s);
    return primary_ray(cam, x, y, rng);
}

struct AovArgs {
    float* albedo;                   // n x 3
    float* normal;                   // n x 3
    float* depth;                    // n
    float* coverage;                 // n
    uint32_t* geometry;              // n
    uint32_t* material;              // n; any of the six may be nullptr: not wanted
    const uint32_t* geo_index;
    uint32_t n, pixels_per_wave;     // local pixels; wave w owns pixels [w * pixels_per_wave, ...)
    uint32_t slots, stragglers;      // as in query.hip QueryArgs
};

struct AovSums { V3 albedo, normal; float depth, coverage; };

// The running sums of a pixel: the buffers' (`load`: a pass that accumulates, or one under way), or 0.
TRT_DEV AovSums aov_begin(const AovArgs& aa, bool load, uint32_t pix) {
    AovSums a;
    a.albedo = v3(0.0f, 0.0f, 0.0f); a.normal = v3(0.0f, 0.0f, 0.0f); a.depth = 0.0f; a.coverage = 0.0f;
    if (load) {
        if (aa.albedo) a.albedo = v3(aa.albedo[3ull * pix], aa.albedo[3ull * pix + 1u], aa.albedo[3ull * pix + 2u]);
        if (aa.normal) a.normal = v3(aa.normal[3ull * pix], aa.normal[3ull * pix + 1u], aa.normal[3ull * pix + 2u]);
        if (aa.depth) a.depth = aa.depth[pix];
        if (aa.coverage) a.coverage = aa.coverage[pix];
    }
    return a;
}

// One sample's first hit folded into the pixel's sums.  The record is the one the queries store (wave_run.h hit_surface); the indices of
// sample 0 go straight to their buffers.
template <int MODE>
TRT_DEV void aov_fold(const SceneAcc<MODE>& sc, const AovArgs& aa, const RenderArgs& ra, uint32_t pix, uint32_t s, const Ray& ray, uint32_t prim,
                      float t, AovSums& a) {
    V3 albedo = v3(ra.background[0], ra.background[1], ra.background[2]);
    V3 normal = v3(0.0f, 0.0f, 0.0f);
    uint32_t geo = 0xFFFFFFFFu, mat = 0xFFFFFFFFu;
    if (prim != PRIM_NONE) {
        const HitSurface h = hit_surface<MODE>(sc, aa.geo_index, ray, prim, t);
        normal = h.normal;
        geo = h.geometry;
        mat = h.material;
        const float4 m = sc.material(mat);
        albedo = v3(m.x, m.y, m.z);                                                // the emitted colour of a light
        a.depth = a.depth + t * ra.inv_spp;                                        // a miss adds nothing
        a.coverage = a.coverage + 1.0f * ra.inv_spp;
    }
    a.albedo = a.albedo + albedo * ra.inv_spp;
    a.normal = a.normal + normal * ra.inv_spp;
    if (s == 0u) {
        if (aa.geometry) aa.geometry[pix] = geo;
        if (aa.material) aa.material[pix] = mat;
    }
}

TRT_DEV void aov_store(const AovArgs& aa, uint32_t pix, const AovSums& a) {
    if (aa.albedo) { aa.albedo[3ull * pix] = a.albedo.x; aa.albedo[3ull * pix + 1u] = a.albedo.y; aa.albedo[3ull * pix + 2u] = a.albedo.z; }
    if (aa.normal) { aa.normal[3ull * pix] = a.normal.x; aa.normal[3ull * pix + 1u] = a.normal.y; aa.normal[3ull * pix + 2u] = a.normal.z; }
    if (aa.depth) aa.depth[pix] = a.depth;
    if (aa.coverage) aa.coverage[pix] = a.coverage;
}

// ra.sample_begin < ra.sample_end (launch_aov: an empty range launches nothing)
template <int MODE, int WALK, int THREADS, int MINW>
__global__ __launch_bounds__(THREADS, MINW) void aov_kernel(SceneDev scd, CameraDev cam, RenderArgs ra, AovArgs aa, const float4* __restrict__ leaf_list,
                                                                 const uint4* __restrict__ nodes16) {
    stage_scene_to_lds<MODE>(scd);
    const FlatReuse flat_reuse = axis_quads_to_lds<MODE, false, WALK>(scd, ra.flat_reuse);
    const SceneAcc<MODE> sc{scd.blob, scd.L};
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long begin64 = wave_begin<THREADS>(aa.pixels_per_wave);
    if (begin64 >= aa.n) return;                                            // (after the barriers above)
    const uint32_t begin = (uint32_t)begin64;
    const uint32_t count = wave_count(aa.n, aa.pixels_per_wave, begin);
    // this lane's postponed-leaf stack: behind the scene copy, slots x 64 x 8 bytes per wave
    float2* const stack = WALK != WALK_REGS ? reinterpret_cast<float2*>(lds_behind_scene(sc)) + (threadIdx.x >> 6) * (64u * aa.slots) + lane : nullptr;
    Counters<false> ctr;
    constexpr bool kResumable = WALK == WALK_COMPACT || WALK == WALK_LDS_STACK;

    if constexpr (kResumable) {
        uint32_t cursor = 0;                                                // wave-uniform
        bool own = false, walking = false;                                  // the lane owns a pixel; its ray's walk is parked
        uint32_t pix = 0, s = 0;
        AovSums sums;
        sums.albedo = v3(0.0f, 0.0f, 0.0f); sums.normal = v3(0.0f, 0.0f, 0.0f); sums.depth = 0.0f; sums.coverage = 0.0f;
        Ray ray;
        ray.o = v3(0.0f, 0.0f, 0.0f); ray.d = v3(0.0f, 0.0f, 0.0f);
        for (;;) {
            const uint64_t need = __builtin_amdgcn_ballot_w64(!own);
            if (need != 0ull && cursor < count) {
                const uint32_t item = cursor + wave_rank(need);
                if (!own && item < count) {
                    pix = begin + item;
                    s = ra.sample_begin;
                    sums = aov_begin(aa, ra.accumulate != 0u, pix);
                    own = true;
                }
                cursor = wave_advance(cursor, need, count);
            }
            if (__builtin_amdgcn_ballot_w64(own) == 0ull) break;            // (a lane without a pixel found none left: the run is done)
            if (own) {
                if (!walking) ray = aov_primary_ray(cam, ra, pix, s);
                Trav tr = trav_begin<MODE, WALK == WALK_COMPACT>(sc, ray, false);      // a new walk, or the frame of a parked one
                if (walking) trav_unpark(stack, tr); else tr.t_best = __builtin_inff();
                const uint32_t entered = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(true));
                walking = !closest_hit_resume<MODE, false, WALK, false>(sc, ray, tr, ctr, aa.slots, stack, leaf_list, nodes16, aa.stragglers, entered);
                if (!walking) {
                    aov_fold<MODE>(sc, aa, ra, pix, s, ray, tr.prim_best, tr.t_best, sums);
                    s += 1u;
                    if (s == ra.sample_end) {
                        aov_store(aa, pix, sums);
                        own = false;
                    }
                }
            }
        }
    } else {
        for (uint32_t base = 0; base < count; base += 64u) {
            if (base + lane < count) {
                const uint32_t pix = begin + base + lane;
                AovSums sums = aov_begin(aa, ra.accumulate != 0u, pix);
                for (uint32_t s = ra.sample_begin; s < ra.sample_end; s++) {
                    const Ray ray = aov_primary_ray(cam, ra, pix, s);
                    float t = 0.0f;
                    const uint32_t prim = closest_hit<MODE, false, WALK, false>(sc, ray, false, t, ctr, aa.slots, stack, leaf_list, nodes16, flat_reuse);
                    aov_fold<MODE>(sc, aa, ra, pix, s, ray, prim, t, sums);
                }
                aov_store(aa, pix, sums);
            }
        }
    }
}

// rays[i] = the primary ray of sample s of local pixel i
__global__ __launch_bounds__(256) void primary_rays_kernel(CameraDev cam, RenderArgs ra, uint32_t s, uint32_t n, float* __restrict__ rays) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const Ray ray = aov_primary_ray(cam, ra, i, s);
    float* const r = rays + 6ull * i;
    r[0] = ray.o.x; r[1] = ray.o.y; r[2] = ray.o.z;
    r[3] = ray.d.x; r[4] = ray.d.y; r[5] = ray.d.z;
}

namespace {

#define TRT_AOV(MODE, WALK, THREADS, MINW) \
    BatchKernel{reinterpret_cast<const void*>(&aov_kernel<MODE, WALK, THREADS, MINW>), MODE, WALK, THREADS, MINW}
// the (scene mode, walk, workgroup shape) set of the queries' table, with its register-slot fallback (query_plan.h), so that every
// scene has a kernel.  Launch bounds: the queries', except for the two walks that run to their end sample after sample with the eight
// sums live across the walk - under the 64 VGPRs of 8 waves per SIMD the lock-step kernel spills 11 VGPRs (40 B of scratch per lane) and
// the register-slot kernel for scenes in global memory 3 (16 B); folding into the output buffers in place instead still spills 7 and 1;
// at 7 waves (72 VGPRs) neither spilled when the bound was chosen.  Since the shade and ray set-up trims of rt_path.h the lock-step
// kernel spills 2 VGPRs (12 B of scratch per lane) at 7 waves again; the bound was not revisited (profiles/aov_resource_usage.txt has
// the current table).  The plan reports the bound (kernel_waves_per_simd).
const BatchKernel kAovKernels[] = {
    TRT_AOV(MODE_LDS, WALK_FLAT, 256, 7),
    TRT_AOV(MODE_LDS, WALK_LDS_STACK, 256, 8),
    TRT_AOV(MODE_LDS, WALK_LDS_STACK, 768, 6),
    TRT_AOV(MODE_LDS, WALK_REGS, 512, 6),
    TRT_AOV(MODE_GLOBAL, WALK_COMPACT, 256, 8),
    TRT_AOV(MODE_GLOBAL, WALK_REGS, 256, 7),
};
#undef TRT_AOV
constexpr size_t kAovShapes = sizeof(kAovKernels) / sizeof(kAovKernels[0]);

bool any_buffer(const trt_aov_buffers* b) { return b->albedo || b->normal || b->depth || b->coverage || b->geometry || b->material; }

hipError_t launch_aov(const QueryScene& qs, const CameraDev& cd, RenderArgs ra, uint32_t n, const trt_aov_buffers& b, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (ra.sample_begin == ra.sample_end) {
        // no sample to fold: the sums start at 0 (as trt_render's frame does), or stay; the indices belong to sample 0
        if (ra.accumulate) return hipSuccess;
        float* const bufs[4] = {b.albedo, b.normal, b.depth, b.coverage};
        const size_t floats[4] = {3u, 3u, 1u, 1u};
        for (int i = 0; i < 4; i++) {
            if (!bufs[i]) continue;
            const hipError_t e = hipMemsetAsync(bufs[i], 0, (size_t)n * floats[i] * sizeof(float), stream);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    SceneDev scd = qs.scene;
    BatchLaunch bl;
    const hipError_t e = batch_prepare(scd, n, kAovKernels, kAovShapes, bl);
    if (e != hipSuccess) return e;
    const trt_query_plan& q = bl.q;
    CameraDev cam = cd;
    ra.flat_reuse = qs.flat_reuse;
    AovArgs aa{b.albedo, b.normal, b.depth, b.coverage, b.geometry, b.material, qs.geo_index, n, q.rays_per_wave, q.leaf_slots, q.stragglers};
    void* args[] = {&scd, &cam, &ra, &aa, &bl.leaf_list, &bl.nodes16};
    return hipLaunchKernel(bl.fn, dim3(q.workgroups), dim3(q.threads_per_workgroup), args, q.lds_bytes, stream);
}

// TRT_ERR_INVALID_ARG before any device work, then TRT_ERR_NO_DEVICE (the queries' order).
int aov_check(const trt_scene* s, const trt_camera* cam, const trt_render_params* p, const trt_aov_buffers* b, RenderArgs& ra, uint32_t& rows,
              CameraDev& cd) {
    if (!s || !cam || !p || !b) return query_fail(TRT_ERR_INVALID_ARG, "null argument");
    if (!any_buffer(b)) return query_fail(TRT_ERR_INVALID_ARG, "no buffer is wanted: all six pointers are null");
    const int rc = batch_render_args(cam, p, ra, rows, cd);
    if (rc != TRT_OK) return rc;
    return query_require_device();
}

int rays_check(const trt_camera* cam, const trt_render_params* p, uint32_t s, const trt_ray* rays, RenderArgs& ra, uint32_t& rows, CameraDev& cd) {
    if (!cam || !p) return query_fail(TRT_ERR_INVALID_ARG, "null argument");
    if (s >= p->samples_per_pixel) return query_fail(TRT_ERR_INVALID_ARG, "sample index must be below samples_per_pixel");
    trt_render_params q = *p;                                       // seed and bands only: the sample range is not read
    q.sample_begin = 0u;
    q.sample_end = 0u;
    const int rc = batch_render_args(cam, &q, ra, rows, cd);
    if (rc != TRT_OK) return rc;
    if (rows && !rays) return query_fail(TRT_ERR_INVALID_ARG, "null buffer");
    return query_require_device();
}

hipError_t launch_primary_rays(const CameraDev& cd, const RenderArgs& ra, uint32_t s, uint32_t n, trt_ray* d_rays, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    primary_rays_kernel<<<dim3((n + 255u) / 256u), dim3(256), 0, stream>>>(cd, ra, s, n, reinterpret_cast<float*>(d_rays));
    return hipGetLastError();
}

}  // namespace
}  // namespace trt

extern "C" {

int trt_primary_rays_device(const trt_camera* cam, const trt_render_params* p, uint32_t s, trt_ray* d_rays, void* stream) {
    trt::RenderArgs ra;
    trt::CameraDev cd;
    uint32_t rows = 0;
    const int rc = trt::rays_check(cam, p, s, d_rays, ra, rows, cd);
    if (rc != TRT_OK) return rc;
    const hipError_t e = trt::launch_primary_rays(cd, ra, s, rows * cam->width, d_rays, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return trt::query_fail_hip(e, "primary ray launch");
    return TRT_OK;
}

// Host buffer: a device copy of the call's own on the default stream, complete when the call returns.
int trt_primary_rays(const trt_camera* cam, const trt_render_params* p, uint32_t s, trt_ray* rays) {
    return trt::host_form([&]() -> int {
        trt::RenderArgs ra;
        trt::CameraDev cd;
        uint32_t rows = 0;
        const int rc = trt::rays_check(cam, p, s, rays, ra, rows, cd);
        if (rc != TRT_OK) return rc;
        const uint32_t n = rows * cam->width;
        if (n == 0) return TRT_OK;
        trt::HostStage st("primary ray buffer");
        const size_t r_rays = st.reserve((size_t)n * sizeof(trt_ray));
        st.alloc();
        if (st.ok()) st.run(trt::launch_primary_rays(cd, ra, s, n, st.ptr<trt_ray>(r_rays), nullptr), "primary ray launch");
        st.down(rays, r_rays, (size_t)n * sizeof(trt_ray), "hipMemcpy of the rays");
        return st.finish();
    });
}

int trt_render_aov_device(trt_scene* s, const trt_camera* cam, const trt_render_params* p, const trt_aov_buffers* d_buffers, void* stream) {
    trt::RenderArgs ra;
    trt::CameraDev cd;
    uint32_t rows = 0;
    int rc = trt::aov_check(s, cam, p, d_buffers, ra, rows, cd);
    if (rc != TRT_OK) return rc;
    trt::QueryScene qs;
    rc = trt::query_scene_on_device(s, qs);
    if (rc != TRT_OK) return rc;
    const hipError_t e = trt::launch_aov(qs, cd, ra, rows * cam->width, *d_buffers, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return trt::query_fail_hip(e, "feature buffer launch");
    return TRT_OK;
}

// Host buffers: device copies of the ones wanted, one stream-ordered sequence on the default stream, complete when the call returns.
int trt_render_aov(trt_scene* s, const trt_camera* cam, const trt_render_params* p, const trt_aov_buffers* buffers) {
    return trt::host_form([&]() -> int {
        trt::RenderArgs ra;
        trt::CameraDev cd;
        uint32_t rows = 0;
        int rc = trt::aov_check(s, cam, p, buffers, ra, rows, cd);
        if (rc != TRT_OK) return rc;
        const uint32_t n = rows * cam->width;
        if (n == 0) return TRT_OK;
        trt::QueryScene qs;
        rc = trt::query_scene_on_device(s, qs);
        if (rc != TRT_OK) return rc;
        void* const host[6] = {buffers->albedo, buffers->normal, buffers->depth, buffers->coverage, buffers->geometry, buffers->material};
        const size_t item[6] = {12u, 12u, 4u, 4u, 4u, 4u};
        trt::HostStage st("feature buffers");
        size_t r[6];
        for (int i = 0; i < 6; i++) r[i] = st.reserve(trt::q_align16((size_t)n * item[i]), host[i] != nullptr);      // (whole 16s: the last one too)
        st.alloc();
        // what the pass does not write goes up first: the running sums it continues, the indices if it does not hold sample 0
        const bool sums_up = ra.accumulate != 0u, indices_up = !(ra.sample_begin == 0u && ra.sample_end > 0u);
        for (int i = 0; i < 6; i++)
            if (i < 4 ? sums_up : indices_up) st.up(r[i], host[i], (size_t)n * item[i], "hipMemcpy of the buffers");
        const trt_aov_buffers db{st.ptr<float>(r[0]), st.ptr<float>(r[1]), st.ptr<float>(r[2]), st.ptr<float>(r[3]), st.ptr<uint32_t>(r[4]), st.ptr<uint32_t>(r[5])};
        if (st.ok()) st.run(trt::launch_aov(qs, cd, ra, n, db, nullptr), "feature buffer launch");
        for (int i = 0; i < 6; i++) st.down(host[i], r[i], (size_t)n * item[i], "hipMemcpy of the results");
        return st.finish();
    });
}

// How launch_aov would launch a local image of n_pixels on this scene.
int trt_aov_launch_plan(const trt_scene* s, uint32_t n_pixels, uint32_t compute_units, trt_query_plan* out) {
    return trt::batch_launch_plan(s, n_pixels, compute_units, trt::kAovKernels, trt::kAovShapes, out);
}

}  // extern "C"
