// capi.hip — the extern "C" boundary declared in include/tinyrt.h.
//
// Mirrors the reference's World / Camera / Renderer::render() surface (hittable/world.rs:16-45,
// camera.rs:17-56, renderer/renderer.rs:21-79) as opaque handles + POD structs.  The reference
// panics on misuse; here every failure is a negative status plus a thread-local message, and no
// C++ exception leaves this file.  There is no CPU fallback: without a gfx950 device every
// compute entry point fails with TRT_ERR_NO_DEVICE.
//
// What a scene keeps on its devices, and the scaffold of the blocking entry points, are scene_cache.h.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "axis_quads.h"
#include "nearest_first.h"
#include "flat_reuse.h"
#include "host_stage.h"
#include "kernels.h"
#include "scene.h"
#include "scene_adopt.h"
#include "scene_cache.h"
#include "scene_facts.h"
#include "scene_query.h"
#include "stream_plan.h"

using namespace trt;

struct trt_world {
    World w;
};

// trt_kernel_timing_begin / _end: HIP events around every dominant-kernel launch.  A launcher calls timing_mark(stream, true)
// before and timing_mark(stream, false) after the launch ON THE SAME HOST THREAD, so the open `begin` is thread-local: pairs
// never mix threads, streams or devices (round 2 kept one process-wide list and paired marks by parity).
namespace trt {
namespace {
std::mutex g_timing_mu;
bool g_timing_on = false;
unsigned g_timing_epoch = 0;                              // bumped by every _begin: a stale thread-local `begin` is dropped
struct TimingPair { hipEvent_t begin, end; int device; };
std::vector<TimingPair> g_timing_pairs;                   // completed pairs, appended under g_timing_mu
struct TimingOpen { hipEvent_t ev = nullptr; hipStream_t stream = nullptr; int device = -1; unsigned epoch = 0; };
thread_local TimingOpen t_open;
}  // namespace
void timing_mark(hipStream_t stream, bool begin) {
    unsigned epoch;
    {
        std::lock_guard<std::mutex> lock(g_timing_mu);
        if (!g_timing_on) return;
        epoch = g_timing_epoch;
    }
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return; }
    if (begin) {
        if (t_open.ev) { (void)hipEventDestroy(t_open.ev); t_open = TimingOpen{}; }       // a begin without its end: dropped
        hipEvent_t ev = nullptr;
        if (hipEventCreate(&ev) != hipSuccess) { (void)hipGetLastError(); return; }
        if (hipEventRecord(ev, stream) != hipSuccess) { (void)hipGetLastError(); (void)hipEventDestroy(ev); return; }
        t_open.ev = ev; t_open.stream = stream; t_open.device = dev; t_open.epoch = epoch;
        return;
    }
    if (!t_open.ev) return;
    TimingOpen o = t_open;
    t_open = TimingOpen{};
    hipEvent_t ev = nullptr;
    if (o.stream != stream || o.device != dev || o.epoch != epoch || hipEventCreate(&ev) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipEventDestroy(o.ev);
        return;
    }
    if (hipEventRecord(ev, stream) != hipSuccess) { (void)hipGetLastError(); (void)hipEventDestroy(ev); (void)hipEventDestroy(o.ev); return; }
    std::lock_guard<std::mutex> lock(g_timing_mu);
    if (g_timing_on && g_timing_epoch == epoch) g_timing_pairs.push_back(TimingPair{o.ev, ev, dev});
    else { (void)hipEventDestroy(o.ev); (void)hipEventDestroy(ev); }
}
}  // namespace trt

struct trt_scene {
    SceneHost host;
    FlatReuse flat_reuse{};                       // the lock-step leaf walk's reuse schedule (flat_reuse.h) and axis-exact-quads switch (axis_quads.h), derived once from host.blob
    SceneFacts facts;                             // what the scene's own kernel may be told about it (scene_facts.h), derived with flat_reuse; TRT_SCENE_FACTS=0: nothing
    std::vector<uint32_t> geo_index;              // ray queries: geometry insertion index of sphere k at [k], of quad k at [n_spheres + k] (the kernels know a
                                                  // primitive as kind bit | index within its kind); derived once from the reference tree, outside the packed scene
    SceneCache cache;                             // what the scene keeps on its devices (scene_cache.h); destroyed with the handle
};

namespace {

thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}
int fail_hip(hipError_t e, const char* what) {
    return fail(TRT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define TRT_HIP(call)                                        \
    do {                                                     \
        hipError_t e_ = (call);                              \
        if (e_ != hipSuccess) return fail_hip(e_, #call);    \
    } while (0)

// The library defaults: the built-in values (kernels.h tuning_builtin, scene_host.cpp scene_options_builtin), overridden by the TRT_*
// environment variables ONCE (a function-local static: initialised exactly once, thread-safe; first touched when the library is loaded).  This is
// the only place the library reads its environment; nothing on the launch path does (round 3 read it in 21 places there).
struct Defaults {
    trt_tuning tuning;
    trt_scene_options scene;
    bool flat_reuse = true;                       // TRT_FLAT_REUSE=0: the lock-step leaf walk computes every leaf box in full (A/B runs, tests)
    bool axis_quads = true;                       // TRT_AXIS_QUADS=0: the lock-step kernel keeps the generic quad test on axis-exact scenes too (A/B runs, tests)
    bool nearest_first = true;                    // TRT_NEAREST_FIRST=0: the lock-step kernel keeps the walk-order leaf phase on all-axis-exact-quad scenes too (A/B runs, tests)
    uint32_t flat_literal = 2;                    // TRT_FLAT_LITERAL: the lock-step kernel compiled per scene at run time (literal_kernel.h): 0 never, 1 at the first
                                                  // streamed render of the scene, unset (2): at the first render call of kLiteralAutoSamples samples or more
    bool flat_literal_test_fail = false;          // TRT_FLAT_LITERAL_TEST_FAIL=1: that compilation is handed an empty source (tests of the fallback)
    uint32_t flat_literal_pairs = kLiteralIntervalPairs;   // TRT_FLAT_LITERAL_PAIRS (3 ... 8), TRT_FLAT_LITERAL_PLANES (0 ... 8): the registers of that kernel's
    uint32_t flat_literal_planes = kLiteralPlaneRegs;      // interval cache (flat_literal.h); a value out of range leaves the built-in one; 3 and 0: no cache
    uint32_t scene_facts = SCENE_FACTS_ALL;       // TRT_SCENE_FACTS: what that kernel is told about its scene (scene_facts.h): 0 nothing, 1 the facts as constants,
                                                  // anything else and unset: those and the straight-line shade (A/B runs, tests)
};
const Defaults& defaults() {
    static const Defaults d = [] {
        Defaults x;
        x.tuning = tuning_builtin();
        x.scene = scene_options_builtin();
        auto env = [](const char* name) -> const char* { const char* e = getenv(name); return (e && *e) ? e : nullptr; };
        auto u32 = [&](const char* name, uint32_t& field) { if (const char* e = env(name)) field = (uint32_t)strtoul(e, nullptr, 10); };
        trt_tuning& t = x.tuning;
        u32("TRT_STREAM_MINW", t.stream_waves_per_simd); u32("TRT_BIG_THREADS", t.stream_big_threads); u32("TRT_STREAM_BATCH_SPP", t.stream_batch_spp);
        u32("TRT_RADIANCE_GB", t.radiance_gb); u32("TRT_LEAF_SLOTS", t.leaf_slots); u32("TRT_LDS_LEAF_STACK", t.lds_leaf_stack);
        u32("TRT_RAY_POOL", t.ray_pool); u32("TRT_STRAGGLERS", t.stragglers); u32("TRT_LDS_STRAGGLERS", t.lds_stragglers);
        u32("TRT_DUAL_WALK", t.dual_walk); u32("TRT_RUNTIME_WALK", t.runtime_walk); u32("TRT_XCD_REMAP", t.xcd_remap);
        u32("TRT_MINW", t.mega_waves_per_simd); u32("TRT_MEGA_THREADS", t.mega_threads); u32("TRT_MINW8", t.mega_global_waves8);
        u32("TRT_WF_MINW", t.wf_waves_per_simd); u32("TRT_WF_SERVE_MIN", t.wf_serve_min);
        trt_scene_options& o = x.scene;
        if (const char* e = env("TRT_CULL_PRUNE")) {                       // outside (0, 1] (or not a number): the built-in value stays (such a
            const float v = (float)atof(e);                                //   value made every trt_scene_create of the process fail with INVALID_ARG)
            if (v > 0.0f && v <= 1.0f) o.cull_prune = v;
        }
        if (const char* e = env("TRT_FLAT_WALK")) o.flat_walk = atoi(e) ? 1 : 0;
        if (const char* e = env("TRT_FLAT_REUSE")) x.flat_reuse = atoi(e) != 0;
        if (const char* e = env("TRT_AXIS_QUADS")) x.axis_quads = atoi(e) != 0;
        if (const char* e = env("TRT_NEAREST_FIRST")) x.nearest_first = atoi(e) != 0;
        if (const char* e = env("TRT_FLAT_LITERAL")) x.flat_literal = atoi(e) != 0 ? 1u : 0u;
        if (const char* e = env("TRT_FLAT_LITERAL_TEST_FAIL")) x.flat_literal_test_fail = atoi(e) != 0;
        if (const char* e = env("TRT_FLAT_LITERAL_PAIRS")) { const int v = atoi(e); if (v >= 3 && v <= 8) x.flat_literal_pairs = (uint32_t)v; }
        if (const char* e = env("TRT_FLAT_LITERAL_PLANES")) { const int v = atoi(e); if (v >= 0 && v <= 8 && *e >= '0' && *e <= '9') x.flat_literal_planes = (uint32_t)v; }
        if (const char* e = env("TRT_SCENE_FACTS")) {                      // "0" and "1" as numbers; anything else, text included: all
            char* end = nullptr;
            const long v = strtol(e, &end, 10);
            const bool number = end != e && *end == '\0';
            x.scene_facts = (number && v == 0) ? SCENE_FACTS_NONE : (number && v == 1) ? SCENE_FACTS_CONSTANTS : SCENE_FACTS_ALL;
        }
        if (const char* e = env("TRT_COMPACT_NODES")) o.compact_nodes = atoi(e) ? 1 : 0;
        if (const char* e = env("TRT_SCRATCH_CAP_MB")) o.scratch_cap_bytes = (uint64_t)strtoull(e, nullptr, 10) << 20;
        return x;
    }();
    return d;
}

// ... and that first need is the library's own load: a namespace-scope initialiser, so that "once, at load" holds whatever the host does later
[[maybe_unused]] const bool g_defaults_read_at_load = (defaults(), true);

int require_device() {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return fail(TRT_ERR_NO_DEVICE, "no HIP device visible: libtinyrt has no CPU path, it needs a gfx950 GPU");
    }
    return TRT_OK;
}

// The packed scene on the current device, uploaded on first use.
int scene_on_device(trt_scene* s, SceneDev& out) {
    out.L = s->host.layout;
    return s->cache.on_device(SceneCache::PACKED_SCENE, s->host.blob.data(), s->host.layout.blob_bytes, "scene upload", out.blob);
}

void to_camera_dev(const trt_camera& c, CameraDev& d) {
    const trt_vec3* src[6] = {&c.position, &c.viewport_upper_left, &c.horizontal, &c.vertical, &c.defocus_disk_u, &c.defocus_disk_v};
    float* dst[6] = {d.pos, d.upper_left, d.horizontal, d.vertical, d.du, d.dv};
    for (int i = 0; i < 6; i++) { dst[i][0] = src[i]->x; dst[i][1] = src[i]->y; dst[i][2] = src[i]->z; }
    d.width = c.width;
    d.height = c.height;
}

// Validates params against the camera and fills the kernel arguments.  rows = rows the call owns.
int to_render_args(const trt_camera* cam, const trt_render_params* p, RenderArgs& ra, uint32_t& rows, trt_tuning& tn) {
    if (cam->width < 2 || cam->height < 2) return fail(TRT_ERR_INVALID_ARG, "camera width and height must be at least 2 (pointgen.rs:41-42 divides by width-1, height-1)");
    if (p->samples_per_pixel == 0) return fail(TRT_ERR_INVALID_ARG, "samples_per_pixel must be positive");
    uint32_t s1 = p->sample_end == 0 ? p->samples_per_pixel : p->sample_end;
    if (p->sample_begin > s1 || s1 > p->samples_per_pixel) return fail(TRT_ERR_INVALID_ARG, "sample range must satisfy begin <= end <= samples_per_pixel");
    if (p->backend > TRT_BACKEND_STREAMED) return fail(TRT_ERR_INVALID_ARG, "unknown backend");
    ra.background[0] = p->background.x; ra.background[1] = p->background.y; ra.background[2] = p->background.z;
    ra.inv_spp = 1.0f / (float)p->samples_per_pixel;
    ra.max_bounces = p->max_bounces;
    ra.seed_key = rng_seed_key(p->seed);
    ra.sample_begin = p->sample_begin;
    ra.sample_end = s1;
    ra.accumulate = p->accumulate ? 1u : 0u;
    if (p->band_rows == 0) {
        ra.band_rows = 0; ra.band_stride = 1; ra.band_offset = 0;
        rows = cam->height;
    } else {
        if (p->band_stride == 0 || p->band_offset >= p->band_stride) return fail(TRT_ERR_INVALID_ARG, "band_offset must be below band_stride");
        rows = p->rows_local;
        if (rows > 0) {
            uint32_t last = rows - 1;
            uint64_t y = ((uint64_t)(last / p->band_rows) * p->band_stride + p->band_offset) * p->band_rows + last % p->band_rows;
            if (y >= cam->height) return fail(TRT_ERR_INVALID_ARG, "rows_local maps past the last image row");
        }
        ra.band_rows = p->band_rows; ra.band_stride = p->band_stride; ra.band_offset = p->band_offset;
    }
    ra.rows_local = rows;
    // scheduling (tinyrt.h trt_tuning): the caller's, else the library defaults; scheduling only, any value renders the same frame
    tn = p->tuning ? *p->tuning : defaults().tuning;
    // whatever a caller writes into the knobs, the launch arithmetic stays in range (the launch plan clamps waves, lanes and slots itself)
    if (tn.stream_batch_spp > 256u) tn.stream_batch_spp = 256u;      // a batch is at most one launch's samples of a tile
    if (tn.stragglers > 63u) tn.stragglers = 63u;
    if (tn.lds_stragglers > 63u) tn.lds_stragglers = 63u;
    if (tn.radiance_gb > 64u) tn.radiance_gb = 64u;
    ra.leaf_slots = tn.leaf_slots;                         // rt_path.h walk_fast; 0 = the backend's default
    ra.lds_leaf_stack = tn.lds_leaf_stack;                 // 0 off, 1 where it costs no occupancy, 2 always
    ra.xcd_aware = tn.xcd_remap ? 1u : 0u;                 // off: contiguous image regions per XCD measured 2x slower (load imbalance)
    ra.stragglers = tn.stragglers;                         // profiles/r03_stragglers_sweep.txt
    ra.ref_tree = p->collect_stats == 1 ? 1u : 0u;      // 1: counters comparable with the CPU path; 2: count the culling tree's own tests
    ra.flat_reuse = FlatReuse{0u, 0u, 0u};                 // the scene's schedule is filled in by enqueue_render
    return TRT_OK;
}

// The argument errors of to_render_args alone.  rows = rows the call owns.
int check_render_args(const trt_camera* cam, const trt_render_params* p, uint32_t& rows) {
    RenderArgs ra;
    trt_tuning tn;
    return to_render_args(cam, p, ra, rows, tn);
}

// `d_moment2` with `launch_moments` (trt_render_moments*, streamed backend only - query_render_moments* refuse every other): a second
// frame-shaped buffer for the second moments and the launcher that fills both (scene_query.h MomentsLaunch).
int enqueue_render(trt_scene* s, const trt_camera* cam, const trt_render_params* p, float* d_accum, uint64_t* d_counters,
                   hipStream_t stream, uint32_t* rows_out, float* d_moment2 = nullptr, MomentsLaunch launch_moments = nullptr) {
    RenderArgs ra;
    trt_tuning tn;
    uint32_t rows = 0;
    int rc = to_render_args(cam, p, ra, rows, tn);
    if (rc != TRT_OK) return rc;
    if (rows_out) *rows_out = rows;
    SceneDev sc;
    rc = scene_on_device(s, sc);
    if (rc != TRT_OK) return rc;
    CameraDev cd;
    to_camera_dev(*cam, cd);
    ra.flat_reuse = s->flat_reuse;
    const size_t bytes = (size_t)rows * cam->width * 3 * sizeof(float);
    if (rows == 0 || ra.sample_begin == ra.sample_end || ra.max_bounces == 0) {
        // nothing to trace: a path with no bounce budget returns colour 0 (cpu.rs:43-47,64)
        if (!ra.accumulate && bytes) TRT_HIP(hipMemsetAsync(d_accum, 0, bytes, stream));
        if (!ra.accumulate && bytes && d_moment2) TRT_HIP(hipMemsetAsync(d_moment2, 0, bytes, stream));
        return TRT_OK;
    }
    const bool wavefront = p->backend == TRT_BACKEND_WAVEFRONT;
    const bool streamed = p->backend == TRT_BACKEND_STREAMED || p->backend == TRT_BACKEND_AUTO;     // fastest on every scene measured
    if (wavefront || streamed) {
        // Device workspace (wavefront: 72 B of path state per pixel; streamed: 12 B per pixel and sample of a launch), private
        // to this render until its last kernel has run (SceneCache::workspace_acquire): concurrent renders of one scene are safe.
        int dev = 0;
        TRT_HIP(hipGetDevice(&dev));
        Workspace* ws = nullptr;
        if (wavefront) {
            rc = s->cache.workspace_acquire(dev, wavefront_workspace_bytes(cam->width, rows), stream, &ws);
        } else {
            // The streamed launch is sized for 288 GB (up to 16 GB of records).  If the device cannot give that much right now - HBM held by
            // another scene's cached scratch, by the host application, by torch - ask for half the samples per launch, and half again: the
            // render then runs more, shorter launches (same frame: the fold adds the samples in order whatever the launch boundaries).
            uint32_t samples = ra.sample_end - ra.sample_begin;
            const uint32_t full = streamed_chunk_spp(cam->width, rows, tn.radiance_gb);
            if (samples > full) samples = full;
            const uint32_t wanted = samples;
            // Lasting pressure: while the device still cannot hold the full request, start where the last render ended up instead
            // of freeing the cached shorter workspace, failing the full-size hipMalloc and allocating the shorter one again on every render.
            // hipMemGetInfo says when the pressure is gone: free memory + this scene's own idle scratch (a regrow frees it first) covers the request.
            const uint32_t short_samples = s->cache.short_samples(dev);
            if (short_samples != 0u && short_samples < samples) {
                const size_t idle = s->cache.idle_workspace_bytes(dev);
                size_t free_b = 0, total_b = 0;
                const bool known = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
                (void)hipGetLastError();
                if (!known || free_b + idle < streamed_workspace_bytes(cam->width, rows, samples, tn.radiance_gb)) samples = short_samples;
            }
            bool trimmed = false;
            for (;;) {
                rc = s->cache.workspace_acquire(dev, streamed_workspace_bytes(cam->width, rows, samples, tn.radiance_gb), stream, &ws);
                if (rc != TRT_ERR_OOM) break;
                if (!trimmed) {                      // first give back what this scene itself keeps idle on the device (frames of idle contexts, other workspaces), then ask again
                    trimmed = true;
                    s->cache.trim(dev, 0);
                    continue;
                }
                if (samples <= 1u) break;
                samples = (samples + 1u) / 2u;
            }
            s->cache.set_short_samples(dev, (rc == TRT_OK && samples < wanted) ? samples : 0u);
        }
        if (rc != TRT_OK) return rc;
        // the scene's own kernel (literal_kernel.h): the streamed launcher finds this request for the length of its call
        LiteralRequest lit;
        const SceneLayout& L = s->host.layout;
        if (streamed && defaults().flat_literal != 0u && L.flat_walk != 0u && L.n_leaves > 0u &&
            s->host.blob.size() >= 16u * ((size_t)L.off_leaf_list + 2u * (size_t)L.n_leaves)) {
            lit.slot = s->cache.literal_kernel(dev);
            lit.leaf_list = s->host.blob.data() + 16u * (size_t)L.off_leaf_list;
            lit.n_leaves = L.n_leaves;
            const uint64_t call_samples = (uint64_t)cam->width * rows * (ra.sample_end - ra.sample_begin);
            lit.wanted = defaults().flat_literal == 1u || call_samples >= kLiteralAutoSamples;
            lit.empty_source = defaults().flat_literal_test_fail;
            // TRT_FLAT_REUSE=0 asks for every box in full: no cache either
            lit.interval_pairs = defaults().flat_reuse ? defaults().flat_literal_pairs : 3u;
            lit.plane_regs = defaults().flat_reuse ? defaults().flat_literal_planes : 0u;
            lit.facts = s->facts;
        }
        const LiteralScope lit_scope(lit.slot ? &lit : nullptr);
        hipError_t le;
        if (streamed && d_moment2) {
            le = launch_moments ? launch_moments(sc, cd, ra, tn, ws->ptr, ws->bytes, d_accum, d_moment2, reinterpret_cast<unsigned long long*>(d_counters),
                                                 p->collect_stats != 0, stream)
                                : hipErrorInvalidDeviceFunction;                 // no launcher handed over: a bug, never a fallback
        } else if (streamed) {
            le = launch_streamed(sc, cd, ra, tn, ws->ptr, ws->bytes, d_accum, reinterpret_cast<unsigned long long*>(d_counters), p->collect_stats != 0, stream);
        } else {
            le = launch_wavefront(sc, cd, ra, tn, ws->ptr, d_accum, reinterpret_cast<unsigned long long*>(d_counters), p->collect_stats != 0, stream);
        }
        rc = s->cache.workspace_release(dev, ws, stream);
        if (le != hipSuccess) return fail_hip(le, streamed ? "launch_streamed" : "launch_wavefront");
        return rc;
    }
    TRT_HIP(launch_megakernel(sc, cd, ra, tn, d_accum, reinterpret_cast<unsigned long long*>(d_counters), p->collect_stats != 0, stream));
    return TRT_OK;
}

// The reuse schedule of a flat-walk scene's leaf list and its axis-exact-quads switch, from the host copy of its blob (both scene compilers leave one).
void set_flat_reuse(trt_scene* s) {
    const SceneLayout& L = s->host.layout;
    const size_t end = 16u * ((size_t)L.off_leaf_list + 2u * (size_t)L.n_leaves);
    const bool have = L.flat_walk != 0u && L.n_leaves > 0u && s->host.blob.size() >= end;
    uint32_t m[3];
    flat_reuse_masks(have ? s->host.blob.data() + 16u * (size_t)L.off_leaf_list : nullptr, L.n_leaves, have && defaults().flat_reuse, m);
    // ... and whether every quad is axis-exact (axis_quads.h): the lock-step kernel then runs the two-dot-product inside test
    const size_t qend = 16u * ((size_t)L.off_quad + 5u * (size_t)L.n_quads);
    const bool have_quads = have && L.n_quads > 0u && s->host.blob.size() >= qend;
    const uint32_t aq = axis_quads_flag(have_quads ? s->host.blob.data() + 16u * (size_t)L.off_quad : nullptr, L.n_quads, L.n_leaves, L.flat_walk != 0u,
                                        scene_mode(L) == 1, defaults().axis_quads);
    // ... and whether the leaf phase may test the nearest pending leaf first, with the planes its margin is built from (nearest_first.h)
    float planes[3];
    const uint32_t nf = nearest_first_flag(have ? s->host.blob.data() + 16u * (size_t)L.off_leaf_list : nullptr, L.n_leaves,
                                           have_quads ? s->host.blob.data() + 16u * (size_t)L.off_quad : nullptr, L.n_quads, L.n_spheres, aq,
                                           defaults().nearest_first, planes);
    s->flat_reuse = FlatReuse{m[0], m[1], m[2], aq, nf, planes[0], planes[1], planes[2]};
    // ... and what the kernel compiled for this scene may take as constants (scene_facts.h), from the same host copy
    const size_t kend = 4u * ((size_t)L.off_material_kind + L.n_materials), smend = 4u * ((size_t)L.off_sphere_mat + L.n_spheres);
    const bool have_mats = have && s->host.blob.size() >= kend && s->host.blob.size() >= smend && (L.n_quads == 0u || have_quads);
    s->facts = have_mats ? scene_facts_derive(s->host.blob.data() + 16u * (size_t)L.off_leaf_list, L.n_leaves,
                                              have_quads ? s->host.blob.data() + 16u * (size_t)L.off_quad : nullptr, L.n_quads, L.n_spheres,
                                              reinterpret_cast<const uint32_t*>(s->host.blob.data()) + L.off_sphere_mat,
                                              reinterpret_cast<const uint32_t*>(s->host.blob.data()) + L.off_material_kind, L.n_materials, aq, nf,
                                              L.lazy_color, defaults().scene_facts)
                           : SceneFacts{};
}

// The per-kind -> insertion-index table of the ray queries, from what both scene compilers leave on the handle: leaf i of the reference tree's
// dump names its geometry (prim_geo), the packed node's link names the same primitive the kernels' way.
void set_geo_index(trt_scene* s) {
    const SceneLayout& L = s->host.layout;
    const std::vector<int32_t>& geo = s->host.reference.prim_geo;
    s->geo_index.assign((size_t)L.n_spheres + L.n_quads, 0xFFFFFFFFu);
    const size_t end = 16u * ((size_t)L.off_ref_nodes + 2u * (size_t)L.n_nodes);
    if (geo.size() < L.n_nodes || s->host.blob.size() < end) return;
    for (uint32_t i = 0; i < L.n_nodes; i++) {
        if (geo[i] < 0) continue;
        uint32_t link;
        memcpy(&link, s->host.blob.data() + 16u * ((size_t)L.off_ref_nodes + 2u * (size_t)i + 1u) + 12u, 4);
        const size_t slot = (size_t)(link & PRIM_INDEX_MASK) + ((link & PRIM_QUAD_BIT) ? L.n_spheres : 0u);
        if (!(link & NODE_INNER_BIT) && slot < s->geo_index.size()) s->geo_index[slot] = (uint32_t)geo[i];
    }
}

// The handle of a compiled scene: what both scene compilers' entry points end in.  May throw std::bad_alloc.
trt_scene* scene_from_host(SceneHost&& host, const trt_scene_options& opt) {
    std::unique_ptr<trt_scene> s(new trt_scene());
    s->host = std::move(host);
    set_flat_reuse(s.get());
    set_geo_index(s.get());
    s->cache.set_cap((size_t)opt.scratch_cap_bytes);
    return s.release();
}

}  // namespace

// The ray-query unit's view of this layer (scene_query.h)
namespace trt {
int query_fail(int code, const std::string& msg) { return fail(code, msg); }
int query_fail_hip(hipError_t e, const char* what) { return fail_hip(e, what); }
int query_require_device() { return require_device(); }
const SceneLayout& query_scene_layout(const trt_scene* s) { return s->host.layout; }
// The scene and its index table on the current device, both uploaded on first use (SceneCache::on_device).
int query_scene_on_device(trt_scene* s, QueryScene& out) {
    int rc = scene_on_device(s, out.scene);
    if (rc != TRT_OK) return rc;
    out.flat_reuse = s->flat_reuse;
    return s->cache.on_device(SceneCache::GEO_INDEX, s->geo_index.data(), s->geo_index.size() * sizeof(uint32_t), "geometry index upload", out.geo_index);
}
int query_render_args(const trt_camera* cam, const trt_render_params* p, RenderArgs& ra, uint32_t& rows) {
    trt_render_params q = *p;
    q.backend = TRT_BACKEND_AUTO;
    q.tuning = nullptr;
    trt_tuning tn;
    return to_render_args(cam, &q, ra, rows, tn);
}
void query_camera_dev(const trt_camera& cam, CameraDev& out) { to_camera_dev(cam, out); }
}  // namespace trt

// The device scene compiler's view of this layer (scene_adopt.h)
namespace trt {
int scene_options_check(const trt_scene_options& opt) {
    if (!(opt.cull_prune > 0.0f && opt.cull_prune <= 1.0f)) return fail(TRT_ERR_INVALID_ARG, "cull_prune must be in (0, 1]");
    return TRT_OK;
}
trt_scene_options scene_options_or_defaults(const trt_scene_options* options) { return options ? *options : defaults().scene; }
int scene_fail(int code, const std::string& msg) { return fail(code, msg); }
const World& world_of(const trt_world* w) { return w->w; }
trt_scene* scene_adopt(SceneHost&& host, const trt_scene_options& opt, int device, void* d_blob) {
    try {
        trt_scene* s = scene_from_host(std::move(host), opt);
        if (d_blob) s->cache.adopt_packed_scene(device, d_blob);             // the first render on `device` does not upload again
        return s;
    } catch (const std::bad_alloc&) {
        fail(TRT_ERR_OOM, "out of memory");
        return nullptr;
    }
}
}  // namespace trt

extern "C" {

uint32_t trt_abi_version(void) { return TRT_ABI_VERSION; }
const char* trt_last_error(void) { return g_last_error.c_str(); }

int trt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}
int trt_set_device(int ordinal) {
    int rc = require_device();
    if (rc != TRT_OK) return rc;
    TRT_HIP(hipSetDevice(ordinal));
    return TRT_OK;
}

// ---- World ----
int trt_world_create(trt_world** out) {
    if (!out) return fail(TRT_ERR_INVALID_ARG, "out is null");
    trt_world* w = new (std::nothrow) trt_world();
    if (!w) return fail(TRT_ERR_OOM, "out of memory");
    *out = w;
    return TRT_OK;
}
void trt_world_destroy(trt_world* w) { delete w; }

int trt_world_add_material(trt_world* w, const char* name, const trt_material* m) {
    if (!w || !name || !m) return fail(TRT_ERR_INVALID_ARG, "null argument");
    if (m->kind > TRT_LIGHT) return fail(TRT_ERR_INVALID_ARG, "unknown material kind");
    try {
        std::string key(name);
        if (w->w.material_index.count(key)) return fail(TRT_ERR_DUPLICATE, key + " key is already in the material table");   // world.rs:30
        trt_material mm = *m;
        if (mm.kind == TRT_METAL) mm.param = fminf(fmaxf(mm.param, 0.0f), 1.0f);      // Metal::new clamps fuzz (metal.rs:12-14)
        w->w.material_index.emplace(key, (uint32_t)w->w.materials.size());
        w->w.materials.push_back(mm);
    } catch (const std::bad_alloc&) {
        return fail(TRT_ERR_OOM, "out of memory");
    }
    return TRT_OK;
}
int trt_world_get_material(const trt_world* w, const char* name, uint32_t* index) {
    if (!w || !name || !index) return fail(TRT_ERR_INVALID_ARG, "null argument");
    auto it = w->w.material_index.find(name);
    if (it == w->w.material_index.end()) return fail(TRT_ERR_NOT_FOUND, std::string("no material named ") + name);
    *index = it->second;
    return TRT_OK;
}
int trt_world_add_sphere(trt_world* w, trt_vec3 center, float radius, uint32_t material) {
    if (!w) return fail(TRT_ERR_INVALID_ARG, "world is null");
    if (material >= w->w.materials.size()) return fail(TRT_ERR_INVALID_ARG, "material index out of range");
    try {
        w->w.geometries.push_back(Geometry{0u, material, center, trt_vec3{radius, 0.0f, 0.0f}, trt_vec3{0.0f, 0.0f, 0.0f}});
    } catch (const std::bad_alloc&) {
        return fail(TRT_ERR_OOM, "out of memory");
    }
    return TRT_OK;
}
int trt_world_add_spheres(trt_world* w, uint32_t n, const float* center_radius, const uint32_t* material) {
    if (!w) return fail(TRT_ERR_INVALID_ARG, "world is null");
    if (n == 0) return TRT_OK;
    if (!center_radius || !material) return fail(TRT_ERR_INVALID_ARG, "null array");
    for (uint32_t i = 0; i < n; i++)
        if (material[i] >= w->w.materials.size()) return fail(TRT_ERR_INVALID_ARG, "material index out of range");      // nothing is added then
    try {
        w->w.geometries.reserve(w->w.geometries.size() + n);
        for (uint32_t i = 0; i < n; i++) {
            const float* c = center_radius + 4u * (size_t)i;
            w->w.geometries.push_back(Geometry{0u, material[i], trt_vec3{c[0], c[1], c[2]}, trt_vec3{c[3], 0.0f, 0.0f}, trt_vec3{0.0f, 0.0f, 0.0f}});
        }
    } catch (const std::bad_alloc&) {
        return fail(TRT_ERR_OOM, "out of memory");
    }
    return TRT_OK;
}
int trt_world_add_quad(trt_world* w, trt_vec3 corner, trt_vec3 u, trt_vec3 v, uint32_t material) {
    if (!w) return fail(TRT_ERR_INVALID_ARG, "world is null");
    if (material >= w->w.materials.size()) return fail(TRT_ERR_INVALID_ARG, "material index out of range");
    try {
        w->w.geometries.push_back(Geometry{1u, material, corner, u, v});
    } catch (const std::bad_alloc&) {
        return fail(TRT_ERR_OOM, "out of memory");
    }
    return TRT_OK;
}
int trt_world_num_geometries(const trt_world* w) { return w ? (int)w->w.geometries.size() : 0; }
int trt_world_num_materials(const trt_world* w) { return w ? (int)w->w.materials.size() : 0; }

// ---- Scene ----
void trt_scene_options_default(trt_scene_options* out) { if (out) *out = defaults().scene; }
void trt_tuning_default(trt_tuning* out) { if (out) *out = defaults().tuning; }

int trt_scene_create_ex(const trt_world* w, const trt_scene_options* options, trt_scene** out) {
    if (!w || !out) return fail(TRT_ERR_INVALID_ARG, "null argument");
    try {
        const trt_scene_options opt = scene_options_or_defaults(options);
        if (scene_options_check(opt) != TRT_OK) return TRT_ERR_INVALID_ARG;
        SceneHost host;
        std::string msg;
        if (!compile_scene(w->w, opt, host, msg)) return fail(TRT_ERR_INVALID_ARG, msg);
        *out = scene_from_host(std::move(host), opt);
    } catch (const std::bad_alloc&) {
        return fail(TRT_ERR_OOM, "out of memory");
    } catch (const std::exception& e) {                         // (the scene compiler builds its trees on several threads: nothing may leave the C ABI)
        return fail(TRT_ERR_INVALID_ARG, std::string("scene compilation failed: ") + e.what());
    }
    return TRT_OK;
}
int trt_scene_create(const trt_world* w, trt_scene** out) { return trt_scene_create_ex(w, nullptr, out); }
// Frees every idle cached device buffer of the scene (workspaces whose render has finished, idle contexts' frames); the
// packed scene stays.  Safe while renders of the scene run: what they own is skipped.
int trt_scene_trim(trt_scene* s) {
    if (!s) return fail(TRT_ERR_INVALID_ARG, "scene is null");
    s->cache.trim_all();
    (void)hipGetLastError();
    return TRT_OK;
}
// Must not run while another host thread is inside a render call on this scene.  Renders enqueued through trt_render_device
// that are still running on the device are waited for (their workspace events) before anything is freed (~SceneCache).
void trt_scene_destroy(trt_scene* s) {
    if (!s) return;
    delete s;
    (void)hipGetLastError();
}
int trt_scene_get_info(const trt_scene* s, trt_scene_info* out) {
    if (!s || !out) return fail(TRT_ERR_INVALID_ARG, "null argument");
    const SceneLayout& L = s->host.layout;
    out->num_nodes = L.n_nodes; out->num_spheres = L.n_spheres; out->num_quads = L.n_quads; out->num_materials = L.n_materials;
    out->max_depth = s->host.max_depth;
    out->device_bytes = L.blob_bytes;
    out->lds_bytes = scene_lds_bytes(L);
    out->num_cull_nodes = L.n_cull_nodes;
    return TRT_OK;
}
static int copy_nodes(const NodeDump& d, float* bbox6, int32_t* prim, int32_t* skip, uint32_t cap) {
    const uint32_t n = (uint32_t)d.skip.size();
    if (cap < n) return fail(TRT_ERR_INVALID_ARG, "cap is smaller than the node count");
    for (size_t k = 0; k < 6 * (size_t)n; k++) bbox6[k] = d.bbox6[k];
    for (uint32_t i = 0; i < n; i++) { prim[i] = d.prim_geo[i]; skip[i] = d.skip[i]; }
    return TRT_OK;
}
int trt_scene_get_nodes(const trt_scene* s, float* bbox6, int32_t* prim, int32_t* skip, uint32_t cap) {
    if (!s || !bbox6 || !prim || !skip) return fail(TRT_ERR_INVALID_ARG, "null argument");
    return copy_nodes(s->host.reference, bbox6, prim, skip, cap);
}
int trt_scene_get_cull_nodes(const trt_scene* s, float* bbox6, int32_t* prim, int32_t* skip, uint32_t cap) {
    if (!s || !bbox6 || !prim || !skip) return fail(TRT_ERR_INVALID_ARG, "null argument");
    return copy_nodes(s->host.culling, bbox6, prim, skip, cap);
}

int trt_scene_get_compact_nodes(const trt_scene* s, uint32_t* words4, uint32_t cap) {
    if (!s || !words4) return fail(TRT_ERR_INVALID_ARG, "null argument");
    const SceneLayout& L = s->host.layout;
    if (L.off_compact == 0u) return fail(TRT_ERR_NOT_FOUND, "scene has no compact node array (it is walked from LDS)");
    if (cap < L.n_cull_nodes) return fail(TRT_ERR_INVALID_ARG, "buffer too small");
    memcpy(words4, s->host.blob.data() + 16u * (size_t)L.off_compact, 16u * (size_t)L.n_cull_nodes);
    for (uint32_t i = 0; i < L.n_cull_nodes; i++)                       // stored as byte offsets (the walk's cursor); reported as node indices
        if (!(words4[4u * (size_t)i + 3u] & 0x80000000u)) words4[4u * (size_t)i + 3u] >>= 4;
    return TRT_OK;
}
uint32_t trt_scene_facts(const trt_scene* s) { return s ? s->facts.word() : 0u; }

int trt_scene_get_packed(const trt_scene* s, uint8_t* bytes, uint32_t cap) {
    if (!s || !bytes) return fail(TRT_ERR_INVALID_ARG, "null argument");
    const uint32_t n = s->host.layout.blob_bytes;
    if (cap < n) return fail(TRT_ERR_INVALID_ARG, "cap is smaller than the packed scene (trt_scene_info.device_bytes)");
    memcpy(bytes, s->host.blob.data(), n);
    return TRT_OK;
}
// The scene's own lights for trt_direct, read back from the packed scene: primitive k of a kind names its material (spheres in the u32
// plane, quads in their record), the material its kind and colour, geo_index its insertion index.  Host only.
int trt_scene_emitters(const trt_scene* s, trt_emitter* out, uint32_t cap, uint32_t* count) {
    if (!s || !count) return fail(TRT_ERR_INVALID_ARG, "null argument");
    if (cap > 0u && !out) return fail(TRT_ERR_INVALID_ARG, "out is null");
    const SceneLayout& L = s->host.layout;
    const F4* const f4 = reinterpret_cast<const F4*>(s->host.blob.data());
    const uint32_t* const u32 = reinterpret_cast<const uint32_t*>(s->host.blob.data());
    try {
        std::vector<trt_emitter> lights;
        for (uint32_t k = 0; k < L.n_spheres + L.n_quads; k++) {
            const bool quad = k >= L.n_spheres;
            const F4* const q = f4 + L.off_quad + 5u * (size_t)(k - L.n_spheres);         // (read only where quad)
            uint32_t material;
            if (quad) memcpy(&material, &q[1].w, 4); else material = u32[L.off_sphere_mat + k];
            if (material >= L.n_materials || u32[L.off_material_kind + material] != TRT_LIGHT) continue;
            const F4 m = f4[L.off_material + material];
            const trt_vec3 color{m.x, m.y, m.z};
            trt_emitter e;
            if (quad) emitter_init_quad(e, trt_vec3{q[1].x, q[1].y, q[1].z}, trt_vec3{q[3].z, q[3].w, q[4].x}, trt_vec3{q[2].x, q[2].y, q[2].z}, color);
            else emitter_init_sphere(e, trt_vec3{f4[L.off_sphere + k].x, f4[L.off_sphere + k].y, f4[L.off_sphere + k].z}, f4[L.off_sphere + k].w, color);
            e.geometry = s->geo_index[k];
            lights.push_back(e);
        }
        std::sort(lights.begin(), lights.end(), [](const trt_emitter& a, const trt_emitter& b) { return a.geometry < b.geometry; });
        *count = (uint32_t)lights.size();
        for (uint32_t i = 0; i < cap && i < lights.size(); i++) out[i] = lights[i];
    } catch (const std::bad_alloc&) {
        return fail(TRT_ERR_OOM, "out of memory");
    }
    return TRT_OK;
}
void trt_emitter_init_quad(trt_emitter* out, trt_vec3 corner, trt_vec3 u, trt_vec3 v, trt_vec3 color) {
    if (out) emitter_init_quad(*out, corner, u, v, color);
}
void trt_emitter_init_sphere(trt_emitter* out, trt_vec3 centre, float radius, trt_vec3 color) {
    if (out) emitter_init_sphere(*out, centre, radius, color);
}

// ---- Camera ----
int trt_camera_init(trt_camera* out, float focus_distance, float defocus_angle_deg, trt_vec3 position, trt_vec3 look_at,
                    trt_vec3 up, float vertical_fov_deg, uint32_t width, uint32_t height) {
    if (!out) return fail(TRT_ERR_INVALID_ARG, "out is null");
    if (width == 0 || height == 0) return fail(TRT_ERR_INVALID_ARG, "width and height must be positive");
    camera_init(*out, focus_distance, defocus_angle_deg, position, look_at, up, vertical_fov_deg, width, height);
    return TRT_OK;
}

// ---- Renderer::render ----
int trt_render_device(trt_scene* s, const trt_camera* cam, const trt_render_params* p, float* d_accum, uint64_t* d_counters,
                      void* stream) {
    if (!s || !cam || !p || !d_accum) return fail(TRT_ERR_INVALID_ARG, "null argument");
    int rc = require_device();
    if (rc != TRT_OK) return rc;
    return enqueue_render(s, cam, p, d_accum, d_counters, reinterpret_cast<hipStream_t>(stream), nullptr);
}

}  // extern "C"

namespace {

// What trt_render_moments* asks beyond trt_render: a second buffer, and a backend that keeps per-sample records.
int check_moments(const trt_render_params* p, const float* moment2) {
    if (!moment2) return fail(TRT_ERR_INVALID_ARG, "moment2 is null");
    if (p->backend != TRT_BACKEND_STREAMED && p->backend != TRT_BACKEND_AUTO)
        return fail(TRT_ERR_INVALID_ARG, "second moments come from the streamed backend's fold: backend must be TRT_BACKEND_STREAMED or TRT_BACKEND_AUTO");
    return TRT_OK;
}

// trt_render, and with `moment2` trt_render_moments.  The second moments' device frame is the call's own: allocated here and freed before
// the call returns, so what trt_render allocates and what a context keeps are as they were.
int render_host(trt_scene* s, const trt_camera* cam, const trt_render_params* p, float* accum, float* moment2, trt_stats* stats,
                MomentsLaunch launch_moments) {
    int rc = require_device();
    if (rc != TRT_OK) return rc;
    uint32_t rows = 0;
    rc = check_render_args(cam, p, rows);
    if (rc != TRT_OK) return rc;
    const size_t bytes = (size_t)rows * cam->width * 3 * sizeof(float);
    CtxRun run(s->cache);
    run.acquire(bytes ? bytes : 16);
    float* d_m2 = nullptr;
    if (moment2) run.alloc(&d_m2, bytes ? bytes : 16, "second-moment frame", TRT_ERR_OOM);
    run.zero_counters();
    if (run.ok() && p->accumulate && bytes) run.step(hipMemcpyAsync(run.frame(), accum, bytes, hipMemcpyHostToDevice, run.stream()), "hipMemcpyAsync(frame to device)");
    if (run.ok() && p->accumulate && bytes && d_m2) run.step(hipMemcpyAsync(d_m2, moment2, bytes, hipMemcpyHostToDevice, run.stream()), "hipMemcpyAsync(second moments to device)");
    run.time_begin();
    if (run.ok()) run.step(enqueue_render(s, cam, p, run.frame(), reinterpret_cast<uint64_t*>(run.counters()), run.stream(), nullptr, d_m2, launch_moments));
    run.time_end();
    if (run.ok() && bytes) run.step(hipMemcpyAsync(accum, run.frame(), bytes, hipMemcpyDeviceToHost, run.stream()), "hipMemcpyAsync(frame to host)");
    if (run.ok() && bytes && d_m2) run.step(hipMemcpyAsync(moment2, d_m2, bytes, hipMemcpyDeviceToHost, run.stream()), "hipMemcpyAsync(second moments to host)");
    return run.finish(stats);
}

}  // namespace

namespace trt {
int query_render_moments(trt_scene* s, const trt_camera* cam, const trt_render_params* p, float* accum, float* moment2, trt_stats* stats,
                         MomentsLaunch launch) {
    if (!s || !cam || !p || !accum) return fail(TRT_ERR_INVALID_ARG, "null argument");
    const int rc = check_moments(p, moment2);
    if (rc != TRT_OK) return rc;
    return render_host(s, cam, p, accum, moment2, stats, launch);
}
int query_render_moments_device(trt_scene* s, const trt_camera* cam, const trt_render_params* p, float* d_accum, float* d_moment2,
                                uint64_t* d_counters, hipStream_t stream, MomentsLaunch launch) {
    if (!s || !cam || !p || !d_accum) return fail(TRT_ERR_INVALID_ARG, "null argument");
    int rc = check_moments(p, d_moment2);
    if (rc != TRT_OK) return rc;
    rc = require_device();
    if (rc != TRT_OK) return rc;
    return enqueue_render(s, cam, p, d_accum, d_counters, stream, nullptr, d_moment2, launch);
}
}  // namespace trt

extern "C" {

int trt_render(trt_scene* s, const trt_camera* cam, const trt_render_params* p, float* accum, trt_stats* stats) {
    if (!s || !cam || !p || !accum) return fail(TRT_ERR_INVALID_ARG, "null argument");
    return render_host(s, cam, p, accum, nullptr, stats, nullptr);
}

// ---- Renderer::render over several GPUs of one node ----
//
// renderer.rs:37-79 is ONE call that returns the whole Image; so is this.  The path shards by pixels (every sample reads
// only the immutable scene, cpu.rs:39-65): the scene is replicated, the image is cut into bands of kMultiBandRows rows dealt
// round-robin (band b -> shard b % ndev, so expensive regions spread over all devices), the RNG is keyed by the image
// pixel, and every device folds its own pixels in sample order - the frame is bit-identical for every ndev.  One host
// thread per shard drives its device on a cached context (stream, events, counters, band buffer: nothing is created per
// call once the pool is warm).  The only exchange is the gather of the finished f32 sums: a shard's bands sit at a
// constant pitch of ndev x 16 rows in the frame, so ONE strided 2-D copy moves all its full bands straight to their place
// (a host buffer: D2H; a buffer on devices[0]: device to device over xGMI), plus one 1-D copy if the shard owns the ragged
// last band.  No padded gather buffer and no un-interleave pass exist.
namespace {

constexpr uint32_t kMultiBandRows = 16;

struct MultiShard {
    int device = 0;
    uint32_t rank = 0, rows_local = 0;
    bool peer_ok = true;                      // the gather may address the destination device directly
    bool per_band = false;                    // the gather went band by band (no peer access, or the strided peer copy was refused)
    int rc = TRT_OK;
    std::string error;
    unsigned long long ctr[CTR_COUNT] = {0};
    float ms = 0.0f;
};

uint32_t band_rows_local(uint32_t height, uint32_t ndev, uint32_t rank, uint32_t band_rows) {
    const uint32_t n_bands = (height + band_rows - 1u) / band_rows;
    uint32_t rows = 0;
    for (uint32_t b = rank; b < n_bands; b += ndev) rows += (b + 1u) * band_rows <= height ? band_rows : height - b * band_rows;
    return rows;
}

// Where shard `rank` of `ndev` keeps its rows and where they belong in the frame (bytes).  Local rows are contiguous; in the
// frame the shard's k-th band starts at row (k * ndev + rank) * 16.
void band_copy_plan(uint32_t width, uint32_t height, uint32_t ndev, uint32_t rank, trt_band_copy* o) {
    const uint64_t row_bytes = (uint64_t)width * 3u * sizeof(float);
    const uint32_t rows = band_rows_local(height, ndev, rank, kMultiBandRows);
    o->rows_local = rows;
    o->full_bands = rows / kMultiBandRows;
    o->tail_rows = rows % kMultiBandRows;                                   // only the image's last band can be short
    o->band_bytes = row_bytes * kMultiBandRows;
    o->local_pitch = o->band_bytes;
    o->frame_pitch = o->band_bytes * ndev;
    o->frame_offset = (uint64_t)rank * o->band_bytes;
    o->tail_bytes = row_bytes * o->tail_rows;
    o->tail_local_offset = (uint64_t)o->full_bands * o->band_bytes;
    o->tail_frame_offset = ((uint64_t)o->full_bands * ndev + rank) * o->band_bytes;
}

// Moves one shard's rows between its local buffer and the frame (to_frame: the gather; else: reading the running sums).
// *per_band (may be null) is set when the rows went band by band instead of as one strided 2-D copy: two devices without peer
// access, or a runtime that refused the strided copy between two devices (never seen, but that path has only ever run against
// the simulated runtime of tests/native: on refusal the per-band peer copies - round 2's gather - take over).
hipError_t copy_bands(const trt_band_copy& pl, char* local, char* frame, bool to_frame, int local_device, int frame_device,
                      bool peer_ok, hipStream_t stream, bool* per_band = nullptr) {
    const bool host_frame = frame_device < 0;
    const hipMemcpyKind kind = host_frame ? (to_frame ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice) : hipMemcpyDeviceToDevice;
    const bool cross = !host_frame && frame_device != local_device;
    bool direct = host_frame || !cross || peer_ok;
    if (pl.full_bands) {
        if (direct) {
            hipError_t e = to_frame
                ? hipMemcpy2DAsync(frame + pl.frame_offset, pl.frame_pitch, local, pl.local_pitch, pl.band_bytes, pl.full_bands, kind, stream)
                : hipMemcpy2DAsync(local, pl.local_pitch, frame + pl.frame_offset, pl.frame_pitch, pl.band_bytes, pl.full_bands, kind, stream);
            if (e != hipSuccess) {
                if (!cross) return e;
                (void)hipGetLastError();
                direct = false;                                   // the strided cross-device copy was refused: band by band
            }
        }
        if (!direct) {                                            // no peer access (the runtime stages each band through the host), or the fallback
            if (per_band) *per_band = true;
            for (uint32_t k = 0; k < pl.full_bands; k++) {
                char* l = local + (uint64_t)k * pl.local_pitch;
                char* f = frame + pl.frame_offset + (uint64_t)k * pl.frame_pitch;
                hipError_t e = to_frame ? hipMemcpyPeerAsync(f, frame_device, l, local_device, pl.band_bytes, stream)
                                        : hipMemcpyPeerAsync(l, local_device, f, frame_device, pl.band_bytes, stream);
                if (e != hipSuccess) return e;
            }
        }
    }
    if (pl.tail_rows) {
        char* l = local + pl.tail_local_offset;
        char* f = frame + pl.tail_frame_offset;
        if (direct) return to_frame ? hipMemcpyAsync(f, l, pl.tail_bytes, kind, stream) : hipMemcpyAsync(l, f, pl.tail_bytes, kind, stream);
        if (per_band) *per_band = true;
        return to_frame ? hipMemcpyPeerAsync(f, frame_device, l, local_device, pl.tail_bytes, stream)
                        : hipMemcpyPeerAsync(l, local_device, f, frame_device, pl.tail_bytes, stream);
    }
    return hipSuccess;
}

// One device's share.  dst: the whole frame, on the host (dst_device < 0) or on device dst_device.
int render_shard(trt_scene* s, const trt_camera* cam, const trt_render_params* p, uint32_t ndev, MultiShard* sh, float* dst, int dst_device) {
    hipError_t e = hipSetDevice(sh->device);
    if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
    if (sh->rows_local == 0) return TRT_OK;                                 // more shards than bands
    trt_band_copy pl;
    band_copy_plan(cam->width, cam->height, ndev, sh->rank, &pl);
    trt_render_params q = *p;
    q.band_rows = kMultiBandRows; q.band_stride = ndev; q.band_offset = sh->rank; q.rows_local = sh->rows_local;
    CtxRun run(s->cache, sh->device);
    run.acquire((size_t)pl.rows_local * cam->width * 3 * sizeof(float));
    char* local = reinterpret_cast<char*>(run.frame());
    char* frame = reinterpret_cast<char*>(dst);
    run.zero_counters();
    if (run.ok() && p->accumulate) run.step(copy_bands(pl, local, frame, false, sh->device, dst_device, sh->peer_ok, run.stream()), "copy_bands: hipMemcpy*Async of the running sums");   // continue the frame's running sums
    run.time_begin();
    if (run.ok()) run.step(enqueue_render(s, cam, &q, run.frame(), reinterpret_cast<uint64_t*>(run.counters()), run.stream(), nullptr));
    run.time_end();
    if (run.ok()) run.step(copy_bands(pl, local, frame, true, sh->device, dst_device, sh->peer_ok, run.stream(), &sh->per_band), "copy_bands: hipMemcpy*Async of the gather");
    return run.finish(sh->ctr, &sh->ms);
}

int render_multi(trt_scene* s, const trt_camera* cam, const trt_render_params* p, const int* devices, uint32_t ndev, float* dst,
                 bool dst_on_device, trt_stats* stats) {
    if (!s || !cam || !p || !dst) return fail(TRT_ERR_INVALID_ARG, "null argument");
    int rc = require_device();
    if (rc != TRT_OK) return rc;
    if (p->band_rows != 0) return fail(TRT_ERR_INVALID_ARG, "trt_render_multi lays out the bands itself: band_rows must be 0");
    const int visible = trt_device_count();
    if (ndev == 0) ndev = (uint32_t)visible;
    if (ndev > 64) return fail(TRT_ERR_INVALID_ARG, "at most 64 shards");
    std::vector<MultiShard> shards(ndev);
    for (uint32_t r = 0; r < ndev; r++) {
        const int d = devices ? devices[r] : (int)r;
        if (d < 0 || d >= visible) return fail(TRT_ERR_INVALID_ARG, "device ordinal out of range");
        shards[r].device = d;
        shards[r].rank = r;
        shards[r].rows_local = band_rows_local(cam->height, ndev, r, kMultiBandRows);
    }
    uint32_t rows = 0;                                                      // validate once on the calling thread, so argument errors do not depend on a device
    rc = check_render_args(cam, p, rows);
    if (rc != TRT_OK) return rc;
    DeviceRestore restore;                                                  // the shards and the peer-access loop set other devices
    if (restore.error() != hipSuccess) return fail_hip(restore.error(), "hipGetDevice");
    const int dst_device = dst_on_device ? shards[0].device : -1;
    if (dst_on_device) {
        for (uint32_t r = 0; r < ndev; r++) {                               // peer access for the gather (xGMI)
            if (shards[r].device == dst_device) continue;
            int can = 0;
            hipError_t e = hipDeviceCanAccessPeer(&can, shards[r].device, dst_device);
            if (e != hipSuccess) return fail_hip(e, "hipDeviceCanAccessPeer");
            if (!can) { shards[r].peer_ok = false; continue; }             // hipMemcpyPeerAsync then stages through the host
            e = hipSetDevice(shards[r].device);
            if (e == hipSuccess) e = hipDeviceEnablePeerAccess(dst_device, 0);
            if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return fail_hip(e, "hipDeviceEnablePeerAccess");
            (void)hipGetLastError();
        }
        TRT_HIP(hipSetDevice(restore.device()));
    }
    auto shard = [&](MultiShard* sh) {                                     // (on a worker thread: the message is thread-local)
        sh->rc = render_shard(s, cam, p, ndev, sh, dst, dst_device);
        if (sh->rc != TRT_OK) sh->error = g_last_error;
    };
    if (ndev == 1) {
        shard(&shards[0]);
    } else {
        std::vector<std::thread> workers;
        try {
            for (uint32_t r = 0; r < ndev; r++) workers.emplace_back(shard, &shards[r]);
        } catch (...) {
            for (auto& t : workers) t.join();
            return fail(TRT_ERR_OOM, "could not start a host thread per device");
        }
        for (auto& t : workers) t.join();
    }
    unsigned long long total[CTR_COUNT] = {0};
    float ms = 0.0f;
    uint64_t per_band = 0;
    for (const MultiShard& sh : shards) {
        if (sh.rc != TRT_OK) return fail(sh.rc, "device " + std::to_string(sh.device) + ": " + sh.error);
        for (int k = 0; k < CTR_COUNT; k++) total[k] += sh.ctr[k];
        if (sh.ms > ms) ms = sh.ms;
        per_band += sh.per_band ? 1u : 0u;
    }
    if (stats) { counters_to_stats(total, stats); stats->kernel_ms = ms; stats->gather_per_band = per_band; }      // kernel_ms: the slowest device's
    return TRT_OK;
}

}  // namespace

int trt_render_multi(trt_scene* s, const trt_camera* cam, const trt_render_params* p, const int* devices, uint32_t ndev, float* accum,
                     trt_stats* stats) {
    return host_form([&] { return render_multi(s, cam, p, devices, ndev, accum, false, stats); });
}

int trt_render_multi_device(trt_scene* s, const trt_camera* cam, const trt_render_params* p, const int* devices, uint32_t ndev,
                            float* d_accum, trt_stats* stats) {
    return host_form([&] { return render_multi(s, cam, p, devices, ndev, d_accum, true, stats); });
}

int trt_band_rows_local(uint32_t height, uint32_t ndev, uint32_t rank, uint32_t* rows_local) {
    if (!rows_local || ndev == 0 || rank >= ndev) return fail(TRT_ERR_INVALID_ARG, "need 0 <= rank < ndev and a result pointer");
    *rows_local = band_rows_local(height, ndev, rank, kMultiBandRows);
    return TRT_OK;
}

int trt_band_copy_plan(uint32_t width, uint32_t height, uint32_t ndev, uint32_t rank, trt_band_copy* out) {
    if (!out || ndev == 0 || rank >= ndev || width == 0) return fail(TRT_ERR_INVALID_ARG, "need 0 <= rank < ndev, a positive width and a result pointer");
    band_copy_plan(width, height, ndev, rank, out);
    return TRT_OK;
}

// ---- Sampler::sampling, batch form ----
int trt_sample_batch(trt_scene* s, const trt_sample_point* in, uint32_t n, trt_sampled_color* out, uint32_t max_bounces,
                     trt_vec3 background, uint32_t seed, trt_stats* stats) {
    if (!s || (n && (!in || !out))) return fail(TRT_ERR_INVALID_ARG, "null argument");
    int rc = require_device();
    if (rc != TRT_OK) return rc;
    if (stats) { *stats = trt_stats{}; }
    if (n == 0) return TRT_OK;
    if (max_bounces == 0) {                       // cpu.rs:43-47: the loop body never runs, colour stays 0
        for (uint32_t i = 0; i < n; i++) { out[i].x = in[i].x; out[i].y = in[i].y; out[i].color = trt_vec3{0.0f, 0.0f, 0.0f}; }
        if (stats) stats->samples = n;
        return TRT_OK;
    }
    SceneDev sc;
    rc = scene_on_device(s, sc);
    if (rc != TRT_OK) return rc;
    RenderArgs ra{};
    ra.background[0] = background.x; ra.background[1] = background.y; ra.background[2] = background.z;
    ra.inv_spp = 1.0f;
    ra.max_bounces = max_bounces;
    ra.seed_key = rng_seed_key(seed);
    // with `stats` the counting kernel walks the reference tree (its counters then equal the CPU path's); without, the production
    // kernel walks the culling tree with postponed leaves: same colours, several times faster
    const bool counting = stats != nullptr;
    ra.ref_tree = counting ? 1u : 0u;
    ra.leaf_slots = counting ? 1u : 4u;
    CtxRun run(s->cache);
    run.acquire(0);
    trt_sample_point* d_in = nullptr;
    trt_sampled_color* d_out = nullptr;
    run.alloc(&d_in, (size_t)n * sizeof(trt_sample_point), "hipMalloc(sample points)", TRT_ERR_HIP);
    run.alloc(&d_out, (size_t)n * sizeof(trt_sampled_color), "hipMalloc(sampled colours)", TRT_ERR_HIP);
    run.zero_counters();
    if (run.ok()) run.step(hipMemcpyAsync(d_in, in, (size_t)n * sizeof(trt_sample_point), hipMemcpyHostToDevice, run.stream()), "hipMemcpyAsync(sample points to device)");
    run.time_begin();
    if (run.ok()) run.step(launch_sample_batch(sc, d_in, n, d_out, ra, run.counters(), counting, run.stream()), "launch_sample_batch");
    run.time_end();
    if (run.ok()) run.step(hipMemcpyAsync(out, d_out, (size_t)n * sizeof(trt_sampled_color), hipMemcpyDeviceToHost, run.stream()), "hipMemcpyAsync(sampled colours to host)");
    return run.finish(stats);
}

uint32_t trt_streamed_chunk_spp(uint32_t width, uint32_t rows) { return streamed_chunk_spp(width, rows, defaults().tuning.radiance_gb); }

// How the streamed backend would launch this render (host arithmetic only: works without a GPU).
int trt_streamed_launch_plan(const trt_scene* s, const trt_camera* cam, const trt_render_params* p, trt_launch_plan* out) {
    if (!s || !cam || !p || !out) return fail(TRT_ERR_INVALID_ARG, "null argument");
    RenderArgs ra;
    trt_tuning tn;
    uint32_t rows = 0;
    int rc = to_render_args(cam, p, ra, rows, tn);
    if (rc != TRT_OK) return rc;
    const StreamLaunchPlan pl = streamed_launch_plan(s->host.layout, ra, tn, p->collect_stats != 0);
    memset(out, 0, sizeof(*out));
    out->scene_mode = (uint32_t)pl.mode;
    out->threads_per_workgroup = (uint32_t)pl.threads;
    out->waves_per_simd = (uint32_t)pl.waves_per_simd;
    out->workgroups_per_cu = pl.wg_per_cu;
    out->lds_bytes = (uint32_t)pl.lds_bytes;
    out->scene_lds_bytes = (uint32_t)pl.scene_lds_bytes;
    out->leaf_slots = pl.slots;
    out->lds_leaf_stack = pl.lds_stack ? 1u : 0u;
    out->ray_pool = pl.pool ? 1u : 0u;
    out->walk = (uint32_t)pl.walk;
    out->specialised = pl.specialised ? 1u : 0u;
    out->has_kernel = pl.kernel_index >= 0 ? 1u : 0u;
    out->kernel_waves_per_simd = (uint32_t)pl.kernel_minw;
    out->kernel_threads = (uint32_t)pl.kernel_threads;
    out->kernel_walk = (uint32_t)pl.kernel_walk;
    out->kernel_ray_pool = pl.kernel_pool ? 1u : 0u;
    out->kernel_counting = pl.kernel_stats ? 1u : 0u;
    out->chunk_spp = streamed_chunk_spp(cam->width, rows, tn.radiance_gb);
    out->dual_walk = pl.dual ? 1u : 0u;
    out->workspace_bytes = streamed_workspace_bytes(cam->width, rows, ra.sample_end - ra.sample_begin, tn.radiance_gb);
    return TRT_OK;
}

int trt_kernel_timing_begin(void) {
    std::lock_guard<std::mutex> lock(trt::g_timing_mu);
    for (const trt::TimingPair& pr : trt::g_timing_pairs) { (void)hipEventDestroy(pr.begin); (void)hipEventDestroy(pr.end); }
    trt::g_timing_pairs.clear();
    trt::g_timing_epoch++;
    trt::g_timing_on = true;
    return TRT_OK;
}
int trt_kernel_timing_end(double* total_ms, uint32_t* launches) {
    std::vector<trt::TimingPair> pairs;
    {
        std::lock_guard<std::mutex> lock(trt::g_timing_mu);
        trt::g_timing_on = false;
        pairs.swap(trt::g_timing_pairs);
    }
    double sum = 0.0;
    uint32_t n = 0;
    int rc = TRT_OK;
    {
        DeviceRestore restore;
        for (const trt::TimingPair& pr : pairs) {
            float ms = 0.0f;
            hipError_t e = hipSetDevice(pr.device);
            if (e == hipSuccess) e = hipEventSynchronize(pr.end);
            if (e == hipSuccess) e = hipEventElapsedTime(&ms, pr.begin, pr.end);
            if (e != hipSuccess) { if (rc == TRT_OK) rc = fail_hip(e, "kernel timing events"); continue; }
            sum += ms;
            n++;
        }
        for (const trt::TimingPair& pr : pairs) { (void)hipEventDestroy(pr.begin); (void)hipEventDestroy(pr.end); }
    }
    (void)hipGetLastError();
    if (total_ms) *total_ms = sum;
    if (launches) *launches = n;
    return rc;
}

// Name of the kernel that dominates a render with these settings (what a profile of it shows).
const char* trt_dominant_kernel(const trt_scene* s, const trt_camera* cam, const trt_render_params* p) {
    if (!s || !cam || !p) return "";
    RenderArgs ra;
    trt_tuning tn;
    uint32_t rows = 0;
    if (to_render_args(cam, p, ra, rows, tn) != TRT_OK) return "";
    if (p->backend == TRT_BACKEND_WAVEFRONT) return "trt::wavefront_kernel";
    if (p->backend == TRT_BACKEND_MEGAKERNEL) return "trt::megakernel";
    return streamed_kernel_name(s->host.layout, ra, tn);
}

// ---- Imager finalisation ----
int trt_tonemap_u8(const float* accum, uint32_t npixels, float gamma, uint8_t* rgb) {
    if (npixels && (!accum || !rgb)) return fail(TRT_ERR_INVALID_ARG, "null argument");
    tonemap_u8(accum, npixels, gamma, rgb);
    return TRT_OK;
}

// The same on buffers resident in HBM; asynchronous on `stream`.
int trt_tonemap_u8_device(const float* d_accum, uint32_t npixels, float gamma, uint8_t* d_rgb, void* stream) {
    if (npixels && (!d_accum || !d_rgb)) return fail(TRT_ERR_INVALID_ARG, "null argument");
    if (!(gamma > 0.0f)) return fail(TRT_ERR_INVALID_ARG, "gamma must be positive");
    int rc = require_device();
    if (rc != TRT_OK) return rc;
    TRT_HIP(launch_tonemap_u8(d_accum, npixels, gamma, d_rgb, reinterpret_cast<hipStream_t>(stream)));
    return TRT_OK;
}

}  // extern "C"
