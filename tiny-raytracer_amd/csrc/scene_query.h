// scene_query.h - what the ray-query unit (query.hip) and the feature-buffer unit (aov.hip) need from the C ABI layer (capi.hip): the thread-local error message, the device
// check and the device view of a scene handle - the packed scene plus the queries' index table, both uploaded on first use and freed
// with the scene.  capi.hip calls nothing in query.hip, so the host-only build of capi.hip links without it.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "kernels.h"

namespace trt {
struct QueryScene {
    SceneDev scene;
    const uint32_t* geo_index;       // geometry insertion index of sphere k at [k], of quad k at [n_spheres + k]
    FlatReuse flat_reuse;            // the lock-step walk's schedule for this scene (kernels.h)
};
// sets the thread-local message trt_last_error returns; returns `code`
int query_fail(int code, const std::string& msg);
int query_fail_hip(hipError_t e, const char* what);
// TRT_OK, or TRT_ERR_NO_DEVICE (message set)
int query_require_device();
// the layout of the packed scene behind a handle (host memory: no device needed)
const SceneLayout& query_scene_layout(const trt_scene* s);
// the scene on the calling thread's current device
int query_scene_on_device(trt_scene* s, QueryScene& out);
// The kernel arguments of a camera and of the render parameters the feature-buffer unit (aov.hip) reads - seed, 1/spp, background, sample
// range, accumulate, bands - validated as trt_render validates them (backend and tuning are not looked at).  rows = rows the call owns.
int query_render_args(const trt_camera* cam, const trt_render_params* p, RenderArgs& ra, uint32_t& rows);
void query_camera_dev(const trt_camera& cam, CameraDev& out);
// trt_render / trt_render_device with a second frame-shaped buffer for the per-pixel second moments (streamed.hip trt_render_moments*): the
// whole render path of capi.hip - validation (moment2 non-NULL, a backend that keeps per-sample records), contexts, workspaces - with the
// streamed launch made through `launch` (kernels.h launch_streamed_moments), so that capi.hip itself names no launcher its host-only build
// has no stand-in for.
using MomentsLaunch = hipError_t (*)(const SceneDev& sc, const CameraDev& cam, const RenderArgs& ra, const trt_tuning& tn, void* workspace,
                                     size_t workspace_bytes, float* d_accum, float* d_moment2, unsigned long long* d_counters, bool stats,
                                     hipStream_t stream);
int query_render_moments(trt_scene* s, const trt_camera* cam, const trt_render_params* p, float* accum, float* moment2, trt_stats* stats,
                         MomentsLaunch launch);
int query_render_moments_device(trt_scene* s, const trt_camera* cam, const trt_render_params* p, float* d_accum, float* d_moment2,
                                uint64_t* d_counters, hipStream_t stream, MomentsLaunch launch);
}  // namespace trt
