// scene_adopt.h — what the device scene compiler (scene_build.hip) needs from the C ABI layer (capi.hip): option checks, the
// thread-local error message and turning a compiled SceneHost plus its device-resident blob into a trt_scene handle.  capi.hip
// calls nothing in scene_build.hip, so the host-only build of capi.hip links without it.
#pragma once

#include <string>

#include "scene.h"

namespace trt {
// 0 or TRT_ERR_INVALID_ARG (message set): the checks trt_scene_create_ex makes before it compiles
int scene_options_check(const trt_scene_options& opt);
// the options trt_scene_create_ex uses for `options` (NULL = the library defaults)
trt_scene_options scene_options_or_defaults(const trt_scene_options* options);
// sets the thread-local message trt_last_error returns; returns `code`
int scene_fail(int code, const std::string& msg);
// A handle over `host` (moved in).  d_blob != nullptr: the packed scene is already on `device` (the handle owns it from now on).
// Returns nullptr (message set, d_blob NOT freed) if the handle cannot be allocated.
trt_scene* scene_adopt(SceneHost&& host, const trt_scene_options& opt, int device, void* d_blob);
// the World a trt_world wraps
const World& world_of(const trt_world* w);
}  // namespace trt
