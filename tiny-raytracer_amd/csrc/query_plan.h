// query_plan.h - the host side of the units that give every wave a contiguous run of work items: the ray queries (query.hip: a run of the
// caller's rays), the feature buffers (aov.hip: a run of the local image's pixels) and the sparse render (pixels.hip: a run of the pixel
// list).  ONE copy of what a launch does before hipLaunchKernel (batch_prepare), of the launch-plan entry point (batch_launch_plan) and of
// the argument checks of the units that trace camera rays (batch_render_args).  The kernel table's entry (BatchKernel) and the launch rule
// over the unit's own table (plan_batch) are host arithmetic only and live in stream_plan.h, beside the streamed rule they follow.  The
// device side of the same units is wave_run.h; their host-buffer forms stage through host_stage.h.
// The sample queries (radiance.hip: radiance and gather, a run of the caller's rays or surfels; ambient.hip, probe.hip, passes.hip,
// direct.hip, nee.hip: a run of surfels or rays) use the same table entry, rule, preamble and plan entry point with tables of their own,
// and with pixels.hip the ONE launch tail (batch_launch); "nothing to trace" is ONE zero kernel for all of them (batch_zero).  What
// their two forms do around the launch is host_stage.h's sample_query_on_device / sample_query_on_host.
// For the units only: batch_prepare and batch_launch_plan call the HIP runtime and scene_query.h's helpers, so capi.hip, whose
// host-only build links without the units, must not include this header.
#pragma once

#include <stddef.h>

#include "host_stage.h"
#include "kernels.h"
#include "rt_path.h"
#include "scene_query.h"
#include "stream_plan.h"

namespace trt {

// What a launch of n > 0 items does before hipLaunchKernel: the plan for the current device, the checks of what the walks assume, the
// dynamic LDS attribute, and the two scene pointers the walks read.
struct BatchLaunch {
    trt_query_plan q;
    const void* fn;
    const float4* leaf_list;         // lock-step list and 16-byte nodes only
    const uint4* nodes16;            // 16-byte nodes only
};
inline hipError_t batch_prepare(const SceneDev& scd, uint32_t n, const BatchKernel* table, size_t count, BatchLaunch& b) {
    const SceneLayout& L = scd.L;
    int dev = 0, cus = 256;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    const BatchKernel* const k = plan_batch(L, n, (uint32_t)cus, table, count, b.q);
    if (k == nullptr) return hipErrorInvalidDeviceFunction;                         // no instantiation for this plan: a bug, never a fallback
    const trt_query_plan& q = b.q;
    const bool flat = k->walk == WALK_FLAT, compact = k->walk == WALK_COMPACT;
    // what the walks assume, checked where the launch is made
    if (q.lds_bytes > kLdsPerCu || (flat && q.leaf_slots < 2u) || (compact && L.off_compact == 0u) ||
        (k->walk != WALK_REGS && (q.leaf_slots < 1u || q.leaf_slots > kLdsLeafSlotsMax)))
        return hipErrorInvalidConfiguration;
    b.fn = k->fn;
    if (q.lds_bytes > 48u * 1024u) {
        e = hipFuncSetAttribute(b.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)q.lds_bytes);
        if (e != hipSuccess) return e;
    }
    b.leaf_list = (flat || compact) ? scd.blob + L.off_leaf_list : nullptr;
    b.nodes16 = compact ? reinterpret_cast<const uint4*>(scd.blob + L.off_compact) : nullptr;
    return hipSuccess;
}

// The launch itself, for the units whose kernel trt_kernel_timing_* measures: the launch pattern of kernels.hip, timing_mark brackets it.
inline hipError_t batch_launch(const BatchLaunch& b, void** args, hipStream_t stream) {
    const trt_query_plan& q = b.q;
    timing_mark(stream, true);
    const hipError_t le = hipLaunchKernel(b.fn, dim3(q.workgroups), dim3(q.threads_per_workgroup), args, q.lds_bytes, stream);
    timing_mark(stream, false);
    return le;
}

// Nothing to trace without accumulate, for the sample queries: n_a floats of d_a and, where d_b is not null, n_b floats of d_b become 0
// (one kernel for all of them, radiance.hip sums_zero_kernel).
hipError_t batch_zero(float* d_a, unsigned long long n_a, float* d_b, unsigned long long n_b, hipStream_t stream);

// The trt_*_launch_plan entry points: how batch_prepare would launch n items on this scene (host arithmetic only: works without a GPU
// when the CU count is given).
inline int batch_launch_plan(const trt_scene* s, uint32_t n, uint32_t compute_units, const BatchKernel* table, size_t count, trt_query_plan* out) {
    if (!s || !out) return query_fail(TRT_ERR_INVALID_ARG, "null argument");
    if (compute_units == 0u) {
        const int rc = query_require_device();
        if (rc != TRT_OK) return rc;
        int dev = 0, cus = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        if (e != hipSuccess || cus <= 0) return query_fail_hip(e, "compute unit count of the current device");
        compute_units = (uint32_t)cus;
    }
    (void)plan_batch(query_scene_layout(s), n, compute_units, table, count, *out);     // no instantiation: has_kernel = 0 says so
    return TRT_OK;
}

// The parameters the units that trace camera rays read, validated as trt_render validates them, and the camera.  rows = rows the call
// owns; rows x width fits 32 bits.
inline int batch_render_args(const trt_camera* cam, const trt_render_params* p, RenderArgs& ra, uint32_t& rows, CameraDev& cd) {
    const int rc = query_render_args(cam, p, ra, rows);
    if (rc != TRT_OK) return rc;
    if ((unsigned long long)rows * cam->width > 0xFFFFFFFFull) return query_fail(TRT_ERR_INVALID_ARG, "more than 2^32 - 1 pixels");
    query_camera_dev(*cam, cd);
    return TRT_OK;
}

}  // namespace trt
