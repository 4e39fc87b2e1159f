// query_plan.h - the host side of the units that give every wave a contiguous run of work items: the ray queries (query.hip: a run of the
// caller's rays), the feature buffers (aov.hip: a run of the local image's pixels) and the sparse render (pixels.hip: a run of the pixel
// list).  ONE copy of the kernel table's entry, of the launch rule over the unit's own table (plan_batch: host arithmetic only), of what
// a launch does before hipLaunchKernel (batch_prepare), of the launch-plan entry point (batch_launch_plan) and of the argument checks of
// the units that trace camera rays (batch_render_args).  The device side of the same units is wave_run.h; their host-buffer forms stage
// through host_stage.h, which also has q_align16.
// The radiance and gather queries (radiance.hip: a run of the caller's rays or surfels) and the ambient queries (ambient.hip: a run of
// surfels) use the same table entry, rule, preamble and plan entry point with tables of their own.
// For those three units only: batch_prepare and batch_launch_plan call the HIP runtime and scene_query.h's helpers, so capi.hip, whose
// host-only build links without the units, must not include this header.
#pragma once

#include <stddef.h>

#include "host_stage.h"
#include "kernels.h"
#include "rt_path.h"
#include "scene_query.h"

namespace trt {

// One kernel instantiation of a unit: (scene mode, walk, workgroup shape) and the waves per SIMD of its launch bounds.
struct BatchKernel {
    const void* fn;
    int mode, walk, threads, minw;
};

constexpr size_t kQueryLdsPerCu = 160u * 1024u;

// How a batch of n items is launched on this scene with `cus` compute units.  The walk, workgroup shape and leaf-stack depth are those of
// the streamed launch plan under the built-in tuning (streamed.hip streamed_launch_plan: that rule lives there and is not restated),
// without the ray pool.  `table`: the unit's instantiations; a plan that has none runs the register-slot walk of its scene mode (fallback),
// which walks the culling tree every compiled scene carries and needs neither the leaf list nor the 16-byte nodes.  Returns the
// instantiation, nullptr if there is none.
inline const BatchKernel* plan_batch(const SceneLayout& L, uint32_t n, uint32_t cus, const BatchKernel* table, size_t count, trt_query_plan& q) {
    const trt_tuning tn = tuning_builtin();
    RenderArgs ra{};
    ra.lds_leaf_stack = tn.lds_leaf_stack;
    ra.leaf_slots = tn.leaf_slots;
    const StreamLaunchPlan pl = streamed_launch_plan(L, ra, tn, false);
    q = trt_query_plan{};
    q.scene_mode = (uint32_t)pl.mode;
    q.streamed_walk = (uint32_t)pl.walk;
    q.streamed_threads = (uint32_t)pl.threads;
    q.scene_lds_bytes = (uint32_t)pl.scene_lds_bytes;
    q.compute_units = cus;
    int walk = pl.walk, threads = pl.threads;
    auto find = [&] {
        for (size_t i = 0; i < count; i++)
            if (table[i].mode == pl.mode && table[i].walk == walk && table[i].threads == threads) return table + i;
        return static_cast<const BatchKernel*>(nullptr);
    };
    const BatchKernel* k = find();
    if (!k) {
        // a plan without an instantiation: the register-slot walk, which every scene has
        walk = WALK_REGS;
        threads = pl.mode == MODE_LDS ? 512 : 256;
        q.fallback = 1u;
        k = find();
    }
    if (!k) return nullptr;
    q.has_kernel = 1u;
    q.walk = (uint32_t)walk;
    q.threads_per_workgroup = (uint32_t)threads;
    q.kernel_waves_per_simd = (uint32_t)k->minw;
    q.leaf_slots = walk == WALK_REGS ? 0u : pl.slots;
    q.stragglers = walk == WALK_LDS_STACK ? tn.lds_stragglers : walk == WALK_COMPACT ? tn.stragglers : 0u;
    if (q.leaf_slots < 2u) q.stragglers = 0u;                                       // a parked walk occupies two slots (rt_path.h trav_park)
    const size_t scene_b = pl.scene_lds_bytes;
    const size_t lds_bytes = q.leaf_slots ? q_align16(scene_b) + (size_t)threads * q.leaf_slots * sizeof(float2) : scene_b;
    q.lds_bytes = (uint32_t)lds_bytes;
    q.workgroups_per_cu = (uint32_t)(k->minw * 4 * 64 / k->threads);
    if (lds_bytes) { const uint32_t by_lds = (uint32_t)(kQueryLdsPerCu / lds_bytes); if (by_lds < q.workgroups_per_cu) q.workgroups_per_cu = by_lds ? by_lds : 1u; }
    // a wave's run: 256 items (four refills of a wave, so that stragglers resume beside fresh items) unless that makes more than four waves
    // per resident wave slot - a workgroup of an LDS scene pays for its scene copy once, whatever the length of its runs
    const uint32_t waves_per_wg = (uint32_t)threads / 64u;
    q.wave_slots = 4ull * (unsigned long long)cus * q.workgroups_per_cu * waves_per_wg;
    unsigned long long per_wave = 256ull;
    if (((unsigned long long)n + per_wave - 1ull) / per_wave > q.wave_slots) per_wave = (((unsigned long long)n + q.wave_slots - 1ull) / q.wave_slots + 63ull) & ~63ull;
    q.rays_per_wave = (uint32_t)per_wave;
    q.waves = ((unsigned long long)n + per_wave - 1ull) / per_wave;
    q.workgroups = (uint32_t)((q.waves + waves_per_wg - 1ull) / waves_per_wg);
    return k;
}

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
    if (q.lds_bytes > kQueryLdsPerCu || (flat && q.leaf_slots < 2u) || (compact && L.off_compact == 0u) ||
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
