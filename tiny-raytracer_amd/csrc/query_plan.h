// query_plan.h - the launch rule of the units that give every wave a contiguous run of work items: the ray queries (query.hip: a run of
// the caller's rays) and the feature buffers (aov.hip: a run of the local image's pixels).  ONE copy of the rule, over the unit's own table
// of kernel instantiations; host arithmetic only.
#pragma once

#include <stddef.h>

#include "kernels.h"
#include "rt_path.h"

namespace trt {

constexpr size_t kQueryLdsPerCu = 160u * 1024u;
inline size_t q_align16(size_t b) { return (b + 15u) & ~(size_t)15u; }

// How a batch of n items is launched on this scene with `cus` compute units.  The walk, workgroup shape and leaf-stack depth are those of
// the streamed launch plan under the built-in tuning (streamed.hip streamed_launch_plan: that rule lives there and is not restated),
// without the ray pool.  `table`: the unit's instantiations, each with the members mode, walk, threads, minw; a plan that has none runs the
// register-slot walk of its scene mode (fallback), which walks the culling tree every compiled scene carries and needs neither the leaf
// list nor the 16-byte nodes.  Returns the instantiation, nullptr if there is none.
template <typename Kernel>
const Kernel* plan_batch(const SceneLayout& L, uint32_t n, uint32_t cus, const Kernel* table, size_t count, trt_query_plan& q) {
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
        return static_cast<const Kernel*>(nullptr);
    };
    const Kernel* k = find();
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

}  // namespace trt
