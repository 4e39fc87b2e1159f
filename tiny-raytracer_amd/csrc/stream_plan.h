// stream_plan.h - how the streamed backend launches a scene, and how the batch units (query_plan.h) launch theirs: HOST ARITHMETIC ONLY.
// No kernel, no HIP call, no function pointer: the header compiles with a plain C++ compiler (tests/native/stream_plan_check.cpp sweeps
// the rule over every threshold and knob on the CPU and pins every plan), and the host-only builds of capi.hip link the real rule.
//   * the constants the rule and the kernels share (scene modes, walks, slot and pool sizes, the CU's LDS);
//   * LdsLayout: the ONE statement of the dynamic LDS of a workgroup - scene copy | leaf stacks | ray pool - and of how many fit a CU;
//   * the two tables of streamed kernel instantiations as lists (TRT_STREAM_SPECIALISED, TRT_STREAM_GENERAL): expanded here into shape
//     rows, and by streamed.hip - the same lists - into the kernels' addresses; a plan names its instantiation by row index;
//   * streamed_launch_plan: six stages, each a function of values - workgroup shape, slot depth, LDS stack or registers, ray pool,
//     two-path walk, instantiation.  A stage that revises an earlier choice returns the revised value and says so;
//   * plan_batch: the launch rule of the units that give every wave a run of items, over the unit's own table.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "kernels.h"

namespace trt {

// Scene access of a kernel instantiation: LDS copy or global blob, same element offsets (scene.h).
enum { MODE_GLOBAL = 0,      // scene read through L1/L2
       MODE_LDS = 1 };       // the whole hot part of the blob (culling tree, primitives, materials) copied into LDS

// Which walk a kernel instantiation runs.  WALK_RUNTIME picks by the launch arguments (every knob combination; counting
// kernels); the others fix the walk at compile time, which is what the production launches use: the kernel then holds ONE
// walk instead of five, with the SGPRs, VGPRs and instruction-cache footprint of one (stream_pool_kernel on Cornell:
// 6849 lines of ISA, 44 spilled SGPRs and 16 spilled VGPRs with the runtime choice).
enum { WALK_RUNTIME = 0, WALK_LDS_STACK = 1, WALK_FLAT = 2, WALK_COMPACT = 3, WALK_REGS = 5 };

constexpr uint32_t kLdsLeafSlotsMax = 16; // most slots per lane of the LDS leaf stack (8 bytes each)
constexpr uint32_t kPoolDwords = 9u;      // a ray-pool entry: origin, direction, rng state, radiance slot
constexpr uint32_t kBatchSpp = 8;         // samples per pixel in one batch of the streamed kernels
constexpr size_t kLdsPerCu = 160u * 1024u;

// Workgroups of `threads` lanes a CU holds at w waves per SIMD (four SIMDs of 64-lane waves).
inline uint32_t wg_per_cu(int w, int threads) { return (uint32_t)(w * 4 * 64 / threads); }

// The dynamic LDS of one workgroup: scene copy, aligned to 16 | `stacks` postponed-leaf stacks of threads x slots x 8 bytes (two for the
// two-path walk) | ray pool, 36 bytes per lane.  slots == 0: the postponed leaves live in registers and the scene copy is all there is,
// as long as it is.  The kernels compute the same addresses themselves (streamed.hip stream_pool_kernel and stream_dual_kernel: the
// pool's place; wave_run.h lds_behind_scene: the stacks'), because wrapping those expressions changes their code; every SIZE is from here.
struct LdsLayout {
    size_t scene_bytes;
    int threads;
    uint32_t slots, stacks;
    bool pool;
    size_t stack_bytes() const { return (size_t)stacks * (size_t)threads * slots * 8u; }
    size_t pool_bytes() const { return pool ? (size_t)threads * kPoolDwords * sizeof(uint32_t) : 0u; }
    size_t total() const { return slots == 0u ? scene_bytes : q_align16(scene_bytes) + stack_bytes() + pool_bytes(); }
    bool fits(uint32_t workgroups) const { return total() * workgroups <= kLdsPerCu; }
    // of `cap` workgroups per CU, those whose LDS fits (at least one: a layout past the CU's LDS is refused where the launch is made)
    uint32_t resident(uint32_t cap) const {
        if (total() == 0u) return cap;
        const uint32_t by_lds = (uint32_t)(kLdsPerCu / total());
        return by_lds < cap ? (by_lds ? by_lds : 1u) : cap;
    }
};

// ---- the streamed kernel instantiations ----
// One row per instantiation: P = stream_pool_kernel, S = stream_sample_kernel, both (MODE, STATS, MINW, THREADS, WALK, LAZY);
// D = stream_dual_kernel (MINW) at 256 lanes: two paths per lane, MODE_GLOBAL, 16-byte nodes, ray pool, lazy colour.
// production launches: walk fixed at compile time, lazy colour, no counters
#define TRT_STREAM_SPECIALISED(P, S, D)                  \
    P(MODE_LDS, false, 6, 256, WALK_FLAT, true)          \
    P(MODE_LDS, false, 7, 256, WALK_FLAT, true)          \
    P(MODE_LDS, false, 8, 256, WALK_FLAT, true)          \
    P(MODE_LDS, false, 6, 256, WALK_LDS_STACK, true)     \
    S(MODE_LDS, false, 6, 512, WALK_REGS, true)          \
    S(MODE_LDS, false, 6, 768, WALK_LDS_STACK, true)     \
    P(MODE_GLOBAL, false, 8, 256, WALK_COMPACT, true)    \
    P(MODE_GLOBAL, false, 7, 256, WALK_COMPACT, true) /* 72 VGPRs: nothing spilled (at 8 waves the fused slab arithmetic spills ten registers) */ \
    D(4) D(5) D(6) D(7) D(8)
// every other knob combination and the counting variants: runtime choice of the walk
#define TRT_STREAM_GENERAL(P, S, D)                                                                          \
    S(MODE_LDS, false, 6, 768, WALK_RUNTIME, false)    S(MODE_LDS, true, 6, 768, WALK_RUNTIME, false)      \
    S(MODE_LDS, false, 6, 512, WALK_RUNTIME, false)    S(MODE_LDS, true, 6, 512, WALK_RUNTIME, false)      \
    S(MODE_LDS, false, 5, 512, WALK_RUNTIME, false)    S(MODE_LDS, true, 5, 512, WALK_RUNTIME, false)      \
    S(MODE_LDS, false, 7, 256, WALK_RUNTIME, false)    S(MODE_LDS, true, 7, 256, WALK_RUNTIME, false)      \
    P(MODE_LDS, false, 6, 256, WALK_RUNTIME, false)    P(MODE_LDS, true, 6, 256, WALK_RUNTIME, false)      \
    S(MODE_LDS, false, 6, 256, WALK_RUNTIME, false)    S(MODE_LDS, true, 6, 256, WALK_RUNTIME, false)      \
    S(MODE_LDS, false, 5, 256, WALK_RUNTIME, false)    S(MODE_LDS, true, 5, 256, WALK_RUNTIME, false)      \
    P(MODE_GLOBAL, false, 8, 256, WALK_RUNTIME, false) P(MODE_GLOBAL, true, 8, 256, WALK_RUNTIME, false)   \
    S(MODE_GLOBAL, false, 8, 256, WALK_RUNTIME, false) S(MODE_GLOBAL, true, 8, 256, WALK_RUNTIME, false)   \
    S(MODE_GLOBAL, false, 7, 256, WALK_RUNTIME, false) S(MODE_GLOBAL, true, 7, 256, WALK_RUNTIME, false)   \
    S(MODE_GLOBAL, false, 6, 256, WALK_RUNTIME, false) S(MODE_GLOBAL, true, 6, 256, WALK_RUNTIME, false)   \
    S(MODE_GLOBAL, false, 1, 256, WALK_RUNTIME, false) S(MODE_GLOBAL, true, 1, 256, WALK_RUNTIME, false)

// The template arguments of a row: scene mode, lanes per workgroup, launch bound (waves per SIMD), walk (WALK_RUNTIME: the kernel picks
// the walk from its arguments), and which kernel it is.  Every instantiation has the same parameter list.
struct StreamKernelShape {
    int mode, threads, minw, walk;
    bool pool, stats, lazy, dual;
};
#define TRT_SHAPE_POOL(MODE, STATS, MINW, THREADS, WALK, LAZY) StreamKernelShape{MODE, THREADS, MINW, WALK, true, STATS, LAZY, false},
#define TRT_SHAPE_SAMPLE(MODE, STATS, MINW, THREADS, WALK, LAZY) StreamKernelShape{MODE, THREADS, MINW, WALK, false, STATS, LAZY, false},
#define TRT_SHAPE_DUAL(MINW) StreamKernelShape{MODE_GLOBAL, 256, MINW, WALK_COMPACT, true, false, true, true},
// the rows a plan's kernel_index counts: the specialised list, then the general one
constexpr StreamKernelShape kStreamKernels[] = {
    TRT_STREAM_SPECIALISED(TRT_SHAPE_POOL, TRT_SHAPE_SAMPLE, TRT_SHAPE_DUAL)
    TRT_STREAM_GENERAL(TRT_SHAPE_POOL, TRT_SHAPE_SAMPLE, TRT_SHAPE_DUAL)
};
#undef TRT_SHAPE_POOL
#undef TRT_SHAPE_SAMPLE
#undef TRT_SHAPE_DUAL
#define TRT_ONE_ROW(...) +1u
constexpr size_t kSpecialisedCount = 0u TRT_STREAM_SPECIALISED(TRT_ONE_ROW, TRT_ONE_ROW, TRT_ONE_ROW);
#undef TRT_ONE_ROW
constexpr size_t kStreamKernelCount = sizeof(kStreamKernels) / sizeof(kStreamKernels[0]);

// ---- the rule, stage by stage ----

// Stage 1: lanes per workgroup, waves per SIMD, and whether two paths per lane are wanted.
struct StreamShape {
    int threads, w;
    bool want_dual;
    bool dual_by_scene;     // the wish is the plan's own (trt_tuning.dual_walk == 0), not the caller's
};
inline StreamShape plan_shape(const SceneLayout& L, int mode, size_t scene_bytes, const RenderArgs& ra, const trt_tuning& tn, bool stats) {
    // waves per SIMD / lanes per workgroup: 256-lane workgroups for small LDS copies; a big LDS copy (> 20 KB) is shared by
    // more waves: 768 lanes (12 waves, two workgroups per CU = 6 waves per SIMD) if the copy and a 4-slot LDS leaf stack
    // fit twice into the CU's 160 KB (random-spheres: 49.6 + 24 KB; 19.0 Gray/s against 18.0 for 512 lanes with register
    // slots and 18.7 for 1024 lanes at 8 waves per SIMD, one box: tools/sweep_rs.sh), else 512 lanes with the slots in registers;
    // 8 waves per SIMD for scenes read from global memory
    int threads = 256;
    if (mode == MODE_LDS && L.hot_bytes > 20u * 1024u) {
        threads = LdsLayout{scene_bytes, 768, 4u, 1u, false}.fits(2u) && ra.lds_leaf_stack != 0u ? 768 : 512;
        if (tn.stream_big_threads == 512u || tn.stream_big_threads == 768u) threads = (int)tn.stream_big_threads;
    }
    // LDS scenes: 6 waves per SIMD.  Scenes in global memory: rounds 1-4 ran them at 8 (100 k spheres: 2.03 Gray/s at 5 waves, 2.25 at 6, 2.29 at 8 -
    // measured with NaN rays walking the whole tree in every launch: rt_path.h ray_has_nan)
    // (round 5, without the NaN-ray tail and with the fused slab arithmetic: a tree that fits the chip's 32 MiB of L2 runs 5 % faster at 7 waves
    // with no spilled register than at 8 with ten; a scene whose walk waits for memory - sphere_field, 1 M spheres and up - wants the eighth wave:
    // profiles/r05_waves7_ab.txt)
    // Two paths per lane (stream_dual_kernel; trt_tuning.dual_walk: 0 by scene, 1 wherever the kernel exists, 2 never): with the fused box step in its loop
    // it LOSES 2.6 % where the tree fits L2 and WINS 2.7 % / 4.2 % on sphere_field 1 M / 4 M at 6 waves - where the walk's loads really miss, a second
    // node load in flight per lane pays (profiles/r05_dual_walk_fused_ab.txt): by scene = beyond L2, when nothing else about the launch was asked for.
    const bool beyond_l2 = mode == MODE_GLOBAL && L.hot_bytes > (32u << 20);
    const bool by_scene = mode == MODE_GLOBAL && tn.dual_walk == 0u && beyond_l2 && tn.stream_waves_per_simd == 0u && !stats && !ra.ref_tree && L.lazy_color &&
                          tn.runtime_walk == 0u && tn.ray_pool != 0u && ra.lds_leaf_stack != 0u && L.off_compact != 0u;
    const bool want_dual = (mode == MODE_GLOBAL && tn.dual_walk == 1u) || by_scene;
    int w = mode == MODE_LDS ? 6 : (beyond_l2 ? (want_dual ? 6 : 8) : 7);
    if (tn.stream_waves_per_simd) w = (int)tn.stream_waves_per_simd;
    if (w < 5 && !(want_dual && w == 4)) w = 5;      // (4: the two-path kernel only - eight rays per SIMD like 8 x 1)
    if (w > 8) w = 8;
    if (threads == 512 && w > 6) w = 6;
    if (threads == 768) w = 6;
    return StreamShape{threads, w, want_dual, want_dual && tn.dual_walk == 0u};
}

// Stage 2: slots per lane of the leaf stack.
inline uint32_t plan_slots(int mode, size_t scene_bytes, bool flat, int threads, int w, uint32_t asked) {
    // slots of the LDS stack: 4 for tree walks (5 in the 768-lane plan if they fit: random-spheres +3 %, profiles/r03_defaults_sweep.txt);
    // 7 for the lock-step leaf list, whose t_best stays stale for a whole walk (Cornell 34.0 Gray/s at 4, 35.1 at 6..12) and which
    // steps two leaves per trip, so a lane must have two free
    if (asked != 0u) {
        const uint32_t slots = asked > kLdsLeafSlotsMax ? kLdsLeafSlotsMax : asked;
        return flat && slots < 2u ? 2u : slots;                               // walk_flat pushes up to two leaves per trip
    }
    uint32_t slots = flat ? 7u : (threads == 768 ? 5u : 4u);
    const uint32_t wgs = wg_per_cu(w, threads);
    // the default depth gives way to occupancy: the deepest stack (<= 7, >= 4) with which stack + ray pool + scene copy of
    // all the CU's workgroups fit its 160 KB of LDS (Cornell: 7 slots at 6 waves per SIMD, 5 at 7, 4 at 8)
    if (flat && mode == MODE_LDS && threads == 256)
        while (slots > 4u && !LdsLayout{scene_bytes, threads, slots, 1u, true}.fits(wgs)) slots--;
    if (threads > 512)
        while (slots > 3u && !LdsLayout{scene_bytes, threads, slots, 1u, false}.fits(wgs)) slots--;
    return slots;
}

// Stage 3: the leaf stack in LDS (true) or the slots in registers.  `setting`: RenderArgs.lds_leaf_stack (0 no, 1 where it costs no
// occupancy, 2 always).
inline bool plan_lds_stack(size_t scene_bytes, int threads, uint32_t slots, int w, uint32_t setting) {
    // LDS: scene copy + the postponed-leaf stack (8 bytes per lane and slot), the latter only where it does not cost a
    // resident workgroup (random-spheres: 49.6 KB scene copy, 3 workgroups of 512 lanes per CU without it, 2 with it:
    // measured 7 % slower than register slots); otherwise the slots are registers
    const LdsLayout with_stack{scene_bytes, threads, slots, 1u, false}, plain{scene_bytes, threads, 0u, 1u, false};
    if (setting == 0u || !with_stack.fits(1u)) return false;
    const uint32_t wgs = wg_per_cu(w, threads);
    return setting == 2u || with_stack.resident(wgs) >= plain.resident(wgs);
}

// Stage 4: the per-wave pool of primary rays (stream_pool_kernel): needs the LDS stack and 256-lane workgroups (LDS scenes at 6
// waves per SIMD and more, global-memory scenes at 7 and more or with two paths per lane), and must not cost a resident workgroup either.
inline bool plan_pool(int mode, size_t scene_bytes, const StreamShape& s, uint32_t slots, bool lds_stack, bool ref_tree, bool asked) {
    const bool shape_ok = (mode == MODE_LDS && s.w >= 6) || (mode == MODE_GLOBAL && (s.w >= 7 || s.want_dual));
    return lds_stack && s.threads == 256 && !ref_tree && shape_ok && asked && LdsLayout{scene_bytes, s.threads, slots, 1u, true}.fits(wg_per_cu(s.w, s.threads));
}

// Stage 5: two paths per lane (stream_dual_kernel): scenes in global memory on 16-byte nodes with the ray pool; two leaf stacks per
// lane, as deep as fit beside the pool (2..4 slots: a parked walk needs two).  REVISES THE SLOT DEPTH where it says yes: slots is then
// the depth of each of the two stacks.  `eligible`: wanted, and the plan so far is the one the kernel is built for.
struct TwoPaths {
    bool dual;
    uint32_t slots;
};
inline TwoPaths plan_two_paths(bool eligible, size_t scene_bytes, int threads, int w, uint32_t slots, uint32_t asked) {
    if (!eligible) return TwoPaths{false, slots};
    uint32_t ds = asked == 0u ? 4u : (asked < 2u ? 2u : (asked > kLdsLeafSlotsMax ? kLdsLeafSlotsMax : asked));
    const uint32_t wgs = wg_per_cu(w, threads);
    while (ds > 2u && !LdsLayout{scene_bytes, threads, ds, 2u, true}.fits(wgs)) ds--;
    if (!LdsLayout{scene_bytes, threads, ds, 2u, true}.fits(wgs)) return TwoPaths{false, slots};
    return TwoPaths{true, ds};
}

// Stage 6: the kernel instantiation - the specialised row of exactly this shape, else the nearest general row.
inline int find_specialised(int mode, int threads, int w, int walk, bool pool, bool dual) {
    for (size_t i = 0; i < kSpecialisedCount; i++) {
        const StreamKernelShape& e = kStreamKernels[i];
        if (e.mode == mode && e.threads == threads && e.minw == w && e.pool == pool && e.walk == walk && e.dual == dual) return (int)i;
    }
    return -1;
}
// The general instantiations exist for fewer (waves, pool) combinations than the knobs can ask for: for this mode, workgroup shape and
// counting flag, the row with the highest launch bound not above w; the pool only where that row has it.
inline int nearest_general(int mode, int threads, int w, bool pool, bool stats) {
    int best = -1;
    for (size_t i = kSpecialisedCount; i < kStreamKernelCount; i++) {
        const StreamKernelShape& e = kStreamKernels[i];
        if (e.mode != mode || e.threads != threads || e.stats != stats || e.minw > w || (e.pool && !pool)) continue;
        if (best < 0 || e.minw > kStreamKernels[best].minw || (e.minw == kStreamKernels[best].minw && e.pool)) best = (int)i;
    }
    return best;
}
// REVISES the waves per SIMD, the pool and the two-path walk: a plan follows the kernel it gets, so that grid and LDS are sized for
// what really runs.
struct StreamKernelChoice {
    int index;              // row of kStreamKernels, -1: none
    int w;
    bool pool, dual;
};
inline StreamKernelChoice plan_kernel(int mode, const StreamShape& s, int walk, bool pool, bool dual, bool specialise, bool stats) {
    StreamKernelChoice c{specialise ? find_specialised(mode, s.threads, s.w, walk, pool, dual) : -1, s.w, pool, dual};
    if (c.index < 0) c.dual = false;
    if (!c.dual && c.w < 5) c.w = 5;                        // four waves per SIMD exist for the two-path kernel only
    if (!c.dual && s.dual_by_scene) c.w = 8;                // the plan's own wish fell through: the one-path shape of a scene beyond L2
    if (c.index >= 0) return c;
    c.index = nearest_general(mode, s.threads, c.w, pool, stats);
    if (c.index < 0) { c.pool = false; return c; }
    const StreamKernelShape& k = kStreamKernels[c.index];
    c.pool = k.pool;
    if (k.minw >= 5 && k.minw < c.w) c.w = k.minw;          // (the one-wave bound of MODE_GLOBAL serves 5 waves per SIMD)
    return c;
}

// The LDS a plan's launch asks for, from its fields: what launch_streamed_folds and the tests hold lds_bytes against.
inline LdsLayout plan_lds_layout(const StreamLaunchPlan& pl) {
    return LdsLayout{pl.scene_lds_bytes, pl.threads, pl.lds_stack ? pl.slots : 0u, pl.dual ? 2u : 1u, pl.pool};
}

// How a scene is launched: workgroup shape, waves per SIMD, where the postponed leaves live, which walk, which kernel.
// Everything the kernels assume about their LDS is LdsLayout; trt_streamed_launch_plan exposes the result, and the CPU tests check
// its invariants for every scene size and every knob (tests/native/stream_plan_check.cpp, tests/test_host_boundary.py).
inline StreamLaunchPlan streamed_launch_plan(const SceneLayout& L, const RenderArgs& ra, const trt_tuning& tn, bool stats) {
    const size_t scene_bytes = scene_lds_bytes(L);
    const int mode = scene_mode(L);
    const bool flat = L.flat_walk && !ra.ref_tree;
    const StreamShape shape = plan_shape(L, mode, scene_bytes, ra, tn, stats);
    const uint32_t tree_slots = plan_slots(mode, scene_bytes, flat, shape.threads, shape.w, ra.leaf_slots);
    const bool lds_stack = plan_lds_stack(scene_bytes, shape.threads, tree_slots, shape.w, ra.lds_leaf_stack);
    const bool want_pool = plan_pool(mode, scene_bytes, shape, tree_slots, lds_stack, ra.ref_tree != 0u, tn.ray_pool != 0u);
    // few primitives: lock-step leaf list (rt_path.h walk_flat); scenes read from global memory: 16-byte culling nodes
    // (walk_compact).  Both need the LDS stack.
    const bool compact = lds_stack && mode == MODE_GLOBAL && L.off_compact != 0u && !ra.ref_tree;
    const int walk = compact ? WALK_COMPACT : (flat && lds_stack) ? WALK_FLAT : lds_stack ? WALK_LDS_STACK : WALK_REGS;
    const bool slots_ok = lds_stack || ra.leaf_slots == 0u || ra.leaf_slots >= 4u;      // WALK_REGS has 4 register slots
    const bool specialise = !stats && slots_ok && L.lazy_color && tn.runtime_walk == 0u;
    const TwoPaths two = plan_two_paths(shape.want_dual && specialise && compact && want_pool && shape.threads == 256, scene_bytes, shape.threads, shape.w, tree_slots, ra.leaf_slots);
    const StreamKernelChoice k = plan_kernel(mode, shape, walk, want_pool, two.dual, specialise, stats);

    StreamLaunchPlan pl{};
    pl.mode = mode; pl.threads = shape.threads; pl.waves_per_simd = k.w; pl.slots = two.slots;
    pl.lds_stack = lds_stack; pl.flat = flat && lds_stack; pl.compact = compact; pl.pool = k.pool; pl.walk = walk; pl.dual = k.dual;
    pl.scene_lds_bytes = scene_bytes;
    const LdsLayout lds = plan_lds_layout(pl);
    pl.lds_bytes = lds.total();
    pl.wg_per_cu = lds.resident(wg_per_cu(k.w, shape.threads));
    pl.kernel_index = k.index;
    pl.specialised = k.index >= 0 && k.index < (int)kSpecialisedCount;
    if (k.index >= 0) {
        const StreamKernelShape& e = kStreamKernels[k.index];
        pl.kernel_minw = e.minw; pl.kernel_threads = e.threads; pl.kernel_walk = e.walk; pl.kernel_pool = e.pool; pl.kernel_stats = e.stats;
    }
    pl.kernel_name = k.dual ? "trt::stream_dual_kernel" : k.pool ? "trt::stream_pool_kernel" : "trt::stream_sample_kernel";
    return pl;
}

// Name of the kernel that dominates a streamed render of this scene (for profiles and bench.py's roofline line).
inline const char* streamed_kernel_name(const SceneLayout& L, const RenderArgs& ra, const trt_tuning& tn) { return streamed_launch_plan(L, ra, tn, false).kernel_name; }

// ---- the batch units ----

// One kernel instantiation of a unit: (scene mode, walk, workgroup shape) and the waves per SIMD of its launch bounds.
struct BatchKernel {
    const void* fn;
    int mode, walk, threads, minw;
};

// How a batch of n items is launched on this scene with `cus` compute units.  The walk, workgroup shape and leaf-stack depth are those of
// the streamed launch plan under the built-in tuning (streamed_launch_plan above: the rule is not restated), without the ray pool.
// `table`: the unit's instantiations; a plan that has none runs the register-slot walk of its scene mode (fallback), which walks the
// culling tree every compiled scene carries and needs neither the leaf list nor the 16-byte nodes.  Returns the instantiation, nullptr
// if there is none.
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
    const LdsLayout lds{pl.scene_lds_bytes, threads, q.leaf_slots, 1u, false};
    q.lds_bytes = (uint32_t)lds.total();
    q.workgroups_per_cu = lds.resident(wg_per_cu(k->minw, k->threads));
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
