// stream_plan_check.cpp - the streamed launch rule (csrc/stream_plan.h) swept over a synthetic domain on the CPU: host arithmetic only,
// nothing is launched.  tests/test_stream_plan.py builds this with g++, plain and under ASan + UBSan, and runs it.
//   * the pin: a digest over every field of every plan, compared with a constant that was recorded from the rule as it stood in
//     streamed.hip before it was split into stages (that function's text, compiled into this same sweep with the kernel pointers replaced
//     by table indices) - never from the code under test.  The same for plan_batch and the rule as it stood in query_plan.h.
//   * the invariants tests/test_host_boundary.py checks on 17 constructible scenes, here on every combination;
//   * coverage: every row of both streamed kernel tables is chosen by at least one plan.
// The domain sets hot_bytes on either side of each threshold (20 KB: workgroup shape, 64 KB: scene mode, 32 MiB: L2) and combines
// the layout's flags and every knob freely, which no compiled scene can.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../tiny-raytracer_amd/csrc/stream_plan.h"

using namespace trt;

namespace {

struct Digest {
    uint64_t h = 0xcbf29ce484222325ull;                                  // FNV-1a, 64 bits, one value at a time
    void add(uint64_t v) { for (int i = 0; i < 8; i++) { h ^= (v >> (8 * i)) & 0xffu; h *= 0x100000001b3ull; } }
    void add(const char* s) { for (; *s; s++) { h ^= (uint8_t)*s; h *= 0x100000001b3ull; } add((uint64_t)0); }
};

int g_failures = 0;
// the first combination of each kind of failure is printed, the rest are counted
void fail(const char* what, const SceneLayout& L, const RenderArgs& ra, const trt_tuning& tn, bool stats) {
    static const char* seen[64];
    static int n_seen = 0;
    g_failures++;
    for (int i = 0; i < n_seen; i++) if (seen[i] == what) return;
    if (n_seen < 64) seen[n_seen++] = what;
    fprintf(stderr, "FAIL %s: hot_bytes %u flat %u lazy %u compact %u | leaf_slots %u lds_leaf_stack %u ref_tree %u | waves %u big %u pool %u runtime %u dual %u | stats %d\n",
            what, L.hot_bytes, L.flat_walk, L.lazy_color, L.off_compact, ra.leaf_slots, ra.lds_leaf_stack, ra.ref_tree,
            tn.stream_waves_per_simd, tn.stream_big_threads, tn.ray_pool, tn.runtime_walk, tn.dual_walk, (int)stats);
}

// 30 sizes of the scene's hot part: nothing, small, 16 bytes either side of each threshold of the rule, sizes where the LDS parts just
// fit or just do not (49.6 KB is random-spheres' copy), and scenes far beyond L2
const uint32_t kHotBytes[] = {
    0u, 16u, 1000u, 4096u, 8u * 1024u, 16u * 1024u,
    20u * 1024u - 16u, 20u * 1024u, 20u * 1024u + 16u,
    24u * 1024u, 32u * 1024u, 40u * 1024u, 48u * 1024u, 50784u, 56u * 1024u, 60u * 1024u,
    64u * 1024u - 16u, 64u * 1024u, 64u * 1024u + 16u,
    100u * 1024u, (uint32_t)kLdsPerCu, 1u << 20, 3200016u, 16u << 20,
    (32u << 20) - 16u, 32u << 20, (32u << 20) + 16u,
    64u << 20, 100u << 20, 200u << 20,
};
const uint32_t kWaves[] = {0, 4, 5, 6, 7, 8, 9};
const uint32_t kLeafSlots[] = {0, 1, 2, 3, 4, 5, 7, 8, 16, 64};
const uint32_t kBigThreads[] = {0, 512, 768};

SceneLayout layout_of(uint32_t hot_bytes, uint32_t flags) {
    SceneLayout L{};
    L.hot_bytes = hot_bytes;
    L.flat_walk = flags & 1u;
    L.lazy_color = (flags >> 1) & 1u;
    L.off_compact = (flags & 4u) ? 4096u : 0u;           // any non-zero offset: the rule only asks whether the 16-byte nodes exist
    return L;
}

void digest_plan(Digest& d, const StreamLaunchPlan& pl) {
    d.add((uint64_t)pl.mode); d.add((uint64_t)pl.threads); d.add((uint64_t)pl.waves_per_simd); d.add(pl.wg_per_cu); d.add(pl.slots);
    d.add(pl.lds_stack); d.add(pl.flat); d.add(pl.compact); d.add(pl.pool); d.add(pl.specialised); d.add(pl.dual);
    d.add((uint64_t)pl.walk); d.add(pl.lds_bytes); d.add(pl.scene_lds_bytes);
    d.add((uint64_t)(int64_t)pl.kernel_index);
    d.add((uint64_t)pl.kernel_minw); d.add((uint64_t)pl.kernel_threads); d.add((uint64_t)pl.kernel_walk); d.add(pl.kernel_pool); d.add(pl.kernel_stats);
    d.add(pl.kernel_name);
}

// tests/test_host_boundary.py _check_plan, and what launch_streamed_folds refuses
void check_plan(const StreamLaunchPlan& pl, const SceneLayout& L, const RenderArgs& ra, const trt_tuning& tn, bool stats) {
    auto need = [&](bool ok, const char* what) { if (!ok) fail(what, L, ra, tn, stats); };
    need(pl.kernel_index >= 0 && pl.kernel_index < (int)kStreamKernelCount, "has a kernel");
    if (pl.kernel_index < 0 || pl.kernel_index >= (int)kStreamKernelCount) return;
    const StreamKernelShape& k = kStreamKernels[pl.kernel_index];
    const LdsLayout lds = plan_lds_layout(pl);
    need(lds.total() == pl.lds_bytes, "the LDS parts add up");
    need(pl.lds_bytes * pl.wg_per_cu <= kLdsPerCu && pl.wg_per_cu >= 1u, "the resident workgroups fit the CU");
    need(pl.wg_per_cu <= wg_per_cu(pl.waves_per_simd, pl.threads), "no more workgroups than the waves allow");
    need(pl.threads == 256 || pl.threads == 512 || pl.threads == 768, "workgroup shape");
    need(pl.waves_per_simd >= 4 && pl.waves_per_simd <= 8, "waves per SIMD");
    need(pl.mode == scene_mode(L) && pl.scene_lds_bytes == scene_lds_bytes(L), "scene mode and copy");
    need(pl.slots >= 1u && pl.slots <= kLdsLeafSlotsMax, "slot depth");
    need(!pl.flat || pl.slots >= 2u, "the lock-step walk has two slots");
    need(!pl.pool || pl.lds_stack, "the pool needs the LDS stack");
    need(pl.walk != WALK_FLAT || (pl.flat && pl.lds_stack && L.flat_walk != 0u), "lock-step walk");
    need(!pl.compact || (pl.lds_stack && pl.walk == WALK_COMPACT && pl.mode == MODE_GLOBAL && L.off_compact != 0u), "16-byte nodes");
    need(pl.lds_stack == (pl.walk != WALK_REGS), "register slots exactly without the LDS stack");
    need(!pl.dual || (pl.walk == WALK_COMPACT && pl.pool && pl.slots >= 2u && pl.specialised && pl.threads == 256), "two-path plan");
    need(pl.dual == k.dual, "the kernel's path count is the plan's");
    need(k.mode == pl.mode && k.threads == pl.threads && k.pool == pl.pool && k.stats == stats, "the kernel's mode, threads, pool and counting flag are the plan's");
    need(k.minw == pl.kernel_minw && k.threads == pl.kernel_threads && k.walk == pl.kernel_walk && k.pool == pl.kernel_pool && k.stats == pl.kernel_stats, "the reported shape is the row's");
    need(pl.specialised == (pl.kernel_index < (int)kSpecialisedCount), "specialised = a row of the first table");
    need(pl.specialised ? k.walk == pl.walk : k.walk == WALK_RUNTIME, "the kernel runs the plan's walk");
    need(!k.lazy || L.lazy_color != 0u, "a lazy-colour kernel only on a lazy-colour scene");
    need(k.minw < 5 || pl.wg_per_cu * (uint32_t)pl.threads <= (uint32_t)k.minw * 256u || pl.threads == 768, "the grid is not sized past the kernel's launch bound");
    need(pl.wg_per_cu * (uint32_t)pl.threads <= 8u * 256u, "at most 8 waves per SIMD");
    need(strcmp(pl.kernel_name, pl.dual ? "trt::stream_dual_kernel" : pl.pool ? "trt::stream_pool_kernel" : "trt::stream_sample_kernel") == 0, "kernel name");
}

unsigned long long sweep_streamed(Digest& d, unsigned long long* chosen) {
    unsigned long long n = 0;
    for (uint32_t hot : kHotBytes)
    for (uint32_t flags = 0; flags < 8u; flags++)
    for (uint32_t ref_tree = 0; ref_tree < 2u; ref_tree++)
    for (uint32_t waves : kWaves)
    for (uint32_t leaf_slots : kLeafSlots)
    for (uint32_t lds_leaf_stack = 0; lds_leaf_stack < 3u; lds_leaf_stack++)
    for (uint32_t ray_pool = 0; ray_pool < 2u; ray_pool++)
    for (uint32_t big : kBigThreads)
    for (uint32_t runtime_walk = 0; runtime_walk < 2u; runtime_walk++)
    for (uint32_t dual_walk = 0; dual_walk < 3u; dual_walk++)
    for (int stats = 0; stats < 2; stats++) {
        const SceneLayout L = layout_of(hot, flags);
        RenderArgs ra{};
        ra.ref_tree = ref_tree; ra.leaf_slots = leaf_slots; ra.lds_leaf_stack = lds_leaf_stack;
        trt_tuning tn = tuning_builtin();
        tn.stream_waves_per_simd = waves; tn.ray_pool = ray_pool; tn.stream_big_threads = big; tn.runtime_walk = runtime_walk; tn.dual_walk = dual_walk;
        const StreamLaunchPlan pl = streamed_launch_plan(L, ra, tn, stats != 0);
        digest_plan(d, pl);
        check_plan(pl, L, ra, tn, stats != 0);
        if (pl.kernel_index >= 0 && pl.kernel_index < (int)kStreamKernelCount) chosen[pl.kernel_index]++;
        n++;
    }
    return n;
}

// ---- plan_batch: the units' table shape (six (mode, walk, threads) rows), every waves-per-SIMD bound the units use ----
struct BatchRow { int mode, walk, threads; };
const BatchRow kBatchRows[6] = {
    {MODE_LDS, WALK_FLAT, 256}, {MODE_LDS, WALK_LDS_STACK, 256}, {MODE_LDS, WALK_LDS_STACK, 768}, {MODE_LDS, WALK_REGS, 512},
    {MODE_GLOBAL, WALK_COMPACT, 256}, {MODE_GLOBAL, WALK_REGS, 256},
};
// per row: uniform bounds 5..8, then the mixed bounds of the feature buffers, the ray queries and the gather and ambient queries
const int kBatchMinw[][6] = {
    {5, 5, 5, 5, 5, 5}, {6, 6, 6, 6, 6, 6}, {7, 7, 7, 7, 7, 7}, {8, 8, 8, 8, 8, 8},
    {7, 8, 6, 6, 8, 7}, {8, 8, 6, 6, 8, 8}, {6, 7, 7, 7, 7, 7}, {8, 8, 8, 7, 8, 7},
};
const uint32_t kBatchCus[] = {1, 64, 256};
const uint32_t kBatchN[] = {0u, 1u, 63u, 64u, 65u, 255u, 256u, 257u, 1u << 20, 0xFFFFFFFFu};

void check_batch(const trt_query_plan& q, const BatchKernel* k, const SceneLayout& L, uint32_t n) {
    const RenderArgs ra{};
    const trt_tuning tn = tuning_builtin();
    auto need = [&](bool ok, const char* what) { if (!ok) fail(what, L, ra, tn, false); };
    need((k != nullptr) == (q.has_kernel != 0u), "has_kernel says whether there is one");
    if (!k) return;
    const LdsLayout lds{q.scene_lds_bytes, (int)q.threads_per_workgroup, q.leaf_slots, 1u, false};
    need(lds.total() == q.lds_bytes, "batch: the LDS parts add up");
    need((size_t)q.lds_bytes * q.workgroups_per_cu <= kLdsPerCu && q.workgroups_per_cu >= 1u, "batch: the resident workgroups fit the CU");
    need(q.workgroups_per_cu <= wg_per_cu(k->minw, k->threads), "batch: no more workgroups than the launch bound allows");
    need((int)q.walk == k->walk && (int)q.threads_per_workgroup == k->threads && (int)q.scene_mode == k->mode && (int)q.kernel_waves_per_simd == k->minw, "batch: the kernel's shape is the plan's");
    need(q.walk != (uint32_t)WALK_FLAT || q.leaf_slots >= 2u, "batch: the lock-step walk has two slots");
    need((q.walk == (uint32_t)WALK_REGS) == (q.leaf_slots == 0u), "batch: register slots exactly without the LDS stack");
    need(q.stragglers == 0u || q.leaf_slots >= 2u, "batch: a parked walk has two slots");
    need((unsigned long long)q.rays_per_wave * q.waves >= n && q.rays_per_wave % 64u == 0u, "batch: the runs cover the items");
    need(q.waves <= 4ull * q.wave_slots || q.rays_per_wave > 256u, "batch: run length");
    need((unsigned long long)q.workgroups * (q.threads_per_workgroup / 64u) >= q.waves, "batch: the grid covers the waves");
}

unsigned long long sweep_batch(Digest& d) {
    unsigned long long count = 0;
    for (const auto& minw : kBatchMinw)
    for (size_t rows = 0; rows < 3u; rows++) {                 // the whole table; without its lock-step row (the fallback answers); no table
        BatchKernel table[6];
        size_t m = 0;
        for (int i = 0; i < 6; i++) {
            if (rows == 1u && kBatchRows[i].walk == WALK_FLAT) continue;
            if (rows == 2u) continue;
            table[m++] = BatchKernel{&kBatchRows[i], kBatchRows[i].mode, kBatchRows[i].walk, kBatchRows[i].threads, minw[i]};
        }
        for (uint32_t hot : kHotBytes)
        for (uint32_t flags = 0; flags < 8u; flags++)
        for (uint32_t cus : kBatchCus)
        for (uint32_t n : kBatchN) {
            const SceneLayout L = layout_of(hot, flags);
            trt_query_plan q;
            const BatchKernel* k = plan_batch(L, n, cus, table, m, q);
            d.add((uint64_t)(k ? k - table : -1));
            d.add(q.scene_mode); d.add(q.walk); d.add(q.threads_per_workgroup); d.add(q.kernel_waves_per_simd); d.add(q.workgroups_per_cu);
            d.add(q.leaf_slots); d.add(q.stragglers); d.add(q.lds_bytes); d.add(q.scene_lds_bytes); d.add(q.has_kernel); d.add(q.fallback);
            d.add(q.streamed_walk); d.add(q.streamed_threads); d.add(q.compute_units); d.add(q.rays_per_wave); d.add(q.workgroups);
            d.add(q.wave_slots); d.add(q.waves);
            check_batch(q, k, L, n);
            count++;
        }
    }
    return count;
}

// Recorded from the rule of the commit before stream_plan.h existed (see the head of this file); a change of either is a change of a plan.
constexpr uint64_t kStreamedPin = 0x72f3b8a3d8072a35ull;
constexpr uint64_t kBatchPin = 0x4d887b3319049775ull;

}  // namespace

int main() {
    Digest ds, db;
    unsigned long long chosen[kStreamKernelCount] = {0};
    const unsigned long long ns = sweep_streamed(ds, chosen);
    const unsigned long long nb = sweep_batch(db);
    printf("streamed plans %llu digest %016llx\nbatch plans %llu digest %016llx\n", ns, (unsigned long long)ds.h, nb, (unsigned long long)db.h);
    for (size_t i = 0; i < kStreamKernelCount; i++)
        if (chosen[i] == 0) { fprintf(stderr, "FAIL coverage: no plan of the sweep chose row %zu of the streamed kernel tables\n", i); g_failures++; }
    if (ds.h != kStreamedPin) { fprintf(stderr, "FAIL pin: streamed plans digest %016llx, recorded %016llx\n", (unsigned long long)ds.h, (unsigned long long)kStreamedPin); g_failures++; }
    if (db.h != kBatchPin) { fprintf(stderr, "FAIL pin: batch plans digest %016llx, recorded %016llx\n", (unsigned long long)db.h, (unsigned long long)kBatchPin); g_failures++; }
    if (g_failures) { fprintf(stderr, "%d failure(s)\n", g_failures); return 1; }
    printf("stream_plan_check ok: %zu kernel rows all chosen\n", kStreamKernelCount);
    return 0;
}
