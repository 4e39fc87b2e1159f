// Test program (tests/test_gpu_walk_rays.py builds and runs it on the GPU box, once with the hand-written box loops and once with
// -DTRT_ASM_BOX_LOOP=0): chosen rays through EVERY walk of rt_path.h, one small kernel per walk, answers written out ray by ray
// - prim_best, the bits of t_best, and the fast / ref flags trav_begin gave the ray - for the Python side to compare with the
// oracle's closest hit.  There is no walk code in this file: the kernels call the entry points streamed.hip calls (trav_begin,
// closest_hit, closest_hit_resume, walk_compact2, trav_park / trav_unpark, stage_scene_to_lds) with the LDS laid out as
// stream_plan.h LdsLayout lays it out (scene copy | leaf stack: threads x slots x 8 bytes, two stacks per lane in the two-path kernel), and the
// resumable kernels mirror the round structure of stream_sample_kernel / stream_dual_kernel: a lane whose walk completed takes the
// next ray of its wave's list, a parked one resumes beside it.
//
//   walk_rays plain|controls <scene.bin> <rays.bin> <out.bin> <out.txt> [<scene.bin> <rays.bin> <out.bin> <out.txt> ...]
//
// (one group of four files per scene: the scenes run one after another in one process)
// scene.bin: u32 'WRS1', n_materials, n_geometries, f32 cull_prune, i32 flat_walk, i32 compact_nodes; n_materials x (kind, albedo[3], param);
//            n_geometries x (kind, material, a[3], b[3], c[3]) - scene.h Geometry.
// rays.bin:  u32 'WRR1', n_rays, n_tasks; n_rays x (origin[3], direction[3]) f32 bits, used as given; n_tasks x (begin, count): the ray
//            list of one wave.  The tasks partition the rays.
// out.txt:   one `layout ...` line (what the host-side scene says: the Python side predicts the flags from it), one `variant NAME` line
//            per walk variant run, in the order of their records in out.bin: n_rays x (prim_best, bits(t_best), fast | ref << 1) each.
// `controls` adds the two negative controls (they read in-bounds memory only and merely compute wrong answers): the lock-step walk
// with every reuse bit set, and the 16-byte-node walk on a device copy of the scene whose LEAF-LIST boxes are the root box.
// Exit status 0 and one summary line on success; any HIP error ends the program with status 2; nothing is retried.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "flat_reuse.h"
#include "kernels.h"
#include "rt_path.h"

using namespace trt;

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("%s: %s\n", #x, hipGetErrorString(e_)); std::exit(2); } } while (0)

constexpr int kThreads = 256;                 // four waves per workgroup, as the production pool kernels
constexpr uint32_t kUnwritten = 0xCDCDCDCDu;  // out.bin is filled with it: a ray no kernel answered shows

TRT_DEV uint32_t lane_rank(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
TRT_DEV Ray load_ray(const float* __restrict__ rays, uint32_t idx) {
    const float* r = rays + 6ull * idx;
    Ray ray;
    ray.o = v3(r[0], r[1], r[2]);
    ray.d = v3(r[3], r[4], r[5]);
    return ray;
}
TRT_DEV void store_answer(uint32_t* __restrict__ out, uint32_t idx, uint32_t prim, float t, bool fast, bool ref) {
    out[3ull * idx] = prim;
    out[3ull * idx + 1u] = __float_as_uint(t);
    out[3ull * idx + 2u] = (fast ? 1u : 0u) | (ref ? 2u : 0u);
}
// this lane's slot 0 of the wave's leaf stack (streamed.hip: behind the scene copy, slots x 64 x 8 bytes per wave)
template <int MODE>
TRT_DEV float2* leaf_stack_of(const SceneAcc<MODE>& sc, uint32_t slots, uint32_t stacks_per_lane) {
    char* const tail = reinterpret_cast<char*>(g_lds) + ((sc.lds_bytes() + 15u) & ~15u);
    return reinterpret_cast<float2*>(tail) + (stacks_per_lane * (threadIdx.x >> 6)) * (64u * slots) + (threadIdx.x & 63u);
}

// Walks that run to their end in one call (closest_hit): a wave goes through its list 64 rays at a time.
template <int MODE, int WALK>
__global__ __launch_bounds__(kThreads) void direct_kernel(SceneDev scd, const float* __restrict__ rays, const uint2* __restrict__ tasks, uint32_t n_tasks,
                                                          uint32_t* __restrict__ out, uint32_t slots, uint32_t use_stack, uint32_t ref_tree,
                                                          const float4* __restrict__ leaf_list, const uint4* __restrict__ nodes16, FlatReuse reuse) {
    stage_scene_to_lds<MODE>(scd);
    const SceneAcc<MODE> sc{scd.blob, scd.L};
    const uint32_t lane = threadIdx.x & 63u, wave = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (wave >= n_tasks) return;
    float2* const stack = use_stack ? leaf_stack_of<MODE>(sc, slots, 1u) : nullptr;
    const uint2 task = tasks[wave];
    Counters<false> ctr;
    for (uint32_t base = 0; base < task.y; base += 64u) {
        if (base + lane < task.y) {
            const uint32_t idx = task.x + base + lane;
            const Ray ray = load_ray(rays, idx);
            // closest_hit keeps its Trav to itself, so these flags come from a SECOND trav_begin whose last argument restates closest_hit's
            // private `fused_loop` expression: they show which path the ray is meant to take, and would go stale if rt_path.h changed
            // that expression.  Only the resumable and two-path kernels below report the flags of the Trav that actually walked.
            const bool fused = kAsmBoxLoop && (WALK == WALK_COMPACT || (WALK == WALK_RUNTIME && stack != nullptr && nodes16 != nullptr));
            const Trav t0 = trav_begin<MODE>(sc, ray, ref_tree != 0u, fused);
            float t;
            const uint32_t prim = closest_hit<MODE, false, WALK>(sc, ray, ref_tree != 0u, t, ctr, slots, stack, leaf_list, nodes16, reuse);
            store_answer(out, idx, prim, t, t0.fast, t0.ref);
        }
    }
}

// The resumable per-lane tree walks, in the rounds of stream_sample_kernel: every lane without a ray takes the next one of the wave's
// list; every lane with a ray sets its walk up (or takes a parked one back) and walks; a finished walk is written out, an unfinished
// one stays parked in the lane's leaf stack.
template <int MODE, int WALK>
__global__ __launch_bounds__(kThreads) void resume_kernel(SceneDev scd, const float* __restrict__ rays, const uint2* __restrict__ tasks, uint32_t n_tasks,
                                                          uint32_t* __restrict__ out, uint32_t slots, uint32_t stragglers,
                                                          const float4* __restrict__ leaf_list, const uint4* __restrict__ nodes16) {
    stage_scene_to_lds<MODE>(scd);
    const SceneAcc<MODE> sc{scd.blob, scd.L};
    const uint32_t wave = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (wave >= n_tasks) return;
    float2* const stack = leaf_stack_of<MODE>(sc, slots, 1u);
    const uint2 task = tasks[wave];
    Counters<false> ctr;
    uint32_t cursor = 0;                                                   // wave-uniform
    bool has = false, walking = false;
    uint32_t idx = 0;
    Ray ray;
    ray.o = v3(0.0f, 0.0f, 0.0f); ray.d = v3(0.0f, 0.0f, 0.0f);
    for (;;) {
        const uint64_t need = __builtin_amdgcn_ballot_w64(!has);
        if (need != 0ull && cursor < task.y) {
            const uint32_t item = cursor + lane_rank(need);
            if (!has && item < task.y) { idx = task.x + item; ray = load_ray(rays, idx); has = true; }
            cursor += (uint32_t)__builtin_popcountll(need);
            if (cursor > task.y) cursor = task.y;
        }
        if (__builtin_amdgcn_ballot_w64(has) == 0ull) break;
        if (has) {
            Trav tr = trav_begin<MODE, WALK == WALK_COMPACT>(sc, ray, false);
            if (walking) trav_unpark(stack, tr);
            const uint32_t entered = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(true));
            walking = !closest_hit_resume<MODE, false, WALK>(sc, ray, tr, ctr, slots, stack, leaf_list, nodes16, stragglers, entered);
            if (!walking) {
                store_answer(out, idx, tr.prim_best, tr.t_best, tr.fast, tr.ref);
                has = false;
            }
        }
    }
}

// Two rays per lane, in the rounds of stream_dual_kernel (slot A's stack, then slot B's).
struct DualRay {
    Ray ray;
    uint32_t idx = 0;
    bool has = false, walking = false;
};
__global__ __launch_bounds__(kThreads) void dual_kernel(SceneDev scd, const float* __restrict__ rays, const uint2* __restrict__ tasks, uint32_t n_tasks,
                                                        uint32_t* __restrict__ out, uint32_t slots, uint32_t stragglers,
                                                        const float4* __restrict__ leaf_list, const uint4* __restrict__ nodes16) {
    constexpr int MODE = MODE_GLOBAL;
    const SceneAcc<MODE> sc{scd.blob, scd.L};
    const uint32_t wave = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (wave >= n_tasks) return;
    float2* const stkA = leaf_stack_of<MODE>(sc, slots, 2u);
    float2* const stkB = stkA + 64u * slots;
    const uint2 task = tasks[wave];
    Counters<false> ctr;
    uint32_t cursor = 0;                                                   // wave-uniform
    DualRay A, B;
    A.ray.o = A.ray.d = B.ray.o = B.ray.d = v3(0.0f, 0.0f, 0.0f);
    auto take = [&](DualRay& S) {
        const uint64_t need = __builtin_amdgcn_ballot_w64(!S.has);
        if (need == 0ull || cursor >= task.y) return;
        const uint32_t item = cursor + lane_rank(need);
        if (!S.has && item < task.y) { S.idx = task.x + item; S.ray = load_ray(rays, S.idx); S.has = true; }
        cursor += (uint32_t)__builtin_popcountll(need);
        if (cursor > task.y) cursor = task.y;
    };
    auto settle = [&](DualRay& S, Trav& tr, bool done, float2* stk) {
        if (!S.has) return;
        if (!done) { trav_park(stk, tr); S.walking = true; return; }
        S.walking = false;
        store_answer(out, S.idx, tr.prim_best, tr.t_best, tr.fast, tr.ref);
        S.has = false;
    };
    for (;;) {
        take(A);
        take(B);
        if (__builtin_amdgcn_ballot_w64(A.has || B.has) == 0ull) break;
        Trav trA = trav_begin<MODE, true>(sc, A.ray, false), trB = trav_begin<MODE, true>(sc, B.ray, false);
        if (A.has && A.walking) trav_unpark(stkA, trA);
        if (B.has && B.walking) trav_unpark(stkB, trB);
        const uint32_t entered = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(A.has)) +
                                 (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(B.has));
        bool doneA = false, doneB = false;
        walk_compact2<MODE>(sc, nodes16, leaf_list, A.ray, trA, A.has, B.ray, trB, B.has, ctr, stkA, stkB, slots, stragglers, entered, doneA, doneB);
        settle(A, trA, doneA, stkA);
        settle(B, trB, doneB, stkB);
    }
}

// ------------------------------------------------------------------------------------------------------------------
namespace {

std::vector<uint32_t> read_words(const char* path) {
    std::vector<uint32_t> w;
    FILE* f = std::fopen(path, "rb");
    if (!f) { std::printf("cannot open %s\n", path); std::exit(3); }
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    w.resize((size_t)n / 4u);
    if (n > 0 && std::fread(w.data(), 4, w.size(), f) != w.size()) { std::printf("short read of %s\n", path); std::exit(3); }
    std::fclose(f);
    return w;
}
float as_float(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
uint32_t as_bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

enum Kind { DIRECT, RESUME, DUAL };
struct Variant {
    std::string name;
    Kind kind;
    int walk;                           // WALK_* of the kernel
    uint32_t slots, stragglers;
    bool stack, list, nodes, ref_tree;  // direct kernels: what closest_hit is handed
    int reuse;                          // lock-step walk: 0 no reuse, 1 the scene's masks, 2 every bit set (negative control)
    bool root_leaf_boxes;               // negative control: the device copy whose leaf-list boxes are the root box
};

struct Run {
    SceneDev scd, scd_control;
    const SceneLayout* L;
    int mode;
    const float* d_rays;
    const uint2* d_tasks;
    uint32_t n_rays, n_tasks;
    uint32_t* d_out;
    FlatReuse reuse;
};

template <typename K>
void set_lds(K kernel, size_t bytes) {
    if (bytes > kLdsPerCu) { std::printf("LDS plan of %zu bytes\n", bytes); std::exit(3); }
    CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
}

template <int MODE, int WALK>
void launch_direct(const Run& r, const Variant& v, const SceneDev& scd, const float4* list, const uint4* nodes, FlatReuse reuse) {
    const size_t lds = LdsLayout{MODE == MODE_LDS ? r.L->hot_bytes : 0u, kThreads, v.stack ? v.slots : 0u, 1u, false}.total();
    set_lds(direct_kernel<MODE, WALK>, lds);
    const uint32_t blocks = (r.n_tasks + 3u) / 4u;
    hipLaunchKernelGGL((direct_kernel<MODE, WALK>), dim3(blocks), dim3(kThreads), lds, 0, scd, r.d_rays, r.d_tasks, r.n_tasks, r.d_out, v.slots,
                       v.stack ? 1u : 0u, v.ref_tree ? 1u : 0u, list, nodes, reuse);
}
template <int MODE, int WALK>
void launch_resume(const Run& r, const Variant& v, const SceneDev& scd, const float4* list, const uint4* nodes) {
    const size_t lds = LdsLayout{MODE == MODE_LDS ? r.L->hot_bytes : 0u, kThreads, v.slots, 1u, false}.total();
    set_lds(resume_kernel<MODE, WALK>, lds);
    const uint32_t blocks = (r.n_tasks + 3u) / 4u;
    hipLaunchKernelGGL((resume_kernel<MODE, WALK>), dim3(blocks), dim3(kThreads), lds, 0, scd, r.d_rays, r.d_tasks, r.n_tasks, r.d_out, v.slots,
                       v.stragglers, list, nodes);
}

void run_variant(const Run& r, const Variant& v) {
    const SceneDev& scd = v.root_leaf_boxes ? r.scd_control : r.scd;
    const float4* list = v.list ? scd.blob + r.L->off_leaf_list : nullptr;
    const uint4* nodes = v.nodes ? reinterpret_cast<const uint4*>(scd.blob + r.L->off_compact) : nullptr;
    const FlatReuse reuse = v.reuse == 1 ? r.reuse : v.reuse == 2 ? FlatReuse{~0u, ~0u, ~0u} : FlatReuse{0u, 0u, 0u};
    // what the walks assume, checked where the launch is made
    const bool lock_step = v.walk == WALK_FLAT || (v.stack && v.list && !v.nodes);           // walk_flat: two leaves per trip, at most 32 leaves
    const bool two_slots = v.kind != DIRECT || lock_step;                                     // a parked walk occupies two slots too
    if (v.slots < 1u || v.slots > kLdsLeafSlotsMax || (two_slots && v.slots < 2u) || (lock_step && (r.L->n_leaves > kFlatWalkMaxLeaves || r.mode != MODE_LDS)) ||
        (v.nodes && r.L->off_compact == 0u) || (v.walk == WALK_LDS_STACK && r.mode != MODE_LDS) || ((v.walk == WALK_COMPACT || v.kind == DUAL) && r.mode != MODE_GLOBAL)) {
        std::printf("variant %s does not fit this scene\n", v.name.c_str());
        std::exit(3);
    }
    CHECK(hipMemset(r.d_out, 0xCD, 12ull * r.n_rays));
    if (v.kind == DUAL) {
        const size_t lds = LdsLayout{0u, kThreads, v.slots, 2u, false}.total();
        set_lds(dual_kernel, lds);
        hipLaunchKernelGGL(dual_kernel, dim3((r.n_tasks + 3u) / 4u), dim3(kThreads), lds, 0, scd, r.d_rays, r.d_tasks, r.n_tasks, r.d_out, v.slots,
                           v.stragglers, list, nodes);
    } else if (v.kind == RESUME) {
        if (v.walk == WALK_COMPACT) launch_resume<MODE_GLOBAL, WALK_COMPACT>(r, v, scd, list, nodes);
        else launch_resume<MODE_LDS, WALK_LDS_STACK>(r, v, scd, list, nodes);
    } else if (v.walk == WALK_FLAT) {
        launch_direct<MODE_LDS, WALK_FLAT>(r, v, scd, list, nodes, reuse);
    } else if (v.walk == WALK_REGS) {
        if (r.mode == MODE_LDS) launch_direct<MODE_LDS, WALK_REGS>(r, v, scd, list, nodes, reuse);
        else launch_direct<MODE_GLOBAL, WALK_REGS>(r, v, scd, list, nodes, reuse);
    } else {
        if (r.mode == MODE_LDS) launch_direct<MODE_LDS, WALK_RUNTIME>(r, v, scd, list, nodes, reuse);
        else launch_direct<MODE_GLOBAL, WALK_RUNTIME>(r, v, scd, list, nodes, reuse);
    }
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
}

// One scene: its rays through every walk variant it has.  Returns the number of rays no kernel answered; *n_variants = variants run.
unsigned long long run_scene(const char* scene_path, const char* rays_path, const char* out_bin, const char* out_txt, bool controls, size_t* n_variants,
                             uint32_t* n_rays_out) {
    // ---- the scene: World -> compile_scene, as capi.hip does ----
    const std::vector<uint32_t> sw = read_words(scene_path);
    if (sw.size() < 6 || sw[0] != 0x31535257u || sw.size() != 6u + 5ull * sw[1] + 11ull * sw[2]) { std::printf("bad scene file\n"); std::exit(3); }
    World world;
    for (uint32_t m = 0; m < sw[1]; m++) {
        const uint32_t* p = &sw[6u + 5ull * m];
        world.material_index.emplace("m" + std::to_string(m), m);
        world.materials.push_back(trt_material{p[0], trt_vec3{as_float(p[1]), as_float(p[2]), as_float(p[3])}, as_float(p[4])});
    }
    for (uint32_t g = 0; g < sw[2]; g++) {
        const uint32_t* p = &sw[6u + 5ull * sw[1] + 11ull * g];
        Geometry geo{};
        geo.kind = p[0]; geo.material = p[1];
        geo.a = trt_vec3{as_float(p[2]), as_float(p[3]), as_float(p[4])};
        geo.b = trt_vec3{as_float(p[5]), as_float(p[6]), as_float(p[7])};
        geo.c = trt_vec3{as_float(p[8]), as_float(p[9]), as_float(p[10])};
        world.geometries.push_back(geo);
    }
    trt_scene_options opt = scene_options_builtin();
    opt.cull_prune = as_float(sw[3]); opt.flat_walk = (int32_t)sw[4]; opt.compact_nodes = (int32_t)sw[5];
    SceneHost host;
    std::string msg;
    if (!compile_scene(world, opt, host, msg)) { std::printf("compile_scene: %s\n", msg.c_str()); std::exit(3); }
    const SceneLayout& L = host.layout;
    const int mode = scene_mode(L) == 1 ? MODE_LDS : MODE_GLOBAL;
    uint32_t masks[3];
    flat_reuse_masks(L.flat_walk ? host.blob.data() + 16u * (size_t)L.off_leaf_list : nullptr, L.n_leaves, L.flat_walk != 0u, masks);

    // ---- the rays ----
    const std::vector<uint32_t> rw = read_words(rays_path);
    if (rw.size() < 3 || rw[0] != 0x31525257u || rw.size() != 3u + 6ull * rw[1] + 2ull * rw[2]) { std::printf("bad ray file\n"); std::exit(3); }
    const uint32_t n_rays = rw[1], n_tasks = rw[2];
    {   // the tasks partition the rays: every output record is written once, none out of bounds
        std::vector<uint8_t> seen(n_rays, 0);
        for (uint32_t k = 0; k < n_tasks; k++) {
            const uint32_t b = rw[3u + 6ull * n_rays + 2ull * k], c = rw[3u + 6ull * n_rays + 2ull * k + 1u];
            if (b > n_rays || c > n_rays - b) { std::printf("task %u out of range\n", k); std::exit(3); }
            for (uint32_t i = b; i < b + c; i++) { if (seen[i]++) { std::printf("ray %u in two tasks\n", i); std::exit(3); } }
        }
        for (uint32_t i = 0; i < n_rays; i++) if (!seen[i]) { std::printf("ray %u in no task\n", i); std::exit(3); }
    }
    if (n_rays == 0 || n_tasks == 0) { std::printf("no rays\n"); std::exit(3); }

    // ---- device copies ----
    Run r{};
    float4* d_blob = nullptr;
    CHECK(hipMalloc(&d_blob, host.blob.size()));
    CHECK(hipMemcpy(d_blob, host.blob.data(), host.blob.size(), hipMemcpyHostToDevice));
    r.scd = SceneDev{d_blob, L};
    r.scd_control = r.scd;
    if (controls && L.off_compact != 0u) {
        std::vector<uint8_t> blob2 = host.blob;                               // leaf-list boxes := the culling root's box (links kept)
        const float* root = reinterpret_cast<const float*>(host.blob.data());
        for (uint32_t k = 0; k < L.n_leaves + kLeafListPad; k++)
            std::memcpy(blob2.data() + 16u * ((size_t)L.off_leaf_list + 2u * k), root, 6 * sizeof(float));
        float4* d_blob2 = nullptr;
        CHECK(hipMalloc(&d_blob2, blob2.size()));
        CHECK(hipMemcpy(d_blob2, blob2.data(), blob2.size(), hipMemcpyHostToDevice));
        r.scd_control = SceneDev{d_blob2, L};
    }
    float* d_rays = nullptr;
    uint2* d_tasks = nullptr;
    uint32_t* d_out = nullptr;
    CHECK(hipMalloc(&d_rays, 24ull * n_rays));
    CHECK(hipMemcpy(d_rays, &rw[3], 24ull * n_rays, hipMemcpyHostToDevice));
    CHECK(hipMalloc(&d_tasks, 8ull * n_tasks));
    CHECK(hipMemcpy(d_tasks, &rw[3u + 6ull * n_rays], 8ull * n_tasks, hipMemcpyHostToDevice));
    CHECK(hipMalloc(&d_out, 12ull * n_rays));
    r.L = &L; r.mode = mode; r.d_rays = d_rays; r.d_tasks = d_tasks; r.n_rays = n_rays; r.n_tasks = n_tasks; r.d_out = d_out;
    r.reuse = FlatReuse{masks[0], masks[1], masks[2]};

    // ---- the variants this scene has (only parameter values the launch plan can produce: a parked walk needs two slots) ----
    std::vector<Variant> vs;
    auto name = [](const char* base, uint32_t slots, int extra, const char* extra_name) {
        std::string s = std::string(base) + "_s" + std::to_string(slots);
        if (extra >= 0) s += std::string("_") + extra_name + std::to_string(extra);
        return s;
    };
    const bool flat = L.flat_walk != 0u && mode == MODE_LDS && L.n_leaves <= kFlatWalkMaxLeaves;
    const bool compact = L.off_compact != 0u && mode == MODE_GLOBAL;
    if (flat) {
        for (int reuse = 1; reuse >= 0; reuse--)
            for (uint32_t slots : {2u, 7u, 16u}) vs.push_back(Variant{name("flat", slots, reuse, "reuse"), DIRECT, WALK_FLAT, slots, 0u, true, true, false, false, reuse, false});
    }
    if (mode == MODE_LDS) {
        for (uint32_t slots : {2u, 5u, 16u})
            for (uint32_t st : {0u, 1u, 8u, 63u}) vs.push_back(Variant{name("lds", slots, (int)st, "strag"), RESUME, WALK_LDS_STACK, slots, st, true, false, false, false, 0, false});
    }
    if (compact) {
        for (uint32_t slots : {2u, 4u})
            for (uint32_t st : {0u, 8u}) {
                vs.push_back(Variant{name("compact", slots, (int)st, "strag"), RESUME, WALK_COMPACT, slots, st, true, true, true, false, 0, false});
                vs.push_back(Variant{name("compact2", slots, (int)st, "strag"), DUAL, WALK_COMPACT, slots, st, true, true, true, false, 0, false});
            }
    }
    vs.push_back(Variant{"regs", DIRECT, WALK_REGS, 4u, 0u, false, false, false, false, 0, false});
    for (uint32_t slots : {1u, 2u, 4u}) vs.push_back(Variant{name("runtime_regs", slots, -1, ""), DIRECT, WALK_RUNTIME, slots, 0u, false, false, false, false, 0, false});
    if (flat) vs.push_back(Variant{"runtime_flat_s7", DIRECT, WALK_RUNTIME, 7u, 0u, true, true, false, false, 1, false});
    if (mode == MODE_LDS) vs.push_back(Variant{"runtime_lds_s5", DIRECT, WALK_RUNTIME, 5u, 0u, true, false, false, false, 0, false});
    if (compact) vs.push_back(Variant{"runtime_compact_s4", DIRECT, WALK_RUNTIME, 4u, 0u, true, true, true, false, 0, false});
    vs.push_back(Variant{"ref_tree", DIRECT, WALK_RUNTIME, 4u, 0u, false, false, false, true, 0, false});
    if (controls && flat) vs.push_back(Variant{"control_flat_s7_reuse_all_ones", DIRECT, WALK_FLAT, 7u, 0u, true, true, false, false, 2, false});
    if (controls && compact) vs.push_back(Variant{"control_compact_s4_root_leaf_boxes", RESUME, WALK_COMPACT, 4u, 8u, true, true, true, false, 0, true});

    FILE* fo = std::fopen(out_bin, "wb");
    FILE* ft = std::fopen(out_txt, "w");
    if (!fo || !ft) { std::printf("cannot write the output files\n"); std::exit(3); }
    std::fprintf(ft, "layout mode=%d flat=%d compact=%d n_leaves=%u all_finite=%u limit=%08x,%08x,%08x asm=%d reuse=%08x,%08x,%08x\n", mode, flat ? 1 : 0,
                 compact ? 1 : 0, L.n_leaves, L.all_finite, as_bits(L.compact_origin_limit[0]), as_bits(L.compact_origin_limit[1]),
                 as_bits(L.compact_origin_limit[2]), kAsmBoxLoop ? 1 : 0, masks[0], masks[1], masks[2]);
    std::vector<uint32_t> h(3ull * n_rays);
    unsigned long long unwritten = 0;
    for (const Variant& v : vs) {
        run_variant(r, v);
        CHECK(hipMemcpy(h.data(), d_out, 12ull * n_rays, hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < n_rays; i++) unwritten += h[3ull * i + 2u] == kUnwritten;
        if (std::fwrite(h.data(), 4, h.size(), fo) != h.size()) { std::printf("short write\n"); std::exit(3); }
        std::fprintf(ft, "variant %s\n", v.name.c_str());
    }
    std::fclose(fo);
    std::fclose(ft);
    CHECK(hipFree(d_out));
    CHECK(hipFree(d_tasks));
    CHECK(hipFree(d_rays));
    if (r.scd_control.blob != r.scd.blob) CHECK(hipFree(const_cast<float4*>(r.scd_control.blob)));
    CHECK(hipFree(d_blob));
    *n_variants = vs.size();
    *n_rays_out = n_rays;
    return unwritten;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 6 || (argc - 2) % 4 != 0 || (std::strcmp(argv[1], "plain") != 0 && std::strcmp(argv[1], "controls") != 0)) {
        std::printf("usage: walk_rays plain|controls scene.bin rays.bin out.bin out.txt [...]\n");
        return 3;
    }
    const bool controls = std::strcmp(argv[1], "controls") == 0;
    unsigned long long unwritten = 0, answers = 0;
    int scenes = 0;
    for (int k = 2; k + 3 < argc; k += 4, scenes++) {
        size_t n_variants = 0;
        uint32_t n_rays = 0;
        unwritten += run_scene(argv[k], argv[k + 1], argv[k + 2], argv[k + 3], controls, &n_variants, &n_rays);
        answers += (unsigned long long)n_variants * n_rays;
    }
    std::printf("walk_rays: %d scenes, %llu answers, %llu unanswered\n", scenes, answers, unwritten);
    return unwritten ? 1 : 0;
}
