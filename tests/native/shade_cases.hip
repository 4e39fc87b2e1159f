// Test program (tests/test_gpu_shade.py builds and runs it on the GPU box): the shade cases of tests/shade_cases.py through the
// product's shade_hit and shade_hit_info (rt_path.h: two forwarders to one body), one case per lane, and a list of vectors through the helpers of rt_device.h (normalized, ray_new,
// reflect, refract, near_zero, ray_at).  There is no shading or vector code in this file: the kernels load a Path, call shade_hit /
// the helpers and write every word back for the Python side to compare with the oracle, bit for bit.
//
//   shade_cases [run <scene.bin> <cases.bin> <out.bin> <out.txt>]... [vec <vec.bin> <out.bin>]
//
// scene.bin: the scene file of tests/native/walk_rays.hip ('WRS1'; tests/walk_ray_cases.write_scene_file).
// cases.bin: u32 'SHC1', n_cases, n_tasks; n_cases x 22 words: origin[3], direction[3], color[3], atten[3], remain, s0, s1,
//            prim (rt_path.h reference: kind bit | index within kind; 0xFFFFFFFF = miss), bits(t), background[3], lazy_ok;
//            n_tasks x (begin, count): the case list of one wave.  The tasks partition the cases.
// out.txt:   one `layout ...` line and one `variant NAME` line per instantiation run, in the order of their records in out.bin:
//            n_cases x 21 words each - the 15 words of the Path afterwards, `ended`, and the five shade counters of the lane
//            (shade, lambertian, metal, dielectric, light; zero without STATS).
//            lds_carried <LDS, false, false>   lds_lazy <LDS, false, true>   lds_stats <LDS, true, false>
//            global_carried <GLOBAL, false, false>   global_lazy <GLOBAL, false, true>
//            lds_info, lds_info_hidden <LDS, false>   global_info, global_info_hidden <GLOBAL, false>: shade_hit_info, the forwarder
//            the next-event queries call, with hide_light = 0 and = 1.  Words 16 .. 19 of a record are info.kind and info.normal as
//            the call left them (set beforehand to 0x5EEDC0DE and to three floats of those bits), word 20 is 0.
//            The GLOBAL forms read the same packed scene through SceneAcc<MODE_GLOBAL> (same element offsets, rt_path.h), whatever its size.
//            The LAZY forms run only the cases flagged lazy_ok and leave the others' records unwritten (0xCDCDCDCD); a flagged case whose
//            incoming colour is not +0, or a flag on a scene without SceneLayout::lazy_color, is refused (exit status 3).
// vec.bin:   u32 'SHV1', n; n x 7 words: a[3], b[3], s.  out.bin: n x 20 words: normalized(a)[3], ray_new(b, a) origin[3] direction[3],
//            reflect(a, b)[3], refract(a, b, s)[3], near_zero(a), ray_at(Ray{a, b}, s)[3], 0.
// Exit status 0 on success; any HIP error ends the program with status 2, a bad input with 3; nothing is retried.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "kernels.h"
#include "rt_path.h"

using namespace trt;

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("%s: %s\n", #x, hipGetErrorString(e_)); std::exit(2); } } while (0)

constexpr int kThreads = 256;                 // four waves per workgroup, as the production pool kernels
constexpr uint32_t kCaseWords = 22, kOutWords = 21, kVecWords = 7, kVecOutWords = 20;

template <int MODE, bool STATS, bool LAZY>
__global__ __launch_bounds__(kThreads) void shade_kernel(SceneDev scd, const uint32_t* __restrict__ cases, const uint2* __restrict__ tasks, uint32_t n_tasks,
                                                         uint32_t* __restrict__ out) {
    stage_scene_to_lds<MODE>(scd);
    const SceneAcc<MODE> sc{scd.blob, scd.L};
    const uint32_t lane = threadIdx.x & 63u, wave = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (wave >= n_tasks) return;
    const uint2 task = tasks[wave];
    for (uint32_t base = 0; base < task.y; base += 64u) {
        if (base + lane >= task.y) continue;
        const uint32_t idx = task.x + base + lane;
        const uint32_t* c = cases + (size_t)kCaseWords * idx;
        if (LAZY && c[21] == 0u) continue;
        auto f = [&](uint32_t k) { return __uint_as_float(c[k]); };
        Path p;
        p.ray.o = v3(f(0), f(1), f(2));
        p.ray.d = v3(f(3), f(4), f(5));
        p.color = v3(f(6), f(7), f(8));
        p.atten = v3(f(9), f(10), f(11));
        p.remain = c[12];
        p.rng.s0 = c[13]; p.rng.s1 = c[14];
        Counters<STATS> ctr;
        const bool ended = shade_hit<MODE, STATS, LAZY>(sc, p, c[15], f(16), v3(f(17), f(18), f(19)), ctr);
        uint32_t* o = out + (size_t)kOutWords * idx;
        o[0] = __float_as_uint(p.ray.o.x); o[1] = __float_as_uint(p.ray.o.y); o[2] = __float_as_uint(p.ray.o.z);
        o[3] = __float_as_uint(p.ray.d.x); o[4] = __float_as_uint(p.ray.d.y); o[5] = __float_as_uint(p.ray.d.z);
        o[6] = __float_as_uint(p.color.x); o[7] = __float_as_uint(p.color.y); o[8] = __float_as_uint(p.color.z);
        o[9] = __float_as_uint(p.atten.x); o[10] = __float_as_uint(p.atten.y); o[11] = __float_as_uint(p.atten.z);
        o[12] = p.remain; o[13] = p.rng.s0; o[14] = p.rng.s1;
        o[15] = ended ? 1u : 0u;
        if constexpr (STATS) {
            o[16] = ctr.shade; o[17] = ctr.shade_lambertian; o[18] = ctr.shade_metal; o[19] = ctr.shade_dielectric; o[20] = ctr.shade_light;
        } else {
            o[16] = o[17] = o[18] = o[19] = o[20] = 0u;
        }
    }
}

// The same cases through shade_hit_info<MODE, false>: the 16 words above, then what the call left in `info`.
constexpr uint32_t kInfoUnset = 0x5EEDC0DEu;
template <int MODE>
__global__ __launch_bounds__(kThreads) void shade_info_kernel(SceneDev scd, const uint32_t* __restrict__ cases, const uint2* __restrict__ tasks,
                                                              uint32_t n_tasks, uint32_t hide_light, uint32_t* __restrict__ out) {
    stage_scene_to_lds<MODE>(scd);
    const SceneAcc<MODE> sc{scd.blob, scd.L};
    const uint32_t lane = threadIdx.x & 63u, wave = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (wave >= n_tasks) return;
    const uint2 task = tasks[wave];
    for (uint32_t base = 0; base < task.y; base += 64u) {
        if (base + lane >= task.y) continue;
        const uint32_t idx = task.x + base + lane;
        const uint32_t* c = cases + (size_t)kCaseWords * idx;
        auto f = [&](uint32_t k) { return __uint_as_float(c[k]); };
        Path p;
        p.ray.o = v3(f(0), f(1), f(2));
        p.ray.d = v3(f(3), f(4), f(5));
        p.color = v3(f(6), f(7), f(8));
        p.atten = v3(f(9), f(10), f(11));
        p.remain = c[12];
        p.rng.s0 = c[13]; p.rng.s1 = c[14];
        Counters<false> ctr;
        ShadeInfo info;
        info.hide_light = hide_light != 0u;
        info.kind = kInfoUnset;
        info.normal = v3(__uint_as_float(kInfoUnset), __uint_as_float(kInfoUnset), __uint_as_float(kInfoUnset));
        const bool ended = shade_hit_info<MODE, false>(sc, p, c[15], f(16), v3(f(17), f(18), f(19)), ctr, info);
        uint32_t* o = out + (size_t)kOutWords * idx;
        o[0] = __float_as_uint(p.ray.o.x); o[1] = __float_as_uint(p.ray.o.y); o[2] = __float_as_uint(p.ray.o.z);
        o[3] = __float_as_uint(p.ray.d.x); o[4] = __float_as_uint(p.ray.d.y); o[5] = __float_as_uint(p.ray.d.z);
        o[6] = __float_as_uint(p.color.x); o[7] = __float_as_uint(p.color.y); o[8] = __float_as_uint(p.color.z);
        o[9] = __float_as_uint(p.atten.x); o[10] = __float_as_uint(p.atten.y); o[11] = __float_as_uint(p.atten.z);
        o[12] = p.remain; o[13] = p.rng.s0; o[14] = p.rng.s1;
        o[15] = ended ? 1u : 0u;
        o[16] = info.kind;
        o[17] = __float_as_uint(info.normal.x); o[18] = __float_as_uint(info.normal.y); o[19] = __float_as_uint(info.normal.z);
        o[20] = 0u;
    }
}

__global__ __launch_bounds__(kThreads) void vec_kernel(const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t* c = in + (size_t)kVecWords * i;
    const V3 a = v3(__uint_as_float(c[0]), __uint_as_float(c[1]), __uint_as_float(c[2]));
    const V3 b = v3(__uint_as_float(c[3]), __uint_as_float(c[4]), __uint_as_float(c[5]));
    const float s = __uint_as_float(c[6]);
    uint32_t* o = out + (size_t)kVecOutWords * i;
    auto put = [&](uint32_t k, V3 v) { o[k] = __float_as_uint(v.x); o[k + 1u] = __float_as_uint(v.y); o[k + 2u] = __float_as_uint(v.z); };
    put(0, normalized(a));
    const Ray r = ray_new(b, a);
    put(3, r.o);
    put(6, r.d);
    put(9, reflect(a, b));
    put(12, refract(a, b, s));
    o[15] = near_zero(a) ? 1u : 0u;
    put(16, ray_at(Ray{a, b}, s));
    o[19] = 0u;
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

void write_words(const char* path, const std::vector<uint32_t>& w, const char* mode) {
    FILE* f = std::fopen(path, mode);
    if (!f || std::fwrite(w.data(), 4, w.size(), f) != w.size()) { std::printf("cannot write %s\n", path); std::exit(3); }
    std::fclose(f);
}

template <int MODE, bool STATS, bool LAZY>
void launch(const SceneDev& scd, const uint32_t* d_cases, const uint2* d_tasks, uint32_t n_tasks, uint32_t* d_out) {
    const size_t lds = MODE == MODE_LDS ? ((size_t)scd.L.hot_bytes + 15u) & ~(size_t)15u : 0u;
    if (lds > 64u * 1024u) { std::printf("LDS plan of %zu bytes\n", lds); std::exit(3); }
    CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(shade_kernel<MODE, STATS, LAZY>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((shade_kernel<MODE, STATS, LAZY>), dim3((n_tasks + 3u) / 4u), dim3(kThreads), lds, 0, scd, d_cases, d_tasks, n_tasks, d_out);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
}

template <int MODE>
void launch_info(const SceneDev& scd, const uint32_t* d_cases, const uint2* d_tasks, uint32_t n_tasks, uint32_t hide_light, uint32_t* d_out) {
    const size_t lds = MODE == MODE_LDS ? ((size_t)scd.L.hot_bytes + 15u) & ~(size_t)15u : 0u;
    if (lds > 64u * 1024u) { std::printf("LDS plan of %zu bytes\n", lds); std::exit(3); }
    CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(shade_info_kernel<MODE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((shade_info_kernel<MODE>), dim3((n_tasks + 3u) / 4u), dim3(kThreads), lds, 0, scd, d_cases, d_tasks, n_tasks, hide_light, d_out);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
}

unsigned long long run_scene(const char* scene_path, const char* cases_path, const char* out_bin, const char* out_txt) {
    // ---- the scene: World -> compile_scene, as capi.hip does (the fuzz of a metal arrives clamped: capi.hip does that at creation) ----
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
        if (geo.material >= sw[1] || geo.kind > 1u) { std::printf("geometry %u: bad kind or material\n", g); std::exit(3); }
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
    if (scene_mode(L) != 1 || L.hot_bytes > kLdsSceneMaxBytes) { std::printf("the scene does not fit the LDS\n"); std::exit(3); }

    // ---- the cases: every primitive reference inside the scene, the tasks a partition, the LAZY flags legal ----
    const std::vector<uint32_t> cw = read_words(cases_path);
    if (cw.size() < 3 || cw[0] != 0x31434853u || cw.size() != 3u + (size_t)kCaseWords * cw[1] + 2ull * cw[2]) { std::printf("bad case file\n"); std::exit(3); }
    const uint32_t n_cases = cw[1], n_tasks = cw[2];
    if (n_cases == 0 || n_tasks == 0) { std::printf("no cases\n"); std::exit(3); }
    for (uint32_t i = 0; i < n_cases; i++) {
        const uint32_t* c = &cw[3u + (size_t)kCaseWords * i];
        const uint32_t prim = c[15], idx = prim & PRIM_INDEX_MASK;
        const bool ok = prim == PRIM_NONE || ((prim & ~(PRIM_QUAD_BIT | PRIM_INDEX_MASK)) == 0u && idx < ((prim & PRIM_QUAD_BIT) ? L.n_quads : L.n_spheres));
        if (!ok) { std::printf("case %u: primitive reference %08x outside the scene\n", i, prim); std::exit(3); }
        if (c[21] != 0u && (L.lazy_color == 0u || c[6] != 0u || c[7] != 0u || c[8] != 0u)) {
            std::printf("case %u: the LAZY form is not legal here (lazy_color %u, colour %08x %08x %08x)\n", i, L.lazy_color, c[6], c[7], c[8]);
            std::exit(3);
        }
    }
    {
        std::vector<uint8_t> seen(n_cases, 0);
        const uint32_t* t = &cw[3u + (size_t)kCaseWords * n_cases];
        for (uint32_t k = 0; k < n_tasks; k++) {
            const uint32_t b = t[2u * k], c = t[2u * k + 1u];
            if (b > n_cases || c > n_cases - b) { std::printf("task %u out of range\n", k); std::exit(3); }
            for (uint32_t i = b; i < b + c; i++) { if (seen[i]++) { std::printf("case %u in two tasks\n", i); std::exit(3); } }
        }
        for (uint32_t i = 0; i < n_cases; i++) if (!seen[i]) { std::printf("case %u in no task\n", i); std::exit(3); }
    }

    // ---- device copies ----
    float4* d_blob = nullptr;
    uint32_t *d_cases = nullptr, *d_out = nullptr;
    uint2* d_tasks = nullptr;
    const size_t out_bytes = 4ull * kOutWords * n_cases;
    CHECK(hipMalloc(&d_blob, host.blob.size()));
    CHECK(hipMemcpy(d_blob, host.blob.data(), host.blob.size(), hipMemcpyHostToDevice));
    CHECK(hipMalloc(&d_cases, 4ull * kCaseWords * n_cases));
    CHECK(hipMemcpy(d_cases, &cw[3], 4ull * kCaseWords * n_cases, hipMemcpyHostToDevice));
    CHECK(hipMalloc(&d_tasks, 8ull * n_tasks));
    CHECK(hipMemcpy(d_tasks, &cw[3u + (size_t)kCaseWords * n_cases], 8ull * n_tasks, hipMemcpyHostToDevice));
    CHECK(hipMalloc(&d_out, out_bytes));
    const SceneDev scd{d_blob, L};

    FILE* ft = std::fopen(out_txt, "w");
    if (!ft) { std::printf("cannot write %s\n", out_txt); std::exit(3); }
    std::fprintf(ft, "layout n_spheres=%u n_quads=%u n_materials=%u hot_bytes=%u lazy_color=%u\n", L.n_spheres, L.n_quads, L.n_materials, L.hot_bytes, L.lazy_color);
    std::vector<uint32_t> h((size_t)kOutWords * n_cases);
    constexpr int kVariants = 9;
    const char* names[kVariants] = {"lds_carried", "lds_lazy", "lds_stats", "global_carried", "global_lazy",
                                    "lds_info", "lds_info_hidden", "global_info", "global_info_hidden"};
    for (int v = 0; v < kVariants; v++) {
        CHECK(hipMemset(d_out, 0xCD, out_bytes));
        switch (v) {
            case 0: launch<MODE_LDS, false, false>(scd, d_cases, d_tasks, n_tasks, d_out); break;
            case 1: launch<MODE_LDS, false, true>(scd, d_cases, d_tasks, n_tasks, d_out); break;
            case 2: launch<MODE_LDS, true, false>(scd, d_cases, d_tasks, n_tasks, d_out); break;
            case 3: launch<MODE_GLOBAL, false, false>(scd, d_cases, d_tasks, n_tasks, d_out); break;
            case 4: launch<MODE_GLOBAL, false, true>(scd, d_cases, d_tasks, n_tasks, d_out); break;
            case 5: launch_info<MODE_LDS>(scd, d_cases, d_tasks, n_tasks, 0u, d_out); break;
            case 6: launch_info<MODE_LDS>(scd, d_cases, d_tasks, n_tasks, 1u, d_out); break;
            case 7: launch_info<MODE_GLOBAL>(scd, d_cases, d_tasks, n_tasks, 0u, d_out); break;
            default: launch_info<MODE_GLOBAL>(scd, d_cases, d_tasks, n_tasks, 1u, d_out); break;
        }
        CHECK(hipMemcpy(h.data(), d_out, out_bytes, hipMemcpyDeviceToHost));
        write_words(out_bin, h, v == 0 ? "wb" : "ab");
        std::fprintf(ft, "variant %s\n", names[v]);
    }
    std::fclose(ft);
    CHECK(hipFree(d_out));
    CHECK(hipFree(d_tasks));
    CHECK(hipFree(d_cases));
    CHECK(hipFree(d_blob));
    return (unsigned long long)kVariants * n_cases;
}

unsigned long long run_vectors(const char* in_path, const char* out_path) {
    const std::vector<uint32_t> vw = read_words(in_path);
    if (vw.size() < 2 || vw[0] != 0x31564853u || vw[1] == 0u || vw.size() != 2u + (size_t)kVecWords * vw[1]) { std::printf("bad vector file\n"); std::exit(3); }
    const uint32_t n = vw[1];
    uint32_t *d_in = nullptr, *d_out = nullptr;
    CHECK(hipMalloc(&d_in, 4ull * kVecWords * n));
    CHECK(hipMemcpy(d_in, &vw[2], 4ull * kVecWords * n, hipMemcpyHostToDevice));
    CHECK(hipMalloc(&d_out, 4ull * kVecOutWords * n));
    CHECK(hipMemset(d_out, 0xCD, 4ull * kVecOutWords * n));
    hipLaunchKernelGGL(vec_kernel, dim3((n + kThreads - 1u) / kThreads), dim3(kThreads), 0, 0, d_in, n, d_out);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    std::vector<uint32_t> h((size_t)kVecOutWords * n);
    CHECK(hipMemcpy(h.data(), d_out, 4ull * kVecOutWords * n, hipMemcpyDeviceToHost));
    write_words(out_path, h, "wb");
    CHECK(hipFree(d_out));
    CHECK(hipFree(d_in));
    return n;
}

}  // namespace

int main(int argc, char** argv) {
    unsigned long long answers = 0, vectors = 0;
    int scenes = 0, k = 1;
    while (k < argc) {
        if (std::strcmp(argv[k], "run") == 0 && k + 4 <= argc - 1) {
            answers += run_scene(argv[k + 1], argv[k + 2], argv[k + 3], argv[k + 4]);
            scenes++;
            k += 5;
        } else if (std::strcmp(argv[k], "vec") == 0 && k + 2 <= argc - 1) {
            vectors += run_vectors(argv[k + 1], argv[k + 2]);
            k += 3;
        } else {
            std::printf("usage: shade_cases [run scene.bin cases.bin out.bin out.txt]... [vec vec.bin out.bin]\n");
            return 3;
        }
    }
    if (scenes == 0 && vectors == 0) { std::printf("usage: shade_cases [run scene.bin cases.bin out.bin out.txt]... [vec vec.bin out.bin]\n"); return 3; }
    std::printf("shade_cases: %d scene runs, %llu case answers, %llu vectors\n", scenes, answers, vectors);
    return 0;
}
