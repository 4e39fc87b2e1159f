// Test program (tests/test_gpu_draws.py builds and runs it on the GPU box): the draw cases of tests/draw_cases.py through the product's
// rng_seed (rt_device.h) and gather_ray / probe_ray (gather_draw.h), one case per lane.  There is no sampling code in this file: the
// kernel seeds stream (seed_key, j + shift, 1), calls the draw of the case's kind and writes back the six words of the ray and the two of
// the generator afterwards for the Python side to compare with the oracle, bit for bit.
//
//   draw_cases <cases.bin> [<shift> <out.bin>]...
//
// cases.bin: u32 'DRC1', n_cases, n_tasks, seed_key; n_cases x 9 words: kind (0 cosine, 1 cone: gather_ray; 2 sphere, 3 hemisphere:
//            probe_ray), bits(spread), stream j, item[6] (point, axis); n_tasks x (begin, count): the case list of one wave.  The tasks
//            partition the cases.  The kind is per LANE here (in the product it is per launch): the lanes of a wave mix lobes and domains.
// out.bin:   n_cases x 8 words - ray origin[3], direction[3], s0, s1 - of a run with `shift` added to every stream (mod 2^32).
// Exit status 0 on success; any HIP error ends the program with status 2, a bad input with 3; nothing is retried.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gather_draw.h"

using namespace trt;

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("%s: %s\n", #x, hipGetErrorString(e_)); std::exit(2); } } while (0)

constexpr int kThreads = 256;                 // four waves per workgroup, as the production pool kernels
constexpr uint32_t kCaseWords = 9, kOutWords = 8;

__global__ __launch_bounds__(kThreads) void draw_kernel(const uint32_t* __restrict__ cases, const float* __restrict__ items, const uint2* __restrict__ tasks,
                                                        uint32_t n_tasks, uint32_t seed_key, uint32_t shift, uint32_t* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u, wave = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (wave >= n_tasks) return;
    const uint2 task = tasks[wave];
    for (uint32_t base = 0; base < task.y; base += 64u) {
        if (base + lane >= task.y) continue;
        const uint32_t idx = task.x + base + lane;
        const uint32_t* c = cases + (size_t)kCaseWords * idx;
        const uint32_t kind = c[0];
        Rng g = rng_seed(seed_key, c[2] + shift, 1u);
        Ray r;
        if (kind < 2u) r = gather_ray(items, idx, kind == 0u ? (uint32_t)TRT_LOBE_COSINE : (uint32_t)TRT_LOBE_CONE, __uint_as_float(c[1]), g);
        else r = probe_ray(items, idx, kind == 3u, g);
        uint32_t* o = out + (size_t)kOutWords * idx;
        o[0] = __float_as_uint(r.o.x); o[1] = __float_as_uint(r.o.y); o[2] = __float_as_uint(r.o.z);
        o[3] = __float_as_uint(r.d.x); o[4] = __float_as_uint(r.d.y); o[5] = __float_as_uint(r.d.z);
        o[6] = g.s0; o[7] = g.s1;
    }
}

int main(int argc, char** argv) {
    if (argc < 4 || (argc - 2) % 2 != 0) { std::printf("usage: draw_cases cases.bin [shift out.bin]...\n"); return 3; }
    std::vector<uint32_t> cw;
    {
        FILE* f = std::fopen(argv[1], "rb");
        if (!f) { std::printf("cannot open %s\n", argv[1]); return 3; }
        std::fseek(f, 0, SEEK_END);
        const long n = std::ftell(f);
        std::fseek(f, 0, SEEK_SET);
        cw.resize((size_t)n / 4u);
        if (n > 0 && std::fread(cw.data(), 4, cw.size(), f) != cw.size()) { std::printf("short read of %s\n", argv[1]); return 3; }
        std::fclose(f);
    }
    if (cw.size() < 4 || cw[0] != 0x31435244u || cw.size() != 4u + (size_t)kCaseWords * cw[1] + 2ull * cw[2]) { std::printf("bad case file\n"); return 3; }
    const uint32_t n_cases = cw[1], n_tasks = cw[2], seed_key = cw[3];
    if (n_cases == 0 || n_tasks == 0) { std::printf("no cases\n"); return 3; }
    // ---- every kind known, the tasks a partition of the cases: no lane reads or writes outside its record ----
    std::vector<float> items(6ull * n_cases);
    for (uint32_t i = 0; i < n_cases; i++) {
        const uint32_t* c = &cw[4u + (size_t)kCaseWords * i];
        if (c[0] > 3u) { std::printf("case %u: kind %u\n", i, c[0]); return 3; }
        std::memcpy(&items[6ull * i], c + 3, 24);
    }
    const uint32_t* t = &cw[4u + (size_t)kCaseWords * n_cases];
    {
        std::vector<uint8_t> seen(n_cases, 0);
        for (uint32_t k = 0; k < n_tasks; k++) {
            const uint32_t b = t[2u * k], c = t[2u * k + 1u];
            if (b > n_cases || c > n_cases - b) { std::printf("task %u out of range\n", k); return 3; }
            for (uint32_t i = b; i < b + c; i++) { if (seen[i]++) { std::printf("case %u in two tasks\n", i); return 3; } }
        }
        for (uint32_t i = 0; i < n_cases; i++) if (!seen[i]) { std::printf("case %u in no task\n", i); return 3; }
    }

    uint32_t *d_cases = nullptr, *d_out = nullptr;
    float* d_items = nullptr;
    uint2* d_tasks = nullptr;
    const size_t out_bytes = 4ull * kOutWords * n_cases;
    CHECK(hipMalloc(&d_cases, 4ull * kCaseWords * n_cases));
    CHECK(hipMemcpy(d_cases, &cw[4], 4ull * kCaseWords * n_cases, hipMemcpyHostToDevice));
    CHECK(hipMalloc(&d_items, 24ull * n_cases));
    CHECK(hipMemcpy(d_items, items.data(), 24ull * n_cases, hipMemcpyHostToDevice));
    CHECK(hipMalloc(&d_tasks, 8ull * n_tasks));
    CHECK(hipMemcpy(d_tasks, t, 8ull * n_tasks, hipMemcpyHostToDevice));
    CHECK(hipMalloc(&d_out, out_bytes));
    std::vector<uint32_t> h((size_t)kOutWords * n_cases);
    int runs = 0;
    for (int k = 2; k + 1 < argc; k += 2, runs++) {
        const uint32_t shift = (uint32_t)std::strtoul(argv[k], nullptr, 10);
        CHECK(hipMemset(d_out, 0xCD, out_bytes));
        hipLaunchKernelGGL(draw_kernel, dim3((n_tasks + 3u) / 4u), dim3(kThreads), 0, 0, d_cases, d_items, d_tasks, n_tasks, seed_key, shift, d_out);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        CHECK(hipMemcpy(h.data(), d_out, out_bytes, hipMemcpyDeviceToHost));
        FILE* f = std::fopen(argv[k + 1], "wb");
        if (!f || std::fwrite(h.data(), 4, h.size(), f) != h.size()) { std::printf("cannot write %s\n", argv[k + 1]); return 3; }
        std::fclose(f);
    }
    CHECK(hipFree(d_out));
    CHECK(hipFree(d_tasks));
    CHECK(hipFree(d_items));
    CHECK(hipFree(d_cases));
    std::printf("draw_cases: %u cases, %u wave lists, %d runs\n", n_cases, n_tasks, runs);
    return 0;
}
