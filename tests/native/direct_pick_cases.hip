// Test program (tests/test_gpu_direct_pick_draws.py builds and runs it on the GPU box): the alias draw of trt_direct_pick /
// trt_direct_mis_pick, one case per lane, through the product's rng_seed (rt_device.h) and direct_draw_item<true, WeightedDirectSample>
// (gather_draw.h: direct_draw_from with the AliasPick policy, the forwarder both PICK kernels call).  There is no sampling code in this
// file: the kernel seeds stream (seed_key, j, 1), calls the forwarder on the case's own tables and writes back the words of the sample and
// of the generator afterwards for the Python side to compare with tests/direct_pick_cases.py, bit for bit.
//
//   direct_pick_cases <cases.bin> <out.bin>
//
// cases.bin: u32 'DPC1', n_cases, n_tables, seed; n_cases x 9 words: table, stream j, bits(shadow_end), x[3], n[3]; then per table: E,
//            E x 20 words of emitter records (tinyrt.h trt_emitter), E x 4 words of pick records (trt_emitter_pick).  The table is per
//            LANE here (in the product it is per launch): the lanes of a wave mix tables, quads and spheres, kept slots and aliases, live
//            and dead samples.  Case i is lane i mod 64 of wave i / 64; the list's length need be no multiple of 64.
// out.bin:   n_cases x 15 words - ray origin[3], direction[3], c[3], t_max, live (0 / 1), wgt, geometry, s0, s1.
// Exit status 0 on success; any HIP error ends the program with status 2, a bad input with 3; nothing is retried.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gather_draw.h"

using namespace trt;

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("%s: %s\n", #x, hipGetErrorString(e_)); std::exit(2); } } while (0)

constexpr int kThreads = 256;
constexpr uint32_t kCaseWords = 9, kOutWords = 15, kRecordWords = 20, kPickWords = 4, kMaxEmitters = 1u << 20;

__global__ __launch_bounds__(kThreads) void pick_kernel(const uint32_t* __restrict__ cases, const float* __restrict__ items, uint32_t n_cases,
                                                        const float* __restrict__ records, const float* __restrict__ picks,
                                                        const uint2* __restrict__ tables, uint32_t seed_key, uint32_t* __restrict__ out) {
    const uint32_t idx = blockIdx.x * kThreads + threadIdx.x;
    if (idx >= n_cases) return;
    const uint32_t* c = cases + (size_t)kCaseWords * idx;
    const uint2 table = tables[c[0]];                                       // (first record, E)
    const float* emitters = records + (size_t)kRecordWords * table.x;
    const float* pick = picks + (size_t)kPickWords * table.x;
    Rng g = rng_seed(seed_key, c[1], 1u);
    const WeightedDirectSample s = direct_draw_item<true, WeightedDirectSample>(items, idx, emitters, pick, table.y, __uint_as_float(c[2]), g);
    uint32_t* o = out + (size_t)kOutWords * idx;
    o[0] = __float_as_uint(s.ray.o.x); o[1] = __float_as_uint(s.ray.o.y); o[2] = __float_as_uint(s.ray.o.z);
    o[3] = __float_as_uint(s.ray.d.x); o[4] = __float_as_uint(s.ray.d.y); o[5] = __float_as_uint(s.ray.d.z);
    o[6] = __float_as_uint(s.c.x); o[7] = __float_as_uint(s.c.y); o[8] = __float_as_uint(s.c.z);
    o[9] = __float_as_uint(s.t_max);
    o[10] = s.live ? 1u : 0u;
    o[11] = __float_as_uint(s.wgt);
    o[12] = s.geometry;
    o[13] = g.s0; o[14] = g.s1;
}

int main(int argc, char** argv) {
    if (argc != 3) { std::printf("usage: direct_pick_cases cases.bin out.bin\n"); return 3; }
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
    if (cw.size() < 4 || cw[0] != 0x31435044u) { std::printf("bad case file\n"); return 3; }
    const uint32_t n_cases = cw[1], n_tables = cw[2], seed = cw[3];
    if (n_cases == 0 || n_tables == 0 || n_cases > (1u << 24)) { std::printf("no cases\n"); return 3; }
    size_t at = 4u + (size_t)kCaseWords * n_cases;
    if (cw.size() < at) { std::printf("bad case file\n"); return 3; }
    // ---- the tables: every E in range and every record inside the file; gathered into one buffer each ----
    std::vector<uint2> tables(n_tables);
    std::vector<uint32_t> records, picks;
    size_t n_records = 0;
    for (uint32_t k = 0; k < n_tables; k++) {
        if (cw.size() < at + 1u) { std::printf("table %u: file ends\n", k); return 3; }
        const uint32_t E = cw[at];
        if (E == 0 || E > kMaxEmitters) { std::printf("table %u: E %u\n", k, E); return 3; }
        if (cw.size() < at + 1u + (size_t)(kRecordWords + kPickWords) * E) { std::printf("table %u: file ends\n", k); return 3; }
        tables[k] = make_uint2((uint32_t)n_records, E);
        records.insert(records.end(), cw.begin() + at + 1u, cw.begin() + at + 1u + (size_t)kRecordWords * E);
        picks.insert(picks.end(), cw.begin() + at + 1u + (size_t)kRecordWords * E, cw.begin() + at + 1u + (size_t)(kRecordWords + kPickWords) * E);
        n_records += E;
        at += 1u + (size_t)(kRecordWords + kPickWords) * E;
    }
    if (at != cw.size() || n_records > 0xFFFFFFFFull / kRecordWords) { std::printf("bad case file\n"); return 3; }
    // ---- every case names a table that exists: no lane reads outside its tables (the draw clamps slot and alias to E - 1) ----
    std::vector<float> items(6ull * n_cases);
    for (uint32_t i = 0; i < n_cases; i++) {
        const uint32_t* c = &cw[4u + (size_t)kCaseWords * i];
        if (c[0] >= n_tables) { std::printf("case %u: table %u\n", i, c[0]); return 3; }
        std::memcpy(&items[6ull * i], c + 3, 24);
    }

    uint32_t *d_cases = nullptr, *d_out = nullptr;
    float *d_items = nullptr, *d_records = nullptr, *d_picks = nullptr;
    uint2* d_tables = nullptr;
    const size_t out_bytes = 4ull * kOutWords * n_cases;
    CHECK(hipMalloc(&d_cases, 4ull * kCaseWords * n_cases));
    CHECK(hipMemcpy(d_cases, &cw[4], 4ull * kCaseWords * n_cases, hipMemcpyHostToDevice));
    CHECK(hipMalloc(&d_items, 24ull * n_cases));
    CHECK(hipMemcpy(d_items, items.data(), 24ull * n_cases, hipMemcpyHostToDevice));
    CHECK(hipMalloc(&d_records, 4ull * records.size()));
    CHECK(hipMemcpy(d_records, records.data(), 4ull * records.size(), hipMemcpyHostToDevice));
    CHECK(hipMalloc(&d_picks, 4ull * picks.size()));
    CHECK(hipMemcpy(d_picks, picks.data(), 4ull * picks.size(), hipMemcpyHostToDevice));
    CHECK(hipMalloc(&d_tables, 8ull * n_tables));
    CHECK(hipMemcpy(d_tables, tables.data(), 8ull * n_tables, hipMemcpyHostToDevice));
    CHECK(hipMalloc(&d_out, out_bytes));
    CHECK(hipMemset(d_out, 0xCD, out_bytes));
    hipLaunchKernelGGL(pick_kernel, dim3((n_cases + kThreads - 1u) / kThreads), dim3(kThreads), 0, 0, d_cases, d_items, n_cases, d_records, d_picks,
                       d_tables, rng_seed_key(seed), d_out);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    std::vector<uint32_t> h((size_t)kOutWords * n_cases);
    CHECK(hipMemcpy(h.data(), d_out, out_bytes, hipMemcpyDeviceToHost));
    FILE* f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(h.data(), 4, h.size(), f) != h.size()) { std::printf("cannot write %s\n", argv[2]); return 3; }
    std::fclose(f);
    CHECK(hipFree(d_out));
    CHECK(hipFree(d_tables));
    CHECK(hipFree(d_picks));
    CHECK(hipFree(d_records));
    CHECK(hipFree(d_items));
    CHECK(hipFree(d_cases));
    std::printf("direct_pick_cases: %u cases, %u tables of %zu records\n", n_cases, n_tables, n_records);
    return 0;
}
