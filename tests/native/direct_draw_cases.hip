// Test program (tests/test_gpu_direct_draws.py builds and runs it on the GPU box): the cases of tests/direct_draw_cases.py through the
// product's rng_seed (rt_device.h) and direct_draw / direct_draw_at (gather_draw.h), one case per lane.  There is no sampling code in this
// file: the kernel seeds stream (seed_key, j + shift, word), calls the forwarder of the case's form and writes back the thirteen words of
// the sample and of the generator afterwards for the Python side to compare with the oracle, bit for bit.
//
//   direct_draw_cases <cases.bin> [<shift> <out.bin>]...
//
// cases.bin: u32 'DDC1', n_cases, n_tasks, n_tables, seed_key; n_cases x 11 words: form (0 item: direct_draw, the surfel loaded from an
//            items array; 1 vertex: direct_draw_at, the surfel in registers), table, stream j, sample word, bits(shadow_end), x[3], n[3];
//            n_tasks x (begin, count): the case list of one wave (the tasks partition the cases); n_tables x (E, P, P x 20 words): a table
//            of E records (tinyrt.h trt_emitter) whose record e is records[e mod P].  The tables are expanded here, on the host, into one
//            device buffer.  Form, table, word and shadow_end are per LANE here (in the product they are per launch): the lanes of a wave
//            mix quads and spheres, live and dead samples and both forms.
// out.bin:   n_cases x 13 words - ray origin[3], direction[3], c[3], t_max, live (0 / 1), s0, s1 - of a run with `shift` added to every
//            stream (mod 2^32).
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
constexpr uint32_t kCaseWords = 11, kOutWords = 13, kRecordWords = 20, kMaxPeriod = 64, kMaxEmitters = 1u << 20;

__global__ __launch_bounds__(kThreads) void draw_kernel(const uint32_t* __restrict__ cases, const float* __restrict__ items, const uint2* __restrict__ tasks,
                                                        uint32_t n_tasks, const float* __restrict__ records, const uint2* __restrict__ tables,
                                                        uint32_t seed_key, uint32_t shift, uint32_t* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u, wave = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (wave >= n_tasks) return;
    const uint2 task = tasks[wave];
    for (uint32_t base = 0; base < task.y; base += 64u) {
        if (base + lane >= task.y) continue;
        const uint32_t idx = task.x + base + lane;
        const uint32_t* c = cases + (size_t)kCaseWords * idx;
        const uint2 table = tables[c[1]];                                   // (first record in `records`, E)
        const float* emitters = records + (size_t)kRecordWords * table.x;
        const float shadow_end = __uint_as_float(c[4]);
        Rng g = rng_seed(seed_key, c[2] + shift, c[3]);
        DirectSample s;
        if (c[0] == 0u) {
            s = direct_draw(items, idx, emitters, table.y, shadow_end, g);
        } else {
            const V3 x = v3(__uint_as_float(c[5]), __uint_as_float(c[6]), __uint_as_float(c[7]));
            const V3 n = v3(__uint_as_float(c[8]), __uint_as_float(c[9]), __uint_as_float(c[10]));
            s = direct_draw_at(x, n, emitters, table.y, shadow_end, g);
        }
        uint32_t* o = out + (size_t)kOutWords * idx;
        o[0] = __float_as_uint(s.ray.o.x); o[1] = __float_as_uint(s.ray.o.y); o[2] = __float_as_uint(s.ray.o.z);
        o[3] = __float_as_uint(s.ray.d.x); o[4] = __float_as_uint(s.ray.d.y); o[5] = __float_as_uint(s.ray.d.z);
        o[6] = __float_as_uint(s.c.x); o[7] = __float_as_uint(s.c.y); o[8] = __float_as_uint(s.c.z);
        o[9] = __float_as_uint(s.t_max);
        o[10] = s.live ? 1u : 0u;
        o[11] = g.s0; o[12] = g.s1;
    }
}

int main(int argc, char** argv) {
    if (argc < 4 || (argc - 2) % 2 != 0) { std::printf("usage: direct_draw_cases cases.bin [shift out.bin]...\n"); return 3; }
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
    if (cw.size() < 5 || cw[0] != 0x31434444u) { std::printf("bad case file\n"); return 3; }
    const uint32_t n_cases = cw[1], n_tasks = cw[2], n_tables = cw[3], seed_key = cw[4];
    if (n_cases == 0 || n_tasks == 0 || n_tables == 0) { std::printf("no cases\n"); return 3; }
    const size_t tables_at = 5u + (size_t)kCaseWords * n_cases + 2ull * n_tasks;
    if (cw.size() < tables_at) { std::printf("bad case file\n"); return 3; }
    // ---- the tables: every (E, P) in range and every record inside the file; expanded into one buffer ----
    std::vector<uint2> tables(n_tables);
    std::vector<size_t> period_at(n_tables);
    std::vector<uint32_t> period(n_tables);
    size_t at = tables_at, n_records = 0;
    for (uint32_t k = 0; k < n_tables; k++) {
        if (cw.size() < at + 2u) { std::printf("table %u: file ends\n", k); return 3; }
        const uint32_t E = cw[at], P = cw[at + 1u];
        if (E == 0 || E > kMaxEmitters || P == 0 || P > kMaxPeriod || P > E) { std::printf("table %u: E %u, P %u\n", k, E, P); return 3; }
        if (cw.size() < at + 2u + (size_t)kRecordWords * P) { std::printf("table %u: file ends\n", k); return 3; }
        tables[k] = make_uint2((uint32_t)n_records, E);
        period_at[k] = at + 2u;
        period[k] = P;
        n_records += E;
        at += 2u + (size_t)kRecordWords * P;
    }
    if (at != cw.size() || n_records > 0xFFFFFFFFull / kRecordWords) { std::printf("bad case file\n"); return 3; }
    std::vector<uint32_t> records((size_t)kRecordWords * n_records);
    for (uint32_t k = 0; k < n_tables; k++)
        for (uint32_t e = 0; e < tables[k].y; e++)
            std::memcpy(&records[(size_t)kRecordWords * (tables[k].x + e)], &cw[period_at[k] + (size_t)kRecordWords * (e % period[k])], 4u * kRecordWords);
    // ---- every form and table known, the tasks a partition of the cases: no lane reads or writes outside its record or its table ----
    std::vector<float> items(6ull * n_cases);
    for (uint32_t i = 0; i < n_cases; i++) {
        const uint32_t* c = &cw[5u + (size_t)kCaseWords * i];
        if (c[0] > 1u || c[1] >= n_tables) { std::printf("case %u: form %u, table %u\n", i, c[0], c[1]); return 3; }
        std::memcpy(&items[6ull * i], c + 5, 24);
    }
    const uint32_t* t = &cw[5u + (size_t)kCaseWords * n_cases];
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
    float *d_items = nullptr, *d_records = nullptr;
    uint2 *d_tasks = nullptr, *d_tables = nullptr;
    const size_t out_bytes = 4ull * kOutWords * n_cases;
    CHECK(hipMalloc(&d_cases, 4ull * kCaseWords * n_cases));
    CHECK(hipMemcpy(d_cases, &cw[5], 4ull * kCaseWords * n_cases, hipMemcpyHostToDevice));
    CHECK(hipMalloc(&d_items, 24ull * n_cases));
    CHECK(hipMemcpy(d_items, items.data(), 24ull * n_cases, hipMemcpyHostToDevice));
    CHECK(hipMalloc(&d_tasks, 8ull * n_tasks));
    CHECK(hipMemcpy(d_tasks, t, 8ull * n_tasks, hipMemcpyHostToDevice));
    CHECK(hipMalloc(&d_records, 4ull * records.size()));
    CHECK(hipMemcpy(d_records, records.data(), 4ull * records.size(), hipMemcpyHostToDevice));
    CHECK(hipMalloc(&d_tables, 8ull * n_tables));
    CHECK(hipMemcpy(d_tables, tables.data(), 8ull * n_tables, hipMemcpyHostToDevice));
    CHECK(hipMalloc(&d_out, out_bytes));
    std::vector<uint32_t> h((size_t)kOutWords * n_cases);
    int runs = 0;
    for (int k = 2; k + 1 < argc; k += 2, runs++) {
        const uint32_t shift = (uint32_t)std::strtoul(argv[k], nullptr, 10);
        CHECK(hipMemset(d_out, 0xCD, out_bytes));
        hipLaunchKernelGGL(draw_kernel, dim3((n_tasks + 3u) / 4u), dim3(kThreads), 0, 0, d_cases, d_items, d_tasks, n_tasks, d_records, d_tables, seed_key, shift, d_out);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        CHECK(hipMemcpy(h.data(), d_out, out_bytes, hipMemcpyDeviceToHost));
        FILE* f = std::fopen(argv[k + 1], "wb");
        if (!f || std::fwrite(h.data(), 4, h.size(), f) != h.size()) { std::printf("cannot write %s\n", argv[k + 1]); return 3; }
        std::fclose(f);
    }
    CHECK(hipFree(d_out));
    CHECK(hipFree(d_tables));
    CHECK(hipFree(d_records));
    CHECK(hipFree(d_tasks));
    CHECK(hipFree(d_items));
    CHECK(hipFree(d_cases));
    std::printf("direct_draw_cases: %u cases, %u wave lists, %u tables of %zu records, %d runs\n", n_cases, n_tasks, n_tables, n_records, runs);
    return 0;
}
