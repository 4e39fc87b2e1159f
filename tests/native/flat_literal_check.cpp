// flat_literal_check.cpp - the generator of the per-scene box phase (tiny-raytracer_amd/csrc/flat_literal.h) on the CPU.  Stand-alone:
//   flat_literal_check <leaf file> <n_leaves> <reuse 0|1>   prints "masks x y z", then the asm text; exit 2 if the list is refused
//   flat_literal_check --self                                built-in lists: determinism, refusals, literals; exit 1 on the first failure
// Build: g++ -std=c++17 -I tiny-raytracer_amd/csrc tests/native/flat_literal_check.cpp [-fsanitize=address,undefined]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "flat_literal.h"

static int g_failed = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); g_failed = 1; } } while (0)

static size_t count(const std::string& s, const std::string& what) {
    size_t n = 0;
    for (size_t p = s.find(what); p != std::string::npos; p = s.find(what, p + 1)) n++;
    return n;
}
static std::string hex(uint32_t v) { char b[16]; snprintf(b, sizeof b, "0x%08x", v); return b; }

// k leaves; leaf i's planes are base + i on every axis unless `same`, then all leaves are one box
static std::vector<uint32_t> make(uint32_t k, bool same) {
    std::vector<uint32_t> w(8u * k);
    for (uint32_t i = 0; i < k; i++) {
        for (uint32_t j = 0; j < 6; j++) { const float f = (float)(j + 1u) + (same ? 0.0f : 16.0f * (float)i); memcpy(&w[8u * i + j], &f, 4); }
        w[8u * i + 6] = i + 1u;
        w[8u * i + 7] = 0x40000000u | (i * 3u + 1u);
    }
    return w;
}

static int self() {
    uint32_t zero[3] = {0, 0, 0};
    std::string a, b;
    for (uint32_t k : {1u, 2u, 3u, 18u, 32u}) {
        for (bool same : {false, true}) {
            const std::vector<uint32_t> w = make(k, same);
            uint32_t m[3];
            trt::flat_reuse_masks(w.data(), k, true, m);
            CHECK(trt::flat_literal_asm(w.data(), k, m, a));
            CHECK(trt::flat_literal_asm(w.data(), k, m, b));
            CHECK(a == b);                                                      // deterministic
            uint32_t reused = 0, fresh = 0;
            for (uint32_t i = 1; i < k; i++) {
                const uint32_t r = ((m[0] >> i) & 1u) + ((m[1] >> i) & 1u) + ((m[2] >> i) & 1u);
                reused += r;
                if (!(i & 1u) && r) fresh++;
            }
            CHECK(reused == (same ? 3u * (k - 1u) : 0u));
            // every computed axis is two subtractions; every box (main stream and fresh copies) one push
            CHECK(count(a, "v_sub_f32_e32") == 2u * (3u * k - reused + 3u * fresh));
            CHECK(count(a, "ds_write2_b32") == k + fresh);
            CHECK(count(a, "s_getpc_b64") == 1u);
            for (uint32_t i = 0; i < k; i++) CHECK(a.find("v_mov_b32_e32 %[lk], " + hex(w[8u * i + 7])) != std::string::npos);
            if (!same) for (uint32_t i = 0; i < k; i++) for (uint32_t j = 0; j < 6; j++) CHECK(a.find(hex(w[8u * i + j]) + ",") != std::string::npos);
            CHECK(a.find('.') == std::string::npos);                            // no decimal text anywhere
        }
    }
    const std::vector<uint32_t> big = make(33u, false);
    a = "untouched";
    CHECK(!trt::flat_literal_asm(big.data(), 33u, zero, a));
    CHECK(!trt::flat_literal_asm(big.data(), 0u, zero, a));
    CHECK(!trt::flat_literal_asm(nullptr, 4u, zero, a));
    CHECK(a == "untouched");
    // signed zeros, inf and NaN planes keep their bits
    std::vector<uint32_t> odd = make(4u, true);
    odd[0] = 0x80000000u; odd[8] = 0x00000000u; odd[16 + 1] = 0x7f800000u; odd[24 + 2] = 0x7fc12345u;
    uint32_t m[3];
    trt::flat_reuse_masks(odd.data(), 4u, true, m);
    CHECK((m[0] & 2u) == 0u);                                                   // -0 then +0 on x: not reused
    CHECK(trt::flat_literal_asm(odd.data(), 4u, m, a));
    for (uint32_t v : {0x80000000u, 0x00000000u, 0x7f800000u, 0x7fc12345u}) CHECK(a.find("v_sub_f32_e32 %[t0], " + hex(v) + ",") != std::string::npos);
    CHECK(trt::flat_literal_define("X", "a\nb\n") == "#define X \\\n\"a\\n\" \\\n\"b\\n\" \\\n\"\"\n");
    printf(g_failed ? "self check FAILED\n" : "self check ok\n");
    return g_failed;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--self")) return self();
    if (argc != 4) { fprintf(stderr, "usage: %s <leaf file> <n_leaves> <reuse 0|1> | --self\n", argv[0]); return 64; }
    std::vector<unsigned char> bytes;
    if (FILE* f = fopen(argv[1], "rb")) { int c; while ((c = fgetc(f)) != EOF) bytes.push_back((unsigned char)c); fclose(f); }
    const uint32_t n = (uint32_t)strtoul(argv[2], nullptr, 10);
    if (bytes.size() < 32u * (size_t)n) { fprintf(stderr, "file shorter than the list\n"); return 64; }
    uint32_t m[3];
    trt::flat_reuse_masks(bytes.empty() ? nullptr : bytes.data(), n, atoi(argv[3]) != 0, m);
    std::string text;
    if (!trt::flat_literal_asm(bytes.empty() ? nullptr : bytes.data(), n, m, text)) { printf("refused\n"); return 2; }
    printf("masks %u %u %u\n%s", m[0], m[1], m[2], text.c_str());
    return 0;
}
