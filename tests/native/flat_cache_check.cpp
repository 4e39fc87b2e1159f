// flat_cache_check.cpp - the interval cache of the per-scene box phase (tiny-raytracer_amd/csrc/flat_literal.h flat_literal_cached_asm) on
// the CPU.  Stand-alone:
//   flat_cache_check <leaf file> <n_leaves> <reuse 0|1> <pairs> <planes>
//       prints "masks x y z", "stats intervals plane_distances evictions far_reuses extra_operands cached", then the asm text;
//       exit 2 if the list or the setting is refused
//   flat_cache_check --self    built-in lists over every setting: determinism, refusals, the two identical-text cases, counts that can only
//                              fall with more registers; exit 1 on the first failure
// Build: g++ -std=c++17 -I tiny-raytracer_amd/csrc tests/native/flat_cache_check.cpp [-fsanitize=address,undefined]
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

// k leaves whose planes on each axis cycle through `period` boxes (period 0: all different)
static std::vector<uint32_t> make(uint32_t k, uint32_t period) {
    std::vector<uint32_t> w(8u * k);
    for (uint32_t i = 0; i < k; i++) {
        for (uint32_t j = 0; j < 6; j++) {
            const uint32_t phase = period ? (i * (j % 3u + 1u)) % period : i;
            const float f = (float)(j + 1u) + 16.0f * (float)phase;
            memcpy(&w[8u * i + j], &f, 4);
        }
        w[8u * i + 6] = i + 1u;
        w[8u * i + 7] = 0x40000000u | (i * 3u + 1u);
    }
    return w;
}

static int self() {
    std::string plain, a, b;
    for (uint32_t k : {1u, 2u, 3u, 7u, 18u, 32u}) {
        for (uint32_t period : {0u, 1u, 2u, 5u, 11u}) {
            const std::vector<uint32_t> w = make(k, period);
            uint32_t m[3];
            trt::flat_reuse_masks(w.data(), k, true, m);
            CHECK(trt::flat_literal_asm(w.data(), k, m, plain));
            uint32_t plain_intervals = 3u * k;
            for (uint32_t i = 1; i < k; i++) plain_intervals -= ((m[0] >> i) & 1u) + ((m[1] >> i) & 1u) + ((m[2] >> i) & 1u);
            for (uint32_t planes = 0; planes <= trt::kFlatCacheMaxPlanes; planes++) {
                uint32_t last_intervals = 0xffffffffu;
                for (uint32_t pairs = 3; pairs <= trt::kFlatCacheMaxPairs; pairs++) {
                    trt::FlatCacheStats sa, sb;
                    CHECK(trt::flat_literal_cached_asm(w.data(), k, m, pairs, planes, a, sa));
                    CHECK(trt::flat_literal_cached_asm(w.data(), k, m, pairs, planes, b, sb));
                    CHECK(a == b && sa.intervals == sb.intervals && sa.plane_distances == sb.plane_distances);      // deterministic
                    CHECK(sa.intervals <= plain_intervals && sa.intervals <= last_intervals);
                    CHECK(sa.plane_distances <= 2u * sa.intervals);
                    last_intervals = sa.intervals;
                    if (pairs == 3u && planes == 0u) CHECK(!sa.cached && a == plain && sa.extra_operands == 0u);
                    if (!sa.cached) {
                        CHECK(a == plain && sa.extra_operands == 0u && sa.intervals == plain_intervals);
                        continue;
                    }
                    CHECK(sa.intervals < plain_intervals || sa.plane_distances < 2u * plain_intervals);
                    CHECK(sa.extra_operands == 2u * (pairs - 3u) + planes);
                    // the old text whole behind label 1000, the cached stream in front: one push per leaf, two instructions per plane distance
                    const size_t at = a.find("1000:\n");
                    CHECK(at != std::string::npos && a.substr(at + 6u) == plain);
                    const std::string head = a.substr(0, at);
                    CHECK(count(head, "ds_write2_b32") == k);
                    CHECK(count(head, "v_sub_f32_e32") == sa.plane_distances && count(head, "v_mul_f32_e32") == sa.plane_distances);
                    CHECK(count(head, "v_med3_f32") + count(head, "v_min_f32_e32") + count(head, "v_max_f32_e32") == 2u * sa.intervals);
                    CHECK(a.find('.') == std::string::npos);
                    for (uint32_t j = sa.extra_operands; j <= trt::kFlatCacheMaxExtra; j++) CHECK(a.find("%[c" + std::to_string(j) + "]") == std::string::npos);
                }
            }
        }
    }
    // refusals leave the output alone
    const std::vector<uint32_t> big = make(33u, 0u);
    uint32_t zero[3] = {0, 0, 0};
    trt::FlatCacheStats st;
    a = "untouched";
    CHECK(!trt::flat_literal_cached_asm(big.data(), 33u, zero, 4u, 0u, a, st));
    CHECK(!trt::flat_literal_cached_asm(big.data(), 0u, zero, 4u, 0u, a, st));
    CHECK(!trt::flat_literal_cached_asm(nullptr, 4u, zero, 4u, 0u, a, st));
    CHECK(!trt::flat_literal_cached_asm(big.data(), 4u, zero, 2u, 0u, a, st));
    CHECK(!trt::flat_literal_cached_asm(big.data(), 4u, zero, 9u, 0u, a, st));
    CHECK(!trt::flat_literal_cached_asm(big.data(), 4u, zero, 4u, 9u, a, st));
    CHECK(a == "untouched");
    // all leaves different: nothing to cache, the text is flat_literal_asm's at every setting
    CHECK(trt::flat_literal_asm(big.data(), 32u, zero, plain));
    CHECK(trt::flat_literal_cached_asm(big.data(), 32u, zero, 8u, 8u, a, st) && a == plain && !st.cached && st.intervals == 96u && st.plane_distances == 192u);
    // -0 / +0 never merge, inf and NaN planes are never shared: A, B, A on every axis, where B differs from A in the sign of a zero
    std::vector<uint32_t> odd = make(3u, 1u);
    odd[0] = odd[16] = 0x80000000u; odd[8] = 0x00000000u;
    CHECK(trt::flat_literal_cached_asm(odd.data(), 3u, zero, 8u, 0u, a, st) && st.cached && st.intervals == 4u && st.far_reuses == 5u);
    odd[1] = odd[8 + 1] = odd[16 + 1] = 0x7f800000u;                            // an inf plane on y: computed three times
    odd[2] = odd[8 + 2] = odd[16 + 2] = 0x7fc12345u;                            // a NaN plane on z: computed three times
    CHECK(trt::flat_literal_cached_asm(odd.data(), 3u, zero, 8u, 8u, a, st) && st.cached && st.intervals == 8u);
    CHECK(count(a.substr(0, a.find("1000:\n")), "0x7f800000,") == 3u && count(a.substr(0, a.find("1000:\n")), "0x7fc12345,") == 3u);
    printf(g_failed ? "self check FAILED\n" : "self check ok\n");
    return g_failed;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--self")) return self();
    if (argc != 6) { fprintf(stderr, "usage: %s <leaf file> <n_leaves> <reuse 0|1> <pairs> <planes> | --self\n", argv[0]); return 64; }
    std::vector<unsigned char> bytes;
    if (FILE* f = fopen(argv[1], "rb")) { int c; while ((c = fgetc(f)) != EOF) bytes.push_back((unsigned char)c); fclose(f); }
    const uint32_t n = (uint32_t)strtoul(argv[2], nullptr, 10);
    if (bytes.size() < 32u * (size_t)n) { fprintf(stderr, "file shorter than the list\n"); return 64; }
    uint32_t m[3];
    trt::flat_reuse_masks(bytes.empty() ? nullptr : bytes.data(), n, atoi(argv[3]) != 0, m);
    std::string text;
    trt::FlatCacheStats st;
    if (!trt::flat_literal_cached_asm(bytes.empty() ? nullptr : bytes.data(), n, m, (uint32_t)strtoul(argv[4], nullptr, 10), (uint32_t)strtoul(argv[5], nullptr, 10), text, st)) {
        printf("refused\n");
        return 2;
    }
    printf("masks %u %u %u\nstats %u %u %u %u %u %d\n%s", m[0], m[1], m[2], st.intervals, st.plane_distances, st.evictions, st.far_reuses, st.extra_operands,
           st.cached ? 1 : 0, text.c_str());
    return 0;
}
