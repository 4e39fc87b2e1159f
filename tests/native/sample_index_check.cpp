// sample_index_check.cpp - a stand-alone program (its own main; plain C++, no GPU, nothing of the project but the header under test) that
// holds csrc/sample_index.h against 64-bit division:
//   sample_index(q, R, b) = (q / R, b + q % R) for the range lengths and work indices at the edges of every width involved, and
//   fold_row(e, fold_row_magic(len)) = e / len for EVERY e < 64 * len and every row length 1 .. 48 the tile fold can ask for.
// Prints "ok all" and returns 0, or the first mismatch and 1.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "sample_index.h"

static int g_bad = 0;

static void check_index(uint64_t n, uint32_t R, uint32_t b, uint64_t q) {
    if (q >= n * R) return;                                                 // clipped to the work of the call
    const trt::SampleIndex x = trt::sample_index((uint32_t)q, R, b);
    const uint64_t item = q / R, sample = (uint64_t)b + q % R;
    if (x.item != item || x.sample != sample) {
        if (!g_bad) std::printf("sample_index(q = %llu, R = %u, b = %u) = (%u, %u), want (%llu, %llu)\n", (unsigned long long)q, R, b, x.item, x.sample,
                                (unsigned long long)item, (unsigned long long)sample);
        g_bad = 1;
    }
}

int main() {
    const uint64_t top = 0xFFFFFFFFull;                                     // n * R <= 2^32 - 1
    const uint32_t lengths[] = {1u, 2u, 3u, 5u, 63u, 64u, 65u, 255u, 256u, 257u, 65535u, 65537u, 0x80000000u, 0xFFFFFFFFu};
    unsigned long long checked = 0;
    for (uint32_t R : lengths) {
        const uint64_t n = top / R;                                         // the most items a call of this range may have
        // b: 0, a few, and the largest begin of a range of this length (b + R <= K <= 2^32 - 1)
        const uint32_t room = (uint32_t)(top - R), begins[] = {0u, room < 3u ? room : 3u, room};
        std::vector<uint64_t> at = {0, (uint64_t)R - 1, R};
        for (uint64_t near : {(uint64_t)0x80000000ull, top})
            for (uint64_t m : {near / R * R, (near / R + 1) * R})           // the multiples of R on either side
                for (int d = -1; d <= 1; d++)
                    if (m + d <= top && (m > 0 || d >= 0)) at.push_back(m + d);
        at.push_back(n * R - 1);                                            // the last work index of the largest call
        for (uint32_t b : begins)
            for (uint64_t q : at) { check_index(n, R, b, q); checked++; }
        // and a sweep over the first 4 R work indices
        for (uint64_t q = 0; q < 4ull * R && q < 100000ull; q++) { check_index(n, R, begins[1], q); checked++; }
    }
    for (uint32_t len = 1; len <= 48; len++) {
        const uint32_t magic = trt::fold_row_magic(len);
        for (uint32_t e = 0; e < 64u * len; e++) {
            if (trt::fold_row(e, magic) != e / len) {
                if (!g_bad) std::printf("fold_row(e = %u, len = %u) = %u, want %u\n", e, len, trt::fold_row(e, magic), e / len);
                g_bad = 1;
            }
            checked++;
        }
    }
    if (g_bad) return 1;
    std::printf("ok all (%llu cases)\n", checked);
    return 0;
}
