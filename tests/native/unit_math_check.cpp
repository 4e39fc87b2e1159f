// Test program (tests/test_unit_math.py builds and runs it, no GPU): the unit-domain forms of the sampling math (rt_device.h
// dm_sincos_nonneg, dm_acos_unit, dm_cbrt_unit, random_in_unit_sphere_unit) against the general functions they are cut from, on the HOST.
// rt_device.h is compiled as plain C++ (tests/native/hipstub stands in for <hip/hip_runtime.h>; the few device builtins are defined
// below), so both sides run the same operation sequences with IEEE f32 and only the steps that were left out can make a difference.
//
//   unit_math_check math     all 2^23 values u = k 2^-23 of random::<f32>(): sin / cos of theta = 2 pi u, phi = acos(1 - 2u), sin / cos of
//                            phi, cbrt(u), new form against general form bit for bit; that theta, phi and u are inside the stated domains
//   unit_math_check sphere   random_in_unit_sphere_unit against random_in_unit_sphere on 2^22 generator states, generator state included
//   unit_math_check div      pixel_uv (the primary ray's (x + u) / (W - 1), one refined reciprocal per denominator) against `/` at
//                            W = 2, 3, 300, 2048, 3840 for every numerator a pixel column x in [0, W) and a draw u can give, and at
//                            W = 1 (division by zero: the plain division, inf / NaN included).  The numerators: x = 0 gives the 2^23
//                            values k 2^-23; for x >= 1 the sum x + u is rounded to a float of [x, x + 1], whose spacing is coarser
//                            than u's, so the sums over all x are exactly the floats of [1, W] - enumerated once, not per (x, u).
//
// The host's 1 / x stands in for v_rcp_f32 in `div` (the device's own estimate: tools/micro/div_exact.hip, tests/test_gpu_primary_div.py).
// The host's sqrtf stands in for v_sqrt_f32 here (both forms of acos go through the same sqrt_in_range, so the comparison does not
// depend on it); the device's own instructions are compared in tests/native/unit_math_exhaustive.hip.
// Exit status 0 and " 0 mismatches" on success.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <thread>
#include <vector>

#define __device__
#define __forceinline__ inline
#define __noinline__
static inline float __uint_as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static inline uint32_t __float_as_uint(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline float unit_math_sqrt_estimate(float x) { return sqrtf(x); }
static inline float unit_math_rcp_estimate(float x) { return 1.0f / x; }
static inline uint32_t unit_math_rotl(uint32_t x, int k) { return (x << k) | (x >> (32 - k)); }
#define __builtin_amdgcn_sqrtf unit_math_sqrt_estimate
#define __builtin_amdgcn_rcpf unit_math_rcp_estimate
#define __builtin_rotateleft32 unit_math_rotl
#include "rt_device.h"

static const unsigned kThreads = 8;

template <class F>
static unsigned long long in_parallel(uint32_t n, F body) {                  // body(k) returns the number of mismatches at k
    std::vector<unsigned long long> bad(kThreads, 0);
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < kThreads; t++)
        pool.emplace_back([&, t] {
            const uint32_t lo = (uint32_t)((uint64_t)n * t / kThreads), hi = (uint32_t)((uint64_t)n * (t + 1) / kThreads);
            for (uint32_t k = lo; k < hi; k++) bad[t] += body(k);
        });
    for (auto& th : pool) th.join();
    unsigned long long sum = 0;
    for (auto b : bad) sum += b;
    return sum;
}

static unsigned differ(const char* what, uint32_t k, float got, float want) {
    if (__float_as_uint(got) == __float_as_uint(want)) return 0;
    printf("k %u %s: unit form %a general %a\n", k, what, got, want);
    return 1;
}

static int check_math() {
    const uint32_t n = 1u << 23;
    const unsigned long long bad = in_parallel(n, [](uint32_t k) -> unsigned long long {
        const float u = __uint_as_float(0x3f800000u | k) - 1.0f;             // rng_random's mapping
        const float theta = (2.0f * 3.14159265358979323846f) * u;
        const float x = 1.0f - 2.0f * u;
        unsigned bad = 0;
        // the domains the forms are specified for
        if (!(theta >= 0.0f && theta < 8192.0f) || signbit(theta)) bad += differ("theta outside [+0, 8192)", k, theta, 0.0f);
        if ((double)x != 1.0 - (double)k * 0x1p-22) bad += differ("1 - 2u not exact", k, x, (float)(1.0 - (double)k * 0x1p-22));
        if (!(u == 0.0f ? !signbit(u) : (u >= 0x1p-23f && u < 1.0f))) bad += differ("u outside {+0} + [2^-23, 1)", k, u, 0.0f);
        const float phi = trt::dm_acos(x);
        if (!(phi >= 0.0f && phi < 8192.0f) || signbit(phi)) bad += differ("phi outside [+0, 8192)", k, phi, 0.0f);
        float s0, c0, s1, c1;
        trt::dm_sincos(theta, s0, c0); trt::dm_sincos_nonneg(theta, s1, c1);
        bad += differ("sin theta", k, s1, s0) + differ("cos theta", k, c1, c0);
        bad += differ("acos", k, trt::dm_acos_unit(x), phi);
        trt::dm_sincos(phi, s0, c0); trt::dm_sincos_nonneg(phi, s1, c1);
        bad += differ("sin phi", k, s1, s0) + differ("cos phi", k, c1, c0);
        bad += differ("cbrt", k, trt::dm_cbrt_unit(u), trt::dm_cbrt(u));
        return bad;
    });
    printf("math: %u inputs x 6 values: %llu mismatches\n", n, bad);
    return bad ? 1 : 0;
}

static int check_sphere() {
    const uint32_t n = 1u << 22;
    const unsigned long long bad = in_parallel(n, [](uint32_t k) -> unsigned long long {
        trt::Rng a = trt::rng_seed(trt::mix32(7u + 0x9E3779B9u), k, k >> 7), b = a;
        unsigned bad = 0;
        for (int draw = 0; draw < 2; draw++) {                               // the second draw starts from the state the first one left
            const trt::V3 p = trt::random_in_unit_sphere(a), q = trt::random_in_unit_sphere_unit(b);
            bad += differ("x", k, q.x, p.x) + differ("y", k, q.y, p.y) + differ("z", k, q.z, p.z);
        }
        if (a.s0 != b.s0 || a.s1 != b.s1) { printf("state %u: generator states differ\n", k); bad++; }
        return bad;
    });
    printf("sphere: %u generator states x 2 draws x 3 values: %llu mismatches\n", n, bad);
    return bad ? 1 : 0;
}

static unsigned long long check_div_range(uint32_t w, uint32_t first_bits, uint32_t count) {
    return in_parallel(count, [=](uint32_t k) -> unsigned long long {
        const float n = __uint_as_float(first_bits + k);
        float u, v;
        trt::pixel_uv(w, w + 7u, n, n, u, v);
        const float want_u = n / (float)(w - 1u), want_v = n / (float)(w + 6u);
        unsigned bad = 0;
        if (__float_as_uint(u) != __float_as_uint(want_u)) { printf("W %u numerator %a: short form %a division %a\n", w, n, u, want_u); bad++; }
        if (__float_as_uint(v) != __float_as_uint(want_v)) { printf("H %u numerator %a: short form %a division %a\n", w + 7u, n, v, want_v); bad++; }
        return bad;
    });
}

static int check_div() {
    unsigned long long bad = 0, n = 0;
    static const uint32_t widths[5] = {2u, 3u, 300u, 2048u, 3840u};
    for (uint32_t w : widths) {
        // x = 0: u = k 2^-23, the numerator 0 + 0 included
        bad += in_parallel(1u << 23, [=](uint32_t k) -> unsigned long long {
            const float num = 0.0f + (__uint_as_float(0x3f800000u | k) - 1.0f);
            float u, v;
            trt::pixel_uv(w, w, num, num, u, v);
            const float want = num / (float)(w - 1u);
            if (__float_as_uint(u) == __float_as_uint(want) && __float_as_uint(v) == __float_as_uint(want)) return 0;
            printf("W %u numerator %a: short form %a %a division %a\n", w, num, u, v, want);
            return 1;
        });
        // x >= 1: every float of [1, W] (also as a row quotient against H = W + 7)
        const uint32_t first = __float_as_uint(1.0f), last = __float_as_uint((float)w);
        bad += check_div_range(w, first, last - first + 1u);
        n += (1ull << 23) + (last - first + 1u);
    }
    // a 1-wide or 1-high image divides by zero: both quotients are the plain divisions
    for (uint32_t k = 0; k < (1u << 23); k += 4099u) {
        const float num = __uint_as_float(0x3f800000u | k) - 1.0f;
        for (int high = 0; high < 2; high++) {
            const uint32_t w = high ? 5u : 1u, h = high ? 1u : 5u;
            float u, v;
            trt::pixel_uv(w, h, num, num + 3.0f, u, v);
            const float want_u = num / (float)(w - 1u), want_v = (num + 3.0f) / (float)(h - 1u);
            const bool same_u = __float_as_uint(u) == __float_as_uint(want_u) || (u != u && want_u != want_u);
            const bool same_v = __float_as_uint(v) == __float_as_uint(want_v) || (v != v && want_v != want_v);
            if (!same_u || !same_v) { printf("%u x %u numerator %a: %a %a, divisions %a %a\n", w, h, num, u, v, want_u, want_v); bad++; }
            n++;
        }
    }
    printf("div: %llu numerators over 5 widths and the 1-wide / 1-high images: %llu mismatches\n", n, bad);
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    const char* what = argc > 1 ? argv[1] : "";
    if (!strcmp(what, "math")) return check_math();
    if (!strcmp(what, "sphere")) return check_sphere();
    if (!strcmp(what, "div")) return check_div();
    printf("usage: unit_math_check math|sphere|div\n");
    return 2;
}
