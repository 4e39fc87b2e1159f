// Test program (tests/test_gpu_unit_math.py builds and runs it on the GPU box): the device's unit-domain forms of trt-math v2
// (rt_device.h dm_sincos_nonneg / dm_acos_unit / dm_cbrt_unit / random_in_unit_sphere_unit) against the device's general forms AND against
// the CPU checker's statement of the functions (liboracle: orc_sinf / orc_cosf / orc_acosf / orc_cbrtf) on all 2^23 values u = k / 2^23 of
// random::<f32>(): sin / cos of theta = 2 pi u, phi = acos(1 - 2u), sin / cos of phi, cbrt(u).  Six floats per k and form, compared bit
// for bit; also the composed sampler on 2^22 generator states against random_in_unit_sphere on the device and orc_random_in_unit_sphere.
// Exit status 0 and " 0 mismatches" on success.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "rt_device.h"
extern "C" {
#include "rt_oracle.h"
}

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)

// out[12 k .. 12 k + 5]: unit forms; out[12 k + 6 .. 12 k + 11]: general forms
__global__ void eval_all(float* out, uint32_t n) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const float u = __uint_as_float(0x3f800000u | k) - 1.0f;                 // rng_random's mapping, all 2^23 values
    const float theta = (2.0f * 3.14159265358979323846f) * u;
    const float x = 1.0f - 2.0f * u;
    float* o = out + 12ull * k;
    {
        const float phi = trt::dm_acos_unit(x);
        float st, ct, sp, cp;
        trt::dm_sincos_nonneg(theta, st, ct);
        trt::dm_sincos_nonneg(phi, sp, cp);
        o[0] = st; o[1] = ct; o[2] = phi; o[3] = sp; o[4] = cp; o[5] = trt::dm_cbrt_unit(u);
    }
    {
        const float phi = trt::dm_acos(x);
        float st, ct, sp, cp;
        trt::dm_sincos(theta, st, ct);
        trt::dm_sincos(phi, sp, cp);
        o[6] = st; o[7] = ct; o[8] = phi; o[9] = sp; o[10] = cp; o[11] = trt::dm_cbrt(u);
    }
}

// out[6 k .. 6 k + 2]: unit sampler; out[6 k + 3 .. 6 k + 5]: general sampler, both from the same generator state
__global__ void eval_ball(float* out, uint32_t n) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    trt::Rng g = trt::rng_seed(trt::mix32(7u + 0x9E3779B9u), k, k >> 7), h = g;
    const trt::V3 p = trt::random_in_unit_sphere_unit(g);
    const trt::V3 q = trt::random_in_unit_sphere(h);
    float* o = out + 6ull * k;
    o[0] = p.x; o[1] = p.y; o[2] = p.z; o[3] = q.x; o[4] = q.y; o[5] = q.z;
}

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

int main() {
    const uint32_t n = 1u << 23, nb = 1u << 22;
    float* d; CHECK(hipMalloc(&d, 12ull * n * sizeof(float)));
    eval_all<<<(n + 255) / 256, 256>>>(d, n);
    CHECK(hipGetLastError());
    std::vector<float> h(12ull * n);
    CHECK(hipMemcpy(h.data(), d, h.size() * sizeof(float), hipMemcpyDeviceToHost));
    static const char* const name[6] = {"sin theta", "cos theta", "acos", "sin phi", "cos phi", "cbrt"};
    unsigned long long bad = 0;
    for (uint32_t k = 0; k < n; k++) {
        union { uint32_t u; float f; } c; c.u = 0x3f800000u | k;
        const float u = c.f - 1.0f;
        const float theta = (2.0f * 3.14159265358979323846f) * u;
        const float phi = orc_acosf(1.0f - 2.0f * u);
        const float want[6] = {orc_sinf(theta), orc_cosf(theta), phi, orc_sinf(phi), orc_cosf(phi), orc_cbrtf(u)};
        const float* o = &h[12ull * k];
        for (int j = 0; j < 6; j++)
            if (bits(o[j]) != bits(want[j]) || bits(o[j]) != bits(o[6 + j])) {
                if (bad++ < 10) printf("k %u %s: unit form %a general form %a oracle %a\n", k, name[j], o[j], o[6 + j], want[j]);
            }
    }
    eval_ball<<<(nb + 255) / 256, 256>>>(d, nb);
    CHECK(hipGetLastError());
    CHECK(hipMemcpy(h.data(), d, 6ull * nb * sizeof(float), hipMemcpyDeviceToHost));
    for (uint32_t k = 0; k < nb; k++) {
        uint32_t st[2];
        orc_rng_seed(7u, k, k >> 7, st);
        const orc_vec3 p = orc_random_in_unit_sphere(st);
        const float want[3] = {p.x, p.y, p.z};
        const float* o = &h[6ull * k];
        for (int j = 0; j < 3; j++)
            if (bits(o[j]) != bits(want[j]) || bits(o[j]) != bits(o[3 + j])) {
                if (bad++ < 20) printf("state %u value %d: unit sampler %a general sampler %a oracle %a\n", k, j, o[j], o[3 + j], want[j]);
            }
    }
    CHECK(hipFree(d));
    printf("%u inputs x 6 values + %u generator states x 3 values, unit forms against general forms and the oracle: %llu mismatches\n", n, nb, bad);
    return bad ? 1 : 0;
}
