// Test program (tests/test_gpu_walk_setup.py builds and runs it on the GPU box): the short walk setup of rt_path.h trav_begin.
//
//   recip_exhaustive recip           every float d with 2^-40 <= |d| <= 2^40, both signs (2 x (80 x 2^23 + 1) values), through
//                                    rt_device.h recip_in_range and through `1.0f / d` in the same kernel; the bits must be equal.
//   recip_exhaustive flags           trav_begin and the flags closest_hit derives from it, new code against the formulas of before the
//                                    short setup (copied below: plain divisions, six finiteness tests, the compact domain, nf_in_domain
//                                    on the three 1/d), on every combination of edge values per direction axis x four kinds of origin,
//                                    for both values of compact_domain, of COMPACT_DOMAIN and of ref_tree, and for scene layouts with
//                                    all_finite set and clear.  Every field must be equal bit for bit.
//
// One summary line per mode, ending in "<n> mismatches"; exit status 0 iff n == 0.  Any HIP error ends the program with status 2.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kernels.h"
#include "rt_path.h"

using namespace trt;

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("%s: %s\n", #x, hipGetErrorString(e_)); std::exit(2); } } while (0)

// ---- recip ---------------------------------------------------------------------------------------------------------
constexpr uint32_t kBitsLo = 0x2B800000u, kBitsHi = 0x53800000u;          // 2^-40, 2^40
constexpr uint32_t kPerSign = kBitsHi - kBitsLo + 1u;                      // 80 x 2^23 + 1
constexpr uint32_t kPerThread = 256u;
constexpr uint32_t kMaxReports = 16u;

// out[0] = mismatches, out[1] = reports claimed, out[2..3] = values tested (64 bits), then up to kMaxReports x (d, short form, plain form)
__global__ __launch_bounds__(256) void recip_kernel(uint32_t* __restrict__ out) {
    const uint64_t first = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * kPerThread;
    uint32_t bad = 0, done = 0;
    for (uint32_t k = 0; k < kPerThread; k++) {
        const uint64_t n = first + k;
        if (n >= 2ull * kPerSign) break;
        const uint32_t sign = n >= kPerSign ? 0x80000000u : 0u;
        const uint32_t bits = (kBitsLo + (uint32_t)(n >= kPerSign ? n - kPerSign : n)) | sign;
        const float d = __uint_as_float(bits);
        const uint32_t a = __float_as_uint(recip_in_range(d)), b = __float_as_uint(1.0f / d);
        done++;
        if (a != b) {
            bad++;
            const uint32_t slot = atomicAdd(&out[1], 1u);
            if (slot < kMaxReports) { out[4u + 3u * slot] = bits; out[5u + 3u * slot] = a; out[6u + 3u * slot] = b; }
        }
    }
    if (bad) atomicAdd(&out[0], bad);
    // one add per wave: the count of values really tested
    for (int off = 32; off > 0; off >>= 1) done += __shfl_down(done, off, 64);
    if ((threadIdx.x & 63u) == 0u) atomicAdd(reinterpret_cast<unsigned long long*>(&out[2]), (unsigned long long)done);
}

// ---- flags ---------------------------------------------------------------------------------------------------------
struct Fields {                 // every field of Trav, and what closest_hit makes of them for the nearest-first kernel
    uint32_t inv[3], t_best, prim_best, i, n, fast, ref;
    uint32_t nf_ref, nf_n;      // tr.ref / the node count of the walk after closest_hit's nearest-first rule (flat_reuse.nearest_first != 0)
};

// The setup of before the short form, formula for formula (rt_path.h trav_begin and closest_hit at the parent commit).
template <bool COMPACT_DOMAIN>
__device__ Fields setup_before(const SceneLayout& L, const Ray& ray, bool ref_tree, bool compact_domain) {
    const V3 inv = v3(1.0f / ray.d.x, 1.0f / ray.d.y, 1.0f / ray.d.z);
    bool fast = L.all_finite && finite_f(inv.x) && finite_f(inv.y) && finite_f(inv.z) && finite_f(ray.o.x) && finite_f(ray.o.y) && finite_f(ray.o.z);
    if (COMPACT_DOMAIN || compact_domain) {
        const float big = 1152921504606846976.0f;                    // 2^60
        fast = fast && __builtin_fabsf(ray.o.x) <= L.compact_origin_limit[0] && __builtin_fabsf(ray.o.y) <= L.compact_origin_limit[1] &&
               __builtin_fabsf(ray.o.z) <= L.compact_origin_limit[2] && __builtin_fabsf(inv.x) <= big && __builtin_fabsf(inv.y) <= big &&
               __builtin_fabsf(inv.z) <= big;
    }
    bool ref = ref_tree || !fast;
    uint32_t n = ref ? L.n_nodes : L.n_cull_nodes;
    Fields f;
    f.inv[0] = __float_as_uint(inv.x); f.inv[1] = __float_as_uint(inv.y); f.inv[2] = __float_as_uint(inv.z);
    f.t_best = __float_as_uint(__builtin_inff()); f.prim_best = PRIM_NONE; f.i = 0u; f.n = n; f.fast = fast; f.ref = ref;
    if (!nf_in_domain(inv.x, inv.y, inv.z)) { ref = true; n = L.n_nodes; }
    f.nf_ref = ref; f.nf_n = n;
    return f;
}
template <bool COMPACT_DOMAIN>
__device__ Fields setup_now(const SceneLayout& L, const Ray& ray, bool ref_tree, bool compact_domain) {
    const SceneAcc<MODE_GLOBAL> sc{nullptr, L};
    const Trav tr = trav_begin<MODE_GLOBAL, COMPACT_DOMAIN>(sc, ray, ref_tree, compact_domain);
    Fields f;
    f.inv[0] = __float_as_uint(tr.inv.x); f.inv[1] = __float_as_uint(tr.inv.y); f.inv[2] = __float_as_uint(tr.inv.z);
    f.t_best = __float_as_uint(tr.t_best); f.prim_best = tr.prim_best; f.i = tr.i; f.n = tr.n; f.fast = tr.fast; f.ref = tr.ref;
    // closest_hit: `if (nearest_first && !tr.nf) tr.ref = true`, and a lane with tr.ref walks n_nodes
    const bool ref = tr.ref || !tr.nf;
    f.nf_ref = ref; f.nf_n = ref ? L.n_nodes : tr.n;
    return f;
}

// case c = ((layout * 8 + variant) * n_origins + origin) * n_dirs^3 + direction triple; variant bit 0 compact_domain, 1 COMPACT_DOMAIN, 2 ref_tree
__global__ __launch_bounds__(256) void flags_kernel(const SceneLayout* __restrict__ layouts, const float* __restrict__ dirs, uint32_t n_dirs,
                                                    const float* __restrict__ origins, uint32_t n_origins, uint32_t n_cases, uint32_t* __restrict__ out) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cases) return;
    const uint32_t triples = n_dirs * n_dirs * n_dirs;
    const uint32_t t = c % triples, og = (c / triples) % n_origins, variant = (c / (triples * n_origins)) % 8u, layout = c / (triples * n_origins * 8u);
    Ray ray;
    ray.d = v3(dirs[t % n_dirs], dirs[(t / n_dirs) % n_dirs], dirs[t / (n_dirs * n_dirs)]);
    ray.o = v3(origins[3u * og], origins[3u * og + 1u], origins[3u * og + 2u]);
    const SceneLayout L = layouts[layout];
    const bool cd = (variant & 1u) != 0u, ref_tree = (variant & 4u) != 0u;
    Fields a, b;
    if (variant & 2u) { a = setup_now<true>(L, ray, ref_tree, cd); b = setup_before<true>(L, ray, ref_tree, cd); }
    else              { a = setup_now<false>(L, ray, ref_tree, cd); b = setup_before<false>(L, ray, ref_tree, cd); }
    const uint32_t* pa = reinterpret_cast<const uint32_t*>(&a);
    const uint32_t* pb = reinterpret_cast<const uint32_t*>(&b);
    uint32_t differ = 0;
    for (uint32_t k = 0; k < sizeof(Fields) / 4u; k++) differ |= (pa[k] != pb[k]) ? 1u << k : 0u;
    if (differ) {
        atomicAdd(&out[0], 1u);
        const uint32_t slot = atomicAdd(&out[1], 1u);
        if (slot < kMaxReports) { out[4u + 3u * slot] = c; out[5u + 3u * slot] = differ; out[6u + 3u * slot] = a.fast | (b.fast << 1) | (a.ref << 2) | (b.ref << 3); }
    }
    if (a.fast) atomicAdd(&out[2], 1u);                                      // (how many cases are `fast`: printed, the two kinds must both occur)
}

namespace {

float bits_float(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

int run_recip() {
    uint32_t* d_out = nullptr;
    const size_t words = 4u + 3u * kMaxReports;
    CHECK(hipMalloc(&d_out, 4u * words));
    CHECK(hipMemset(d_out, 0, 4u * words));
    const uint64_t total = 2ull * kPerSign;
    const uint32_t blocks = (uint32_t)((total + 256ull * kPerThread - 1ull) / (256ull * kPerThread));
    hipLaunchKernelGGL(recip_kernel, dim3(blocks), dim3(256), 0, 0, d_out);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    std::vector<uint32_t> h(words);
    CHECK(hipMemcpy(h.data(), d_out, 4u * words, hipMemcpyDeviceToHost));
    CHECK(hipFree(d_out));
    const unsigned long long tested = (unsigned long long)h[2] | ((unsigned long long)h[3] << 32);
    for (uint32_t k = 0; k < h[1] && k < kMaxReports; k++)
        std::printf("  d %08x: recip_in_range %08x, 1.0f / d %08x\n", h[4u + 3u * k], h[5u + 3u * k], h[6u + 3u * k]);
    const unsigned long long bad = h[0] + (tested == total ? 0ull : 1ull);  // a value not tested counts
    std::printf("recip: %llu of %llu values tested, %llu mismatches\n", tested, (unsigned long long)total, bad);
    return bad ? 1 : 0;
}

int run_flags() {
    // direction components: the two ends of the range, the floats just outside them, the ends of the nearest-first domain of 1/d, zeros,
    // a subnormal, infinities, a NaN, and ordinary values; each sign
    std::vector<float> dirs;
    const uint32_t mags[] = {0x2B800000u, 0x2B7FFFFFu, 0x2B800001u, 0x53800000u, 0x53800001u, 0x537FFFFFu,      // 2^-40, below, above; 2^40, above, below
                             0x21800000u, 0x217FFFFFu, 0x5D800000u, 0x5D800001u,                                // 2^-60, below; 2^60, above
                             0x00000000u, 0x00000001u, 0x00400000u, 0x00800000u, 0x7F7FFFFFu, 0x7F800000u,      // 0, subnormals, least normal, largest, inf
                             0x7FC00000u, 0x7F800001u,                                                          // quiet and signalling NaN
                             0x3F800000u, 0x3F13CD3Au};                                                         // 1, 0.57735
    for (uint32_t m : mags) { dirs.push_back(bits_float(m)); dirs.push_back(bits_float(m | 0x80000000u)); }
    const float inf = INFINITY, nan = NAN;
    // origins: finite; huge (beyond every compact origin limit, finite); inf and NaN on one axis each
    const float origins[] = {278.0f, 273.0f, -800.0f,   0.0f, -0.0f, 1.0e-30f,   3.0e38f, 1.0f, 1.0f,   1.0f, -1.0e20f, 1.0f,   1.0f, 1.0f, 2.0e13f,
                             inf, 1.0f, 1.0f,   1.0f, -inf, 1.0f,   1.0f, 1.0f, nan,   nan, nan, nan};
    const uint32_t n_origins = sizeof(origins) / (3u * sizeof(float));
    // layouts: all_finite set and clear; compact origin limits as compile_scene gives them (4 B), and zero ("never")
    SceneLayout layouts[3];
    std::memset(layouts, 0, sizeof layouts);
    for (SceneLayout& L : layouts) { L.n_nodes = 35u; L.n_cull_nodes = 23u; L.all_finite = 1u; L.compact_origin_limit[0] = 2220.0f; L.compact_origin_limit[1] = 2200.0f; L.compact_origin_limit[2] = 3200.0f; }
    layouts[1].all_finite = 0u;
    layouts[2].compact_origin_limit[0] = layouts[2].compact_origin_limit[1] = layouts[2].compact_origin_limit[2] = 0.0f;
    const uint32_t n_dirs = (uint32_t)dirs.size();
    const uint32_t n_cases = 3u * 8u * n_origins * n_dirs * n_dirs * n_dirs;

    SceneLayout* d_layouts = nullptr;
    float *d_dirs = nullptr, *d_origins = nullptr;
    uint32_t* d_out = nullptr;
    const size_t words = 4u + 3u * kMaxReports;
    CHECK(hipMalloc(&d_layouts, sizeof layouts));
    CHECK(hipMemcpy(d_layouts, layouts, sizeof layouts, hipMemcpyHostToDevice));
    CHECK(hipMalloc(&d_dirs, 4u * dirs.size()));
    CHECK(hipMemcpy(d_dirs, dirs.data(), 4u * dirs.size(), hipMemcpyHostToDevice));
    CHECK(hipMalloc(&d_origins, sizeof origins));
    CHECK(hipMemcpy(d_origins, origins, sizeof origins, hipMemcpyHostToDevice));
    CHECK(hipMalloc(&d_out, 4u * words));
    CHECK(hipMemset(d_out, 0, 4u * words));
    hipLaunchKernelGGL(flags_kernel, dim3((n_cases + 255u) / 256u), dim3(256), 0, 0, d_layouts, d_dirs, n_dirs, d_origins, n_origins, n_cases, d_out);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    std::vector<uint32_t> h(words);
    CHECK(hipMemcpy(h.data(), d_out, 4u * words, hipMemcpyDeviceToHost));
    CHECK(hipFree(d_out)); CHECK(hipFree(d_origins)); CHECK(hipFree(d_dirs)); CHECK(hipFree(d_layouts));
    for (uint32_t k = 0; k < h[1] && k < kMaxReports; k++)
        std::printf("  case %u: fields differing (bit k = word k of Fields) %03x, fast now/before ref now/before %x\n", h[4u + 3u * k], h[5u + 3u * k], h[6u + 3u * k]);
    // the cases must exercise both outcomes
    const unsigned long long bad = h[0] + ((h[2] == 0u || h[2] == n_cases) ? 1ull : 0ull);
    std::printf("flags: %u cases (%u directions per axis, %u origins, 3 layouts, 8 variants), %u of them fast, %llu mismatches\n", n_cases, n_dirs, n_origins, h[2], bad);
    return bad ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2 || (std::strcmp(argv[1], "recip") != 0 && std::strcmp(argv[1], "flags") != 0)) {
        std::printf("usage: recip_exhaustive recip|flags\n");
        return 3;
    }
    return std::strcmp(argv[1], "recip") == 0 ? run_recip() : run_flags();
}
