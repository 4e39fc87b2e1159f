// scene_build.hip — the scene compiler on the device: trt_scene_create_on_device.
//
// Produces the same bytes as compile_scene (scene_host.cpp): the same reference tree, culling tree, leaf list, compact nodes
// and packed blob, plus the two node dumps.  The host uploads the world's geometry once, runs the passes below on a private
// stream of the current device and copies the results back; only layout arithmetic and O(materials) work stay on the host.
//
//   1. per primitive: boxes (Sphere::new / Quad::new with the host's f32 operations, NaN results included), finiteness, material check;
//      local indices (sphere / quad number) by a scan
//   2. reference tree, top levels: one level at a time over all objects.  The segments of a level all have floor or ceil of
//      N / 2^level objects, so each is told apart by its index alone: a union reduction per segment gives the node box and the
//      split axis, then ONE stable LSD radix sort of (segment index, key) sorts every segment by its key at once (stable =
//      the host's tie-break by incoming position)
//   3. reference tree, segments of at most kRefLocalMax objects: one workgroup per segment builds the whole subtree in LDS,
//      level by level, sorting by rank (objects before it in (key, position) order)
//   4. culling tree: top-down SAH over the leaf sequence.  Large ranges: one workgroup per range per level (union reduction,
//      suffix and prefix union scans, costs in double, the host's sequential choice of k); ranges of at most kCullSerialMax
//      leaves: one lane each, the host's own loop.  Every emitted node records its leaf range and its CHAIN RANK (emitted
//      ancestors that start at the same leaf); per leaf a the count of emitted nodes starting there is the leaf's chain rank
//      + 1, and with S = exclusive scan of those counts a node's pre-order index is S[a] + rank and its skip is S[b]
//   5. packing: both trees, leaf list, primitives, compact nodes straight into the device blob
//
// Box unions run in whatever order the parallel passes take: box coordinates are never -0 (min - pad / max + pad) and NaN
// operands are dropped by min/max, so the union of a set of boxes does not depend on the order (DESIGN.md §2.1 has the
// argument and the one case it does not cover).
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include <new>
#include <string>
#include <vector>

#include "kernels.h"
#include "scene.h"
#include "scene_adopt.h"
#include "scene_common.h"

namespace trt {
namespace {

constexpr uint32_t kRefLocalMax = 1024;     // reference-tree segments of at most this many objects: whole subtree in one workgroup
constexpr uint32_t kCullSerialMax = 64;     // culling ranges of at most this many leaves: whole subtree on one lane
constexpr uint32_t kThreads = 256;          // lanes per workgroup, every kernel here
constexpr uint32_t kScanItems = 16;         // scan: items per lane
constexpr uint32_t kScanTile = kThreads * kScanItems;
constexpr uint32_t kSortTile = 4096;        // radix pass: objects per workgroup
constexpr uint32_t kCullItems = 8;          // culling split: contiguous leaves per lane per chunk

struct DBox { float lo[3], hi[3]; };

// ---- the host compiler's f32 results, NaNs included ----------------------------------------------------------------------
// A NaN result takes the bits the host's SSE instruction gives it: the first NaN operand, quieted, or the default NaN
// 0xFFC00000 for an invalid operation.  The device's own NaN bits are never used.
__device__ inline float quieted(float a) { return bits_to_f32(f32_to_bits(a) | 0x00400000u); }
__device__ inline float host_nan(float r, float a, float b) {
    if (r == r) return r;
    if (a != a) return quieted(a);
    if (b != b) return quieted(b);
    return bits_to_f32(0xFFC00000u);
}
__device__ inline float hadd(float a, float b) { return host_nan(a + b, a, b); }
__device__ inline float hsub(float a, float b) { return host_nan(a - b, a, b); }
__device__ inline float hmul(float a, float b) { return host_nan(a * b, a, b); }
__device__ inline float hdiv(float a, float b) { return host_nan(a / b, a, b); }
__device__ inline float hsqrt(float a) {
    const float r = sqrtf(a);
    if (r == r) return r;
    return a != a ? quieted(a) : bits_to_f32(0xFFC00000u);
}
// fminf / fmaxf as the host compiler lowers them (select on "x is NaN" around minss/maxss): x NaN -> y, y NaN -> x, both -> y
__device__ inline float hmin(float x, float y) { return x != x ? y : (y < x ? y : x); }
__device__ inline float hmax(float x, float y) { return x != x ? y : (y > x ? y : x); }

__device__ inline DBox box_union(const DBox& a, const DBox& b) {
    DBox r;
    for (int i = 0; i < 3; i++) { r.lo[i] = hmin(a.lo[i], b.lo[i]); r.hi[i] = hmax(a.hi[i], b.hi[i]); }
    return r;
}
// AABB::new (aabb.rs:13-20)
__device__ inline DBox box_from_corners(const float a[3], const float b[3]) {
    const float pad = 0.0001f / 2.0f;
    DBox r;
    for (int i = 0; i < 3; i++) { r.lo[i] = hsub(hmin(a[i], b[i]), pad); r.hi[i] = hadd(hmax(a[i], b[i]), pad); }
    return r;
}
__device__ inline DBox load_box(const float* b6, size_t i) {
    DBox r;
    for (int k = 0; k < 3; k++) { r.lo[k] = b6[6 * i + k]; r.hi[k] = b6[6 * i + 3 + k]; }
    return r;
}
__device__ inline void store_box(float* b6, size_t i, const DBox& b) {
    for (int k = 0; k < 3; k++) { b6[6 * i + k] = b.lo[k]; b6[6 * i + 3 + k] = b.hi[k]; }
}
__device__ inline double box_sa(const DBox& b) { return surface_area6(b.lo, b.hi); }
__device__ inline bool tame3(const float v[3]) { return tame(v[0]) && tame(v[1]) && tame(v[2]); }

// Sphere::new (sphere.rs:16-26) / Quad::new (quad.rs:20-29) exactly as compile_scene evaluates them: the box, the packed
// record (sphere: 1 element, quad: 5) and whether every value is tame.
__device__ inline void eval_primitive(const Geometry& geo, DBox& box, float4 rec[5], bool& finite) {
    if (geo.kind == 0) {
        const float c[3] = {geo.a.x, geo.a.y, geo.a.z}, r = geo.b.x;
        float lo[3], hi[3];
        for (int i = 0; i < 3; i++) { lo[i] = hsub(c[i], r); hi[i] = hadd(c[i], r); }
        box = box_from_corners(lo, hi);
        rec[0] = make_float4(c[0], c[1], c[2], r);
        finite = tame3(c) && tame(r);
    } else {
        const float p[3] = {geo.a.x, geo.a.y, geo.a.z}, u[3] = {geo.b.x, geo.b.y, geo.b.z}, v[3] = {geo.c.x, geo.c.y, geo.c.z};
        float pu[3], puv[3], pv[3];
        for (int i = 0; i < 3; i++) { pu[i] = hadd(p[i], u[i]); puv[i] = hadd(pu[i], v[i]); pv[i] = hadd(p[i], v[i]); }
        box = box_union(box_from_corners(p, puv), box_from_corners(pu, pv));
        const float n[3] = {hsub(hmul(u[1], v[2]), hmul(u[2], v[1])), hsub(hmul(u[2], v[0]), hmul(u[0], v[2])),
                            hsub(hmul(u[0], v[1]), hmul(u[1], v[0]))};
        const float nn = hadd(hadd(hmul(n[0], n[0]), hmul(n[1], n[1])), hmul(n[2], n[2]));
        const float w[3] = {hdiv(n[0], nn), hdiv(n[1], nn), hdiv(n[2], nn)};
        const float d = hadd(hadd(hmul(n[0], p[0]), hmul(n[1], p[1])), hmul(n[2], p[2]));
        const float len = hsqrt(nn);
        const float nu[3] = {hdiv(n[0], len), hdiv(n[1], len), hdiv(n[2], len)};
        rec[0] = make_float4(n[0], n[1], n[2], d);
        rec[1] = make_float4(p[0], p[1], p[2], bits_to_f32(geo.material));
        rec[2] = make_float4(v[0], v[1], v[2], w[0]);
        rec[3] = make_float4(w[1], w[2], u[0], u[1]);
        rec[4] = make_float4(u[2], nu[0], nu[1], nu[2]);
        finite = tame3(p) && tame3(u) && tame3(v) && tame3(n) && tame(d);
    }
    finite = finite && tame3(box.lo) && tame3(box.hi);
}

enum : uint32_t { FLAG_BAD_MATERIAL = 0, FLAG_NOT_FINITE = 1, CTR_NEXT = 2, CTR_SMALL = 3, CTR_RECORDS = 4, N_FLAGS = 8 };

__global__ void __launch_bounds__(kThreads) primitive_kernel(const Geometry* geo, uint32_t ng, uint32_t nm, float* prim_box,
                                                             uint32_t* is_sphere, uint32_t* flags) {
    const uint32_t g = blockIdx.x * kThreads + threadIdx.x;
    if (g >= ng) return;
    const Geometry gg = geo[g];
    DBox box;
    float4 rec[5];
    bool finite;
    eval_primitive(gg, box, rec, finite);
    store_box(prim_box, g, box);
    is_sphere[g] = gg.kind == 0 ? 1u : 0u;
    if (gg.material >= nm) atomicOr(&flags[FLAG_BAD_MATERIAL], 1u);
    if (!finite) atomicOr(&flags[FLAG_NOT_FINITE], 1u);
}

// ---- exclusive scan of u32 (in place allowed) ----------------------------------------------------------------------------
__device__ inline uint32_t block_exclusive_sum(uint32_t v, uint32_t* sh, uint32_t& total) {
    const uint32_t t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (uint32_t off = 1; off < kThreads; off <<= 1) {
        const uint32_t add = t >= off ? sh[t - off] : 0u;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    total = sh[kThreads - 1];
    const uint32_t r = sh[t] - v;
    __syncthreads();
    return r;
}

__global__ void __launch_bounds__(kThreads) scan_tiles_kernel(const uint32_t* in, uint32_t* out, uint32_t n, uint32_t* tile_sums) {
    __shared__ uint32_t sh[kThreads];
    const size_t base = (size_t)blockIdx.x * kScanTile + (size_t)threadIdx.x * kScanItems;
    uint32_t v[kScanItems], sum = 0;
    for (uint32_t j = 0; j < kScanItems; j++) { v[j] = base + j < n ? in[base + j] : 0u; sum += v[j]; }
    uint32_t total;
    uint32_t run = block_exclusive_sum(sum, sh, total);
    for (uint32_t j = 0; j < kScanItems; j++) {
        if (base + j < n) out[base + j] = run;
        run += v[j];
    }
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}
__global__ void __launch_bounds__(kThreads) scan_add_kernel(uint32_t* out, uint32_t n, const uint32_t* tile_offsets) {
    const size_t base = (size_t)blockIdx.x * kScanTile + (size_t)threadIdx.x * kScanItems;
    const uint32_t add = tile_offsets[blockIdx.x];
    for (uint32_t j = 0; j < kScanItems; j++)
        if (base + j < n) out[base + j] += add;
}

// ---- stable LSD radix passes over (key, segment) with the object as payload ----------------------------------------------
__device__ inline uint32_t radix_digit(uint32_t key, uint32_t seg, uint32_t pass) {
    return pass < 4 ? (key >> (8 * pass)) & 255u : (seg >> (8 * (pass - 4))) & 255u;
}
__global__ void __launch_bounds__(kThreads) radix_hist_kernel(const uint32_t* key, const uint32_t* seg, uint32_t n, uint32_t pass,
                                                              uint32_t* hist, uint32_t nblocks) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const size_t start = (size_t)blockIdx.x * kSortTile, end = start + kSortTile < n ? start + kSortTile : n;
    for (size_t i = start + threadIdx.x; i < end; i += kThreads) atomicAdd(&h[radix_digit(key[i], seg[i], pass)], 1u);
    __syncthreads();
    hist[(size_t)threadIdx.x * nblocks + blockIdx.x] = h[threadIdx.x];
}
// Each workgroup moves its tile in order, 256 objects at a time: an object's place is its digit's running offset + the objects
// of the same digit before it in this step (earlier waves, earlier lanes of its own wave: matched by ballots).
__global__ void __launch_bounds__(kThreads) radix_scatter_kernel(const uint32_t* kin, const uint32_t* sin, const uint32_t* vin,
                                                                 uint32_t* kout, uint32_t* sout, uint32_t* vout, uint32_t n,
                                                                 uint32_t pass, const uint32_t* offsets, uint32_t nblocks) {
    constexpr uint32_t kWaves = kThreads / 64;
    __shared__ uint32_t base[256];
    __shared__ uint32_t wcnt[kWaves][256];
    __shared__ uint32_t woff[kWaves][256];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    base[t] = offsets[(size_t)t * nblocks + blockIdx.x];
    for (uint32_t w = 0; w < kWaves; w++) wcnt[w][t] = 0;
    __syncthreads();
    const size_t start = (size_t)blockIdx.x * kSortTile, end = start + kSortTile < n ? start + kSortTile : n;
    const unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (64u - lane));
    for (size_t sub = start; sub < end; sub += kThreads) {
        const size_t i = sub + t;
        const bool valid = i < end;
        uint32_t k = 0, s = 0, v = 0, d = 0;
        if (valid) { k = kin[i]; s = sin[i]; v = vin[i]; d = radix_digit(k, s, pass); }
        unsigned long long peers = __ballot(valid);
        for (uint32_t bit = 0; bit < 8; bit++) {
            const bool on = (d >> bit) & 1u;
            const unsigned long long m = __ballot(on);
            peers &= on ? m : ~m;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & lt);
        if (valid && rank == 0) wcnt[wave][d] = (uint32_t)__popcll(peers);
        __syncthreads();
        uint32_t run = base[t];
        for (uint32_t w = 0; w < kWaves; w++) { woff[w][t] = run; run += wcnt[w][t]; wcnt[w][t] = 0; }
        base[t] = run;
        __syncthreads();
        if (valid) {
            const uint32_t pos = woff[wave][d] + rank;
            kout[pos] = k; sout[pos] = s; vout[pos] = v;
        }
        __syncthreads();
    }
}

// ---- reference tree -----------------------------------------------------------------------------------------------------
// segment `idx` of `level` (its index bits, most significant first, say left / right on the way down)
__device__ inline void ref_segment(uint32_t N, uint32_t level, uint32_t idx, uint32_t& s, uint32_t& n, uint32_t& me) {
    s = 0; n = N; me = 0;
    for (int j = (int)level - 1; j >= 0; j--) {
        const uint32_t mid = n / 2;
        if (((idx >> j) & 1u) == 0u) { n = mid; me += 1; }
        else { s += mid; me += 2 * mid; n -= mid; }
    }
}
__device__ inline uint32_t ref_segment_of(uint32_t N, uint32_t level, uint32_t p) {
    uint32_t s = 0, n = N, idx = 0;
    for (uint32_t j = 0; j < level; j++) {
        const uint32_t mid = n / 2;
        if (p < s + mid) { n = mid; idx = 2 * idx; }
        else { s += mid; n -= mid; idx = 2 * idx + 1; }
    }
    return idx;
}
__device__ inline void write_node(float* box6, int32_t* prim, int32_t* skip, uint32_t me, const DBox& b, int32_t p, uint32_t sk) {
    store_box(box6, me, b);
    prim[me] = p;
    skip[me] = (int32_t)sk;
}

// one workgroup per segment of a top level: its box (the inner node) and split axis
__global__ void __launch_bounds__(kThreads) ref_level_box_kernel(uint32_t N, uint32_t level, const uint32_t* order, const float* prim_box,
                                                                 float* ref_box, int32_t* ref_prim, int32_t* ref_skip, uint8_t* seg_axis) {
    __shared__ DBox sb[kThreads];
    __shared__ int sh[kThreads];
    uint32_t s, n, me;
    ref_segment(N, level, blockIdx.x, s, n, me);
    DBox acc;
    bool has = false;
    for (uint32_t p = s + threadIdx.x; p < s + n; p += kThreads) {
        const DBox b = load_box(prim_box, order[p]);
        acc = has ? box_union(acc, b) : b;
        has = true;
    }
    sb[threadIdx.x] = acc;
    sh[threadIdx.x] = has;
    __syncthreads();
    for (uint32_t off = kThreads / 2; off > 0; off >>= 1) {
        if (threadIdx.x < off && sh[threadIdx.x + off]) {
            sb[threadIdx.x] = sh[threadIdx.x] ? box_union(sb[threadIdx.x], sb[threadIdx.x + off]) : sb[threadIdx.x + off];
            sh[threadIdx.x] = 1;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        write_node(ref_box, ref_prim, ref_skip, me, sb[0], -1, me + 2 * n - 1);
        seg_axis[blockIdx.x] = (uint8_t)box_longest_axis6(sb[0].lo, sb[0].hi);
    }
}
__global__ void __launch_bounds__(kThreads) ref_level_keys_kernel(uint32_t N, uint32_t level, const uint32_t* order, const float* prim_box,
                                                                  const uint8_t* seg_axis, uint32_t* key, uint32_t* seg, uint32_t* val) {
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= N) return;
    const uint32_t idx = ref_segment_of(N, level, p), o = order[p];
    key[p] = total_order_key_u32(prim_box[6 * (size_t)o + seg_axis[idx]]);
    seg[p] = idx;
    val[p] = o;
}

// one workgroup per segment of at most kRefLocalMax objects: the whole subtree, one depth at a time, in LDS
__global__ void __launch_bounds__(kThreads) ref_local_kernel(uint32_t N, uint32_t level, const uint32_t* order, const float* prim_box,
                                                             float* ref_box, int32_t* ref_prim, int32_t* ref_skip, uint32_t* perm) {
    __shared__ DBox lbox[kRefLocalMax];
    __shared__ uint32_t lobj[kRefLocalMax];
    __shared__ uint16_t ord[2][kRefLocalMax];
    __shared__ uint32_t lkey[kRefLocalMax];
    __shared__ uint8_t laxis[kRefLocalMax];
    uint32_t s0, n0, me0;
    ref_segment(N, level, blockIdx.x, s0, n0, me0);
    for (uint32_t j = threadIdx.x; j < n0; j += kThreads) {
        lobj[j] = order[s0 + j];
        lbox[j] = load_box(prim_box, lobj[j]);
        ord[0][j] = (uint16_t)j;
    }
    __syncthreads();
    uint32_t cur = 0;
    for (uint32_t depth = 0;; depth++) {
        uint32_t biggest = n0;                                   // segments at this depth hold floor or ceil of n0 / 2^depth objects
        for (uint32_t j = 0; j < depth; j++) biggest -= biggest / 2;
        // nodes of this depth: leaves, 2-object nodes with their leaves, boxes and axes of the nodes that sort
        for (uint32_t p = threadIdx.x; p < n0; p += kThreads) {
            uint32_t s = 0, n = n0, me = me0;
            bool done = false;
            for (uint32_t j = 0; j < depth && !done; j++) {
                if (n <= 2) { done = true; break; }
                const uint32_t mid = n / 2;
                if (p < s + mid) { n = mid; me += 1; } else { s += mid; me += 2 * mid; n -= mid; }
            }
            if (done || p != s) continue;
            const uint16_t* o = ord[cur];
            if (n == 1) {
                write_node(ref_box, ref_prim, ref_skip, me, lbox[o[s]], (int32_t)lobj[o[s]], me + 1);
            } else if (n == 2) {                                 // children keep the given order: no sort (bvh.rs:58-67)
                const DBox a = lbox[o[s]], b = lbox[o[s + 1]];
                write_node(ref_box, ref_prim, ref_skip, me + 1, a, (int32_t)lobj[o[s]], me + 2);
                write_node(ref_box, ref_prim, ref_skip, me + 2, b, (int32_t)lobj[o[s + 1]], me + 3);
                write_node(ref_box, ref_prim, ref_skip, me, box_union(a, b), -1, me + 3);
            } else {
                DBox all = lbox[o[s]];
                for (uint32_t q = s + 1; q < s + n; q++) all = box_union(all, lbox[o[q]]);
                write_node(ref_box, ref_prim, ref_skip, me, all, -1, me + 2 * n - 1);
                laxis[s] = (uint8_t)box_longest_axis6(all.lo, all.hi);
            }
        }
        __syncthreads();
        if (biggest <= 2) break;
        // keys, then each object's rank in (key, position) order within its segment
        for (uint32_t p = threadIdx.x; p < n0; p += kThreads) {
            uint32_t s = 0, n = n0;
            bool done = false;
            for (uint32_t j = 0; j < depth; j++) {
                if (n <= 2) { done = true; break; }
                const uint32_t mid = n / 2;
                if (p < s + mid) n = mid; else { s += mid; n -= mid; }
            }
            if (!done && n >= 3) {
                // (the first object of the segment wrote laxis[s] above)
                lkey[p] = total_order_key_u32(lbox[ord[cur][p]].lo[laxis[s]]);
            }
        }
        __syncthreads();
        for (uint32_t p = threadIdx.x; p < n0; p += kThreads) {
            uint32_t s = 0, n = n0;
            bool done = false;
            for (uint32_t j = 0; j < depth; j++) {
                if (n <= 2) { done = true; break; }
                const uint32_t mid = n / 2;
                if (p < s + mid) n = mid; else { s += mid; n -= mid; }
            }
            if (done || n <= 2) { ord[cur ^ 1][p] = ord[cur][p]; continue; }
            const uint32_t kp = lkey[p];
            uint32_t rank = 0;
            for (uint32_t q = s; q < s + n; q++) {
                const uint32_t kq = lkey[q];
                rank += (kq < kp || (kq == kp && q < p)) ? 1u : 0u;
            }
            ord[cur ^ 1][s + rank] = ord[cur][p];
        }
        __syncthreads();
        cur ^= 1;
    }
    for (uint32_t p = threadIdx.x; p < n0; p += kThreads) perm[s0 + p] = lobj[ord[cur][p]];
}

// ---- culling tree -------------------------------------------------------------------------------------------------------
struct Range { uint32_t a, b, chain, pad; double parent_sa; };
struct CullRec { uint32_t a, b, chain; int32_t leaf; DBox box; };

__global__ void __launch_bounds__(kThreads) gather_leaves_kernel(const uint32_t* perm, uint32_t n, const float* prim_box, float* leaf_box) {
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
    if (k < n) store_box(leaf_box, k, load_box(prim_box, perm[k]));
}

__device__ inline void emit_record(CullRec* recs, uint32_t* flags, uint32_t a, uint32_t b, uint32_t chain, int32_t leaf, const DBox& box) {
    const uint32_t r = atomicAdd(&flags[CTR_RECORDS], 1u);
    recs[r] = CullRec{a, b, chain, leaf, box};
}
__device__ inline void route_range(const Range& c, Range* next, Range* small, uint32_t* flags) {
    if (c.b - c.a <= kCullSerialMax) small[atomicAdd(&flags[CTR_SMALL], 1u)] = c;
    else next[atomicAdd(&flags[CTR_NEXT], 1u)] = c;
}

// LDS scan of one box per lane (has = the lane holds one): inclusive, forward (lower lanes first) or backward
__device__ inline void block_scan_boxes(DBox& v, int& has, bool backward, DBox* sb, int* sh) {
    const uint32_t t = backward ? kThreads - 1 - threadIdx.x : threadIdx.x;
    sb[t] = v; sh[t] = has;
    __syncthreads();
    for (uint32_t off = 1; off < kThreads; off <<= 1) {
        DBox o;
        int oh = 0;
        if (t >= off) { o = sb[t - off]; oh = sh[t - off]; }
        __syncthreads();
        if (oh) { sb[t] = sh[t] ? box_union(o, sb[t]) : o; sh[t] = 1; }
        __syncthreads();
    }
    v = sb[t]; has = sh[t];
    __syncthreads();
}

// CullBuilder::split over leaves [a, b), b - a > kCullSerialMax, by one workgroup.  suffix_sa: scratch indexed by leaf.
__global__ void __launch_bounds__(kThreads) cull_level_kernel(const Range* ranges, Range* next, Range* small, CullRec* recs, uint32_t* flags,
                                                              const float* leaf_box, double* suffix_sa, double prune) {
    __shared__ DBox sb[kThreads];
    __shared__ int sh[kThreads];
    __shared__ double sbest[kThreads];
    __shared__ uint32_t skk[kThreads];
    __shared__ int c1_nan;
    const Range r = ranges[blockIdx.x];
    const uint32_t a = r.a, m = r.b - r.a, t = threadIdx.x;
    // the whole range
    DBox acc;
    int has = 0;
    for (uint32_t j = t; j < m; j += kThreads) {
        const DBox b = load_box(leaf_box, a + j);
        acc = has ? box_union(acc, b) : b;
        has = 1;
    }
    block_scan_boxes(acc, has, false, sb, sh);
    __shared__ DBox all_s;
    if (t == kThreads - 1) all_s = acc;
    __syncthreads();
    const DBox all = all_s;
    const double sa = box_sa(all);
    const bool emit = r.parent_sa < 0.0 || sa < prune * r.parent_sa;
    // suffix areas: suffix_sa[a + k] = SA(leaves [a + k, b)), k >= 1
    constexpr uint32_t kChunk = kThreads * kCullItems;
    const uint32_t nchunks = (m + kChunk - 1) / kChunk;
    DBox carry;
    int carry_has = 0;
    for (uint32_t c = nchunks; c-- > 0;) {
        const uint32_t lo = c * kChunk + t * kCullItems, hi = lo + kCullItems < m ? lo + kCullItems : m;
        DBox tot;
        int th = 0;
        for (uint32_t j = lo; j < hi; j++) { const DBox b = load_box(leaf_box, a + j); tot = th ? box_union(tot, b) : b; th = 1; }
        DBox incl = tot;
        int ih = th;
        block_scan_boxes(incl, ih, true, sb, sh);           // this lane and every later lane of the chunk
        __shared__ DBox chunk_all;
        __shared__ int chunk_has;
        if (t == 0) { chunk_all = incl; chunk_has = ih; }
        // what follows this lane's leaves: later lanes (inclusive minus own: recomputed by walking) and later chunks
        DBox run = carry;
        int rh = carry_has;
        if (t + 1 < kThreads) {                             // the later lanes' part: the backward scan value of lane t + 1
            sb[t] = incl; sh[t] = ih;
        }
        __syncthreads();
        if (t + 1 < kThreads && sh[t + 1]) { run = rh ? box_union(sb[t + 1], run) : sb[t + 1]; rh = 1; }
        for (uint32_t j = hi; j-- > lo;) {
            const DBox b = load_box(leaf_box, a + j);
            run = rh ? box_union(b, run) : b;
            rh = 1;
            if (j >= 1) suffix_sa[a + j] = box_sa(run);
        }
        __syncthreads();
        if (chunk_has) { carry = carry_has ? box_union(chunk_all, carry) : chunk_all; carry_has = 1; }
        __syncthreads();
    }
    __syncthreads();
    // prefix areas, costs and the host's choice: k = 1 if c(1) is NaN, else the first k of the smallest non-NaN cost
    if (t == 0) c1_nan = 0;
    double best = 0.0;
    uint32_t best_k = 0;                                     // 0: none yet
    carry_has = 0;
    for (uint32_t c = 0; c < nchunks; c++) {
        const uint32_t lo = c * kChunk + t * kCullItems, hi = lo + kCullItems < m ? lo + kCullItems : m;
        DBox tot;
        int th = 0;
        for (uint32_t j = lo; j < hi; j++) { const DBox b = load_box(leaf_box, a + j); tot = th ? box_union(tot, b) : b; th = 1; }
        DBox incl = tot;
        int ih = th;
        block_scan_boxes(incl, ih, false, sb, sh);
        __shared__ DBox chunk_all;
        __shared__ int chunk_has;
        if (t == kThreads - 1) { chunk_all = incl; chunk_has = ih; }
        DBox run = carry;
        int rh = carry_has;
        sb[t] = incl; sh[t] = ih;
        __syncthreads();
        if (t > 0 && sh[t - 1]) { run = rh ? box_union(run, sb[t - 1]) : sb[t - 1]; rh = 1; }
        for (uint32_t j = lo; j < hi; j++) {
            const DBox b = load_box(leaf_box, a + j);
            run = rh ? box_union(run, b) : b;
            rh = 1;
            const uint32_t k = j + 1;
            if (k < m) {
                const double cost = box_sa(run) * k + suffix_sa[a + k] * (m - k);
                if (k == 1 && cost != cost) c1_nan = 1;
                if (cost == cost && (best_k == 0 || cost < best)) { best = cost; best_k = k; }
            }
        }
        __syncthreads();
        if (chunk_has) { carry = carry_has ? box_union(carry, chunk_all) : chunk_all; carry_has = 1; }
        __syncthreads();
    }
    sbest[t] = best; skk[t] = best_k;
    __syncthreads();
    for (uint32_t off = kThreads / 2; off > 0; off >>= 1) {
        if (t < off) {
            const uint32_t k2 = skk[t + off];
            const double b2 = sbest[t + off];
            if (k2 != 0 && (skk[t] == 0 || b2 < sbest[t] || (b2 == sbest[t] && k2 < skk[t]))) { sbest[t] = b2; skk[t] = k2; }
        }
        __syncthreads();
    }
    if (t == 0) {
        const uint32_t k = (c1_nan || skk[0] == 0) ? 1u : skk[0];
        if (emit) emit_record(recs, flags, a, r.b, r.chain, -1, all);
        const double child_sa = emit ? sa : r.parent_sa;
        route_range(Range{a, a + k, r.chain + (emit ? 1u : 0u), 0u, child_sa}, next, small, flags);
        route_range(Range{a + k, r.b, 0u, 0u, child_sa}, next, small, flags);
    }
}

// CullBuilder::build_serial over a range of at most kCullSerialMax leaves, one lane per range (the host's loop and fold order).
// Pending ranges are disjoint parts of the lane's range: their stack lives at stack[a ...].
__global__ void __launch_bounds__(kThreads) cull_serial_kernel(const Range* ranges, uint32_t count, Range* stack, CullRec* recs, uint32_t* flags,
                                                               uint32_t* chain_count, const float* leaf_box, double* suffix_sa, double prune) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= count) return;
    const uint32_t base = ranges[i].a;
    uint32_t sp = 0;
    stack[base + sp++] = ranges[i];
    while (sp > 0) {
        const Range f = stack[base + --sp];
        const uint32_t a = f.a, b = f.b, m = b - a;
        DBox all = load_box(leaf_box, a);
        for (uint32_t k = a + 1; k < b; k++) all = box_union(all, load_box(leaf_box, k));
        if (m == 1) {
            emit_record(recs, flags, a, b, f.chain, (int32_t)a, all);
            chain_count[a] = f.chain + 1;
            continue;
        }
        const double sa = box_sa(all);
        const bool emit = f.parent_sa < 0.0 || sa < prune * f.parent_sa;
        DBox suf = load_box(leaf_box, b - 1);
        suffix_sa[b - 1] = box_sa(suf);
        for (uint32_t k = m - 1; k-- > 1;) { suf = box_union(load_box(leaf_box, a + k), suf); suffix_sa[a + k] = box_sa(suf); }
        DBox prefix = load_box(leaf_box, a);
        double best = 0.0;
        uint32_t kbest = 1;
        for (uint32_t k = 1; k < m; k++) {
            const double c = box_sa(prefix) * k + suffix_sa[a + k] * (m - k);
            if (k == 1 || c < best) { best = c; kbest = k; }
            prefix = box_union(prefix, load_box(leaf_box, a + k));
        }
        if (emit) emit_record(recs, flags, a, b, f.chain, -1, all);
        const double child_sa = emit ? sa : f.parent_sa;
        stack[base + sp++] = Range{a + kbest, b, 0u, 0u, child_sa};
        stack[base + sp++] = Range{a, a + kbest, f.chain + (emit ? 1u : 0u), 0u, child_sa};
    }
}

__global__ void __launch_bounds__(kThreads) cull_place_kernel(const CullRec* recs, uint32_t count, const uint32_t* S, const uint32_t* perm,
                                                              float* cull_box, int32_t* cull_prim, int32_t* cull_skip, int32_t* cull_leaf) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= count) return;
    const CullRec r = recs[i];
    const uint32_t idx = S[r.a] + r.chain;
    if (idx >= count) return;                                // (cannot happen: the host compares the record count with S[n] first)
    store_box(cull_box, idx, r.box);
    cull_skip[idx] = (int32_t)(r.leaf >= 0 ? idx + 1 : S[r.b]);
    cull_leaf[idx] = r.leaf;
    cull_prim[idx] = r.leaf >= 0 ? (int32_t)perm[r.leaf] : -1;
}

// ---- packing ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) pack_primitives_kernel(const Geometry* geo, uint32_t ng, const uint32_t* sphere_before,
                                                                   uint32_t* link_of_geo, float4* f4, uint32_t* u32, SceneLayout L) {
    const uint32_t g = blockIdx.x * kThreads + threadIdx.x;
    if (g >= ng) return;
    const Geometry gg = geo[g];
    DBox box;
    float4 rec[5];
    bool finite;
    eval_primitive(gg, box, rec, finite);
    if (gg.kind == 0) {
        const uint32_t li = sphere_before[g];
        f4[L.off_sphere + li] = rec[0];
        u32[L.off_sphere_mat + li] = gg.material;
        link_of_geo[g] = li;
    } else {
        const uint32_t li = g - sphere_before[g];
        for (int j = 0; j < 5; j++) f4[L.off_quad + 5 * (size_t)li + j] = rec[j];
        link_of_geo[g] = li | PRIM_QUAD_BIT;
    }
}
// pack_nodes of compile_scene (identity placement): a leaf's link is its primitive reference, an inner node's NODE_INNER_BIT | i + 1
__global__ void __launch_bounds__(kThreads) pack_nodes_kernel(const float* box6, const int32_t* prim, const int32_t* skip, uint32_t n,
                                                              const uint32_t* link_of_geo, float4* dst) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const DBox b = load_box(box6, i);
    const uint32_t sk = (uint32_t)skip[i] >= n ? n : (uint32_t)skip[i];
    const uint32_t link = prim[i] >= 0 ? link_of_geo[prim[i]] : (NODE_INNER_BIT | (i + 1 >= n ? n : i + 1));
    dst[2 * (size_t)i] = make_float4(b.lo[0], b.lo[1], b.lo[2], b.hi[0]);
    dst[2 * (size_t)i + 1] = make_float4(b.hi[1], b.hi[2], bits_to_f32(sk), bits_to_f32(link));
}
// the leaf list (skip = successor) and its kLeafListPad copies of the last leaf
__global__ void __launch_bounds__(kThreads) pack_leaf_list_kernel(const float* leaf_box, const uint32_t* perm, uint32_t nl,
                                                                  const uint32_t* link_of_geo, float4* dst) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= nl + kLeafListPad) return;
    const uint32_t k = i < nl ? i : nl - 1;
    const DBox b = load_box(leaf_box, k);
    dst[2 * (size_t)i] = make_float4(b.lo[0], b.lo[1], b.lo[2], b.hi[0]);
    dst[2 * (size_t)i + 1] = make_float4(b.hi[1], b.hi[2], bits_to_f32(k + 1), bits_to_f32(link_of_geo[perm[k]]));
}
__global__ void __launch_bounds__(kThreads) pack_compact_kernel(const float* cull_box, const int32_t* cull_skip, const int32_t* cull_leaf,
                                                                uint32_t nc, bool all_finite, uint32_t* dst) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= nc) return;
    const DBox root = load_box(cull_box, 0);
    float eps[3], limit[3];
    compact_eps_rule(root.lo, root.hi, all_finite, eps, limit);
    const DBox b = load_box(cull_box, i);
    // an inner node's link is its skip node's BYTE offset in this array (box_loop_compact)
    const uint32_t link = cull_leaf[i] >= 0 ? (0x80000000u | (uint32_t)cull_leaf[i]) : (uint32_t)cull_skip[i] << 4;
    uint32_t w[4];
    compact_node_words(b.lo, b.hi, eps, link, w);
    for (int j = 0; j < 4; j++) dst[4 * (size_t)i + j] = w[j];
}

__global__ void __launch_bounds__(kThreads) iota_kernel(uint32_t* o, uint32_t n) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n) o[i] = i;
}

// ---- host side ----------------------------------------------------------------------------------------------------------
inline uint32_t blocks_for(size_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

struct HipError { hipError_t e; const char* what; };
inline void hip_check(hipError_t e, const char* what) { if (e != hipSuccess) throw HipError{e, what}; }
#define BUILD_HIP(call) hip_check((call), #call)

// Every device buffer of one build; freed on every path out (the blob only if it was not handed to the scene)
struct Scratch {
    std::vector<void*> ptrs;
    template <typename T>
    T* alloc(size_t count) {
        void* p = nullptr;
        const hipError_t e = hipMalloc(&p, count * sizeof(T) > 0 ? count * sizeof(T) : 16);
        if (e != hipSuccess) { (void)hipGetLastError(); throw std::bad_alloc(); }
        ptrs.push_back(p);
        return static_cast<T*>(p);
    }
    void release(void* p) {
        for (void*& q : ptrs) if (q == p) q = nullptr;
    }
    ~Scratch() { for (void* p : ptrs) if (p) (void)hipFree(p); }
};

struct Builder {
    hipStream_t st;
    Scratch& mem;
    uint32_t* scan_scratch = nullptr;      // tile sums of every scan level

    // exclusive scan of n u32 (in place allowed); `tmp`: scan_scratch space from here on
    void scan(const uint32_t* in, uint32_t* out, size_t n, uint32_t* tmp) {
        const uint32_t nb = blocks_for(n, kScanTile);
        hipLaunchKernelGGL(scan_tiles_kernel, dim3(nb), dim3(kThreads), 0, st, in, out, (uint32_t)n, tmp);
        BUILD_HIP(hipGetLastError());
        if (nb > 1) {
            scan(tmp, tmp, nb, tmp + nb);
            hipLaunchKernelGGL(scan_add_kernel, dim3(nb), dim3(kThreads), 0, st, out, (uint32_t)n, (const uint32_t*)tmp);
            BUILD_HIP(hipGetLastError());
        }
    }
    static size_t scan_scratch_size(size_t n) {
        size_t total = 0;
        for (size_t m = n; m > 1;) { m = (m + kScanTile - 1) / kScanTile; total += m; }
        return total + 4;
    }
    template <typename T>
    T read_back(const T* d) {
        T v;
        BUILD_HIP(hipMemcpyAsync(&v, d, sizeof(T), hipMemcpyDeviceToHost, st));
        BUILD_HIP(hipStreamSynchronize(st));
        return v;
    }
};

int build_on_device(const World& w, const trt_scene_options& opt, hipStream_t st, Scratch& mem, SceneHost& out, void*& d_blob_out) {
    const uint32_t ng = (uint32_t)w.geometries.size(), nm = (uint32_t)w.materials.size();
    Builder B{st, mem};
    B.scan_scratch = mem.alloc<uint32_t>(Builder::scan_scratch_size((size_t)ng + 1) + Builder::scan_scratch_size(256ull * blocks_for(ng, kSortTile)));

    // 1. primitives
    Geometry* d_geo = mem.alloc<Geometry>(ng);
    float* prim_box = mem.alloc<float>(6ull * ng);
    uint32_t* is_sphere = mem.alloc<uint32_t>(ng + 1ull);
    uint32_t* sphere_before = mem.alloc<uint32_t>(ng + 1ull);
    uint32_t* flags = mem.alloc<uint32_t>(N_FLAGS);
    BUILD_HIP(hipMemcpyAsync(d_geo, w.geometries.data(), sizeof(Geometry) * (size_t)ng, hipMemcpyHostToDevice, st));
    timing_mark(st, true);
    BUILD_HIP(hipMemsetAsync(flags, 0, sizeof(uint32_t) * N_FLAGS, st));
    BUILD_HIP(hipMemsetAsync(is_sphere + ng, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(primitive_kernel, dim3(blocks_for(ng, kThreads)), dim3(kThreads), 0, st, (const Geometry*)d_geo, ng, nm, prim_box, is_sphere, flags);
    BUILD_HIP(hipGetLastError());
    B.scan(is_sphere, sphere_before, (size_t)ng + 1, B.scan_scratch);

    // 2-3. reference tree
    const uint32_t nn = 2 * ng - 1;
    float* ref_box = mem.alloc<float>(6ull * nn);
    int32_t* ref_prim = mem.alloc<int32_t>(nn);
    int32_t* ref_skip = mem.alloc<int32_t>(nn);
    uint32_t* keyA = mem.alloc<uint32_t>(ng);
    uint32_t* segA = mem.alloc<uint32_t>(ng);
    uint32_t* valA = mem.alloc<uint32_t>(ng);
    uint32_t* keyB = mem.alloc<uint32_t>(ng);
    uint32_t* segB = mem.alloc<uint32_t>(ng);
    uint32_t* valB = mem.alloc<uint32_t>(ng);
    uint32_t* perm = mem.alloc<uint32_t>(ng);
    uint32_t local_level = 0;                                    // first level whose segments all fit one workgroup
    while ((((uint64_t)ng + (1ull << local_level) - 1) >> local_level) > kRefLocalMax) local_level++;
    const uint32_t sort_blocks = blocks_for(ng, kSortTile);
    uint32_t* hist = mem.alloc<uint32_t>(256ull * sort_blocks);
    uint8_t* seg_axis = mem.alloc<uint8_t>(1ull << (local_level > 0 ? local_level - 1 : 0));
    uint32_t* order = valB;                                     // BVH::new (bvh.rs:12-22): objects in insertion order
    hipLaunchKernelGGL(iota_kernel, dim3(blocks_for(ng, kThreads)), dim3(kThreads), 0, st, order, ng);
    BUILD_HIP(hipGetLastError());
    for (uint32_t level = 0; level < local_level; level++) {
        hipLaunchKernelGGL(ref_level_box_kernel, dim3(1u << level), dim3(kThreads), 0, st, ng, level, (const uint32_t*)order, (const float*)prim_box,
                           ref_box, ref_prim, ref_skip, seg_axis);
        BUILD_HIP(hipGetLastError());
        hipLaunchKernelGGL(ref_level_keys_kernel, dim3(blocks_for(ng, kThreads)), dim3(kThreads), 0, st, ng, level, (const uint32_t*)order,
                           (const float*)prim_box, (const uint8_t*)seg_axis, keyA, segA, valA);
        BUILD_HIP(hipGetLastError());
        uint32_t *ki = keyA, *si = segA, *vi = valA, *ko = keyB, *so = segB, *vo = valB;
        const uint32_t passes = 4 + (level + 7) / 8;
        for (uint32_t pass = 0; pass < passes; pass++) {
            hipLaunchKernelGGL(radix_hist_kernel, dim3(sort_blocks), dim3(kThreads), 0, st, (const uint32_t*)ki, (const uint32_t*)si, ng, pass, hist, sort_blocks);
            BUILD_HIP(hipGetLastError());
            B.scan(hist, hist, 256ull * sort_blocks, B.scan_scratch);
            hipLaunchKernelGGL(radix_scatter_kernel, dim3(sort_blocks), dim3(kThreads), 0, st, (const uint32_t*)ki, (const uint32_t*)si,
                               (const uint32_t*)vi, ko, so, vo, ng, pass, (const uint32_t*)hist, sort_blocks);
            BUILD_HIP(hipGetLastError());
            std::swap(ki, ko); std::swap(si, so); std::swap(vi, vo);
        }
        order = vi;                                              // (the next level's keys kernel may write over it in place: same index)
    }
    hipLaunchKernelGGL(ref_local_kernel, dim3(1u << local_level), dim3(kThreads), 0, st, ng, local_level, (const uint32_t*)order,
                       (const float*)prim_box, ref_box, ref_prim, ref_skip, perm);
    BUILD_HIP(hipGetLastError());

    // 4. culling tree over the leaf sequence perm
    const uint32_t nl = ng;
    float* leaf_box = mem.alloc<float>(6ull * nl);
    hipLaunchKernelGGL(gather_leaves_kernel, dim3(blocks_for(nl, kThreads)), dim3(kThreads), 0, st, (const uint32_t*)perm, nl, (const float*)prim_box, leaf_box);
    BUILD_HIP(hipGetLastError());
    Range* listA = mem.alloc<Range>(nl);
    Range* listB = mem.alloc<Range>(nl);
    Range* small = mem.alloc<Range>(nl);
    Range* stack = mem.alloc<Range>(nl);
    CullRec* recs = mem.alloc<CullRec>(2ull * nl);
    uint32_t* chain_count = mem.alloc<uint32_t>(nl + 1ull);
    double* suffix_sa = mem.alloc<double>(nl + 1ull);
    BUILD_HIP(hipMemsetAsync(chain_count, 0, sizeof(uint32_t) * (nl + 1ull), st));
    const double prune = opt.cull_prune > 0.0f ? (double)opt.cull_prune : 0.5;
    const Range root{0u, nl, 0u, 0u, -1.0};
    uint32_t nsmall = 0;
    if (nl <= kCullSerialMax) {
        BUILD_HIP(hipMemcpyAsync(small, &root, sizeof(Range), hipMemcpyHostToDevice, st));
        nsmall = 1;
    } else {
        BUILD_HIP(hipMemcpyAsync(listA, &root, sizeof(Range), hipMemcpyHostToDevice, st));
        uint32_t count = 1;
        while (count > 0) {
            BUILD_HIP(hipMemsetAsync(flags + CTR_NEXT, 0, sizeof(uint32_t), st));
            hipLaunchKernelGGL(cull_level_kernel, dim3(count), dim3(kThreads), 0, st, (const Range*)listA, listB, small, recs, flags,
                               (const float*)leaf_box, suffix_sa, prune);
            BUILD_HIP(hipGetLastError());
            count = B.read_back(flags + CTR_NEXT);
            std::swap(listA, listB);
        }
        nsmall = B.read_back(flags + CTR_SMALL);
    }
    hipLaunchKernelGGL(cull_serial_kernel, dim3(blocks_for(nsmall, kThreads)), dim3(kThreads), 0, st, (const Range*)small, nsmall, stack, recs,
                       flags, chain_count, (const float*)leaf_box, suffix_sa, prune);
    BUILD_HIP(hipGetLastError());
    uint32_t* S = chain_count;
    B.scan(chain_count, S, nl + 1ull, B.scan_scratch);
    uint32_t host_flags[N_FLAGS];
    BUILD_HIP(hipMemcpyAsync(host_flags, flags, sizeof(host_flags), hipMemcpyDeviceToHost, st));
    uint32_t ns = 0, nc = 0;
    BUILD_HIP(hipMemcpyAsync(&ns, sphere_before + ng, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    BUILD_HIP(hipMemcpyAsync(&nc, S + nl, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    BUILD_HIP(hipStreamSynchronize(st));
    if (host_flags[FLAG_BAD_MATERIAL]) return scene_fail(TRT_ERR_INVALID_ARG, "geometry refers to a material index that does not exist");
    if (nc != host_flags[CTR_RECORDS] || nc == 0 || nc > 2 * nl - 1)
        return scene_fail(TRT_ERR_HIP, "device scene compiler: inconsistent culling tree (" + std::to_string(nc) + " nodes placed, " +
                                       std::to_string(host_flags[CTR_RECORDS]) + " emitted)");
    const bool all_finite = host_flags[FLAG_NOT_FINITE] == 0;
    float* cull_box = mem.alloc<float>(6ull * nc);
    int32_t* cull_prim = mem.alloc<int32_t>(nc);
    int32_t* cull_skip = mem.alloc<int32_t>(nc);
    int32_t* cull_leaf = mem.alloc<int32_t>(nc);
    hipLaunchKernelGGL(cull_place_kernel, dim3(blocks_for(nc, kThreads)), dim3(kThreads), 0, st, (const CullRec*)recs, nc, (const uint32_t*)S,
                       (const uint32_t*)perm, cull_box, cull_prim, cull_skip, cull_leaf);
    BUILD_HIP(hipGetLastError());

    // 5. layout and packing
    std::string msg;
    SceneLayout& L = out.layout;
    if (!scene_layout(w, opt, ns, ng - ns, nn, nc, all_finite, L, msg)) return scene_fail(TRT_ERR_INVALID_ARG, msg);
    uint8_t* blob = mem.alloc<uint8_t>(L.blob_bytes);
    float4* f4 = reinterpret_cast<float4*>(blob);
    uint32_t* u32 = reinterpret_cast<uint32_t*>(blob);
    uint32_t* link_of_geo = mem.alloc<uint32_t>(ng);
    BUILD_HIP(hipMemsetAsync(blob, 0, L.blob_bytes, st));
    hipLaunchKernelGGL(pack_primitives_kernel, dim3(blocks_for(ng, kThreads)), dim3(kThreads), 0, st, (const Geometry*)d_geo, ng,
                       (const uint32_t*)sphere_before, link_of_geo, f4, u32, L);
    BUILD_HIP(hipGetLastError());
    hipLaunchKernelGGL(pack_nodes_kernel, dim3(blocks_for(nc, kThreads)), dim3(kThreads), 0, st, (const float*)cull_box, (const int32_t*)cull_prim,
                       (const int32_t*)cull_skip, nc, (const uint32_t*)link_of_geo, f4);
    BUILD_HIP(hipGetLastError());
    hipLaunchKernelGGL(pack_nodes_kernel, dim3(blocks_for(nn, kThreads)), dim3(kThreads), 0, st, (const float*)ref_box, (const int32_t*)ref_prim,
                       (const int32_t*)ref_skip, nn, (const uint32_t*)link_of_geo, f4 + L.off_ref_nodes);
    BUILD_HIP(hipGetLastError());
    hipLaunchKernelGGL(pack_leaf_list_kernel, dim3(blocks_for(nl + kLeafListPad, kThreads)), dim3(kThreads), 0, st, (const float*)leaf_box,
                       (const uint32_t*)perm, nl, (const uint32_t*)link_of_geo, f4 + L.off_leaf_list);
    BUILD_HIP(hipGetLastError());
    if (L.off_compact) {
        hipLaunchKernelGGL(pack_compact_kernel, dim3(blocks_for(nc, kThreads)), dim3(kThreads), 0, st, (const float*)cull_box, (const int32_t*)cull_skip,
                           (const int32_t*)cull_leaf, nc, all_finite, u32 + 4ull * L.off_compact);
        BUILD_HIP(hipGetLastError());
    }
    // materials: O(materials), from the host
    std::vector<float4> mat4(nm);
    std::vector<uint32_t> matk(nm);
    for (uint32_t i = 0; i < nm; i++) {
        const trt_material& m = w.materials[i];
        mat4[i] = make_float4(m.albedo.x, m.albedo.y, m.albedo.z, m.param);
        matk[i] = m.kind;
    }
    if (nm) {
        BUILD_HIP(hipMemcpyAsync(f4 + L.off_material, mat4.data(), sizeof(float4) * nm, hipMemcpyHostToDevice, st));
        BUILD_HIP(hipMemcpyAsync(u32 + L.off_material_kind, matk.data(), sizeof(uint32_t) * nm, hipMemcpyHostToDevice, st));
    }
    timing_mark(st, false);

    // copy-back: the blob and both node dumps
    out.blob.resize(L.blob_bytes);
    out.reference.bbox6.resize(6ull * nn); out.reference.prim_geo.resize(nn); out.reference.skip.resize(nn);
    out.culling.bbox6.resize(6ull * nc); out.culling.prim_geo.resize(nc); out.culling.skip.resize(nc);
    BUILD_HIP(hipMemcpyAsync(out.blob.data(), blob, L.blob_bytes, hipMemcpyDeviceToHost, st));
    BUILD_HIP(hipMemcpyAsync(out.reference.bbox6.data(), ref_box, sizeof(float) * 6ull * nn, hipMemcpyDeviceToHost, st));
    BUILD_HIP(hipMemcpyAsync(out.reference.prim_geo.data(), ref_prim, sizeof(int32_t) * nn, hipMemcpyDeviceToHost, st));
    BUILD_HIP(hipMemcpyAsync(out.reference.skip.data(), ref_skip, sizeof(int32_t) * nn, hipMemcpyDeviceToHost, st));
    BUILD_HIP(hipMemcpyAsync(out.culling.bbox6.data(), cull_box, sizeof(float) * 6ull * nc, hipMemcpyDeviceToHost, st));
    BUILD_HIP(hipMemcpyAsync(out.culling.prim_geo.data(), cull_prim, sizeof(int32_t) * nc, hipMemcpyDeviceToHost, st));
    BUILD_HIP(hipMemcpyAsync(out.culling.skip.data(), cull_skip, sizeof(int32_t) * nc, hipMemcpyDeviceToHost, st));
    BUILD_HIP(hipStreamSynchronize(st));
    if (L.off_compact) {
        const float* rb = out.culling.bbox6.data();
        float eps[3];
        compact_eps_rule(rb, rb + 3, all_finite, eps, L.compact_origin_limit);
    }
    out.max_depth = reference_max_depth(ng);
    mem.release(blob);
    d_blob_out = blob;
    return TRT_OK;
}

}  // namespace
}  // namespace trt

using namespace trt;

int trt_scene_create_on_device(const trt_world* w, const trt_scene_options* options, trt_scene** out) {
    if (!w || !out) return scene_fail(TRT_ERR_INVALID_ARG, "null argument");
    try {
        const trt_scene_options opt = scene_options_or_defaults(options);
        if (scene_options_check(opt) != TRT_OK) return TRT_ERR_INVALID_ARG;
        const World& world = world_of(w);
        const size_t ng = world.geometries.size();
        if (ng == 0) return scene_fail(TRT_ERR_INVALID_ARG, "world has no geometry");
        if (ng > PRIM_INDEX_MASK) return scene_fail(TRT_ERR_INVALID_ARG, "too many geometries");
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
            (void)hipGetLastError();
            return scene_fail(TRT_ERR_NO_DEVICE, "no HIP device visible: the device scene compiler needs a gfx950 GPU");
        }
        int device = 0;
        hipError_t e = hipGetDevice(&device);
        if (e != hipSuccess) return scene_fail(TRT_ERR_HIP, std::string("hipGetDevice: ") + hipGetErrorString(e));
        hipStream_t st = nullptr;
        e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
        if (e != hipSuccess) { (void)hipGetLastError(); return scene_fail(TRT_ERR_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e)); }
        int rc = TRT_OK;
        SceneHost host;
        void* d_blob = nullptr;
        {
            Scratch mem;
            try {
                rc = build_on_device(world, opt, st, mem, host, d_blob);
            } catch (const HipError& he) {
                (void)hipGetLastError();
                rc = scene_fail(TRT_ERR_HIP, std::string("device scene compiler: ") + he.what + ": " + hipGetErrorString(he.e));
            } catch (const std::bad_alloc&) {
                rc = scene_fail(TRT_ERR_OOM, "device scene compiler: out of device or host memory");
            }
            (void)hipStreamSynchronize(st);                      // nothing of this build may still run when its scratch is freed
        }
        (void)hipStreamDestroy(st);
        if (rc != TRT_OK) {
            if (d_blob) (void)hipFree(d_blob);
            return rc;
        }
        trt_scene* s = scene_adopt(std::move(host), opt, device, d_blob);
        if (!s) { (void)hipFree(d_blob); return TRT_ERR_OOM; }
        *out = s;
    } catch (const std::bad_alloc&) {
        return scene_fail(TRT_ERR_OOM, "out of memory");
    } catch (const std::exception& ex) {
        return scene_fail(TRT_ERR_INVALID_ARG, std::string("scene compilation failed: ") + ex.what());
    }
    return TRT_OK;
}
