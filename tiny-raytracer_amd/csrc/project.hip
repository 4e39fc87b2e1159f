// project.hip — the probe fold of sample records (tinyrt.h trt_project_samples / trt_project_samples_device) and the probe query built on
// it (trt_probe_parallel / trt_probe_parallel_device), written for gfx950 (CDNA4) only.
//
// trt_probe (probe.hip) lets a lane own an ITEM for all K samples of the call, so a bake of few probes with many samples runs on few
// lanes.  The sample queries (samples.hip) trace the same paths a SAMPLE to a lane and write every sample's colour c and stored first
// direction d; this unit folds those records as the probe contract folds them,
//   t = b_k(d) * inv_K;   sh[k].ch = sh[k].ch + c.ch * t        for k < C = bands^2
// over the samples of the range in order, one IEEE f32 operation per operator (the basis is sh_basis.h's, the one copy): 3 C serial
// chains per item.  A sample whose direction has a NaN component, and every sample of an item whose point has one, is SKIPPED - it adds
// neither 0 nor NaN, and sums no sample touches keep their bits.  Two regimes, one host rule (project_by_wave), the same bytes:
//   tile  a lane owns an item and its 3 C sums; a wave loads the colours and directions of its 64 items coalesced, 8 samples of each at a
//         time, into LDS rows of 49 floats and every lane reads its own row back (fold_tile_kernel's transposition, for both buffers);
//   wave  a wave owns an item: 64 consecutive records are loaded coalesced, a record to a lane; the lane forms the record's C values of t
//         and 3 C products and stores them as a row of a 64 x 3 C array in LDS; lane q < 3 C then adds column q, rows 0 .. 63 in order,
//         to chain q.  The chains run side by side in 3 C lanes where fold_wave_kernel's scheme would run them one after another in
//         every lane.
// trt_probe_parallel runs chunks of items through a record buffer (probe_chunks.h): the sample kernels (samples.hip launch_samples, the
// one copy of that launch), then the projection of the chunk into its rows of `sh`.
#include "host_stage.h"
#include "kernels.h"
#include "probe_call.h"
#include "probe_chunks.h"
#include "query_plan.h"
#include "rt_device.h"
#include "sample_index.h"
#include "samples_call.h"
#include "scene_query.h"
#include "sh_basis.h"

namespace trt {

struct ProjectArgs {
    const float* colors;             // n x K x 3
    const float* directions;         // n x K x 3
    const float* items;              // n x (point, axis), or nullptr: no item is skipped for its point
    float* sh;                       // n x C x 3
    uint32_t n, samples_per_item;    // K
    uint32_t sample_begin, range_length;     // [b, b + R), R >= 1
    uint32_t accumulate;
    float inv_k;                     // 1.0f / float(K)
};

TRT_DEV bool any_nan(const V3& v) { return v.x != v.x || v.y != v.y || v.z != v.z; }

// The 3 NC terms of one record in the contract's parenthesisation: term[3 k + ch] = c.ch * (b_k(d) * inv_K).
template <int NC>
TRT_DEV void project_terms(float (&term)[3 * NC], const V3& d, const V3& c, float inv_k) {
    float b[NC];
    sh_basis<NC>(b, d);
#pragma unroll
    for (int k = 0; k < NC; k++) {
        const float t = b[k] * inv_k;
        term[3 * k + 0] = c.x * t;
        term[3 * k + 1] = c.y * t;
        term[3 * k + 2] = c.z * t;
    }
}

constexpr uint32_t kProjChunk = 8u;                                        // samples of an item in LDS at a time
constexpr uint32_t kProjHalf = 3u * kProjChunk;                            // floats of a row's colours; its directions follow them
constexpr uint32_t kProjRow = 2u * kProjHalf + 1u;                         // floats between two rows: odd, so that 64 rows meet 64 banks
static_assert(4u * 64u * kProjRow * sizeof(float) <= 50176u, "a workgroup's LDS stays at fold_tile_kernel's: three workgroups fit a CU");
static_assert(kProjHalf <= 48u, "fold_row (sample_index.h) is exact for rows of at most 48 floats");

// Tile regime: lane l of wave w owns item (blockIdx.x * 4 + w) * 64 + l.  The four waves of a workgroup work on their own quarter of the
// LDS; the barriers only order a wave's own writes and reads, and every wave passes the same number of them (R is uniform).
template <int NC>
__global__ __launch_bounds__(256) void project_tile_kernel(ProjectArgs pa) {
    __shared__ float tile[4u * 64u * kProjRow];
    const uint32_t lane = threadIdx.x & 63u;
    float* const rows = tile + (threadIdx.x >> 6) * (64u * kProjRow);
    const unsigned long long first = (blockIdx.x * 4ull + (threadIdx.x >> 6)) * 64ull;      // the wave's first item, in 64 bits
    const unsigned long long mine = first + lane;
    const bool own = mine < pa.n;
    bool live = own;                                                        // the item's samples fold: its point has no NaN
    float acc[3 * NC];
#pragma unroll
    for (int j = 0; j < 3 * NC; j++) acc[j] = 0.0f;
    if (own) {                                                              // mine < n: within [0, 6 n) and [0, 3 NC n)
        if (pa.items) {
            const float* const o = pa.items + 6ull * mine;
            live = !any_nan(v3(o[0], o[1], o[2]));
        }
        if (pa.accumulate) {
            const float* const a = pa.sh + (3ull * NC) * mine;
#pragma unroll
            for (int j = 0; j < 3 * NC; j++) acc[j] = a[j];
        }
    }
    for (uint32_t c0 = 0; c0 < pa.range_length; c0 += kProjChunk) {
        const uint32_t cs = pa.range_length - c0 < kProjChunk ? pa.range_length - c0 : kProjChunk;
        const uint32_t len = 3u * cs, magic = fold_row_magic(len);         // floats of a row's part of either buffer in this chunk: 3 .. 24
        for (uint32_t e = lane; e < 64u * len; e += 64u) {
            const uint32_t row = fold_row(e, magic), col = e - row * len;
            const unsigned long long item = first + row;
            // item < n, sample_begin + c0 + col / 3 < sample_begin + R <= K: within [0, 3 n K) of both buffers
            if (item < pa.n) {
                const unsigned long long at = 3ull * (item * pa.samples_per_item + pa.sample_begin + c0) + col;
                rows[row * kProjRow + col] = pa.colors[at];
                rows[row * kProjRow + kProjHalf + col] = pa.directions[at];
            }
        }
        __syncthreads();
        if (live) {
            const float* const r = rows + lane * kProjRow;
            for (uint32_t k = 0; k < cs; k++) {
                const V3 c = v3(r[3u * k], r[3u * k + 1u], r[3u * k + 2u]);
                const V3 d = v3(r[kProjHalf + 3u * k], r[kProjHalf + 3u * k + 1u], r[kProjHalf + 3u * k + 2u]);
                if (!any_nan(d)) {
                    float term[3 * NC];
                    project_terms<NC>(term, d, c, pa.inv_k);
#pragma unroll
                    for (int j = 0; j < 3 * NC; j++) acc[j] = acc[j] + term[j];
                }
            }
        }
        __syncthreads();
    }
    if (own) {
        float* const a = pa.sh + (3ull * NC) * mine;
#pragma unroll
        for (int j = 0; j < 3 * NC; j++) a[j] = acc[j];
    }
}

// Wave regime: workgroup = wave = item blockIdx.x (the grid has n of them).  Lane l holds record b + c0 + l of the item and stores its
// 3 NC terms as row l; lane q < 3 NC owns chain q and adds column q of the rows that fold, in record order.  Which rows fold is a ballot:
// a chain SKIPS a row that does not (x + 0 is not x for x = -0, and 0 * inf is NaN), and only a load whose 64 rows all fold takes the
// straight-line form, where the row offsets are literals and the LDS reads run ahead of the one dependent chain of additions.  The next
// load's records are fetched before the current one's chain, so the memory latency hides behind it.
template <int NC>
__global__ __launch_bounds__(64) void project_wave_kernel(ProjectArgs pa) {
    constexpr uint32_t kChains = 3u * NC;
    constexpr uint32_t kStride = kChains | 1u;                              // floats between two rows: odd (27, 13, 3)
    __shared__ float terms[64u * kStride];
    const uint32_t lane = threadIdx.x;
    const unsigned long long item = blockIdx.x;                             // < n
    bool live = true;                                                       // wave-uniform: every lane reads the same point
    if (pa.items) {
        const float* const o = pa.items + 6ull * item;
        live = !any_nan(v3(o[0], o[1], o[2]));
    }
    float acc = 0.0f;
    if (lane < kChains && pa.accumulate) acc = pa.sh[kChains * item + lane];
    if (live) {
        // record b + x of the item, x < R: within [0, 3 n K) of both buffers
        const float* const cols = pa.colors + 3ull * (item * pa.samples_per_item + pa.sample_begin);
        const float* const dirs = pa.directions + 3ull * (item * pa.samples_per_item + pa.sample_begin);
        V3 c = v3(0.0f, 0.0f, 0.0f), d = v3(0.0f, 0.0f, 0.0f);
        if (lane < pa.range_length) {
            c = v3(cols[3u * lane], cols[3u * lane + 1u], cols[3u * lane + 2u]);
            d = v3(dirs[3u * lane], dirs[3u * lane + 1u], dirs[3u * lane + 2u]);
        }
        for (uint32_t c0 = 0; c0 < pa.range_length; c0 += 64u) {
            const uint32_t cs = pa.range_length - c0 < 64u ? pa.range_length - c0 : 64u;    // wave-uniform
            V3 c_next = v3(0.0f, 0.0f, 0.0f), d_next = v3(0.0f, 0.0f, 0.0f);
            const unsigned long long x = (unsigned long long)c0 + 64ull + lane;             // (c0 + 64 may pass 2^32 at the last load)
            if (x < pa.range_length) {
                c_next = v3(cols[3ull * x], cols[3ull * x + 1ull], cols[3ull * x + 2ull]);
                d_next = v3(dirs[3ull * x], dirs[3ull * x + 1ull], dirs[3ull * x + 2ull]);
            }
            const bool folds = lane < cs && !any_nan(d);
            const uint64_t mask = __builtin_amdgcn_ballot_w64(folds);
            if (folds) {
                float term[kChains];
                project_terms<NC>(term, d, c, pa.inv_k);
#pragma unroll
                for (uint32_t j = 0; j < kChains; j++) terms[lane * kStride + j] = term[j];
            }
            __syncthreads();
            if (lane < kChains) {
                const float* const column = terms + lane;
                if (mask == ~0ull) {
#pragma unroll
                    for (uint32_t l = 0; l < 64u; l++) acc = acc + column[l * kStride];
                } else {
                    for (uint64_t m = mask; m != 0ull; m &= m - 1ull) acc = acc + column[(uint32_t)__builtin_ctzll(m) * kStride];
                }
            }
            __syncthreads();
            c = c_next; d = d_next;
        }
    }
    if (lane < kChains) pa.sh[kChains * item + lane] = acc;
}

namespace {

// The projection's own parameters, as both forms read them.
struct ProjectCall {
    uint32_t samples_per_item, sample_begin, sample_end, accumulate, bands;
    uint32_t range() const { return sample_end - sample_begin; }
    uint32_t coeffs() const { return bands * bands; }
};

// The one host rule of the projection's two regimes, the fold's (samples.hip fold_by_wave) taken over: a wave per item
// where an item has at least one full load of 64 records - below that no load can take the straight-line form - and the items are too
// few to fill the device with a lane each: 4096 items are 64 waves of the tile kernel on 256 CUs, and 4096 waves of this one.  Reasoned,
// not swept.
constexpr uint32_t kProjectWaveMinRange = 64u, kProjectWaveMaxItems = 4096u;
bool project_by_wave(uint32_t n, uint32_t range_length) { return range_length >= kProjectWaveMinRange && n <= kProjectWaveMaxItems; }

template <int NC>
void project_launch_nc(bool by_wave, const ProjectArgs& pa, hipStream_t stream) {
    if (by_wave) hipLaunchKernelGGL(project_wave_kernel<NC>, dim3(pa.n), dim3(64), 0, stream, pa);
    else hipLaunchKernelGGL(project_tile_kernel<NC>, dim3((uint32_t)(((unsigned long long)pa.n + 255ull) / 256ull)), dim3(256), 0, stream, pa);
}

hipError_t launch_project(const ProjectCall& c, const float* d_colors, const float* d_directions, const float* d_items, uint32_t n, float* d_sh,
                          hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint32_t R = c.range();
    if (R == 0u) {
        // an empty range: the sums start at 0, or stay
        if (c.accumulate) return hipSuccess;
        return batch_zero(d_sh, 3ull * c.coeffs() * n, nullptr, 0ull, stream);
    }
    const ProjectArgs pa{d_colors, d_directions, d_items, d_sh, n, c.samples_per_item, c.sample_begin, R, c.accumulate, 1.0f / (float)c.samples_per_item};
    const bool by_wave = project_by_wave(n, R);
    // one instantiation per coefficient count: a lane of the tile kernel carries 3, 12 or 27 sums, a load of the wave kernel 3, 12 or 27
    // LDS columns (profiles/project_resource_usage.txt)
    if (c.bands == 1u) project_launch_nc<1>(by_wave, pa, stream);
    else if (c.bands == 2u) project_launch_nc<4>(by_wave, pa, stream);
    else project_launch_nc<9>(by_wave, pa, stream);
    return hipGetLastError();
}

int project_check(const float* colors, const float* directions, uint32_t n, const trt_probe_params* p, const float* sh, ProjectCall& c) {
    if (!p) return query_fail(TRT_ERR_INVALID_ARG, "null argument");
    const uint32_t K = p->path.samples_per_ray;
    if (K == 0u) return query_fail(TRT_ERR_INVALID_ARG, "samples_per_ray must be positive");
    const uint32_t s1 = p->path.sample_end == 0u ? K : p->path.sample_end;
    if (p->path.sample_begin > s1 || s1 > K) return query_fail(TRT_ERR_INVALID_ARG, "sample range must satisfy begin <= end <= samples_per_ray");
    if (p->bands < 1u || p->bands > 3u) return query_fail(TRT_ERR_INVALID_ARG, "bands must be 1, 2 or 3");
    for (uint32_t r : p->path.reserved)
        if (r != 0u) return query_fail(TRT_ERR_INVALID_ARG, "reserved words must be zero");
    for (uint32_t r : p->reserved)
        if (r != 0u) return query_fail(TRT_ERR_INVALID_ARG, "reserved words must be zero");
    if (n > 0u && (!colors || !directions || !sh)) return query_fail(TRT_ERR_INVALID_ARG, "null buffer");
    c = ProjectCall{K, p->path.sample_begin, s1, p->path.accumulate ? 1u : 0u, p->bands};
    return TRT_OK;
}

// What trt_probe_parallel asks beyond trt_probe, after trt_probe's own checks and for n > 0: the record buffer holds an item.
// *m = items per chunk.
int parallel_check(const ProbeCall& c, uint32_t n, uint64_t record_bytes, uint32_t* m) {
    const uint32_t R = c.nothing() ? 0u : c.ra.sample_end - c.ra.sample_begin;
    *m = probe_chunk_items(n, c.samples_per_item, R, record_bytes);
    if (*m == 0u)
        return query_fail(TRT_ERR_INVALID_ARG, "record_bytes holds no item: the colours and directions of one item need " +
                                                   std::to_string(probe_item_bytes(c.samples_per_item)) + " bytes");
    return TRT_OK;
}

// The chunks of a call, enqueued in order: the sample kernels of chunk [a, a + count) into the record buffer, then the projection of those
// records into rows [a, a + count) of d_sh with the caller's accumulate.  Nothing to trace launches no sample kernel.
hipError_t launch_probe_parallel(const QueryScene& qs, const ProbeCall& c, const float* d_items, uint32_t n, uint32_t m, float* d_sh,
                                 unsigned long long* d_counters, void* d_records, hipStream_t stream) {
    if (c.nothing()) {
        if (c.ra.accumulate) return hipSuccess;
        return batch_zero(d_sh, 3ull * c.coeffs() * n, nullptr, 0ull, stream);
    }
    SamplesCall sc;
    sc.ra = c.ra;
    sc.ra.accumulate = 0u;                                                  // a record is written, never added to
    sc.samples_per_item = c.samples_per_item;
    sc.source = c.hemisphere ? (uint32_t)TRT_SAMPLE_HEMISPHERE : (uint32_t)TRT_SAMPLE_SPHERE;
    sc.spread = 0.0f;
    const ProjectCall pc{c.samples_per_item, c.ra.sample_begin, c.ra.sample_end, c.ra.accumulate, c.bands};
    const uint32_t chunks = probe_chunk_count(n, m);
    for (uint32_t k = 0; k < chunks; k++) {
        const ProbeChunk ch = probe_chunk(k, n, m, c.samples_per_item, c.first_stream);
        float* const colors = static_cast<float*>(d_records);
        float* const directions = reinterpret_cast<float*>(static_cast<char*>(d_records) + ch.directions_at);
        const float* const items = d_items + 6ull * ch.first_item;
        sc.first_stream = ch.first_stream;
        hipError_t e = launch_samples(qs, sc, items, ch.count, colors, directions, d_counters, stream);
        if (e != hipSuccess) return e;
        e = launch_project(pc, colors, directions, items, ch.count, d_sh + 3ull * c.coeffs() * ch.first_item, stream);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// The host form's record buffer where the caller names none (tinyrt.h): 96 MiB, the records of 4 Mi samples.
constexpr uint64_t kProbeParallelRecordBytes = 96ull << 20;

}  // namespace
}  // namespace trt

extern "C" {

int trt_project_samples_device(const float* d_colors, const float* d_directions, const trt_ray* d_items, uint32_t n, const trt_probe_params* p,
                               float* d_sh, void* stream) {
    trt::ProjectCall c;
    const int rc = trt::project_check(d_colors, d_directions, n, p, d_sh, c);
    if (rc != TRT_OK) return rc;
    const unsigned long long records = 12ull * n * c.samples_per_item, sums = 12ull * c.coeffs() * n;
    if (trt::ranges_overlap(d_sh, sums, d_colors, records) || trt::ranges_overlap(d_sh, sums, d_directions, records))
        return trt::query_fail(TRT_ERR_INVALID_ARG, "the sums must not overlap the colours or the directions");
    if (n == 0u) return TRT_OK;
    const int rd = trt::query_require_device();
    if (rd != TRT_OK) return rd;
    const hipError_t e = trt::launch_project(c, d_colors, d_directions, reinterpret_cast<const float*>(d_items), n, d_sh, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return trt::query_fail_hip(e, "sample projection launch");
    return TRT_OK;
}

// Host form: device copies of the call's own, the same kernels, complete when the call returns.  There is no CPU path.
int trt_project_samples(const float* colors, const float* directions, const trt_ray* items, uint32_t n, const trt_probe_params* p, float* sh) {
    return trt::host_form([&]() -> int {
        trt::ProjectCall c;
        const int rc = trt::project_check(colors, directions, n, p, sh, c);
        if (rc != TRT_OK) return rc;
        if (n == 0u) return TRT_OK;
        const int rd = trt::query_require_device();
        if (rd != TRT_OK) return rd;
        const size_t records = (size_t)n * c.samples_per_item * 12u, sums = (size_t)n * c.coeffs() * 12u, points = (size_t)n * sizeof(trt_ray);
        trt::HostStage st("sample projection buffers");
        const size_t r_c = st.reserve(records), r_d = st.reserve(records), r_i = st.reserve(points, items != nullptr), r_s = st.reserve(sums);
        st.alloc();
        st.up(r_c, colors, records, "hipMemcpy of the colours");
        st.up(r_d, directions, records, "hipMemcpy of the directions");
        st.up(r_i, items, points, "hipMemcpy of the items");
        if (c.accumulate) st.up(r_s, sh, sums, "hipMemcpy of the sums");
        if (st.ok())
            st.run(trt::launch_project(c, st.ptr<float>(r_c), st.ptr<float>(r_d), st.ptr<float>(r_i), n, st.ptr<float>(r_s), nullptr),
                   "sample projection launch");
        if (!(c.accumulate && c.range() == 0u)) st.down(sh, r_s, sums, "hipMemcpy of the results");
        return st.finish();
    });
}

int trt_probe_parallel_device(trt_scene* s, const trt_ray* d_items, uint32_t n, const trt_probe_params* p, float* d_sh, uint64_t* d_counters,
                              void* d_records, uint64_t record_bytes, void* stream) {
    trt::ProbeCall c;
    const int rc = trt::probe_check(s, d_items, n, p, d_sh, c);
    if (rc != TRT_OK) return rc;
    if (n == 0u) return TRT_OK;
    uint32_t m = 0;
    const int rm = trt::parallel_check(c, n, record_bytes, &m);
    if (rm != TRT_OK) return rm;
    if (!d_records) return trt::query_fail(TRT_ERR_INVALID_ARG, "null record buffer");
    if (trt::ranges_overlap(d_sh, 12ull * c.coeffs() * n, d_records, trt::probe_item_bytes(c.samples_per_item) * m))
        return trt::query_fail(TRT_ERR_INVALID_ARG, "the sums must not overlap the record buffer");
    return trt::sample_query_on_device(s, n, "parallel probe query launch", [&](const trt::QueryScene& qs) {
        return trt::launch_probe_parallel(qs, c, reinterpret_cast<const float*>(d_items), n, m, d_sh, reinterpret_cast<unsigned long long*>(d_counters),
                                          d_records, static_cast<hipStream_t>(stream));
    });
}

// Host buffers: staged as host_stage.h sample_query_on_host stages trt_probe's (items | sums | counters), with the record buffer behind
// them in the same allocation: the chunk size's bytes, not record_bytes.
int trt_probe_parallel(trt_scene* s, const trt_ray* items, uint32_t n, const trt_probe_params* p, float* sh, trt_stats* stats, uint64_t record_bytes) {
    return trt::host_form([&]() -> int {
        trt::ProbeCall c;
        int rc = trt::probe_check(s, items, n, p, sh, c);
        if (rc != TRT_OK) return rc;
        if (n == 0u) {
            if (stats) *stats = trt_stats{};
            return TRT_OK;
        }
        if (record_bytes == 0u) {
            // the default, or one item's need where that is more: a call that names no size never fails for it
            const uint64_t item = trt::probe_item_bytes(c.samples_per_item);
            record_bytes = item > trt::kProbeParallelRecordBytes ? item : trt::kProbeParallelRecordBytes;
        }
        uint32_t m = 0;
        rc = trt::parallel_check(c, n, record_bytes, &m);
        if (rc != TRT_OK) return rc;
        rc = trt::query_require_device();
        if (rc != TRT_OK) return rc;
        trt::QueryScene qs;
        rc = trt::query_scene_on_device(s, qs);
        if (rc != TRT_OK) return rc;
        const size_t items_b = (size_t)n * sizeof(trt_ray), sums = (size_t)n * 12u * c.coeffs();
        const size_t records = c.nothing() ? 0u : (size_t)(trt::probe_item_bytes(c.samples_per_item) * m);
        const bool continues = c.ra.accumulate != 0u;
        trt::HostStage st("parallel probe query buffers");
        const size_t r_items = st.reserve(items_b), r_sums = st.reserve(sums);
        st.reserve_counters();
        const size_t r_records = st.reserve(records);
        st.alloc();
        st.up(r_items, items, items_b, "hipMemcpy of the items");
        st.zero_counters();
        if (continues) st.up(r_sums, sh, sums, "hipMemcpy of the sums");
        st.time_begin();
        if (st.ok())
            st.run(trt::launch_probe_parallel(qs, c, st.ptr<float>(r_items), n, m, st.ptr<float>(r_sums), st.counters(), st.ptr<void>(r_records), nullptr),
                   "parallel probe query launch");
        if (!(continues && c.nothing())) st.down(sh, r_sums, sums, "hipMemcpy of the results");
        st.read_stats(stats);
        return st.finish();
    });
}

// trt_samples_launch_plan's answer for one chunk of n items with a range of range_length samples.
int trt_probe_parallel_launch_plan(const trt_scene* s, uint32_t n, uint32_t range_length, uint32_t compute_units, trt_query_plan* out) {
    return trt_samples_launch_plan(s, n, range_length, compute_units, out);
}

}  // extern "C"
