// probe_chunks.h - the chunk arithmetic of the K-aware probe query (project.hip; tinyrt.h trt_probe_parallel): a call of n items with K
// samples each, R of them in the call's range, runs chunks of m items through a record buffer of record_bytes bytes,
//   m = min(n, record_bytes / (24 K), (2^32 - 1) / R)
// 24 K bytes being the colours and the directions of one item, and (2^32 - 1) / R the most items one sample launch takes
// (samples.hip samples_check: n x R <= 2^32 - 1).  Chunk c holds items [a, a + count) with a = c m, its samples run on the streams from
// first_stream + a K, and within the record buffer its colours come first (12 count K bytes), then its directions.  Pure functions of
// values with no include of the project's: tests/native/probe_chunks_check.cpp compiles them alone and holds them at their edges.
#pragma once

#include <stdint.h>

namespace trt {

// Bytes of records one item needs: K colours and K directions of three f32 each.  K < 2^32, so the product fits 64 bits.
inline uint64_t probe_item_bytes(uint32_t samples_per_item) { return 24ull * samples_per_item; }

// Items per chunk; 0 where the buffer does not hold one item (and for n == 0).  K >= 1.  range_length == 0 (nothing to trace: no sample
// launch) puts no limit of its own.
inline uint32_t probe_chunk_items(uint32_t n, uint32_t samples_per_item, uint32_t range_length, uint64_t record_bytes) {
    uint64_t m = record_bytes / probe_item_bytes(samples_per_item);
    if (range_length != 0u && m > 0xFFFFFFFFull / range_length) m = 0xFFFFFFFFull / range_length;
    return m < n ? (uint32_t)m : n;
}

struct ProbeChunk {
    uint32_t first_item, count;      // items [first_item, first_item + count)
    uint32_t first_stream;           // the call's first_stream + first_item * K
    uint64_t directions_at;          // byte offset of the chunk's directions in the record buffer; its colours are at 0
};

inline uint32_t probe_chunk_count(uint32_t n, uint32_t m) { return m == 0u ? 0u : (uint32_t)(((uint64_t)n + m - 1u) / m); }

// Chunk c of probe_chunk_count(n, m), m >= 1.  The caller has checked first_stream + n K <= 2^32 (radiance.hip radiance_check), so
// first_stream + first_item K fits 32 bits for every chunk.
inline ProbeChunk probe_chunk(uint32_t c, uint32_t n, uint32_t m, uint32_t samples_per_item, uint32_t first_stream) {
    ProbeChunk k;
    const uint64_t a = (uint64_t)c * m;
    k.first_item = (uint32_t)a;
    k.count = n - a < m ? (uint32_t)(n - a) : m;
    k.first_stream = (uint32_t)(first_stream + a * samples_per_item);
    k.directions_at = 12ull * k.count * samples_per_item;
    return k;
}

}  // namespace trt
