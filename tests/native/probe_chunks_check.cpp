// probe_chunks_check.cpp - csrc/probe_chunks.h, the chunk arithmetic of trt_probe_parallel, compiled alone (no HIP, no project header)
// and held at its edges: a record buffer one byte below and at one item's need, a ragged last chunk, n x R at 2^32 - 1, K = 1, and for
// every case that the chunks tile [0, n) exactly, in order, with the right first streams and the directions behind the colours.
// A stand-alone program: tests/test_project_cases.py builds it with -fsanitize=address,undefined and runs it.
#include <initializer_list>

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "probe_chunks.h"

static int failures = 0;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);                 \
            failures++;                                                              \
        }                                                                            \
    } while (0)

// m as the contract states it, in 64 bits throughout
static uint64_t want_items(uint64_t n, uint64_t K, uint64_t R, uint64_t bytes) {
    uint64_t m = bytes / (24u * K);
    if (R != 0u && m > 0xFFFFFFFFull / R) m = 0xFFFFFFFFull / R;
    return m < n ? m : n;
}

// The chunks of (n, K, R, bytes, first_stream) tile [0, n); walks at most `limit` chunks from either end.
static void tiles(uint32_t n, uint32_t K, uint32_t R, uint64_t bytes, uint32_t first_stream, uint32_t limit) {
    const uint32_t m = trt::probe_chunk_items(n, K, R, bytes);
    CHECK(m == want_items(n, K, R, bytes));
    if (m == 0u) {
        CHECK(trt::probe_chunk_count(n, m) == 0u);
        return;
    }
    CHECK((uint64_t)m * trt::probe_item_bytes(K) <= bytes);                 // a chunk's records fit the buffer
    CHECK(R == 0u || (uint64_t)m * R <= 0xFFFFFFFFull);                      // and one sample launch
    const uint32_t chunks = trt::probe_chunk_count(n, m);
    CHECK((uint64_t)chunks * m >= n && (uint64_t)(chunks - 1u) * m < n);
    uint64_t next = 0;
    for (uint32_t c = 0; c < chunks; c++) {
        if (c == limit && chunks > 2u * limit) {                            // skip the middle of a long run: its chunks are full by the count above
            c = chunks - limit;
            next = (uint64_t)c * m;
        }
        const trt::ProbeChunk k = trt::probe_chunk(c, n, m, K, first_stream);
        CHECK(k.first_item == next);
        CHECK(k.count >= 1u && k.count <= m);
        CHECK(c + 1u == chunks ? (uint64_t)k.first_item + k.count == n : k.count == m);
        CHECK(k.first_stream == (uint32_t)(first_stream + (uint64_t)k.first_item * K));
        CHECK((uint64_t)first_stream + (uint64_t)k.first_item * K <= 0xFFFFFFFFull);       // no wrap: first_stream + n K <= 2^32
        CHECK(k.directions_at == 12ull * k.count * K);
        CHECK(2u * k.directions_at <= bytes);                               // colours | directions, both inside the buffer
        next += k.count;
    }
    CHECK(next == n);
}

int main() {
    const uint32_t Ks[] = {1u, 2u, 7u, 16u, 130u, 16384u, 1u << 20, 0xFFFFFFFFu};
    for (uint32_t K : Ks) {
        const uint64_t item = 24ull * K;
        CHECK(trt::probe_item_bytes(K) == item);
        // one byte below one item's need, at it, one below two items', at two
        CHECK(trt::probe_chunk_items(5u, K, K, item - 1u) == 0u);
        CHECK(trt::probe_chunk_items(5u, K, K, 0u) == 0u);
        CHECK(trt::probe_chunk_items(5u, K, K, item) == 1u);
        CHECK(trt::probe_chunk_items(5u, K, K, 2u * item - 1u) == 1u);
        CHECK(trt::probe_chunk_items(5u, K, K, 2u * item) == (K == 0xFFFFFFFFu ? 1u : 2u));       // (2^32 - 1) / R = 1 there
        CHECK(trt::probe_chunk_items(0u, K, K, item) == 0u);
        const uint32_t n_max = (uint32_t)(0x100000000ull / K) < 1000u ? (uint32_t)(0x100000000ull / K) : 1000u;
        for (uint32_t n : {1u, 2u, 3u, 7u, 64u, 65u, 324u, 1000u}) {
            if (n > n_max) continue;
            const uint32_t first = (uint32_t)(0x100000000ull - (uint64_t)n * K);            // the largest legal first stream
            for (uint64_t bytes : {item - 1u, item, item + 1u, 3u * item, 3u * item + 5u, 100u * item, (uint64_t)n * item, ~(uint64_t)0}) {
                for (uint32_t R : {0u, 1u, K})
                    if (R <= K) {
                        tiles(n, K, R, bytes, 0u, 8u);
                        tiles(n, K, R, bytes, first, 8u);
                    }
            }
        }
    }
    // a ragged last chunk: 7 items in chunks of 3, 3 and 1
    {
        const uint32_t m = trt::probe_chunk_items(7u, 130u, 130u, 3u * 24u * 130u + 11u);
        CHECK(m == 3u && trt::probe_chunk_count(7u, m) == 3u);
        const trt::ProbeChunk last = trt::probe_chunk(2u, 7u, m, 130u, 1000u);
        CHECK(last.first_item == 6u && last.count == 1u && last.first_stream == 1000u + 6u * 130u && last.directions_at == 12u * 130u);
    }
    // n x R at 2^32 - 1: the limit of one sample launch binds, not the buffer
    {
        const uint32_t R = 65535u, n = 65537u;                              // n * R = 2^32 - 1
        CHECK(trt::probe_chunk_items(n, R, R, ~(uint64_t)0) == n);
        tiles(n, R, R, ~(uint64_t)0, 0u, 8u);
        CHECK(trt::probe_chunk_items(n + 1u, R, R, ~(uint64_t)0) == n);            // one item more: two chunks
        CHECK(trt::probe_chunk_count(n + 1u, n) == 2u);
        tiles(n + 1u, R, R, ~(uint64_t)0, 0u, 8u);
        // a short range of a long K: the launch limit follows R, the bytes follow K
        CHECK(trt::probe_chunk_items(0xFFFFFFFFu, 1u, 1u, ~(uint64_t)0) == 0xFFFFFFFFu);
        tiles(0xFFFFFFFFu, 1u, 1u, ~(uint64_t)0, 0u, 8u);
        tiles(0xFFFFFFFFu, 1u, 1u, 24ull * 1000u, 1u, 8u);
        CHECK(trt::probe_chunk_items(1u << 20, 16u, 3u, ~(uint64_t)0) == 1u << 20);
        CHECK(trt::probe_chunk_items(0xFFFFFFFFu, 1u, 0u, ~(uint64_t)0) == 0xFFFFFFFFu);           // nothing to trace: no limit from R
    }
    // K = 1: 24 bytes an item
    {
        CHECK(trt::probe_chunk_items(100u, 1u, 1u, 23u) == 0u && trt::probe_chunk_items(100u, 1u, 1u, 24u) == 1u);
        CHECK(trt::probe_chunk_items(100u, 1u, 1u, 24u * 100u) == 100u && trt::probe_chunk_items(100u, 1u, 1u, 24u * 100u - 1u) == 99u);
        tiles(100u, 1u, 1u, 24u * 33u, 5u, 8u);                             // 33, 33, 33, 1
        CHECK(trt::probe_chunk_count(100u, 33u) == 4u);
    }
    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("ok all\n");
    return 0;
}
