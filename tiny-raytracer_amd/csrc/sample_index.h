// sample_index.h - the work index of the sample queries (samples.hip; tinyrt.h trt_samples): a call traces samples [b, b + R) of each of n
// items, and work index q of 0 .. n * R - 1 is sample s of item i with
//   i = q / R;   s = b + (q - i * R)
// so that a wave's contiguous run of q is a contiguous run of an item's samples, then of the next item's.  A pure function of values for
// the host and the device, with no include of the project's: tests/native/sample_index_check.cpp compiles it alone and holds it against
// 64-bit division at the edges of every width involved.
// The division is the language's own unsigned 32-bit one, exact for every q and every R >= 1 by definition; n * R <= 2^32 - 1 is checked
// where the call is made (samples.hip samples_check), so q, i and s fit 32 bits and i * R does not wrap.  On gfx950 it is about twenty
// vector instructions, once per PATH: a host-computed reciprocal would save a dozen of them and need a proof of its own.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define TRT_SAMPLE_INDEX_FN __host__ __device__ inline
#else
#define TRT_SAMPLE_INDEX_FN inline
#endif

namespace trt {

struct SampleIndex {
    uint32_t item, sample;
};

// range_length = R >= 1, sample_begin = b; q < n * R.
TRT_SAMPLE_INDEX_FN SampleIndex sample_index(uint32_t q, uint32_t range_length, uint32_t sample_begin) {
    SampleIndex x;
    x.item = q / range_length;
    x.sample = sample_begin + (q - x.item * range_length);
    return x;
}

// The tile fold's row of a flat element (samples.hip fold_tile_kernel): e / len for e < 64 * len and 1 <= len <= 48, as a multiplication by
// magic = ceil(2^20 / len).  Exact: magic * len = 2^20 + d with 0 <= d < len, so e * magic / 2^20 = e / len + e * d / (2^20 * len), and the
// excess e * d / (2^20 * len) < 3072 * 47 / 2^20 / len < 1 / len, too little to reach the next integer from a fraction of at most
// (len - 1) / len; e * magic < 3072 * 2^20 < 2^32 does not wrap.
TRT_SAMPLE_INDEX_FN uint32_t fold_row_magic(uint32_t len) { return ((1u << 20) + len - 1u) / len; }
TRT_SAMPLE_INDEX_FN uint32_t fold_row(uint32_t e, uint32_t magic) { return (e * magic) >> 20; }

}  // namespace trt
