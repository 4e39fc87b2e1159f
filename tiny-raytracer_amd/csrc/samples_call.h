// samples_call.h - what a sample query asks of the device after the checks, and its launch: the ONE copy of the launch of the sample
// kernels (samples.hip launch_samples), shared with the unit that traces probes a sample to a lane and folds the records
// (project.hip: trt_probe_parallel).  Host code only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "scene_query.h"

namespace trt {

struct SamplesCall {
    RenderArgs ra;                   // of the path parameters (radiance_check)
    uint32_t samples_per_item, first_stream;
    uint32_t source;                 // enum trt_sample_source
    float spread;
    uint32_t range() const { return ra.sample_end - ra.sample_begin; }
};

// Samples [ra.sample_begin, ra.sample_end) of items [0, n) of d_items, streams from c.first_stream; n x range() <= 2^32 - 1 is the
// caller's to check.  An empty range launches nothing; max_bounces == 0 zeroes the colours of the range and leaves the directions.
// Defined in samples.hip.
hipError_t launch_samples(const QueryScene& qs, const SamplesCall& c, const float* d_items, uint32_t n, float* d_colors, float* d_directions,
                          unsigned long long* d_counters, hipStream_t stream);

// Two device or host ranges share a byte; a NULL or empty range shares none.
inline bool ranges_overlap(const void* a, unsigned long long a_bytes, const void* b, unsigned long long b_bytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a && b && a_bytes && b_bytes && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

}  // namespace trt
