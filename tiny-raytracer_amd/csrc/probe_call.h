// probe_call.h - what a probe call asks of the device after the checks, and the checks: shared by the unit that folds while it traces
// (probe.hip: trt_probe) and the unit that traces a sample to a lane and folds the records (project.hip: trt_probe_parallel), so that the
// two refuse the same arguments in the same order with the same words.  Host code only.
#pragma once

#include "kernels.h"

namespace trt {

struct ProbeCall {
    RenderArgs ra;                   // of the path parameters (radiance_check)
    uint32_t samples_per_item, first_stream;
    uint32_t hemisphere, bands;
    uint32_t coeffs() const { return bands * bands; }
    bool nothing() const { return ra.sample_begin == ra.sample_end || ra.max_bounces == 0u; }
};

// What both forms check before any device work: trt_radiance's rules on p->path (radiance.hip radiance_check), then this struct's fields.
// Defined in probe.hip.
int probe_check(const trt_scene* s, const trt_ray* items, uint32_t n, const trt_probe_params* p, const float* sh, ProbeCall& c);

}  // namespace trt
