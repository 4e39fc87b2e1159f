// sh_basis.h - the real spherical-harmonic basis of the probe contract (tinyrt.h trt_probe): graphics convention, coefficient index
// k = l (l + 1) + m, each product and difference one f32 operation in the header's parenthesisation.  ONE copy for the unit that folds in
// registers while it traces (probe.hip probe_fold) and the unit that folds sample records (project.hip).
#pragma once

#include "rt_device.h"

namespace trt {

// b[k] = b_k(d) for k < NC; NC = 1 evaluates band 0 only, NC = 4 bands 0 and 1.
template <int NC>
TRT_DEV void sh_basis(float (&b)[NC], const V3& d) {
    const float c0 = 0.282094792f, c1 = 0.488602512f, c2 = 1.092548431f, c3 = 0.315391565f, c4 = 0.546274215f;
    const float x = d.x, y = d.y, z = d.z;
    b[0] = c0;
    if constexpr (NC > 1) {
        b[1] = c1 * y;
        b[2] = c1 * z;
        b[3] = c1 * x;
    }
    if constexpr (NC > 4) {
        b[4] = c2 * (x * y);
        b[5] = c2 * (y * z);
        b[6] = c3 * ((3.0f * (z * z)) - 1.0f);
        b[7] = c2 * (x * z);
        b[8] = c4 * ((x * x) - (y * y));
    }
}

}  // namespace trt
