// flat_reuse.h — the reuse schedule of the lock-step leaf walk (rt_path.h box_loop_flat), derived on the host once per scene.
//
// A leaf's slab interval on axis k is (min, max) of fl(fl(plane - o_k) * inv_k) over its two planes lo_k, hi_k (x also folds in
// t_min and t_best).  It depends on the ray and on the two plane bit patterns alone, so where leaf i's planes on axis k are the
// same BITS as leaf i-1's, the walk keeps the interval it computed for leaf i-1 and skips the six instructions of that axis.  The
// comparison is on bit patterns, never float ==: -0 and +0 planes give intervals of different sign on an axis with a zero origin,
// and they must not merge.  NaN and inf coordinates are never reused (conservative: such leaves are rare and recomputing costs
// nothing but time).  Plain C++: the scene layer and the host tests include it.
#pragma once

#include <stdint.h>
#include <string.h>

namespace trt {

// Bit i of masks[k] (k = 0, 1, 2: x, y, z) is set iff leaf i's (lo_k, hi_k) equal leaf i-1's bit for bit, both finite.  Bit 0 is
// always clear, no bit at or beyond n_leaves is set, and all three masks are zero when `enabled` is false, when there is no
// list, or when the list is longer than the 32 leaves one mask holds.  `leaf_list`: n_leaves leaves of 32 bytes in walk order,
// (lo.x lo.y lo.z hi.x) (hi.y hi.z skip link) - scene.h off_leaf_list.
inline void flat_reuse_masks(const void* leaf_list, uint32_t n_leaves, bool enabled, uint32_t masks[3]) {
    masks[0] = masks[1] = masks[2] = 0u;
    if (!enabled || leaf_list == nullptr || n_leaves > 32u) return;
    auto finite = [](uint32_t b) { return (b & 0x7f800000u) != 0x7f800000u; };
    const unsigned char* p = static_cast<const unsigned char*>(leaf_list);
    uint32_t prev[8], cur[8];
    if (n_leaves > 0u) memcpy(prev, p, sizeof prev);
    for (uint32_t i = 1; i < n_leaves; i++) {
        memcpy(cur, p + 32u * (size_t)i, sizeof cur);
        for (int k = 0; k < 3; k++) {
            const uint32_t lo = cur[k], hi = cur[3 + k];
            if (lo == prev[k] && hi == prev[3 + k] && finite(lo) && finite(hi)) masks[k] |= 1u << i;
        }
        memcpy(prev, cur, sizeof prev);
    }
}

}  // namespace trt
