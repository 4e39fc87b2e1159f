"""What tests/test_gpu_ambient.py, tests/test_gpu_ambient_long.py and tests/test_ambient_cases.py share, none of it touching a GPU: the
oracle's restatement of an ambient query (tinyrt.h trt_ambient).

Items are gather_cases.items_of: 324 surfels, one full run of 256 and a ragged one of 68, with the NaN, zero, inf and 1e-9 items.  The
first ray of every sample is gather_cases.first_rays - the oracle's own scatter functions on RNG stream (seed, j, 1).  The answer of a
sample is the oracle's World.hit over [0.001, max_distance) through ow.hit_index_batch, and the fold of the contract is restated in numpy
float32: an unoccluded sample adds inv_K to the visibility and d * inv_K to the bent sum, an occluded one adds nothing.

K = 8, seed 5, first_stream 1000, both lobes, the cone with spread 0.5.  Two distances per scene and lobe: +inf, and D = float32(median of
the finite hit distances of that scene's and lobe's drawn rays at +inf) - scale-free, and by construction it removes about half the hits."""
import numpy as np

import gather_cases as GC

f32 = np.float32
K, SEED, FIRST_STREAM, SPREAD = 8, 5, 1000, GC.SPREAD
N_ITEMS = GC.N_ITEMS
LOBES = GC.LOBES
T_MIN = 0.001
DISTANCES = ("inf", "D")
assert (K, SEED, FIRST_STREAM) == (GC.K, GC.SEED, GC.FIRST_STREAM)


def occlusion(ow, rays, max_distance):
    """bool [n, k]: does BVH::hit over [0.001, max_distance) find anything for rays [n, k, 6].  A max_distance not above 0.001 is an empty
    range: nothing is asked and nothing is occluded."""
    n, k = rays.shape[:2]
    if not max_distance > T_MIN:
        return np.zeros((n, k), bool)
    hit, _, _ = ow.hit_index_batch(rays.reshape(-1, 6), T_MIN, float(max_distance))
    return hit.reshape(n, k)


def median_distance(ow, rays):
    """D: float32 of the median of the finite hit distances of the rays at +inf."""
    hit, t, _ = ow.hit_index_batch(rays.reshape(-1, 6), T_MIN, float("inf"))
    t = t[hit & np.isfinite(t)]
    assert len(t) > 0
    return f32(np.median(t.astype(np.float64)))


def fold(occ, rays, k, begin=0, end=None, vis=None, bent=None):
    """tinyrt.h trt_ambient over samples [begin, end) in order, from (vis, bent) or from 0: where sample s is unoccluded,
    vis = vis + inv_K and bent.ch = bent.ch + d.ch * inv_K; where it is occluded, nothing.  (float32 [n], float32 [n, 3])."""
    end = occ.shape[1] if end is None else end
    inv = f32(1.0) / f32(k)
    V = np.zeros(occ.shape[0], np.float32) if vis is None else vis.copy()
    B = np.zeros((occ.shape[0], 3), np.float32) if bent is None else bent.copy()
    with np.errstate(all="ignore"):
        for s in range(begin, end):
            open_ = ~occ[:, s]
            V = np.where(open_, V + inv, V)
            B = np.where(open_[:, None], B + rays[:, s, 3:6] * inv, B)
    assert V.dtype == np.float32 and B.dtype == np.float32
    return V, B


def reference(orc, ow, items, lobe, k=K, seed=SEED, first_stream=FIRST_STREAM, spread=SPREAD):
    """The oracle's ambient query of one scene and lobe: dict(rays [n, k, 6], distance = D, and per distance name in DISTANCES: dict(max_distance,
    occ bool [n, k], V [n], B [n, 3]))."""
    rays = GC.first_rays(orc, items, lobe, k, spread, seed, first_stream)
    D = median_distance(ow, rays)
    ref = dict(rays=rays, distance=D)
    for name, dist in (("inf", float("inf")), ("D", float(D))):
        occ = occlusion(ow, rays, dist)
        V, B = fold(occ, rays, k)
        ref[name] = dict(max_distance=dist, occ=occ, V=V, B=B)
    return ref


def freeze(ref):
    ref["rays"].setflags(write=False)
    for name in DISTANCES:
        for key in ("occ", "V", "B"):
            ref[name][key].setflags(write=False)
    return ref


def assert_same_bits(got, want, what):
    """radiance_cases.assert_same_bits for one or three floats per item."""
    import radiance_cases as R
    R.assert_same_bits(got.reshape(len(want), -1), want.reshape(len(want), -1), what)
