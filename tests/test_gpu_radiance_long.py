"""Radiance queries past one workgroup: the 324 rays of tests/radiance_cases.py tiled (ray i = ray i mod 324; 324 is no power of two, so
every wave sees another phase of lane mixes, refills and parked stragglers) to three batch sizes - the first ray of workgroup 1, 100 003,
and the smallest n at which a wave's run grows past 256 rays on the device at hand - through the device form with K = 1, and every colour
compared by its bits with orc.sample_batch over the same tiled list (first_stream = 0: trt_sample_batch's own numbering).  No ray is
sampled out of the comparison.

Scenes: cornell (scene in LDS, lock-step list) with max_bounces = 4, and grid3000 (global memory, 16-byte nodes) with max_bounces = 2: the
single-threaded oracle needs about 8 s for the 6.3 M paths of the largest cornell batch at depth 4, and about 37 s for the 7.3 M paths of
the largest grid3000 batch at depth 4 (28 s at depth 2: most of it is the first segment over 3000 spheres), hence the cut there."""
import numpy as np
import pytest

import radiance_cases as R
import test_gpu_queries as G
import walk_ray_cases as W

pytestmark = pytest.mark.gpu

SEED = R.SEED
GUARD = 64
FILL = 0xCD
DEPTH = {"cornell": 4, "grid3000": 2}


@pytest.fixture(scope="module")
def scene(trt, orc):
    cache = {}

    def get(name):
        if name not in cache:
            desc = W.scene(trt, name)
            sc = trt.world_from_description(desc)[0].get_bvh()
            assert G.plan_shape(sc.radiance_plan(1)) == G.DEFAULT_SHAPES[name]
            cache[name] = dict(desc=desc, ow=orc.world_from_description(desc)[0], scene=sc, rays=R.rays_of(desc), bg=tuple(desc["background"]))
        return cache[name]

    return get


def batch_size(sc, which):
    q = sc.radiance_plan(1)
    assert q["rays_per_wave"] == 256
    if which == "workgroup1":
        return 256 * (q["threads_per_workgroup"] // 64) + 1
    if which == "100003":
        return 100003
    n = 256 * q["wave_slots"] + 1                                           # ceil(n / 256) exceeds the resident wave slots
    assert sc.radiance_plan(n - 1)["rays_per_wave"] == 256 and sc.radiance_plan(n)["rays_per_wave"] > 256
    return n


@pytest.mark.parametrize("which", ["workgroup1", "100003", "longer_runs"])
@pytest.mark.parametrize("name", list(DEPTH))
def test_tiled_batches_equal_the_oracle(trt, orc, scene, name, which):
    import torch
    c = scene(name)
    sc, depth = c["scene"], DEPTH[name]
    n = batch_size(sc, which)
    q = sc.radiance_plan(n)
    assert q["workgroups"] >= 2 and q["waves"] * q["rays_per_wave"] >= n
    rays = np.ascontiguousarray(c["rays"][np.arange(n) % len(c["rays"])])
    out, st = orc.sample_batch(c["ow"], R.points_of(orc.SamplePoint, rays), depth, c["bg"], SEED)
    want = R.colors_of(out, n)
    d_rays = torch.from_numpy(rays).to("cuda:0")
    d_s = torch.full(((GUARD + n + GUARD) * 12,), FILL, dtype=torch.uint8, device="cuda:0")
    ctr = torch.zeros(16, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    sc.radiance_device(d_rays.data_ptr(), n, d_s.data_ptr() + GUARD * 12, d_counters_ptr=ctr.data_ptr(), samples_per_ray=1, max_bounces=depth,
                       background=c["bg"], seed=SEED)
    torch.cuda.synchronize()
    h = d_s.cpu().numpy()
    g = GUARD * 12
    assert (h[:g] == FILL).all() and (h[g + n * 12:] == FILL).all(), (name, which, "guard bytes were written")
    got = h[g:g + n * 12].view(np.float32).reshape(n, 3)
    R.assert_same_bits(got, want, (name, which, n))
    assert int(ctr[0]) == n and int(ctr[1]) == st["rays"] and not bool(ctr[2:].any())
