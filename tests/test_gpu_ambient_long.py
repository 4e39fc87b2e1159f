"""Ambient queries past one workgroup: the 324 items of tests/gather_cases.py tiled (item i = item i mod 324; 324 is no power of two, so
every wave sees another phase of lane mixes, refills and parked stragglers; every i has RNG streams of its own, so no two samples repeat)
through the device form, with guards, on cornell (scene in LDS, lock-step list) and grid3000 (global memory, 16-byte nodes).

Two smaller sizes with K = 2 - the first item of workgroup 1, and 100 003 - have every item compared by its bits with the oracle's fold
(tests/ambient_cases.py).  The smallest n at which a wave's run grows past 256 items on the device at hand (some millions) runs with
K = 1: every item of the first, a middle and the last wave's run is compared with the oracle, drawn through first_rays(only=...), and
all items with the same call made in two halves by items - other runs, other lanes, the same bytes.

The cosine lobe at the finite distance D of tests/ambient_cases.py: about half of the hits at +inf lie beyond it, so both answers and the
distance itself are exercised in every wave."""
import numpy as np
import pytest

import ambient_cases as A
import gather_cases as GC
import test_gpu_queries as G
import walk_ray_cases as W

pytestmark = pytest.mark.gpu

SEED, FIRST = A.SEED, A.FIRST_STREAM
GUARD = 64
FILL = 0xCD
SCENES = ("cornell", "grid3000")
LOBE = "cosine"


@pytest.fixture(scope="module")
def scene(trt, orc):
    cache = {}

    def get(name):
        if name not in cache:
            desc = W.scene(trt, name)
            ow = orc.world_from_description(desc)[0]
            sc = trt.world_from_description(desc)[0].get_bvh()
            assert G.plan_shape(sc.ambient_plan(1)) == G.DEFAULT_SHAPES[name]
            items, _ = GC.items_of(orc, ow, desc)
            dist = float(A.median_distance(ow, GC.first_rays(orc, items, LOBE, A.K, A.SPREAD, SEED, FIRST)))
            cache[name] = dict(ow=ow, scene=sc, items=items, dist=dist)
        return cache[name]

    return get


def batch_size(sc, which):
    q = sc.ambient_plan(1)
    assert q["rays_per_wave"] == 256
    if which == "workgroup1":
        return 256 * (q["threads_per_workgroup"] // 64) + 1
    if which == "100003":
        return 100003
    n = 256 * q["wave_slots"] + 1                                           # ceil(n / 256) exceeds the resident wave slots
    assert sc.ambient_plan(n - 1)["rays_per_wave"] == 256 and sc.ambient_plan(n)["rays_per_wave"] > 256
    return n


def on_device(torch, sc, items, k, first_stream, dist):
    """(visibility [n], bent [n, 3], samples, rays) of the device form on guarded buffers; the guards asserted."""
    n = len(items)
    d_items = torch.from_numpy(items).to("cuda:0")
    d_v = torch.full(((GUARD + n + GUARD) * 4,), FILL, dtype=torch.uint8, device="cuda:0")
    d_b = torch.full(((GUARD + n + GUARD) * 12,), FILL, dtype=torch.uint8, device="cuda:0")
    ctr = torch.zeros(16, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    sc.ambient_device(d_items.data_ptr(), n, d_v.data_ptr() + GUARD * 4, d_b.data_ptr() + GUARD * 12, d_counters_ptr=ctr.data_ptr(),
                      samples_per_item=k, lobe=LOBE, max_distance=dist, seed=SEED, first_stream=first_stream)
    torch.cuda.synchronize()
    out = []
    for t, width in ((d_v, 1), (d_b, 3)):
        h = t.cpu().numpy()
        g, b = GUARD * 4 * width, n * 4 * width
        assert (h[:g] == FILL).all() and (h[g + b:] == FILL).all(), (n, width, "guard bytes were written")
        out.append(h[g:g + b].copy().view(np.float32))
    assert not bool(ctr[2:].any())
    return out[0], out[1].reshape(n, 3), int(ctr[0]), int(ctr[1])


@pytest.mark.parametrize("which", ["workgroup1", "100003"])
@pytest.mark.parametrize("name", SCENES)
def test_tiled_batches_equal_the_oracle(trt, orc, scene, name, which):
    import torch
    c = scene(name)
    sc, k = c["scene"], 2
    n = batch_size(sc, which)
    assert n == (100003 if which == "100003" else {256: 1025, 768: 3073}[sc.ambient_plan(1)["threads_per_workgroup"]])
    q = sc.ambient_plan(n)
    assert q["workgroups"] >= 2 and q["waves"] * q["rays_per_wave"] >= n
    items = np.ascontiguousarray(c["items"][np.arange(n) % len(c["items"])])
    rays = GC.first_rays(orc, items, LOBE, k, A.SPREAD, SEED, FIRST)
    occ = A.occlusion(c["ow"], rays, c["dist"])
    want_v, want_b = A.fold(occ, rays, k)
    assert 0.02 < occ.mean() < 0.6 and len(set(want_v.tolist())) == 3      # 0, 0.5 and 1 all occur
    got_v, got_b, samples, walks = on_device(torch, sc, items, k, FIRST, c["dist"])
    A.assert_same_bits(got_v, want_v, (name, which, n, "visibility"))
    A.assert_same_bits(got_b, want_b, (name, which, n, "bent"))
    assert samples == n * k and walks == n * k


@pytest.mark.parametrize("name", SCENES)
def test_a_batch_with_lengthened_runs(trt, orc, scene, name):
    import torch
    c = scene(name)
    sc = c["scene"]
    n = batch_size(sc, "longer_runs")
    q = sc.ambient_plan(n)
    per_wave, waves = q["rays_per_wave"], q["waves"]
    assert per_wave > 256 and q["workgroups"] >= 2 and (waves - 1) * per_wave < n <= waves * per_wave
    items = np.ascontiguousarray(c["items"][np.arange(n) % len(c["items"])])
    one_v, one_b, samples, walks = on_device(torch, sc, items, 1, FIRST, c["dist"])
    assert samples == n and walks == n
    # the same call in two halves by items: other runs and other lanes, the same bytes
    a = n // 2 | 1
    va, ba, _, wa = on_device(torch, sc, np.ascontiguousarray(items[:a]), 1, FIRST, c["dist"])
    vb, bb, _, wb = on_device(torch, sc, np.ascontiguousarray(items[a:]), 1, FIRST + a, c["dist"])
    assert np.concatenate([va, vb]).tobytes() == one_v.tobytes() and np.concatenate([ba, bb]).tobytes() == one_b.tobytes()
    assert wa + wb == walks
    # every item of the first, a middle and the last wave's run against the oracle
    pick = np.concatenate([np.arange(w * per_wave, min((w + 1) * per_wave, n)) for w in (0, waves // 2, waves - 1)])
    assert len(pick) > 2 * per_wave and pick[-1] == n - 1
    rays = GC.first_rays(orc, items, LOBE, 1, A.SPREAD, SEED, FIRST, only=pick)[pick]
    occ = A.occlusion(c["ow"], rays, c["dist"])
    want_v, want_b = A.fold(occ, rays, 1)
    assert 0.02 < occ.mean() < 0.6
    A.assert_same_bits(one_v[pick], want_v, (name, n, "visibility"))
    A.assert_same_bits(one_b[pick], want_b, (name, n, "bent"))
