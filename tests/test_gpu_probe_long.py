"""Probe queries past one workgroup: the 324 items of tests/gather_cases.py tiled (item i = item i mod 324; 324 is no power of two, so
every wave sees another phase of lane mixes, refills and parked stragglers; every i has RNG streams of its own, so no two samples repeat)
on cornell (scene in LDS, lock-step list) and grid3000 (global memory, 16-byte nodes), K = 2, max_bounces = 2, bands 3.

The first item of workgroup 1: every item is compared by its bits with the oracle's fold (tests/probe_cases.py), both domains.  The
smallest n at which a wave's run grows past 256 items on the device at hand (about a million): every item of the first, a middle and the
last wave's run is compared with the oracle, drawn through first_rays(only=...), and all items with the same call made in two halves by
items - other runs, other lanes, the same bytes."""
import numpy as np
import pytest

import probe_cases as PC
import radiance_cases as R
import test_gpu_queries as G
import walk_ray_cases as W

pytestmark = pytest.mark.gpu

SEED, FIRST = PC.SEED, PC.FIRST_STREAM
SCENES = ("cornell", "grid3000")
K, DEPTH, BANDS = 2, 2, 3


@pytest.fixture(scope="module")
def scene(trt, orc):
    cache = {}

    def get(name):
        if name not in cache:
            desc = W.scene(trt, name)
            ow = orc.world_from_description(desc)[0]
            sc = trt.world_from_description(desc)[0].get_bvh()
            assert G.plan_shape(sc.probe_plan(1, BANDS)) == G.DEFAULT_SHAPES[name]
            items, _ = PC.items_of(orc, ow, desc)
            cache[name] = dict(ow=ow, scene=sc, items=items, bg=tuple(desc["background"]))
        return cache[name]

    return get


def oracle_fold(trt, orc, c, items, domain, pick, first_item):
    """The oracle's fold [len(pick), 9, 3] and ray count for the contiguous items `pick` of a batch whose item 0 has stream FIRST: item i's
    samples have streams FIRST + i * K + s, so the run starts at stream FIRST + first_item * K."""
    assert pick[0] == first_item and (np.diff(pick) == 1).all()
    rays = PC.first_rays(orc, items, domain, K, SEED, FIRST, only=pick)[0][pick]
    cols, n_rays = R.oracle_samples(orc, c["ow"], rays.reshape(-1, 6), 1, DEPTH, c["bg"], SEED, FIRST + first_item * K)
    return PC.fold(trt.sh.basis, rays, cols.reshape(len(pick), K, 3), K), n_rays


@pytest.mark.parametrize("domain", PC.DOMAINS)
@pytest.mark.parametrize("name", SCENES)
def test_the_first_item_of_workgroup_1_and_all_before_it_equal_the_oracle(trt, orc, scene, name, domain):
    c = scene(name)
    sc = c["scene"]
    q1 = sc.probe_plan(1, BANDS)
    assert q1["rays_per_wave"] == 256
    n = 256 * (q1["threads_per_workgroup"] // 64) + 1
    assert n == 1025
    q = sc.probe_plan(n, BANDS)
    assert q["workgroups"] == 2 and q["waves"] * q["rays_per_wave"] >= n
    items = np.ascontiguousarray(c["items"][np.arange(n) % len(c["items"])])
    want, n_rays = oracle_fold(trt, orc, c, items, domain, np.arange(n), 0)
    assert len({row.tobytes() for row in want}) >= n // 2                   # the tiles differ: every item has streams of its own
    got, st = sc.probe(items, K, bands=BANDS, domain=domain, max_bounces=DEPTH, background=c["bg"], seed=SEED, first_stream=FIRST)
    R.assert_same_bits(got.reshape(n, -1), want.reshape(n, -1), (name, domain, n))
    assert st["samples"] == n * K and st["rays"] == n_rays


@pytest.mark.parametrize("name", SCENES)
def test_a_batch_with_lengthened_runs(trt, orc, scene, name):
    c = scene(name)
    sc, domain = c["scene"], "hemisphere"
    q1 = sc.probe_plan(1, BANDS)
    n = 256 * q1["wave_slots"] + 1                                          # ceil(n / 256) exceeds the resident wave slots
    assert sc.probe_plan(n - 1, BANDS)["rays_per_wave"] == 256
    q = sc.probe_plan(n, BANDS)
    per_wave, waves = q["rays_per_wave"], q["waves"]
    assert per_wave > 256 and q["workgroups"] >= 2 and (waves - 1) * per_wave < n <= waves * per_wave
    items = np.ascontiguousarray(c["items"][np.arange(n) % len(c["items"])])
    kw = dict(samples_per_item=K, bands=BANDS, domain=domain, max_bounces=DEPTH, background=c["bg"], seed=SEED)
    one, st = sc.probe(items, first_stream=FIRST, **kw)
    assert st["samples"] == n * K
    # the same call in two halves by items: other runs and other lanes, the same bytes
    a = n // 2 | 1
    S = np.full((n, BANDS * BANDS, 3), 7.5, np.float32)
    _, st_a = sc.probe(items[:a], first_stream=FIRST, sh=S[:a], **kw)
    _, st_b = sc.probe(items[a:], first_stream=FIRST + a * K, sh=S[a:], **kw)
    assert S.tobytes() == one.tobytes()
    assert st_a["rays"] + st_b["rays"] == st["rays"]
    # every item of the first, a middle and the last wave's run against the oracle
    for w in (0, waves // 2, waves - 1):
        pick = np.arange(w * per_wave, min((w + 1) * per_wave, n))
        want, _ = oracle_fold(trt, orc, c, items, domain, pick, int(pick[0]))
        assert len({row.tobytes() for row in want}) >= len(pick) // 2
        R.assert_same_bits(one[pick].reshape(len(pick), -1), want.reshape(len(pick), -1), (name, n, "wave", w))
