"""Passes queries past one workgroup: the 324 items of a scene tiled (item i = item i mod 324; 324 is no power of two, so every wave sees
another phase of lane mixes, refills and parked stragglers; every i has RNG streams of its own, so no two samples repeat) on cornell (scene
in LDS, lock-step list) and grid3000 (global memory, 16-byte nodes), K = 2, max_bounces = 3, 2 depth bins.

The first item of workgroup 1: every item is compared by its bits with the oracle's fold (tests/passes_cases.py), sources "cosine" and
"rays".  The smallest n at which a wave's run grows past 256 items on the device at hand (about a million): every item of the first, a
middle and the last wave's run is compared with the oracle, and all items with the same call made in two halves by items - other runs,
other lanes, the same bytes."""
import numpy as np
import pytest

import passes_cases as P
import radiance_cases as R
import test_gpu_queries as G
import walk_ray_cases as W

pytestmark = pytest.mark.gpu

SEED, FIRST = P.SEED, P.FIRST_STREAM
SCENES = ("cornell", "grid3000")
K, DEPTH, BINS = 2, 3, 2


@pytest.fixture(scope="module")
def scene(trt, orc):
    cache = {}

    def get(name):
        if name not in cache:
            desc = W.scene(trt, name)
            ow = orc.world_from_description(desc)[0]
            sc = trt.world_from_description(desc)[0].get_bvh()
            assert G.plan_shape(sc.passes_plan(1, BINS)) == G.DEFAULT_SHAPES[name]
            items = {source: P.items_of(orc, ow, desc, source) for source in ("cosine", "rays")}
            cache[name] = dict(desc=desc, ow=ow, scene=sc, items=items, bg=P.background_of(desc))
        return cache[name]

    return get


def oracle_fold(orc, c, items, source, pick):
    """The oracle's fold (passes [len(pick), 2 B, 3], spent [len(pick)]) and ray count for the contiguous items `pick` of a batch whose
    item 0 has stream FIRST: item i's samples have streams FIRST + i * K + s."""
    assert (np.diff(pick) == 1).all()
    rays = P.first_rays(orc, c["desc"], items, source, K, SEED, FIRST, only=pick)
    cols, kinds, depths, n_rays = P.oracle_paths(orc, c["ow"], c["desc"], rays, DEPTH, c["bg"], SEED, FIRST, only=pick)
    passes, spent = P.fold(cols[pick], kinds[pick], depths[pick], K, BINS)
    return passes, spent, n_rays, np.concatenate([kinds[pick], depths[pick]], axis=1)


@pytest.mark.parametrize("source", ("cosine", "rays"))
@pytest.mark.parametrize("name", SCENES)
def test_the_first_item_of_workgroup_1_and_all_before_it_equal_the_oracle(trt, orc, scene, name, source):
    c = scene(name)
    sc = c["scene"]
    q1 = sc.passes_plan(1, BINS)
    assert q1["rays_per_wave"] == 256
    n = 256 * (q1["threads_per_workgroup"] // 64) + 1
    assert n == 1025
    q = sc.passes_plan(n, BINS)
    assert q["workgroups"] == 2 and q["waves"] * q["rays_per_wave"] >= n
    base = c["items"][source]
    items = np.ascontiguousarray(base[np.arange(n) % len(base)])
    want_p, want_s, n_rays, classes = oracle_fold(orc, c, items, source, np.arange(n))
    # the tiles differ: every item has streams of its own, so the same item ends its paths otherwise in the next tile
    differ = int((classes[:len(base)] != classes[len(base):2 * len(base)]).any(axis=1).sum())
    print(name, source, "items whose classes differ between tile 0 and tile 1:", differ, "of", len(base))
    assert differ >= len(base) // 8, (name, source, differ)                # [129 - 233 of 324, measured with the CPU oracle]
    assert (want_s != 0.0).any() and (want_p[:, BINS:] != 0.0).any()       # spent paths and paths that reached the sky
    got_p, got_s, st = sc.passes(items, K, depth_bins=BINS, source=source, max_bounces=DEPTH, background=c["bg"], seed=SEED, first_stream=FIRST)
    R.assert_same_bits(got_p.reshape(n, -1), want_p.reshape(n, -1), (name, source, n, "passes"))
    R.assert_same_bits(got_s.reshape(n, 1), want_s.reshape(n, 1), (name, source, n, "spent"))
    assert st["samples"] == n * K and st["rays"] == n_rays


@pytest.mark.parametrize("name", SCENES)
def test_a_batch_with_lengthened_runs(trt, orc, scene, name):
    c = scene(name)
    sc, source = c["scene"], "cosine"
    q1 = sc.passes_plan(1, BINS)
    n = 256 * q1["wave_slots"] + 1                                          # ceil(n / 256) exceeds the resident wave slots
    assert sc.passes_plan(n - 1, BINS)["rays_per_wave"] == 256
    q = sc.passes_plan(n, BINS)
    per_wave, waves = q["rays_per_wave"], q["waves"]
    assert per_wave > 256 and q["workgroups"] >= 2 and (waves - 1) * per_wave < n <= waves * per_wave
    base = c["items"][source]
    items = np.ascontiguousarray(base[np.arange(n) % len(base)])
    kw = dict(samples_per_item=K, depth_bins=BINS, source=source, max_bounces=DEPTH, background=c["bg"], seed=SEED)
    one_p, one_s, st = sc.passes(items, first_stream=FIRST, **kw)
    assert st["samples"] == n * K
    # the same call in two halves by items: other runs and other lanes, the same bytes
    a = n // 2 | 1
    passes, spent = np.full((n, 2 * BINS, 3), 7.5, np.float32), np.full(n, 7.5, np.float32)
    _, _, st_a = sc.passes(items[:a], first_stream=FIRST, passes=passes[:a], spent=spent[:a], **kw)
    _, _, st_b = sc.passes(items[a:], first_stream=FIRST + a * K, passes=passes[a:], spent=spent[a:], **kw)
    assert passes.tobytes() == one_p.tobytes() and spent.tobytes() == one_s.tobytes()
    assert st_a["rays"] + st_b["rays"] == st["rays"]
    # every item of the first, a middle and the last wave's run against the oracle
    for w in (0, waves // 2, waves - 1):
        pick = np.arange(w * per_wave, min((w + 1) * per_wave, n))
        want_p, want_s, _, classes = oracle_fold(orc, c, items, source, pick)
        if len(pick) >= 64:                                                 # (the last wave's run may be a single item)
            assert len({row.tobytes() for row in classes}) >= 4             # not one class for the whole run [10 - 18]
        R.assert_same_bits(one_p[pick].reshape(len(pick), -1), want_p.reshape(len(pick), -1), (name, n, "wave", w, "passes"))
        R.assert_same_bits(one_s[pick].reshape(len(pick), 1), want_s.reshape(len(pick), 1), (name, n, "wave", w, "spent"))
