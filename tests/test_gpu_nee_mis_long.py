"""Weighted next-event queries past one workgroup: tests/test_gpu_nee_long.py's batches - the 324 surfels of tests/passes_cases.py tiled
(item i = item i mod 324, every i with RNG streams of its own) through the device form, with guards, on cornell (scene in LDS, lock-step
list) and grid3000 (global memory, 16-byte nodes), cosine source, B = 5, against the table of tests/direct_cases.py - with the weights of
tinyrt.h trt_nee_mis: BALANCE on the 100 003 items (K = 2), POWER on the lengthened runs (K = 1).

Each result is compared byte for byte with the concatenation of the same query made in chunks by items, the counts add up, and 2 000
randomly chosen items - the first and the last among them - are compared with the oracle restatement (tests/nee_mis_cases.py)."""
import numpy as np
import pytest

import nee_mis_cases as M
import test_gpu_nee_long as L
import test_gpu_queries as G

pytestmark = pytest.mark.gpu

SEED, FIRST, DEPTH = M.SEED, M.FIRST_STREAM, M.MAX_BOUNCES
GUARD, FILL = L.GUARD, L.FILL
SCENES = L.SCENES
PICKED = L.PICKED


@pytest.fixture(scope="module")
def scene(trt, orc):
    cache = {}

    def get(name):
        if name not in cache:
            ref = M.scene(trt, orc, name)
            sc = trt.world_from_description(ref["desc"])[0].get_bvh()
            assert G.plan_shape(sc.nee_plan(1, mis="balance")) == G.DEFAULT_SHAPES[name]
            cache[name] = dict(ref, scene=sc, items=ref["cosine"]["items"], table=ref["nee_table"])
        return cache[name]

    return get


def on_device(torch, c, d_items, n, d_table, k, first_stream, mis):
    """(radiance [n, 3], moment2 [n, 3], samples, rays) of the device form on guarded buffers; the guards asserted."""
    d_s = torch.full(((GUARD + n + GUARD) * 12,), FILL, dtype=torch.uint8, device="cuda:0")
    d_m = torch.full(((GUARD + n + GUARD) * 12,), FILL, dtype=torch.uint8, device="cuda:0")
    ctr = torch.zeros(16, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    c["scene"].nee_device(d_items, n, d_table.data_ptr(), len(c["table"]), d_s.data_ptr() + GUARD * 12, d_m.data_ptr() + GUARD * 12,
                          d_counters_ptr=ctr.data_ptr(), samples_per_item=k, source="cosine", max_bounces=DEPTH, background=c["bg"], seed=SEED,
                          first_stream=first_stream, mis=mis)
    torch.cuda.synchronize()
    out = []
    for t in (d_s, d_m):
        h = t.cpu().numpy()
        g, b = GUARD * 12, n * 12
        assert (h[:g] == FILL).all() and (h[g + b:] == FILL).all(), (n, "guard bytes were written")
        out.append(h[g:g + b].copy().view(np.float32).reshape(n, 3))
    assert not bool(ctr[2:].any())
    return out[0], out[1], int(ctr[0]), int(ctr[1])


def check(torch, orc, c, name, n, k, cuts, mis):
    index = np.arange(n) % len(c["items"])
    items = np.ascontiguousarray(c["items"][index])
    d_items = torch.from_numpy(items).to("cuda:0")
    d_table = torch.from_numpy(c["table"].view(np.uint8).copy()).to("cuda:0")
    one_s, one_m, samples, rays = on_device(torch, c, d_items.data_ptr(), n, d_table, k, FIRST, mis)
    assert samples == n * k and samples <= rays <= 2 * DEPTH * samples
    # the same query in chunks by items
    parts, part_rays = [], 0
    for a, b in zip((0,) + cuts, cuts + (n,)):
        s, m, smp, r = on_device(torch, c, d_items.data_ptr() + 24 * a, b - a, d_table, k, FIRST + a * k, mis)
        assert smp == (b - a) * k
        parts.append((s, m))
        part_rays += r
    assert np.concatenate([p[0] for p in parts]).tobytes() == one_s.tobytes(), (name, n, "radiance in chunks")
    assert np.concatenate([p[1] for p in parts]).tobytes() == one_m.tobytes(), (name, n, "moment2 in chunks")
    assert part_rays == rays
    # randomly chosen items against the oracle
    pick = np.unique(np.concatenate([[0, n - 1], np.random.default_rng(n).integers(0, n, PICKED - 2)]))
    rays6 = L.first_rays_of(orc, items, pick, k)
    ref = M.finish(M.mis_paths(orc, c["ow"], c["desc"], rays6, c["table"], background=c["bg"], item_index=pick, heuristic=M.HEURISTICS[mis]), k)
    assert (ref["lit"] > 0).sum() > 0.1 * len(pick) * k and ref["walks"].sum() > ref["lit"].sum(), (int(ref["lit"].sum()), int(ref["walks"].sum()))
    if name == "cornell":
        assert ref["weighted"].sum() >= 1                                   # the box's lamp was reached after a diffuse scatter
    M.assert_same_bits(one_s[pick], ref["S"], (name, n, "radiance"))
    M.assert_same_bits(one_m[pick], ref["M"], (name, n, "moment2"))


@pytest.mark.parametrize("name", SCENES)
def test_100003_items_equal_their_chunks_and_the_oracle(trt, orc, scene, name):
    import torch
    c = scene(name)
    n = 100003
    q = c["scene"].nee_plan(n, mis="balance")
    assert q["workgroups"] >= 2 and q["waves"] * q["rays_per_wave"] >= n
    check(torch, orc, c, name, n, 2, (257, 50001, 99999), "balance")


@pytest.mark.parametrize("name", SCENES)
def test_a_batch_with_lengthened_runs(trt, orc, scene, name):
    import torch
    c = scene(name)
    sc = c["scene"]
    q1 = sc.nee_plan(1, mis="power")
    assert q1["rays_per_wave"] == 256
    n = 256 * q1["wave_slots"] + 1                                          # ceil(n / 256) exceeds the resident wave slots
    assert sc.nee_plan(n - 1, mis="power")["rays_per_wave"] == 256
    q = sc.nee_plan(n, mis="power")
    per_wave, waves = q["rays_per_wave"], q["waves"]
    assert per_wave > 256 and q["workgroups"] >= 2 and (waves - 1) * per_wave < n <= waves * per_wave
    check(torch, orc, c, name, n, 1, (n // 2 | 1,), "power")
