"""Weighted direct-light queries past one workgroup: the fixtures of tests/direct_mis_cases.py tiled (item i = item i mod the fixture's
length, every i with RNG streams of its own) through the device form, with guards, on the Cornell box with the lowered lamp (scene in LDS,
lock-step list; 20 ceiling surfels beside the lamp and 40 floor surfels, the scene's own table) and on the grid with lights (global
memory, 16-byte nodes; the 324 items and the table of tests/direct_cases.py): BALANCE on 100 003 items (K = 2), POWER on the smallest
batch whose runs grow past 256 items on the device at hand (K = 1).

Each result is compared byte for byte with the concatenation of the same query made in chunks by items (first_stream + a * K: other runs,
other lanes, the same bytes), the ray counts add up, and 2 000 randomly chosen items - the first and the last among them - are compared
with the oracle restatement."""
import numpy as np
import pytest

import direct_mis_cases as M
import test_gpu_queries as G

pytestmark = pytest.mark.gpu

SEED, FIRST = M.SEED, M.FIRST_STREAM
GUARD = 64
FILL = 0xCD
SCENES = ("cornell_lowered", "grid3000_lit")
PICKED = 2000


@pytest.fixture(scope="module")
def scene(trt, orc):
    cache = {}

    def get(name):
        if name not in cache:
            if name == "cornell_lowered":
                desc, ow, items, table = M.lowered_cornell(trt, orc)
                shape = G.DEFAULT_SHAPES["cornell"]
            else:
                ref = M.scene(trt, orc, name)
                desc, ow, items, table = ref["desc"], ref["ow"], ref["items"], ref["table"]
                shape = G.DEFAULT_SHAPES["grid3000"]
            sc = trt.world_from_description(desc)[0].get_bvh()
            assert G.plan_shape(sc.direct_plan(1, mis="balance")) == shape
            cache[name] = dict(desc=desc, ow=ow, items=items, table=table, scene=sc)
        return cache[name]

    return get


def on_device(torch, c, d_items, n, d_table, k, first_stream, mis):
    """(radiance [n, 3], moment2 [n, 3], samples, rays) of the device form on guarded buffers; the guards asserted."""
    d_s = torch.full(((GUARD + n + GUARD) * 12,), FILL, dtype=torch.uint8, device="cuda:0")
    d_m = torch.full(((GUARD + n + GUARD) * 12,), FILL, dtype=torch.uint8, device="cuda:0")
    ctr = torch.zeros(16, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    c["scene"].direct_device(d_items, n, d_table.data_ptr(), len(c["table"]), d_s.data_ptr() + GUARD * 12, d_m.data_ptr() + GUARD * 12,
                             d_counters_ptr=ctr.data_ptr(), samples_per_item=k, seed=SEED, first_stream=first_stream, mis=mis)
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
    assert samples == n * k and samples <= rays <= 2 * samples              # one lobe ray per sample, at most one shadow walk
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
    ref = M.finish(M.samples(orc, c["ow"], c["desc"], items[pick], c["table"], heuristic=M.HEURISTICS[mis], k=k, item_index=pick), k)
    # not vacuous: on the grid about 3 % of the samples are lit and as many lobe rays find a light (tests/README_direct_mis.md)
    assert ref["has_l"].sum() >= 50 and (ref["has_b"] & (ref["wb"] < 1)).sum() >= 50 and (ref["has_l"] & (ref["wl"] < 1)).sum() >= 50
    M.assert_same_bits(one_s[pick], ref["S"], (name, n, "radiance"))
    M.assert_same_bits(one_m[pick], ref["M"], (name, n, "moment2"))


@pytest.mark.parametrize("name", SCENES)
def test_100003_items_equal_their_chunks_and_the_oracle(trt, orc, scene, name):
    import torch
    c = scene(name)
    n = 100003
    q = c["scene"].direct_plan(n, mis="balance")
    assert q["workgroups"] >= 2 and q["waves"] * q["rays_per_wave"] >= n
    check(torch, orc, c, name, n, 2, (257, 50001, 99999), "balance")


@pytest.mark.parametrize("name", SCENES)
def test_a_batch_with_lengthened_runs(trt, orc, scene, name):
    import torch
    c = scene(name)
    sc = c["scene"]
    q1 = sc.direct_plan(1, mis="power")
    assert q1["rays_per_wave"] == 256
    n = 256 * q1["wave_slots"] + 1                                          # ceil(n / 256) exceeds the resident wave slots
    assert sc.direct_plan(n - 1, mis="power")["rays_per_wave"] == 256
    q = sc.direct_plan(n, mis="power")
    per_wave, waves = q["rays_per_wave"], q["waves"]
    assert per_wave > 256 and q["workgroups"] >= 2 and (waves - 1) * per_wave < n <= waves * per_wave
    check(torch, orc, c, name, n, 1, (n // 2 | 1,), "power")
