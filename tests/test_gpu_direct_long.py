"""Direct-light queries past one workgroup: the 324 items of tests/gather_cases.py tiled (item i = item i mod 324; 324 is no power of two, so
every wave sees another phase of lane mixes, refills and parked stragglers; every i has RNG streams of its own, so no two samples repeat)
through the device form, with guards, on cornell (scene in LDS, lock-step list) and grid3000 (global memory, 16-byte nodes), against the
table of tests/direct_cases.py.

100 003 items with K = 2, and the smallest n at which a wave's run grows past 256 items on the device at hand (some millions) with K = 1.
Each result is compared byte for byte with the concatenation of the same query made in chunks by items (first_stream + a * K: other runs,
other lanes, the same bytes), and 2 000 randomly chosen items - the first and the last among them - with the oracle restatement."""
import numpy as np
import pytest

import direct_cases as D
import gather_cases as GC
import test_gpu_queries as G
import walk_ray_cases as W

pytestmark = pytest.mark.gpu

SEED, FIRST = D.SEED, D.FIRST_STREAM
GUARD = 64
FILL = 0xCD
SCENES = ("cornell", "grid3000")
PICKED = 2000


@pytest.fixture(scope="module")
def scene(trt, orc):
    cache = {}

    def get(name):
        if name not in cache:
            desc = W.scene(trt, name)
            ow = orc.world_from_description(desc)[0]
            sc = trt.world_from_description(desc)[0].get_bvh()
            assert G.plan_shape(sc.direct_plan(1)) == G.DEFAULT_SHAPES[name]
            items, _ = GC.items_of(orc, ow, desc)
            table = trt.lights.table(sc.emitters(), trt.lights.quad(**D.VIRTUAL_QUAD), trt.lights.sphere(**D.VIRTUAL_SPHERE))
            assert table.tobytes() == D.table_of(orc, desc).tobytes()
            cache[name] = dict(ow=ow, scene=sc, items=items, table=table)
        return cache[name]

    return get


def on_device(torch, sc, d_items, n, d_table, n_emitters, k, first_stream):
    """(radiance [n, 3], moment2 [n, 3], samples, walks) of the device form on guarded buffers; the guards asserted."""
    d_s = torch.full(((GUARD + n + GUARD) * 12,), FILL, dtype=torch.uint8, device="cuda:0")
    d_m = torch.full(((GUARD + n + GUARD) * 12,), FILL, dtype=torch.uint8, device="cuda:0")
    ctr = torch.zeros(16, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    sc.direct_device(d_items, n, d_table.data_ptr(), n_emitters, d_s.data_ptr() + GUARD * 12, d_m.data_ptr() + GUARD * 12,
                     d_counters_ptr=ctr.data_ptr(), samples_per_item=k, seed=SEED, first_stream=first_stream)
    torch.cuda.synchronize()
    out = []
    for t in (d_s, d_m):
        h = t.cpu().numpy()
        g, b = GUARD * 12, n * 12
        assert (h[:g] == FILL).all() and (h[g + b:] == FILL).all(), (n, "guard bytes were written")
        out.append(h[g:g + b].copy().view(np.float32).reshape(n, 3))
    assert not bool(ctr[2:].any())
    return out[0], out[1], int(ctr[0]), int(ctr[1])


def check(torch, orc, c, name, n, k, cuts):
    sc = c["scene"]
    items = np.ascontiguousarray(c["items"][np.arange(n) % len(c["items"])])
    d_items = torch.from_numpy(items).to("cuda:0")
    d_table = torch.from_numpy(c["table"].view(np.uint8).copy()).to("cuda:0")
    E = len(c["table"])
    one_s, one_m, samples, walks = on_device(torch, sc, d_items.data_ptr(), n, d_table, E, k, FIRST)
    assert samples == n * k and 0 < walks <= samples
    # the same query in chunks by items
    parts, part_walks = [], 0
    for a, b in zip((0,) + cuts, cuts + (n,)):
        s, m, smp, w = on_device(torch, sc, d_items.data_ptr() + 24 * a, b - a, d_table, E, k, FIRST + a * k)
        assert smp == (b - a) * k
        parts.append((s, m))
        part_walks += w
    assert np.concatenate([p[0] for p in parts]).tobytes() == one_s.tobytes(), (name, n, "radiance in chunks")
    assert np.concatenate([p[1] for p in parts]).tobytes() == one_m.tobytes(), (name, n, "moment2 in chunks")
    assert part_walks == walks
    # randomly chosen items against the oracle
    pick = np.unique(np.concatenate([[0, n - 1], np.random.default_rng(n).integers(0, n, PICKED - 2)]))
    ref = D.reference(orc, c["ow"], items[pick], c["table"], k=k, item_index=pick)
    lit = ref["live"] & ~ref["occ"]
    assert 0.3 * len(pick) * k < lit.sum() < len(pick) * k and (ref["occ"]).sum() > 20, (int(lit.sum()), int(ref["occ"].sum()))
    D.assert_same_bits(one_s[pick], ref["S"], (name, n, "radiance"))
    D.assert_same_bits(one_m[pick], ref["M"], (name, n, "moment2"))


@pytest.mark.parametrize("name", SCENES)
def test_100003_items_equal_their_chunks_and_the_oracle(trt, orc, scene, name):
    import torch
    c = scene(name)
    n = 100003
    q = c["scene"].direct_plan(n)
    assert q["workgroups"] >= 2 and q["waves"] * q["rays_per_wave"] >= n
    check(torch, orc, c, name, n, 2, (257, 50001, 99999))


@pytest.mark.parametrize("name", SCENES)
def test_a_batch_with_lengthened_runs(trt, orc, scene, name):
    import torch
    c = scene(name)
    sc = c["scene"]
    q1 = sc.direct_plan(1)
    assert q1["rays_per_wave"] == 256
    n = 256 * q1["wave_slots"] + 1                                          # ceil(n / 256) exceeds the resident wave slots
    assert sc.direct_plan(n - 1)["rays_per_wave"] == 256
    q = sc.direct_plan(n)
    per_wave, waves = q["rays_per_wave"], q["waves"]
    assert per_wave > 256 and q["workgroups"] >= 2 and (waves - 1) * per_wave < n <= waves * per_wave
    check(torch, orc, c, name, n, 1, (n // 2 | 1,))
