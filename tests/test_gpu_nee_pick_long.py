"""Alias-table next-event queries past one workgroup: tests/test_gpu_nee_long.py's batch - 100 003 items, the 324 surfels of
tests/passes_cases.py tiled (item i = item i mod 324, every i with RNG streams of its own), many times 256 x the wave slots of one
workgroup, so that every wave's run refills - through the device forms, with guards, K = 2, B = 5, one lobe source per kernel shape (cosine
and cone in turn over the six shapes of tests/test_gpu_nee_pick.py), trt_nee_pick and trt_nee_mis_pick (BALANCE) each.

Each result is compared byte for byte with the concatenation of the same query made in chunks by items, the counts add up, and 600 randomly
chosen items - the first and the last among them - are compared with the oracle restatement (tests/nee_pick_cases.py)."""
import numpy as np
import pytest

import gather_cases as GC
import nee_pick_cases as NP
import test_gpu_nee_long as L
import test_gpu_nee_pick as T
import test_gpu_queries as G

pytestmark = pytest.mark.gpu

SEED, FIRST, DEPTH = NP.SEED, NP.FIRST_STREAM, NP.MAX_BOUNCES
GUARD, FILL = L.GUARD, L.FILL
N_LONG, K_LONG = 100003, 2
PICKED = 600
BY_SHAPE = [(c, ("cosine", "cone")[i % 2]) for i, c in enumerate(T.CASES)]
IDS = ["%s-%s" % (i, s) for i, (_, s) in zip(T.IDS, BY_SHAPE)]


def on_device(torch, c, source, d_items, n, d_table, d_pick, first_stream, mis):
    """(radiance [n, 3], moment2 [n, 3], samples, rays) of the device form on guarded buffers; the guards asserted."""
    d_s = torch.full(((GUARD + n + GUARD) * 12,), FILL, dtype=torch.uint8, device="cuda:0")
    d_m = torch.full(((GUARD + n + GUARD) * 12,), FILL, dtype=torch.uint8, device="cuda:0")
    ctr = torch.zeros(16, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    c["scene"].nee_device(d_items, n, d_table.data_ptr(), len(c["mine"]), d_s.data_ptr() + GUARD * 12, d_m.data_ptr() + GUARD * 12,
                          d_counters_ptr=ctr.data_ptr(), samples_per_item=K_LONG, source=source, spread=NP.SPREAD, max_bounces=DEPTH,
                          background=c["bg"], seed=SEED, first_stream=first_stream, mis=mis,
                          pick=d_pick.data_ptr() if mis is None else (d_pick.data_ptr(), c["total"]))
    torch.cuda.synchronize()
    out = []
    for t in (d_s, d_m):
        h = t.cpu().numpy()
        g, b = GUARD * 12, n * 12
        assert (h[:g] == FILL).all() and (h[g + b:] == FILL).all(), (n, "guard bytes were written")
        out.append(h[g:g + b].copy().view(np.float32).reshape(n, 3))
    assert not bool(ctr[2:].any())
    return out[0], out[1], int(ctr[0]), int(ctr[1])


@pytest.mark.parametrize("mis", (None, "balance"))
@pytest.mark.parametrize("cse,source", BY_SHAPE, ids=IDS)
def test_100003_items_equal_their_chunks_and_the_oracle(trt, orc, case, cse, source, mis):
    import torch
    name, options, shape = cse
    c = case(name, options, shape)
    n, k = N_LONG, K_LONG
    q = c["scene"].nee_plan(n, mis=mis, pick=True)
    assert G.plan_shape(q) == shape
    # more items than 256 x the wave slots of one workgroup, and than the device's resident slots x 256: runs are lengthened and refill
    assert q["workgroups"] >= 2 and q["waves"] * q["rays_per_wave"] >= n and n > 256 * (shape[2] // 64)
    base = c[source]["items"]
    index = np.arange(n) % len(base)
    items = np.ascontiguousarray(base[index])
    d_items = torch.from_numpy(items).to("cuda:0")
    d_table, d_pick = T.padded(torch, c["mine"]), T.padded(torch, c["pick"])
    one_s, one_m, samples, rays = on_device(torch, c, source, d_items.data_ptr(), n, d_table, d_pick, FIRST, mis)
    assert samples == n * k and samples <= rays <= 2 * DEPTH * samples
    parts, part_rays = [], 0
    cuts = (257, 50001, 99999)
    for a, b in zip((0,) + cuts, cuts + (n,)):
        s, m, smp, r = on_device(torch, c, source, d_items.data_ptr() + 24 * a, b - a, d_table, d_pick, FIRST + a * k, mis)
        assert smp == (b - a) * k
        parts.append((s, m))
        part_rays += r
    assert np.concatenate([p[0] for p in parts]).tobytes() == one_s.tobytes(), (name, "radiance in chunks")
    assert np.concatenate([p[1] for p in parts]).tobytes() == one_m.tobytes(), (name, "moment2 in chunks")
    assert part_rays == rays
    chosen = np.unique(np.concatenate([[0, n - 1], np.random.default_rng(n).integers(0, n, PICKED - 2)]))
    rays6 = np.zeros((len(chosen), k, 6), np.float32)
    for r, i in enumerate(chosen):
        rays6[r] = GC.first_rays(orc, items[i:i + 1], source, k, NP.SPREAD, SEED, FIRST + int(i) * k)[0]
    kw = {} if mis is None else dict(heuristic=NP.HEURISTICS[mis], total_power=c["nee_total"])
    ref = NP.finish(NP.pick_paths(orc, c["ow"], c["desc"], rays6, c["nee_table"], c["nee_pick"], background=c["bg"], item_index=chosen, **kw), k)
    assert ref["walks"].sum() >= ref["lit"].sum() > 0 and ref["alias_taken"].sum() > 0, (int(ref["lit"].sum()), int(ref["walks"].sum()))
    NP.assert_same_bits(one_s[chosen], ref["S"], (name, source, mis, "radiance"))
    NP.assert_same_bits(one_m[chosen], ref["M"], (name, source, mis, "moment2"))


case = T.case
