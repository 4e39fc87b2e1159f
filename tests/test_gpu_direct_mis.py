"""Weighted direct-light queries (tinyrt.h trt_direct_mis, trt_direct_mis_device) on the GPU against the CPU oracle, bit for bit and item by
item.

The reference is tests/direct_mis_cases.py: direct_cases' shadow sample with the weight wl, and a cosine-lobe ray from the surfel on stream
(seed, j, 0xFFFFFFFF) whose hit on a light counts with wb.  Items, streams and table are tests/test_gpu_direct.py's: 324 surfels per scene
(a full run of 256 and a ragged one of 68, with the NaN, zero, inf and 1e-9 items), K = 8, seed 5, first_stream 1000, the scene's own
emitters followed by a virtual quad and a virtual sphere.  One scene per kernel shape, with the shape and launch bound that
Scene.direct_plan(n, mis=...) reports asserted, so all six instantiations of direct.hip kDirectKernels[pick][mis], the weighted tables run; random_spheres and grid3000
are the variants with lights of direct_mis_cases.with_lights.  BALANCE on all six, POWER on the two whose fixtures hold the most weighted
terms (tests/README_direct_mis.md).  tests/test_direct_mis_cases.py asserts without a GPU that this reference is not vacuous."""
import numpy as np
import pytest

import direct_cases as D
import direct_mis_cases as M
import test_gpu_queries as G

pytestmark = pytest.mark.gpu

K, SEED, FIRST = M.K, M.SEED, M.FIRST_STREAM
N = M.N_ITEMS
GUARD = 64                                                                  # entries on either side of a device buffer
FILL = 0xCD
# direct.hip kDirectKernels[pick][mis], the weighted tables: (scene mode, walk, threads) -> launch bound (profiles/direct_mis_resource_usage.txt)
BOUNDS = {(1, 2, 256): 5, (1, 1, 256): 7, (1, 1, 768): 7, (1, 5, 512): 5, (0, 3, 256): 7, (0, 5, 256): 5}
KW = dict(samples_per_item=K, seed=SEED, first_stream=FIRST)


def shape_of(stock, options):
    if not options:
        return G.DEFAULT_SHAPES[stock]
    return [s for n, o, s in G.OTHER_WALKS if n == stock and o == options][0]


CASES = [(name, options, shape_of(stock, options)) for name, stock, options in M.CASES]
IDS = ["%s-%s" % (name, "-".join("%s=%s" % kv for kv in sorted(options.items())) or "default") for name, options, _ in CASES]
# the two shapes whose fixtures hold the most weighted terms (lobe hits with wb < 1 plus shadow terms with wl < 1: cornell 679,
# prims33 618, random_spheres_lit 311, grid3000_lit 174, prims600 52; tests/README_direct_mis.md)
POWER_CASES = [c for c in CASES if c[0] in ("cornell", "prims33")]
BY_HEURISTIC = [(c, "balance") for c in CASES] + [(c, "power") for c in POWER_CASES]
BH_IDS = [i + "-balance" for i in IDS] + [i + "-power" for i, c in zip(IDS, CASES) if c in POWER_CASES]


@pytest.fixture(scope="module")
def case(trt, orc):
    """(name, options) -> the scene's fixtures (direct_mis_cases.scene: computed once, never changed), the product scene compiled with the
    options, the shape and bound of the weighted plan asserted, and the product's own table, which must be the restatement's byte for
    byte."""
    cache = {}

    def get(name, options, shape):
        key = (name, tuple(sorted(options.items())))
        if key not in cache:
            sc = M.scene(trt, orc, name)
            scene = trt.world_from_description(sc["desc"])[0].get_bvh(**options)
            for mis in ("balance", "power"):
                q = scene.direct_plan(N, mis=mis)
                assert G.plan_shape(q) == shape, (name, options, q)
                assert q["kernel_waves_per_simd"] == BOUNDS[shape[:3]], (name, options, q)
            mine = trt.lights.table(scene.emitters(), trt.lights.quad(**D.VIRTUAL_QUAD), trt.lights.sphere(**D.VIRTUAL_SPHERE))
            assert mine.tobytes() == sc["table"].tobytes(), (name, options)
            cache[key] = dict(sc, name=name, scene=scene, mine=mine)
        return cache[key]

    return get


def sentinels(n=N):
    return np.full((n, 3), 7.5, np.float32), np.full((n, 3), 7.5, np.float32)


def want_of(trt, orc, name, mis):
    return M.reference(trt, orc, name, heuristic=M.HEURISTICS[mis])


@pytest.mark.parametrize("cse,mis", BY_HEURISTIC, ids=BH_IDS)
def test_host_form_is_the_oracles_fold(trt, orc, case, cse, mis):
    name, options, shape = cse
    c = case(name, options, shape)
    want = want_of(trt, orc, name, mis)
    plain = M.reference(trt, orc, name, plain=True)
    S, M2 = sentinels()
    S, M2, st = c["scene"].direct(c["items"], c["mine"], radiance=S, moment2=M2, mis=mis, **KW)
    M.assert_same_bits(S, want["S"], (name, options, mis, "radiance"))
    M.assert_same_bits(M2, want["M"], (name, options, mis, "moment2"))
    assert st["samples"] == N * K and st["rays"] == want["n_rays"] == want["n_walks"] + N * K, (name, options, st, want["n_rays"])
    # moment2 = NULL: radiance is unchanged
    S1, none, st1 = c["scene"].direct(c["items"], c["mine"], mis=mis, **KW)
    assert none is None and S1.tobytes() == S.tobytes()
    assert st1["samples"] == N * K and st1["rays"] == want["n_rays"]
    # mis=None returns the bytes it returned before (tests/test_gpu_direct.py's job too), and where a term is weighted the two differ
    S0, M0, st0 = c["scene"].direct(c["items"], c["mine"], moment2=True, **KW)
    M.assert_same_bits(S0, plain["S"], (name, options, "mis=None"))
    M.assert_same_bits(M0, plain["M"], (name, options, "mis=None"))
    assert st0["samples"] == N * K and st0["rays"] == want["n_walks"]
    assert M.differing(want["S"], plain["S"]) > 0 and S0.tobytes() != S.tobytes()


def device_buffer(torch, n):
    return torch.full(((GUARD + n + GUARD) * 12,), FILL, dtype=torch.uint8, device="cuda:0")


def payload(t, n):
    """(payload as float32 [n, 3], guards intact?)"""
    h = t.cpu().numpy()
    g, b = GUARD * 12, n * 12
    return h[g:g + b].copy().view(np.float32).reshape(n, 3), bool((h[:g] == FILL).all() and (h[g + b:] == FILL).all())


@pytest.mark.parametrize("cse,mis", BY_HEURISTIC, ids=BH_IDS)
def test_device_form_on_a_side_stream_equals_the_oracle_and_leaves_the_guards(trt, orc, case, cse, mis):
    import torch
    name, options, shape = cse
    c = case(name, options, shape)
    want = want_of(trt, orc, name, mis)
    E = len(c["mine"])
    d_items = torch.from_numpy(c["items"].copy()).to("cuda:0")
    d_table = torch.from_numpy(c["mine"].view(np.uint8).copy()).to("cuda:0")
    side = torch.cuda.Stream()
    d_s, d_m = device_buffer(torch, N), device_buffer(torch, N)
    ctr = torch.full((16,), 3, dtype=torch.int64, device="cuda:0")          # the counters are added to
    torch.cuda.synchronize()
    c["scene"].direct_device(d_items.data_ptr(), N, d_table.data_ptr(), E, d_s.data_ptr() + GUARD * 12, d_m.data_ptr() + GUARD * 12,
                             d_counters_ptr=ctr.data_ptr(), stream_ptr=side.cuda_stream, mis=mis, **KW)
    side.synchronize()
    torch.cuda.synchronize()
    got_s, ok_s = payload(d_s, N)
    got_m, ok_m = payload(d_m, N)
    assert ok_s and ok_m, (name, options, "guard bytes were written")
    M.assert_same_bits(got_s, want["S"], (name, options, mis, "radiance"))
    M.assert_same_bits(got_m, want["M"], (name, options, mis, "moment2"))
    assert int(ctr[0]) == 3 + N * K and int(ctr[1]) == 3 + want["n_rays"] and bool((ctr[2:] == 3).all())
    # without moment2 and without counters: the same radiance, the guards intact
    d_s1 = device_buffer(torch, N)
    c["scene"].direct_device(d_items.data_ptr(), N, d_table.data_ptr(), E, d_s1.data_ptr() + GUARD * 12, mis=mis, **KW)
    torch.cuda.synchronize()
    got_s1, ok_s1 = payload(d_s1, N)
    assert ok_s1 and got_s1.tobytes() == got_s.tobytes()


@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_split_by_samples_leaves_the_bytes_of_one_pass(trt, orc, case, name, options, shape):
    c = case(name, options, shape)
    want = want_of(trt, orc, name, "balance")
    kw = dict(KW, mis="balance")
    walks3 = int(want["walked"][:, :3].sum())
    S, M2 = sentinels()
    _, _, st = c["scene"].direct(c["items"], c["mine"], sample_begin=0, sample_end=3, radiance=S, moment2=M2, **kw)
    S3, M3 = M.fold(want, K, 0, 3)
    M.assert_same_bits(S, S3, (name, options, "radiance [0, 3)"))
    M.assert_same_bits(M2, M3, (name, options, "moment2 [0, 3)"))
    assert st["samples"] == N * 3 and st["rays"] == walks3 + N * 3
    _, _, st = c["scene"].direct(c["items"], c["mine"], sample_begin=3, sample_end=8, accumulate=True, radiance=S, moment2=M2, **kw)
    M.assert_same_bits(S, want["S"], (name, options, "radiance [0, 3) + [3, 8)"))
    M.assert_same_bits(M2, want["M"], (name, options, "moment2 [0, 3) + [3, 8)"))
    assert st["samples"] == N * 5 and st["rays"] == want["n_rays"] - walks3 - N * 3


@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_split_by_items_leaves_the_bytes_of_one_call(trt, orc, case, name, options, shape):
    c = case(name, options, shape)
    want = want_of(trt, orc, name, "balance")
    kw = dict(KW, mis="balance")
    one_s, one_m, _ = c["scene"].direct(c["items"], c["mine"], moment2=True, **kw)
    S, M2 = sentinels()
    a = 100
    c["scene"].direct(c["items"][:a], c["mine"], radiance=S[:a], moment2=M2[:a], **kw)
    assert (S[a:] == 7.5).all() and (M2[a:] == 7.5).all()                   # entries outside the call's range are untouched
    kw["first_stream"] = FIRST + a * K
    head_s, head_m = S[:a].copy(), M2[:a].copy()
    c["scene"].direct(c["items"][a:], c["mine"], radiance=S[a:], moment2=M2[a:], **kw)
    assert S[:a].tobytes() == head_s.tobytes() and M2[:a].tobytes() == head_m.tobytes()
    assert S.tobytes() == one_s.tobytes() and M2.tobytes() == one_m.tobytes(), (name, options)          # byte for byte
    M.assert_same_bits(S, want["S"], (name, options, "radiance"))
    M.assert_same_bits(M2, want["M"], (name, options, "moment2"))


@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_an_empty_sample_range(trt, case, name, options, shape):
    """An empty sample range zeroes the n entries without accumulate and leaves them with it; through the device form no byte outside
    [0, 12 n) is written."""
    import torch
    c = case(name, options, shape)
    kw = dict(KW, sample_begin=3, sample_end=3)
    for accumulate in (False, True):
        S, M2 = sentinels()
        _, _, st = c["scene"].direct(c["items"], c["mine"], accumulate=accumulate, radiance=S, moment2=M2, mis="balance", **kw)
        want = 7.5 if accumulate else 0.0
        assert (S == want).all() and (M2 == want).all(), (name, options, accumulate)
        assert st["rays"] == 0 and st["samples"] == 0
    d_items = torch.from_numpy(c["items"].copy()).to("cuda:0")
    d_table = torch.from_numpy(c["mine"].view(np.uint8).copy()).to("cuda:0")
    for accumulate in (False, True):
        for with_m2 in (True, False):
            d_s, d_m = device_buffer(torch, N), device_buffer(torch, N)
            c["scene"].direct_device(d_items.data_ptr(), N, d_table.data_ptr(), len(c["mine"]), d_s.data_ptr() + GUARD * 12,
                                     d_m.data_ptr() + GUARD * 12 if with_m2 else 0, accumulate=accumulate, mis="power",
                                     **dict(KW, sample_begin=2, sample_end=2))
            torch.cuda.synchronize()
            for t, written in ((d_s, True), (d_m, with_m2)):
                got, ok = payload(t, N)
                assert ok, (name, options, "guard bytes were written")
                assert (got.view(np.uint32) == (0 if written and not accumulate else 0xCDCDCDCD)).all()


@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_identities_2_and_3_the_counters_are_directs_plus_a_one_bounce_gathers(trt, case, name, options, shape):
    c = case(name, options, shape)
    _, _, st_d = c["scene"].direct(c["items"], c["mine"], **KW)
    _, _, st_g = c["scene"].gather(c["items"], samples_per_item=K, lobe="cosine", max_bounces=1, background=(0.0, 0.0, 0.0), seed=SEED,
                                   first_stream=FIRST)
    for mis in ("balance", "power"):
        _, _, st = c["scene"].direct(c["items"], c["mine"], mis=mis, **KW)
        assert st["samples"] == st_d["samples"] == N * K
        assert st["rays"] == st_d["rays"] + st_g["rays"], (name, options, mis, st, st_d, st_g)


def test_identity_1_with_virtual_emitters_only_the_result_is_trt_directs_on_the_device(trt, orc):
    """The stock random_spheres scene holds no TRT_LIGHT geometry and its table is the two virtual emitters: trt_direct's bytes for both
    heuristics, while every sample walks its lobe ray."""
    import gather_cases as GC
    import walk_ray_cases as W
    desc = W.scene(trt, "random_spheres")
    ow, _ = orc.world_from_description(desc)
    items, _ = GC.items_of(orc, ow, desc)
    scene = trt.world_from_description(desc)[0].get_bvh()
    table = trt.lights.table(scene.emitters(), trt.lights.quad(**D.VIRTUAL_QUAD), trt.lights.sphere(**D.VIRTUAL_SPHERE))
    assert len(table) == 2 and (table["geometry"] == D.NO_GEOMETRY).all()
    S0, M0, st0 = scene.direct(items, table, moment2=True, **KW)
    assert (S0[np.isfinite(S0)] != 0).any()
    for mis in ("balance", "power"):
        S, M2, st = scene.direct(items, table, moment2=True, mis=mis, **KW)
        assert S.tobytes() == S0.tobytes() and M2.tobytes() == M0.tobytes(), mis
        assert st["samples"] == st0["samples"] and st["rays"] == st0["rays"] + N * K


@pytest.mark.parametrize("mis", sorted(M.HEURISTICS))
def test_the_lowered_box_with_its_ceiling_surfels(trt, orc, mis):
    """The Cornell box with the lamp at y = 99, the scene's own table (E = 1): 20 ceiling surfels one unit above the lamp, where about
    30 % of the lobe rays reach it and a shadow sample that lands close weighs less than the lobe ray would, and 40 floor surfels."""
    desc, ow, items, table = M.lowered_cornell(trt, orc)
    scene = trt.world_from_description(desc)[0].get_bvh()
    assert scene.emitters().tobytes() == table.tobytes()
    want = M.finish(M.samples(orc, ow, desc, items, table, heuristic=M.HEURISTICS[mis]), K)
    assert 0.2 < want["has_b"][:20].mean() < 0.4 and (want["wl"][:20][want["has_l"][:20]] < 0.5).any()
    assert (want["has_l"][:20] & want["has_b"][:20]).sum() >= 10
    S, M2, st = scene.direct(items, table, moment2=True, mis=mis, **KW)
    M.assert_same_bits(S, want["S"], (mis, "radiance"))
    M.assert_same_bits(M2, want["M"], (mis, "moment2"))
    assert st["samples"] == len(items) * K and st["rays"] == want["n_rays"]
    if mis == "balance":
        assert S[:20].max() <= 30.0 * (1 + 1e-6)                            # a mean of samples that are each within the bound
