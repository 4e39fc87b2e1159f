"""Direct-light queries that choose the emitter through an alias table (tinyrt.h trt_direct_pick, trt_direct_mis_pick and their device
forms) on the GPU against the CPU oracle, bit for bit and item by item.

The reference is tests/direct_pick_cases.py.  One scene per kernel shape - the scenes of tests/test_gpu_direct_mis.py, with the shape and
launch bound that Scene.direct_plan(n, mis=..., pick=True) reports asserted, so all twelve PICK instantiations of direct.hip run.  The
batch is the first 257 of the 324 surfels of direct_cases (past one wave's 256 items; the split by items cuts it at 65, past one wave
of lanes), K = 3, seed 5, first_stream 1000; the table is the scene's own emitters followed by a virtual quad and a virtual sphere,
quads and spheres mixed, and the pick table is the power table the library builds of it, which must be direct_pick_cases.build's bytes.
BALANCE on all six shapes, POWER on the two whose fixtures hold the most weighted terms.  E = 1 (the Cornell box's own table), E = 3
(its table with the virtual emitters) and E = 61 (the many-light room) are run besides."""
import numpy as np
import pytest

import direct_cases as D
import direct_mis_cases as M
import direct_pick_cases as P
import test_gpu_queries as G

pytestmark = pytest.mark.gpu

K, SEED, FIRST = 3, P.SEED, P.FIRST_STREAM
N = 257
CUT = 65
GUARD = 64                                                                  # entries on either side of a device buffer
FILL = 0xCD
# direct.hip kDirectKernels[pick][mis], the PICK tables: (scene mode, walk, threads) -> launch bound (profiles/direct_pick_resource_usage.txt)
BOUNDS = {None: {(1, 2, 256): 7, (1, 1, 256): 8, (1, 1, 768): 8, (1, 5, 512): 7, (0, 3, 256): 7, (0, 5, 256): 6},
          "mis": {(1, 2, 256): 5, (1, 1, 256): 7, (1, 1, 768): 7, (1, 5, 512): 5, (0, 3, 256): 7, (0, 5, 256): 5}}
KW = dict(samples_per_item=K, seed=SEED, first_stream=FIRST)


def shape_of(stock, options):
    if not options:
        return G.DEFAULT_SHAPES[stock]
    return [s for n, o, s in G.OTHER_WALKS if n == stock and o == options][0]


CASES = [(name, options, shape_of(stock, options)) for name, stock, options in M.CASES]
IDS = ["%s-%s" % (name, "-".join("%s=%s" % kv for kv in sorted(options.items())) or "default") for name, options, _ in CASES]
POWER_CASES = [c for c in CASES if c[0] in ("cornell", "prims33")]
# (case, mis): the plain PICK query and BALANCE on every shape, POWER on two
BY_QUERY = [(c, None) for c in CASES] + [(c, "balance") for c in CASES] + [(c, "power") for c in POWER_CASES]
BQ_IDS = [i + "-plain" for i in IDS] + [i + "-balance" for i in IDS] + [i + "-power" for i, c in zip(IDS, CASES) if c in POWER_CASES]

_REFERENCE = {}


def reference(orc, sc, name, mis):
    """The restatement over the batch, computed once per (scene, query) and never changed."""
    if ("base", name) not in _REFERENCE:
        _REFERENCE[("base", name)] = D.freeze(P.samples(orc, sc["ow"], sc["items"][:N], sc["table"], sc["pick"], k=K))
    base = _REFERENCE[("base", name)]
    if (name, mis) not in _REFERENCE:
        if mis is None:
            _REFERENCE[(name, mis)] = P.finish(dict(base), K, False)
        else:
            _REFERENCE[(name, mis)] = P.finish(P.mis_samples(orc, sc["ow"], sc["desc"], sc["items"][:N], sc["table"], sc["pick"], sc["total"],
                                                             heuristic=P.HEURISTICS[mis], k=K, base=base), K, True)
    return _REFERENCE[(name, mis)]


@pytest.fixture(scope="module")
def case(trt, orc):
    """(name, options) -> the scene's fixtures (direct_mis_cases.scene), the product scene compiled with the options, the shapes and bounds
    of the PICK plans asserted, the product's own emitter table and pick table, which must be the restatements' byte for byte."""
    cache = {}

    def get(name, options, shape):
        key = (name, tuple(sorted(options.items())))
        if key not in cache:
            sc = M.scene(trt, orc, name)
            scene = trt.world_from_description(sc["desc"])[0].get_bvh(**options)
            for mis, bounds in ((None, BOUNDS[None]), ("balance", BOUNDS["mis"]), ("power", BOUNDS["mis"])):
                q = scene.direct_plan(N, mis=mis, pick=True)
                assert G.plan_shape(q) == shape, (name, options, q)
                assert q["kernel_waves_per_simd"] == bounds[shape[:3]], (name, options, q)
            mine = trt.lights.table(scene.emitters(), trt.lights.quad(**D.VIRTUAL_QUAD), trt.lights.sphere(**D.VIRTUAL_SPHERE))
            assert mine.tobytes() == sc["table"].tobytes(), (name, options)
            pick, total = trt.lights.pick_table(mine)
            want_pick, want_total = P.build(sc["table"])
            assert pick.tobytes() == want_pick.tobytes() and total == want_total, (name, options)
            assert set(mine["kind"]) == {0, 1} and (mine["geometry"] == D.NO_GEOMETRY).any()
            cache[key] = dict(sc, name=name, scene=scene, mine=mine, pick=pick, total=total)
        return cache[key]

    return get


def sentinels(n=N):
    return np.full((n, 3), 7.5, np.float32), np.full((n, 3), 7.5, np.float32)


def pick_arg(c, mis):
    return c["pick"] if mis is None else (c["pick"], c["total"])


@pytest.mark.parametrize("cse,mis", BY_QUERY, ids=BQ_IDS)
def test_host_form_is_the_oracles_fold(trt, orc, case, cse, mis):
    name, options, shape = cse
    c = case(name, options, shape)
    want = reference(orc, c, name, mis)
    assert want["took_alias"].any() and not want["took_alias"].all()       # both branches of step 2
    S, M2 = sentinels()
    S, M2, st = c["scene"].direct(c["items"][:N], c["mine"], radiance=S, moment2=M2, mis=mis, pick=pick_arg(c, mis), **KW)
    P.assert_same_bits(S, want["S"], (name, options, mis, "radiance"))
    P.assert_same_bits(M2, want["M"], (name, options, mis, "moment2"))
    assert st["samples"] == N * K == want["n_samples"] and st["rays"] == want["n_rays"], (name, options, st, want["n_rays"])
    # moment2 = NULL: radiance is unchanged
    S1, none, st1 = c["scene"].direct(c["items"][:N], c["mine"], mis=mis, pick=pick_arg(c, mis), **KW)
    assert none is None and S1.tobytes() == S.tobytes() and st1["rays"] == want["n_rays"]
    # pick=None draws another emitter: the uniform query's bytes differ
    S0, _, _ = c["scene"].direct(c["items"][:N], c["mine"], mis=mis, **KW)
    assert S0.tobytes() != S.tobytes()


def device_buffer(torch, n):
    return torch.full(((GUARD + n + GUARD) * 12,), FILL, dtype=torch.uint8, device="cuda:0")


def payload(t, n):
    """(payload as float32 [n, 3], guards intact?)"""
    h = t.cpu().numpy()
    g, b = GUARD * 12, n * 12
    return h[g:g + b].copy().view(np.float32).reshape(n, 3), bool((h[:g] == FILL).all() and (h[g + b:] == FILL).all())


def on_device(torch, c, mis, pick, items=None, side=None, counters=None, **kw):
    """The device form over device copies of the case's buffers, the sums between guard words: (radiance, moment2, guards intact?)."""
    items = c["items"][:N] if items is None else items
    n = len(items)
    d_items = torch.from_numpy(items.copy()).to("cuda:0")
    d_table = torch.from_numpy(c["mine"].view(np.uint8).copy()).to("cuda:0")
    d_pick = torch.from_numpy(pick.view(np.uint8).copy()).to("cuda:0")
    d_s, d_m = device_buffer(torch, n), device_buffer(torch, n)
    torch.cuda.synchronize()
    c["scene"].direct_device(d_items.data_ptr(), n, d_table.data_ptr(), len(c["mine"]), d_s.data_ptr() + GUARD * 12, d_m.data_ptr() + GUARD * 12,
                             d_counters_ptr=0 if counters is None else counters.data_ptr(), stream_ptr=0 if side is None else side.cuda_stream,
                             mis=mis, pick=d_pick.data_ptr() if mis is None else (d_pick.data_ptr(), c["total"]), **dict(KW, **kw))
    if side is not None:
        side.synchronize()
    torch.cuda.synchronize()
    got_s, ok_s = payload(d_s, n)
    got_m, ok_m = payload(d_m, n)
    return got_s, got_m, ok_s and ok_m


@pytest.mark.parametrize("cse,mis", BY_QUERY, ids=BQ_IDS)
def test_device_form_on_a_side_stream_equals_the_oracle_and_leaves_the_guards(trt, orc, case, cse, mis):
    import torch
    name, options, shape = cse
    c = case(name, options, shape)
    want = reference(orc, c, name, mis)
    ctr = torch.full((16,), 3, dtype=torch.int64, device="cuda:0")          # the counters are added to
    got_s, got_m, ok = on_device(torch, c, mis, c["pick"], side=torch.cuda.Stream(), counters=ctr)
    assert ok, (name, options, "guard bytes were written")
    P.assert_same_bits(got_s, want["S"], (name, options, mis, "radiance"))
    P.assert_same_bits(got_m, want["M"], (name, options, mis, "moment2"))
    assert int(ctr[0]) == 3 + N * K and int(ctr[1]) == 3 + want["n_rays"] and bool((ctr[2:] == 3).all())


@pytest.mark.parametrize("cse,mis", BY_QUERY[:2 * len(CASES)], ids=BQ_IDS[:2 * len(CASES)])
def test_splits_by_samples_and_by_items_leave_the_bytes_of_one_call(trt, orc, case, cse, mis):
    name, options, shape = cse
    c = case(name, options, shape)
    want = reference(orc, c, name, mis)
    items = c["items"][:N]
    kw = dict(KW, mis=mis, pick=pick_arg(c, mis))
    lobes = 0 if mis is None else 1
    # samples [0, 2), then [2, 3) on top
    walks2 = int(want["walked"][:, :2].sum())
    S, M2 = sentinels()
    _, _, st = c["scene"].direct(items, c["mine"], sample_begin=0, sample_end=2, radiance=S, moment2=M2, **kw)
    fold = M.fold if mis else D.fold
    S2, M2_2 = fold(want, K, 0, 2)
    P.assert_same_bits(S, S2, (name, options, mis, "radiance [0, 2)"))
    P.assert_same_bits(M2, M2_2, (name, options, mis, "moment2 [0, 2)"))
    assert st["samples"] == N * 2 and st["rays"] == walks2 + lobes * N * 2
    _, _, st = c["scene"].direct(items, c["mine"], sample_begin=2, sample_end=3, accumulate=True, radiance=S, moment2=M2, **kw)
    P.assert_same_bits(S, want["S"], (name, options, mis, "radiance [0, 2) + [2, 3)"))
    P.assert_same_bits(M2, want["M"], (name, options, mis, "moment2 [0, 2) + [2, 3)"))
    assert st["samples"] == N and st["rays"] == want["n_rays"] - walks2 - lobes * N * 2
    # items [0, 65), then [65, 257) on their own streams
    S, M2 = sentinels()
    c["scene"].direct(items[:CUT], c["mine"], radiance=S[:CUT], moment2=M2[:CUT], **kw)
    assert (S[CUT:] == 7.5).all() and (M2[CUT:] == 7.5).all()               # entries outside the call's range are untouched
    c["scene"].direct(items[CUT:], c["mine"], radiance=S[CUT:], moment2=M2[CUT:], **dict(kw, first_stream=FIRST + CUT * K))
    P.assert_same_bits(S, want["S"], (name, options, mis, "radiance by items"))
    P.assert_same_bits(M2, want["M"], (name, options, mis, "moment2 by items"))


@pytest.mark.parametrize("cse,mis", BY_QUERY[:2 * len(CASES)], ids=BQ_IDS[:2 * len(CASES)])
def test_device_form_clamps_aliases_past_the_table(trt, orc, case, cse, mis):
    """A table whose aliases are all 0xFFFFFFFF has defined output: step 2's min sends every alias to record E - 1.  The host form
    rejects the table; the device form - of both queries, on every kernel shape - returns the restatement's bytes and reads nothing
    outside the E records."""
    import torch
    name, options, shape = cse
    c = case(name, options, shape)
    wrong = c["pick"].copy()
    wrong["alias"] = 0xFFFFFFFF
    base = P.samples(orc, c["ow"], c["items"][:N], c["table"], wrong, k=K)
    if mis is None:
        want = P.finish(dict(base), K, False)
    else:
        want = P.finish(P.mis_samples(orc, c["ow"], c["desc"], c["items"][:N], c["table"], wrong, c["total"], heuristic=P.HEURISTICS[mis], k=K,
                                      base=base), K, True)
    E = len(c["mine"])
    assert (want["e"][want["took_alias"]] == E - 1).all() and want["took_alias"].sum() > 50
    assert P.differing(want["S"], reference(orc, c, name, mis)["S"]) > 0
    with pytest.raises(Exception):
        c["scene"].direct(c["items"][:N], c["mine"], mis=mis, pick=(wrong, c["total"]), **KW)
    got_s, got_m, ok = on_device(torch, c, mis, wrong)
    assert ok
    P.assert_same_bits(got_s, want["S"], (name, options, mis, "radiance"))
    P.assert_same_bits(got_m, want["M"], (name, options, mis, "moment2"))


@pytest.mark.parametrize("mis", (None, "balance"))
def test_device_form_at_the_edges_of_q_and_prob(trt, orc, case, mis):
    """Cornell, the device form with a table nobody checked: slot 0 has a NaN q (takes its alias, whose prob is 0: dead samples), slot
    1 has q = 0 and an alias past the table (clamped to record 2), slot 2 keeps itself; record 2 is a sphere of radius 0.1 and colour
    1e-30 with a SUBNORMAL prob, where area / prob = 1.26e38 is finite and the samples live with weights above 1e30 - f32 denormals
    are kept.  Defined output, the restatement's bytes."""
    import torch
    name, options, shape = CASES[0]
    c = dict(case(name, options, shape))
    table = c["table"].copy()
    table[2:] = D.sphere_record((50.0, 50.0, 50.0), 0.1, (1e-30, 1e-30, 1e-30))
    pick = c["pick"].copy()
    pick["q"] = [np.nan, 0.0, 1.0]
    pick["alias"] = [1, 7, 2]
    pick["prob"] = [pick["prob"][0], 0.0, 1e-39]
    assert 0 < pick["prob"][2] < np.finfo(np.float32).tiny
    base = P.samples(orc, c["ow"], c["items"][:N], table, pick, k=K)
    if mis is None:
        want = P.finish(dict(base), K, False)
    else:                                                                   # (the lamp is record 0 still: the table rule's areas hold)
        want = P.finish(P.mis_samples(orc, c["ow"], c["desc"], c["items"][:N], table, pick, c["total"], heuristic=P.HEURISTICS[mis], k=K, base=base),
                        K, True)
    e = want["e"]
    assert set(np.unique(e)) == {1, 2} and not want["live"][e == 1].any()
    live = want["live"] & (e == 2)
    assert live.sum() > 100 and want["wgt"][live].max() > 1e30 and np.isfinite(want["wgt"][live]).all()
    assert (want["S"][np.isfinite(want["S"])] > 0).any()
    c["mine"] = table
    got_s, got_m, ok = on_device(torch, c, mis, pick)
    assert ok
    P.assert_same_bits(got_s, want["S"], "radiance")
    P.assert_same_bits(got_m, want["M"], "moment2")


def test_a_caller_weighted_table_and_a_table_of_one(trt, orc, case):
    """Cornell: weights of the caller's own (the virtual sphere never chosen: weight 0) for the plain query, and E = 1 - the scene's own
    table, where every draw ends on record 0 - for both queries."""
    name, options, shape = CASES[0]
    c = case(name, options, shape)
    items = c["items"][:N]
    weights = np.array([1.0, 5.0, 0.0], np.float32)
    pick, total = trt.lights.pick_table(c["mine"], weights)
    assert total == 6.0 and pick.tobytes() == P.build(c["table"], weights)[0].tobytes()
    want = P.finish(P.samples(orc, c["ow"], items, c["table"], pick, k=K), K, False)
    assert (want["e"] != 2).all() and (want["e"] == 1).mean() > 0.7
    S, M2, st = c["scene"].direct(items, c["mine"], moment2=True, pick=pick, **KW)
    P.assert_same_bits(S, want["S"], "weighted, radiance")
    P.assert_same_bits(M2, want["M"], "weighted, moment2")
    assert st["rays"] == want["n_rays"]
    with pytest.raises(Exception):                                          # the weighted query needs the power table
        c["scene"].direct(items, c["mine"], mis="balance", pick=(pick, total), **KW)
    own = c["scene"].emitters()
    assert len(own) == 1
    pick1, total1 = trt.lights.pick_table(own)
    assert pick1["q"][0] == 1.0 and pick1["prob"][0] == 1.0
    base = P.samples(orc, c["ow"], items, own, pick1, k=K)
    for mis in (None, "balance", "power"):
        if mis is None:
            want = P.finish(dict(base), K, False)
        else:
            want = P.finish(P.mis_samples(orc, c["ow"], c["desc"], items, own, pick1, total1, heuristic=P.HEURISTICS[mis], k=K, base=base), K, True)
        S, M2, st = c["scene"].direct(items, own, moment2=True, mis=mis, pick=(pick1, total1), **KW)
        P.assert_same_bits(S, want["S"], (mis, "E = 1, radiance"))
        P.assert_same_bits(M2, want["M"], (mis, "E = 1, moment2"))
        assert st["samples"] == N * K and st["rays"] == want["n_rays"]


def test_the_many_light_room(trt, orc):
    """E = 61: the lowered Cornell box with 60 dim sphere lights, its own table and the power table, 40 floor surfels; both queries."""
    desc, ow, items, table = P.many_light_room(trt, orc)
    scene = trt.world_from_description(desc)[0].get_bvh()
    assert scene.emitters().tobytes() == table.tobytes()
    pick, total = trt.lights.pick_table(table)
    assert pick.tobytes() == P.build(table)[0].tobytes()
    k = 8
    kw = dict(samples_per_item=k, seed=SEED, first_stream=FIRST)
    base = P.samples(orc, ow, items, table, pick, k=k)
    assert (base["e"] == 0).mean() > 0.8 and len(np.unique(base["e"])) > 5
    for mis in (None, "balance", "power"):
        if mis is None:
            want = P.finish(dict(base), k, False)
        else:
            want = P.finish(P.mis_samples(orc, ow, desc, items, table, pick, total, heuristic=P.HEURISTICS[mis], k=k, base=base), k, True)
        S, M2, st = scene.direct(items, table, moment2=True, mis=mis, pick=(pick, total), **kw)
        P.assert_same_bits(S, want["S"], (mis, "radiance"))
        P.assert_same_bits(M2, want["M"], (mis, "moment2"))
        assert st["samples"] == len(items) * k and st["rays"] == want["n_rays"]
