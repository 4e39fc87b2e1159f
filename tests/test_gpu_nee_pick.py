"""Next-event queries that choose their emitter through an alias table (tinyrt.h trt_nee_pick, trt_nee_mis_pick and their device forms) on
the GPU against the CPU oracle, bit for bit and item by item.

The reference is tests/nee_pick_cases.py: nee_cases' / nee_mis_cases' path with the vertex draw through the table.  Items, streams, table and
scenes are tests/test_gpu_nee_mis.py's: 324 rays or surfels per scene and source (a full run of 256 and a ragged one of 68, with the NaN,
zero and inf items), K = 8, seed 5, first_stream 1000, B = 5, the scene's own emitters followed by a virtual quad and a virtual sphere (E >= 2,
unequal powers), the power table from lights.pick_table; one scene per kernel shape, with the shape and launch bound of the PICK plan
asserted against profiles/nee_pick_resource_usage.txt, so all six shapes of the four PICK tables of nee.hip run.  The plain query and
BALANCE on all six, POWER on the two whose fixtures hold the most weighted hits.  tests/test_nee_pick_cases.py asserts without a GPU that
this reference is not vacuous."""
import os
import re

import numpy as np
import pytest

import direct_cases as D
import nee_cases as NC
import nee_mis_cases as NM
import nee_pick_cases as NP
import radiance_cases as R
import test_gpu_nee_mis as TM
import test_gpu_queries as G

pytestmark = pytest.mark.gpu

K, DEPTH, SEED, FIRST = NP.K, NP.MAX_BOUNCES, NP.SEED, NP.FIRST_STREAM
N = NP.N_ITEMS
GUARD, FILL = TM.GUARD, TM.FILL
SOURCES = NP.SOURCES
CASES, IDS = TM.CASES, TM.IDS
CUT = 65
PAD = 2                                                                     # records behind each table on the device: a missing clamp reads them
# (case, query): the plain query and BALANCE on all six shapes, POWER on the two shapes with the most weighted hits
BY_QUERY = [(c, None) for c in CASES] + TM.BY_HEURISTIC
BQ_IDS = [i + "-plain" for i in IDS] + TM.BH_IDS
MODES, WALKS = {"MODE_LDS": 1, "MODE_GLOBAL": 0}, {"WALK_FLAT": 2, "WALK_LDS_STACK": 1, "WALK_REGS": 5, "WALK_COMPACT": 3}


def bounds_of_the_profile():
    """{(weighted?, (scene mode, walk, threads)): launch bound} as profiles/nee_pick_resource_usage.txt reports the 24 kernels: the bound
    is the template's and the occupancy column, no row has a VGPR spill or scratch, and both sources of a shape agree."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "nee_pick_resource_usage.txt")
    rows = re.findall(r"^nee_kernel<(\w+), (\w+), (\d+), (\d+), (NEE_\w+), (plain|MIS), PICK>\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)$",
                      open(path).read(), flags=re.M)
    assert len(rows) == 24
    out, seen = {}, set()
    for mode, walk, threads, bound, source, mis, vgpr, agpr, sgpr, s_spill, v_spill, scratch, occupancy, lds in rows:
        assert int(v_spill) == 0 and int(scratch) == 0 and int(occupancy) == int(bound), (mode, walk, threads, source, mis)
        key = (mis == "MIS", (MODES[mode], WALKS[walk], int(threads)))
        assert out.setdefault(key, int(bound)) == int(bound)
        seen.add(key + (source,))
    assert len(seen) == 24 and len(out) == 12
    return out


def test_the_profile_lists_the_24_kernels_without_scratch():
    assert len(bounds_of_the_profile()) == 12


@pytest.fixture(scope="module")
def case(trt, orc):
    """(name, options) -> the scene's fixtures (nee_pick_cases.scene: computed once, never changed), the product scene compiled with the
    options, the shape and bound of the PICK plans asserted, the product's own tables, which must be the restatement's byte for byte, and
    the keywords per source."""
    cache = {}
    bounds = bounds_of_the_profile()

    def get(name, options, shape):
        key = (name, tuple(sorted(options.items())))
        if key not in cache:
            sc = NP.scene(trt, orc, name)
            scene = trt.world_from_description(sc["desc"])[0].get_bvh(**options)
            for mis in (None, "balance", "power"):
                q = scene.nee_plan(N, mis=mis, pick=True)
                assert G.plan_shape(q) == shape, (name, options, q)
                assert q["kernel_waves_per_simd"] == bounds[(mis is not None, shape[:3])], (name, options, mis, q)
            mine = trt.lights.table(scene.emitters(), trt.lights.quad(**D.VIRTUAL_QUAD), trt.lights.sphere(**D.VIRTUAL_SPHERE))
            assert mine.tobytes() == sc["nee_table"].tobytes(), (name, options)
            pick, total = trt.lights.pick_table(mine)
            assert pick.tobytes() == sc["nee_pick"].tobytes() and np.float32(total) == sc["nee_total"], (name, options)
            assert len(mine) >= 2 and len(np.unique(pick["prob"])) >= 2     # E >= 2 with unequal powers
            kw = dict(samples_per_item=K, max_bounces=DEPTH, background=sc["bg"], seed=SEED, first_stream=FIRST, spread=NP.SPREAD)
            cache[key] = dict(sc, name=name, scene=scene, mine=mine, pick=pick, total=total, kw={s: dict(kw, source=s) for s in SOURCES})
        return cache[key]

    return get


def sentinels(n=N):
    return np.full((n, 3), 7.5, np.float32), np.full((n, 3), 7.5, np.float32)


def want_of(trt, orc, name, source, mis, **kw):
    return NP.reference(trt, orc, name, source, heuristic=None if mis is None else NP.HEURISTICS[mis], **kw)


def pick_arg(c, mis, pick=None):
    pick = c["pick"] if pick is None else pick
    return pick if mis is None else (pick, c["total"])


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("cse,mis", BY_QUERY, ids=BQ_IDS)
def test_host_form_is_the_oracles_fold(trt, orc, case, cse, mis, source):
    name, options, shape = cse
    c = case(name, options, shape)
    want = want_of(trt, orc, name, source, mis)
    S, M2 = sentinels()
    S, M2, st = c["scene"].nee(c[source]["items"], c["mine"], radiance=S, moment2=M2, mis=mis, pick=pick_arg(c, mis), **c["kw"][source])
    NP.assert_same_bits(S, want["S"], (name, options, source, mis, "radiance"))
    NP.assert_same_bits(M2, want["M"], (name, options, source, mis, "moment2"))
    # the counters are the restatement's: the closest-hit walks are trt_nee's, the shadow walks are this table's
    uniform = NC.reference(trt, orc, name, source)
    assert want["hits"].tobytes() == uniform["hits"].tobytes()
    assert st["samples"] == N * K == want["n_samples"] and st["rays"] == want["n_rays"], (name, options, source, st, want["n_rays"])
    # moment2 = NULL: radiance is unchanged
    S1, none, st1 = c["scene"].nee(c[source]["items"], c["mine"], mis=mis, pick=pick_arg(c, mis), **c["kw"][source])
    assert none is None and S1.tobytes() == S.tobytes()
    assert st1["samples"] == N * K and st1["rays"] == want["n_rays"]
    # pick=None returns the bytes of trt_nee / trt_nee_mis, and where the table matters the two differ
    old = uniform if mis is None else NM.reference(trt, orc, name, source, heuristic=NM.HEURISTICS[mis])
    S0, M0, st0 = c["scene"].nee(c[source]["items"], c["mine"], moment2=True, mis=mis, pick=None, **c["kw"][source])
    NC.assert_same_bits(S0, old["S"], (name, options, source, mis, "pick=None"))
    NC.assert_same_bits(M0, old["M"], (name, options, source, mis, "pick=None, moment2"))
    assert (st0["samples"], st0["rays"]) == (N * K, old["n_rays"])
    if NP.differing(want["S"], old["S"]) > 0:
        assert S0.tobytes() != S.tobytes()


def device_buffer(torch, n):
    return torch.full(((GUARD + n + GUARD) * 12,), FILL, dtype=torch.uint8, device="cuda:0")


def padded(torch, records):
    """The records on the device with PAD records of 0xCD bytes behind them: what a read past the table would find is inside the
    allocation and is not a valid record."""
    raw = np.concatenate([np.ascontiguousarray(records).view(np.uint8), np.full(PAD * records.dtype.itemsize, FILL, np.uint8)])
    return torch.from_numpy(raw).to("cuda:0")


def on_device(torch, c, source, mis, pick, table=None, side=None, counters=None, with_m2=True, n=N, items=None, **over):
    table = c["mine"] if table is None else table
    d_items = torch.from_numpy(np.ascontiguousarray(c[source]["items"] if items is None else items).copy()).to("cuda:0")
    d_table, d_pick = padded(torch, table), padded(torch, pick)
    d_s, d_m = device_buffer(torch, n), device_buffer(torch, n)
    torch.cuda.synchronize()
    arg = d_pick.data_ptr() if mis is None else (d_pick.data_ptr(), c["total"])
    c["scene"].nee_device(d_items.data_ptr(), n, d_table.data_ptr(), len(table), d_s.data_ptr() + GUARD * 12,
                          d_m.data_ptr() + GUARD * 12 if with_m2 else 0, d_counters_ptr=0 if counters is None else counters.data_ptr(),
                          stream_ptr=0 if side is None else side.cuda_stream, mis=mis, pick=arg, **dict(c["kw"][source], **over))
    if side is not None:
        side.synchronize()
    torch.cuda.synchronize()
    got_s, ok_s = TM.payload(d_s, n)
    got_m, ok_m = TM.payload(d_m, n)
    if not with_m2:
        ok_m = ok_m and bool((got_m.view(np.uint32) == 0xCDCDCDCD).all())
    return got_s, got_m, ok_s and ok_m


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("cse,mis", BY_QUERY, ids=BQ_IDS)
def test_device_form_on_a_side_stream_equals_the_oracle_and_leaves_the_guards(trt, orc, case, cse, mis, source):
    import torch
    name, options, shape = cse
    c = case(name, options, shape)
    want = want_of(trt, orc, name, source, mis)
    ctr = torch.full((16,), 3, dtype=torch.int64, device="cuda:0")          # the counters are added to
    got_s, got_m, ok = on_device(torch, c, source, mis, c["pick"], side=torch.cuda.Stream(), counters=ctr)
    assert ok, (name, options, "guard bytes were written")
    NP.assert_same_bits(got_s, want["S"], (name, options, source, mis, "radiance"))
    NP.assert_same_bits(got_m, want["M"], (name, options, source, mis, "moment2"))
    assert int(ctr[0]) == 3 + N * K and int(ctr[1]) == 3 + want["n_rays"] and bool((ctr[2:] == 3).all())
    # without moment2 and without counters: the same radiance, the guards intact, the second buffer untouched
    got_s1, _, ok1 = on_device(torch, c, source, mis, c["pick"], with_m2=False)
    assert ok1 and got_s1.tobytes() == got_s.tobytes()


@pytest.mark.parametrize("cse,mis", BY_QUERY[:2 * len(CASES)], ids=BQ_IDS[:2 * len(CASES)])
def test_splits_by_samples_and_by_items_leave_the_bytes_of_one_call(trt, orc, case, cse, mis):
    name, options, shape = cse
    c = case(name, options, shape)
    source = "cosine" if mis is None else "cone"
    want = want_of(trt, orc, name, source, mis)
    kw = dict(c["kw"][source], mis=mis, pick=pick_arg(c, mis))
    items = c[source]["items"]
    # samples [0, 3), then [3, 8) on top with accumulate
    rays3 = int(want["hits"][:, :3].sum() + want["walks"][:, :3].sum())
    S, M2 = sentinels()
    _, _, st = c["scene"].nee(items, c["mine"], sample_begin=0, sample_end=3, radiance=S, moment2=M2, **kw)
    S3, M3 = R.fold(want["cols"], K, 0, 3)
    NP.assert_same_bits(S, S3, (name, options, mis, "radiance [0, 3)"))
    NP.assert_same_bits(M2, M3, (name, options, mis, "moment2 [0, 3)"))
    assert st["samples"] == N * 3 and st["rays"] == rays3
    _, _, st = c["scene"].nee(items, c["mine"], sample_begin=3, sample_end=8, accumulate=True, radiance=S, moment2=M2, **kw)
    NP.assert_same_bits(S, want["S"], (name, options, mis, "radiance [0, 3) + [3, 8)"))
    NP.assert_same_bits(M2, want["M"], (name, options, mis, "moment2 [0, 3) + [3, 8)"))
    assert st["samples"] == N * 5 and st["rays"] == want["n_rays"] - rays3
    # items [0, 65), then [65, 324) on their own streams
    S, M2 = sentinels()
    c["scene"].nee(items[:CUT], c["mine"], radiance=S[:CUT], moment2=M2[:CUT], **kw)
    assert (S[CUT:] == 7.5).all() and (M2[CUT:] == 7.5).all()               # entries outside the call's range are untouched
    c["scene"].nee(items[CUT:], c["mine"], radiance=S[CUT:], moment2=M2[CUT:], **dict(kw, first_stream=FIRST + CUT * K))
    NP.assert_same_bits(S, want["S"], (name, options, mis, "radiance by items"))
    NP.assert_same_bits(M2, want["M"], (name, options, mis, "moment2 by items"))


@pytest.mark.parametrize("source", ("rays", "cosine"))
@pytest.mark.parametrize("cse,mis", BY_QUERY, ids=BQ_IDS)
def test_a_diffuse_source(trt, orc, case, cse, mis, source):
    """source_is_diffuse = 1: the first hit is hidden in full, weighted or not."""
    name, options, shape = cse
    c = case(name, options, shape)
    want = want_of(trt, orc, name, source, mis, source_is_diffuse=True)
    S, M2, st = c["scene"].nee(c[source]["items"], c["mine"], source_is_diffuse=True, moment2=True, mis=mis, pick=pick_arg(c, mis),
                               **c["kw"][source])
    NP.assert_same_bits(S, want["S"], (name, options, source, mis, "radiance"))
    NP.assert_same_bits(M2, want["M"], (name, options, source, mis, "moment2"))
    assert st["samples"] == N * K and st["rays"] == want["n_rays"]
    if name in ("prims33", "prims600"):                                     # first hits on their lights are hidden (tests/test_gpu_nee.py)
        assert want["first_hidden"].sum() >= 8


@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_with_one_bounce_the_result_is_the_gathers_on_the_device(trt, case, name, options, shape):
    """B == 1, source_is_diffuse == 0: no vertex draws; Scene.radiance / Scene.gather byte for byte, stats included, for the three queries."""
    c = case(name, options, shape)
    for source in SOURCES:
        kw = dict(c["kw"][source], max_bounces=1)
        plain = {k: v for k, v in kw.items() if k not in ("source", "spread")}
        if source == "rays":
            plain["samples_per_ray"] = plain.pop("samples_per_item")
            S0, M0, st0 = c["scene"].radiance(c[source]["items"], moment2=True, **plain)
        else:
            S0, M0, st0 = c["scene"].gather(c[source]["items"], lobe=source, spread=NP.SPREAD, moment2=True, **plain)
        for mis in (None, "balance", "power"):
            S, M2, st = c["scene"].nee(c[source]["items"], c["mine"], moment2=True, mis=mis, pick=pick_arg(c, mis), **kw)
            assert S.tobytes() == S0.tobytes() and M2.tobytes() == M0.tobytes(), (name, options, source, mis)
            assert (st["samples"], st["rays"]) == (st0["samples"], st0["rays"])
        assert np.isfinite(S0).any() and (S0[np.isfinite(S0)] != 0).any()


def wrong_tables(pick):
    """Tables the host form rejects and the device form has defined results for: a NaN q (takes the alias), a prob of 0 on the heaviest
    emitter (dead samples), aliases of E and E + 1 (clamped to record E - 1)."""
    E = len(pick)
    out = {}
    t = pick.copy()
    t["q"] = np.nan
    t["alias"] = (np.arange(E) + 1) % E
    out["q_nan"] = t
    t = pick.copy()
    t["prob"][int(np.argmax(pick["prob"]))] = 0.0
    out["prob_0"] = t
    for name, alias in (("alias_E", E), ("alias_E_plus_1", E + 1)):
        t = pick.copy()
        t["q"] = np.minimum(t["q"], np.float32(0.5))                        # every slot sends half its draws past the table
        t["alias"] = alias
        out[name] = t
    return out


@pytest.mark.parametrize("wrong", ("q_nan", "prob_0", "alias_E", "alias_E_plus_1"))
@pytest.mark.parametrize("cse,mis", BY_QUERY[:2 * len(CASES)], ids=BQ_IDS[:2 * len(CASES)])
def test_device_form_with_a_wrong_table_returns_the_restatements_bytes(trt, orc, case, cse, mis, wrong):
    """The device forms check only the pointer.  Both tables lie on the device with two records of 0xCD bytes behind them, so a missing
    clamp shows as wrong bytes; no address outside an allocation is ever handed over."""
    import torch
    name, options, shape = cse
    c = case(name, options, shape)
    pick = wrong_tables(c["pick"])[wrong]
    E = len(pick)
    want = want_of(trt, orc, name, "cosine", mis, pick=pick)
    right = want_of(trt, orc, name, "cosine", mis)
    if wrong.startswith("alias"):
        assert want["alias_taken"].sum() >= 20
    if wrong == "q_nan":
        assert want["alias_taken"].sum() >= max(int(right["alias_taken"].sum()), int(want["walks"].sum()))      # every draw takes its alias
    if name != "prims600":                                                  # (100 emitters, 27 lit samples: the tables may agree there)
        assert NP.differing(want["S"], right["S"]) > 0, (name, wrong)
    with pytest.raises(Exception):
        c["scene"].nee(c["cosine"]["items"], c["mine"], mis=mis, pick=pick_arg(c, mis, pick), **c["kw"]["cosine"])
    got_s, got_m, ok = on_device(torch, c, "cosine", mis, pick)
    assert ok and E == len(c["mine"])
    NP.assert_same_bits(got_s, want["S"], (name, options, mis, wrong, "radiance"))
    NP.assert_same_bits(got_m, want["M"], (name, options, mis, wrong, "moment2"))


def test_a_caller_weighted_table_with_a_zero_weight(trt, orc, case):
    """Cornell, trt_nee_pick: weights of the caller's own, the virtual sphere never chosen (weight 0).  The weighted query refuses it."""
    name, options, shape = CASES[0]
    assert name == "cornell"
    c = case(name, options, shape)
    weights = np.array([1.0, 5.0, 0.0], np.float32)
    pick, total = trt.lights.pick_table(c["mine"], weights)
    assert total == 6.0 and pick["prob"][2] == 0.0 and pick["q"][2] == 0.0
    for source in ("cosine", "rays"):
        want = want_of(trt, orc, name, source, None, pick=pick)
        assert want["lit"].sum() >= 500 and NP.differing(want["S"], want_of(trt, orc, name, source, None)["S"]) > 0
        S, M2, st = c["scene"].nee(c[source]["items"], c["mine"], moment2=True, pick=pick, **c["kw"][source])
        NP.assert_same_bits(S, want["S"], (source, "weighted, radiance"))
        NP.assert_same_bits(M2, want["M"], (source, "weighted, moment2"))
        assert st["rays"] == want["n_rays"]
    with pytest.raises(Exception):                                          # the weighted query needs the power table
        c["scene"].nee(c["cosine"]["items"], c["mine"], mis="balance", pick=(pick, total), **c["kw"]["cosine"])


def test_nothing_to_trace(trt, case):
    """An empty sample range and B == 0 zero the n entries without accumulate and leave them with it."""
    name, options, shape = CASES[0]
    c = case(name, options, shape)
    items = c["cosine"]["items"]
    for kw in (dict(c["kw"]["cosine"], sample_begin=3, sample_end=3), dict(c["kw"]["cosine"], max_bounces=0)):
        for mis in (None, "power"):
            for accumulate in (False, True):
                S, M2 = sentinels()
                _, _, st = c["scene"].nee(items, c["mine"], accumulate=accumulate, radiance=S, moment2=M2, mis=mis, pick=pick_arg(c, mis), **kw)
                want = 7.5 if accumulate else 0.0
                assert (S == want).all() and (M2 == want).all(), (mis, accumulate)
                assert st["rays"] == 0 and st["samples"] == 0
