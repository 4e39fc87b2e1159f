"""Weighted next-event queries (tinyrt.h trt_nee_mis, trt_nee_mis_device) on the GPU against the CPU oracle, bit for bit and item by item.

The reference is tests/nee_mis_cases.py: nee_cases' path and draw with the contract's two weights, wl on the shadow sample and wb on a light
the path reaches after a diffuse scatter.  Items, streams, table and scenes are tests/test_gpu_nee.py's: 324 rays or surfels per scene and
source (a full run of 256 and a ragged one of 68, with the NaN, zero and inf items), K = 8, seed 5, first_stream 1000, B = 5, the scene's own
emitters followed by a virtual quad and a virtual sphere; one scene per kernel shape, with the shape Scene.nee_plan(n, mis=...) reports
asserted, so all six shapes of both weighted tables of nee.hip run.  BALANCE on all six, POWER on the two whose fixtures hold the most
weighted hits (tests/README_nee_mis.md).  tests/test_nee_mis_cases.py asserts without a GPU that this reference is not vacuous."""
import numpy as np
import pytest

import direct_cases as D
import nee_cases as NC
import nee_mis_cases as M
import radiance_cases as R
import test_gpu_queries as G

pytestmark = pytest.mark.gpu

K, DEPTH, SEED, FIRST = M.K, M.MAX_BOUNCES, M.SEED, M.FIRST_STREAM
N = M.N_ITEMS
GUARD = 64                                                                  # entries on either side of a device buffer
FILL = 0xCD
SOURCES = M.SOURCES
# nee.hip kNeeKernels[pick][mis][source], the weighted tables: (scene mode, walk, threads) -> launch bound (profiles/nee_mis_resource_usage.txt)
BOUNDS = {(1, 2, 256): 5, (1, 1, 256): 5, (1, 1, 768): 5, (1, 5, 512): 5, (0, 3, 256): 5, (0, 5, 256): 5}


def shape_of(name, options):
    if not options:
        return G.DEFAULT_SHAPES[name]
    return [s for n, o, s in G.OTHER_WALKS if n == name and o == options][0]


CASES = [(name, options, shape_of(name, options)) for name, options in M.CASES]
IDS = ["%s-%s" % (name, "-".join("%s=%s" % kv for kv in sorted(options.items())) or "default") for name, options, _ in CASES]
# the two shapes whose fixtures hold the most weighted hits (over the three sources: prims600 100, prims33 49, cornell 32, the other
# two scenes hold no light; tests/README_nee_mis.md)
POWER_CASES = [c for c in CASES if c[0] in ("prims600", "prims33")]
POWER_IDS = [i for i, c in zip(IDS, CASES) if c in POWER_CASES]
BY_HEURISTIC = [(c, "balance") for c in CASES] + [(c, "power") for c in POWER_CASES]
BH_IDS = [i + "-balance" for i in IDS] + [i + "-power" for i in POWER_IDS]


@pytest.fixture(scope="module")
def case(trt, orc):
    """(name, options) -> the scene's fixtures (nee_cases.scene: computed once, never changed), the product scene compiled with the
    options, the shape of the weighted plan asserted, the product's own table, which must be the restatement's byte for byte, and the
    keywords per source."""
    cache = {}

    def get(name, options, shape):
        key = (name, tuple(sorted(options.items())))
        if key not in cache:
            sc = M.scene(trt, orc, name)
            scene = trt.world_from_description(sc["desc"])[0].get_bvh(**options)
            for mis in ("balance", "power"):
                q = scene.nee_plan(N, mis=mis)
                assert G.plan_shape(q) == shape, (name, options, q)
                assert q["kernel_waves_per_simd"] == BOUNDS[shape[:3]], (name, options, q)
            mine = trt.lights.table(scene.emitters(), trt.lights.quad(**D.VIRTUAL_QUAD), trt.lights.sphere(**D.VIRTUAL_SPHERE))
            assert mine.tobytes() == sc["nee_table"].tobytes(), (name, options)
            kw = dict(samples_per_item=K, max_bounces=DEPTH, background=sc["bg"], seed=SEED, first_stream=FIRST, spread=M.SPREAD)
            cache[key] = dict(sc, name=name, scene=scene, mine=mine, kw={s: dict(kw, source=s) for s in SOURCES})
        return cache[key]

    return get


def sentinels(n=N):
    return np.full((n, 3), 7.5, np.float32), np.full((n, 3), 7.5, np.float32)


def want_of(trt, orc, name, source, mis, **kw):
    return M.reference(trt, orc, name, source, heuristic=M.HEURISTICS[mis], **kw)


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("cse,mis", BY_HEURISTIC, ids=BH_IDS)
def test_host_form_is_the_oracles_fold(trt, orc, case, cse, mis, source):
    name, options, shape = cse
    c = case(name, options, shape)
    want = want_of(trt, orc, name, source, mis)
    plain = NC.reference(trt, orc, name, source)
    S, M2 = sentinels()
    S, M2, st = c["scene"].nee(c[source]["items"], c["mine"], radiance=S, moment2=M2, mis=mis, **c["kw"][source])
    M.assert_same_bits(S, want["S"], (name, options, source, mis, "radiance"))
    M.assert_same_bits(M2, want["M"], (name, options, source, mis, "moment2"))
    # identity 4: the counters are trt_nee's
    assert st["samples"] == N * K and st["rays"] == want["n_rays"] == plain["n_rays"], (name, options, source, st, want["n_rays"])
    # moment2 = NULL: radiance is unchanged
    S1, none, st1 = c["scene"].nee(c[source]["items"], c["mine"], mis=mis, **c["kw"][source])
    assert none is None and S1.tobytes() == S.tobytes()
    assert st1["samples"] == N * K and st1["rays"] == want["n_rays"]
    # mis=None returns the bytes it returned before (tests/test_gpu_nee.py's job too), and where a light of the scene is weighted the two differ
    S0, _, st0 = c["scene"].nee(c[source]["items"], c["mine"], **c["kw"][source])
    NC.assert_same_bits(S0, plain["S"], (name, options, source, "mis=None"))
    assert (st0["samples"], st0["rays"]) == (st["samples"], st["rays"])
    if M.differing(want["S"], plain["S"]) > 0:
        assert S0.tobytes() != S.tobytes()


def device_buffer(torch, n):
    return torch.full(((GUARD + n + GUARD) * 12,), FILL, dtype=torch.uint8, device="cuda:0")


def payload(t, n):
    """(payload as float32 [n, 3], guards intact?)"""
    h = t.cpu().numpy()
    g, b = GUARD * 12, n * 12
    return h[g:g + b].copy().view(np.float32).reshape(n, 3), bool((h[:g] == FILL).all() and (h[g + b:] == FILL).all())


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("cse,mis", BY_HEURISTIC, ids=BH_IDS)
def test_device_form_on_a_side_stream_equals_the_oracle_and_leaves_the_guards(trt, orc, case, cse, mis, source):
    import torch
    name, options, shape = cse
    c = case(name, options, shape)
    want = want_of(trt, orc, name, source, mis)
    E = len(c["mine"])
    d_items = torch.from_numpy(c[source]["items"].copy()).to("cuda:0")
    d_table = torch.from_numpy(c["mine"].view(np.uint8).copy()).to("cuda:0")
    side = torch.cuda.Stream()
    d_s, d_m = device_buffer(torch, N), device_buffer(torch, N)
    ctr = torch.full((16,), 3, dtype=torch.int64, device="cuda:0")          # the counters are added to
    torch.cuda.synchronize()
    c["scene"].nee_device(d_items.data_ptr(), N, d_table.data_ptr(), E, d_s.data_ptr() + GUARD * 12, d_m.data_ptr() + GUARD * 12,
                          d_counters_ptr=ctr.data_ptr(), stream_ptr=side.cuda_stream, mis=mis, **c["kw"][source])
    side.synchronize()
    torch.cuda.synchronize()
    got_s, ok_s = payload(d_s, N)
    got_m, ok_m = payload(d_m, N)
    assert ok_s and ok_m, (name, options, "guard bytes were written")
    M.assert_same_bits(got_s, want["S"], (name, options, source, mis, "radiance"))
    M.assert_same_bits(got_m, want["M"], (name, options, source, mis, "moment2"))
    assert int(ctr[0]) == 3 + N * K and int(ctr[1]) == 3 + want["n_rays"] and bool((ctr[2:] == 3).all())
    # without moment2 and without counters: the same radiance, the guards intact
    d_s1 = device_buffer(torch, N)
    c["scene"].nee_device(d_items.data_ptr(), N, d_table.data_ptr(), E, d_s1.data_ptr() + GUARD * 12, mis=mis, **c["kw"][source])
    torch.cuda.synchronize()
    got_s1, ok_s1 = payload(d_s1, N)
    assert ok_s1 and got_s1.tobytes() == got_s.tobytes()


@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_split_by_samples_leaves_the_bytes_of_one_pass(trt, orc, case, name, options, shape):
    c = case(name, options, shape)
    want = want_of(trt, orc, name, "cosine", "balance")
    kw = dict(c["kw"]["cosine"], mis="balance")
    items = c["cosine"]["items"]
    rays3 = int(want["hits"][:, :3].sum() + want["walks"][:, :3].sum())
    S, M2 = sentinels()
    _, _, st = c["scene"].nee(items, c["mine"], sample_begin=0, sample_end=3, radiance=S, moment2=M2, **kw)
    S3, M3 = R.fold(want["cols"], K, 0, 3)
    M.assert_same_bits(S, S3, (name, options, "radiance [0, 3)"))
    M.assert_same_bits(M2, M3, (name, options, "moment2 [0, 3)"))
    assert st["samples"] == N * 3 and st["rays"] == rays3
    _, _, st = c["scene"].nee(items, c["mine"], sample_begin=3, sample_end=8, accumulate=True, radiance=S, moment2=M2, **kw)
    M.assert_same_bits(S, want["S"], (name, options, "radiance [0, 3) + [3, 8)"))
    M.assert_same_bits(M2, want["M"], (name, options, "moment2 [0, 3) + [3, 8)"))
    assert st["samples"] == N * 5 and st["rays"] == want["n_rays"] - rays3


@pytest.mark.parametrize("source", ("rays", "cone"))
@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_split_by_items_leaves_the_bytes_of_one_call(trt, orc, case, name, options, shape, source):
    c = case(name, options, shape)
    want = want_of(trt, orc, name, source, "balance")
    kw = dict(c["kw"][source], mis="balance")
    items = c[source]["items"]
    one_s, one_m, _ = c["scene"].nee(items, c["mine"], moment2=True, **kw)
    S, M2 = sentinels()
    a = 100
    c["scene"].nee(items[:a], c["mine"], radiance=S[:a], moment2=M2[:a], **kw)
    assert (S[a:] == 7.5).all() and (M2[a:] == 7.5).all()                   # entries outside the call's range are untouched
    kw["first_stream"] = FIRST + a * K
    head_s, head_m = S[:a].copy(), M2[:a].copy()
    c["scene"].nee(items[a:], c["mine"], radiance=S[a:], moment2=M2[a:], **kw)
    assert S[:a].tobytes() == head_s.tobytes() and M2[:a].tobytes() == head_m.tobytes()
    assert S.tobytes() == one_s.tobytes() and M2.tobytes() == one_m.tobytes(), (name, options)          # byte for byte
    M.assert_same_bits(S, want["S"], (name, options, source, "radiance"))
    M.assert_same_bits(M2, want["M"], (name, options, source, "moment2"))


@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_nothing_to_trace(trt, case, name, options, shape):
    """An empty sample range and B == 0 zero the n entries without accumulate and leave them with it; through the device form no byte
    outside [0, 12 n) is written."""
    import torch
    c = case(name, options, shape)
    items = c["cosine"]["items"]
    nothing = (dict(c["kw"]["cosine"], sample_begin=3, sample_end=3), dict(c["kw"]["cosine"], max_bounces=0), dict(c["kw"]["rays"], max_bounces=0))
    for kw in nothing:
        for accumulate in (False, True):
            S, M2 = sentinels()
            _, _, st = c["scene"].nee(items, c["mine"], accumulate=accumulate, radiance=S, moment2=M2, mis="balance", **kw)
            want = 7.5 if accumulate else 0.0
            assert (S == want).all() and (M2 == want).all(), (name, options, accumulate)
            assert st["rays"] == 0 and st["samples"] == 0
    d_items = torch.from_numpy(items.copy()).to("cuda:0")
    d_table = torch.from_numpy(c["mine"].view(np.uint8).copy()).to("cuda:0")
    for kw in nothing[:2]:
        for accumulate in (False, True):
            for with_m2 in (True, False):
                d_s, d_m = device_buffer(torch, N), device_buffer(torch, N)
                c["scene"].nee_device(d_items.data_ptr(), N, d_table.data_ptr(), len(c["mine"]), d_s.data_ptr() + GUARD * 12,
                                      d_m.data_ptr() + GUARD * 12 if with_m2 else 0, accumulate=accumulate, mis="power", **kw)
                torch.cuda.synchronize()
                for t, written in ((d_s, True), (d_m, with_m2)):
                    got, ok = payload(t, N)
                    assert ok, (name, options, "guard bytes were written")
                    assert (got.view(np.uint32) == (0 if written and not accumulate else 0xCDCDCDCD)).all()


@pytest.mark.parametrize("source", ("rays", "cosine"))
@pytest.mark.parametrize("cse,mis", BY_HEURISTIC, ids=BH_IDS)
def test_a_diffuse_source(trt, orc, case, cse, mis, source):
    """source_is_diffuse = 1: the first hit is hidden in full, not weighted."""
    name, options, shape = cse
    c = case(name, options, shape)
    want = want_of(trt, orc, name, source, mis, source_is_diffuse=True)
    S, M2, st = c["scene"].nee(c[source]["items"], c["mine"], source_is_diffuse=True, moment2=True, mis=mis, **c["kw"][source])
    M.assert_same_bits(S, want["S"], (name, options, source, mis, "radiance"))
    M.assert_same_bits(M2, want["M"], (name, options, source, mis, "moment2"))
    assert st["samples"] == N * K and st["rays"] == want["n_rays"]
    if name in ("prims33", "prims600"):                                     # first hits on their lights are hidden (tests/test_gpu_nee.py)
        assert want["first_hidden"].sum() >= 8


@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_identity_1_with_one_bounce_the_result_is_the_plain_querys_on_the_device(trt, case, name, options, shape):
    """B == 1, source_is_diffuse == 0: Scene.radiance / Scene.gather byte for byte, stats included, for both heuristics."""
    c = case(name, options, shape)
    for source in SOURCES:
        kw = dict(c["kw"][source], max_bounces=1)
        plain = {k: v for k, v in kw.items() if k not in ("source", "spread")}
        if source == "rays":
            plain["samples_per_ray"] = plain.pop("samples_per_item")
            S0, M0, st0 = c["scene"].radiance(c[source]["items"], moment2=True, **plain)
        else:
            S0, M0, st0 = c["scene"].gather(c[source]["items"], lobe=source, spread=M.SPREAD, moment2=True, **plain)
        for mis in ("balance", "power"):
            S, M2, st = c["scene"].nee(c[source]["items"], c["mine"], moment2=True, mis=mis, **kw)
            assert S.tobytes() == S0.tobytes() and M2.tobytes() == M0.tobytes(), (name, options, source, mis)
            assert (st["samples"], st["rays"]) == (st0["samples"], st0["rays"])
        assert np.isfinite(S0).any() and (S0[np.isfinite(S0)] != 0).any()


def test_identity_3_with_virtual_emitters_only_the_result_is_trt_nees_on_the_device(trt, orc, case):
    """random_spheres holds no TRT_LIGHT geometry and its table is the two virtual emitters: trt_nee's bytes for both heuristics."""
    name, options = [c for c in M.CASES if c[0] == "random_spheres"][0]
    c = case(name, options, shape_of(name, options))
    assert len(c["mine"]) == 2 and (c["mine"]["geometry"] == D.NO_GEOMETRY).all() and len(c["scene"].emitters()) == 0
    for source in SOURCES:
        S0, M0, st0 = c["scene"].nee(c[source]["items"], c["mine"], moment2=True, **c["kw"][source])
        NC.assert_same_bits(S0, NC.reference(trt, orc, name, source)["S"], (name, source))
        assert (S0[np.isfinite(S0)] != 0).any()
        for mis in ("balance", "power"):
            S, M2, st = c["scene"].nee(c[source]["items"], c["mine"], moment2=True, mis=mis, **c["kw"][source])
            assert S.tobytes() == S0.tobytes() and M2.tobytes() == M0.tobytes(), (source, mis)
            assert (st["samples"], st["rays"]) == (st0["samples"], st0["rays"])


def test_the_scenes_own_table_alone(trt, orc, case):
    """cornell with E = 1: the lamp itself, the table Scene.emitters() returns; both heuristics."""
    name, options = M.CASES[0]
    assert name == "cornell"
    c = case(name, options, shape_of(name, options))
    table = c["scene"].emitters()
    assert len(table) == 1 and table.tobytes() == D.emitters_of(orc, c["desc"]).tobytes()
    for mis in ("balance", "power"):
        want = M.finish(M.mis_paths(orc, c["ow"], c["desc"], c["cosine"]["rays"], table, background=c["bg"], heuristic=M.HEURISTICS[mis]), K)
        assert want["weighted"].sum() >= 1 and int((want["lit"] > 0).sum()) >= 400
        S, M2, st = c["scene"].nee(c["cosine"]["items"], table, moment2=True, mis=mis, **c["kw"]["cosine"])
        M.assert_same_bits(S, want["S"], (mis, "radiance"))
        M.assert_same_bits(M2, want["M"], (mis, "moment2"))
        assert st["samples"] == N * K and st["rays"] == want["n_rays"]
