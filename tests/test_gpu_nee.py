"""Next-event queries (tinyrt.h trt_nee, trt_nee_device) on the GPU against the CPU oracle, bit for bit and item by item.

Sample s of item i has stream index j = first_stream + i * K + s.  Its path is cpu.rs:39-65 restated from the oracle's pieces with the
contract's hidden emission, and at every Lambertian vertex that leaves bounce budget the draw of direct_cases on stream (seed, j, 2 + d)
with the oracle's World.hit over [0.001, t_max) (tests/nee_cases.py); the fold is radiance_cases.fold.

Items, per scene and source: passes_cases.items_of - 324 rays or surfels, a full run of 256 for one wave and a ragged one of 68 for the
next, with the NaN, zero and inf items.  K = 8, seed 5, first_stream = 1000, B = 5.  The table is the scene's own emitters followed by a
virtual quad and a virtual sphere.  One scene per kernel shape (passes_cases.CASES); each case asserts the shape Scene.nee_plan reports, so
all six shapes of both tables of nee.hip run.  tests/test_nee_cases.py asserts without a GPU that this reference is not vacuous."""
import numpy as np
import pytest

import direct_cases as D
import nee_cases as NC
import passes_cases as P
import radiance_cases as R
import test_gpu_queries as G

pytestmark = pytest.mark.gpu

K, DEPTH, SEED, FIRST = NC.K, NC.MAX_BOUNCES, NC.SEED, NC.FIRST_STREAM
N = NC.N_ITEMS
GUARD = 64                                                                  # entries on either side of a device buffer
FILL = 0xCD
SOURCES = NC.SOURCES


def shape_of(name, options):
    if not options:
        return G.DEFAULT_SHAPES[name]
    return [s for n, o, s in G.OTHER_WALKS if n == name and o == options][0]


CASES = [(name, options, shape_of(name, options)) for name, options in NC.CASES]
IDS = ["%s-%s" % (name, "-".join("%s=%s" % kv for kv in sorted(options.items())) or "default") for name, options, _ in CASES]


@pytest.fixture(scope="module")
def case(trt, orc):
    """(name, options) -> the scene's fixtures (nee_cases.scene: computed once, never changed), the product scene compiled with the
    options, its shape asserted, the product's own table, which must be the restatement's byte for byte, and the keywords per source."""
    cache = {}

    def get(name, options, shape):
        key = (name, tuple(sorted(options.items())))
        if key not in cache:
            sc = NC.scene(trt, orc, name)
            scene = trt.world_from_description(sc["desc"])[0].get_bvh(**options)
            q = scene.nee_plan(N)
            assert G.plan_shape(q) == shape, (name, options, q)
            mine = trt.lights.table(scene.emitters(), trt.lights.quad(**D.VIRTUAL_QUAD), trt.lights.sphere(**D.VIRTUAL_SPHERE))
            assert mine.tobytes() == sc["nee_table"].tobytes(), (name, options)
            kw = dict(samples_per_item=K, max_bounces=DEPTH, background=sc["bg"], seed=SEED, first_stream=FIRST, spread=NC.SPREAD)
            cache[key] = dict(sc, name=name, scene=scene, mine=mine, kw={s: dict(kw, source=s) for s in SOURCES})
        return cache[key]

    return get


def sentinels(n=N):
    return np.full((n, 3), 7.5, np.float32), np.full((n, 3), 7.5, np.float32)


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_host_form_is_the_oracles_fold(trt, orc, case, name, options, shape, source):
    c = case(name, options, shape)
    want = NC.reference(trt, orc, name, source)
    S, M = sentinels()
    S, M, st = c["scene"].nee(c[source]["items"], c["mine"], radiance=S, moment2=M, **c["kw"][source])
    NC.assert_same_bits(S, want["S"], (name, options, source, "radiance"))
    NC.assert_same_bits(M, want["M"], (name, options, source, "moment2"))
    assert st["samples"] == N * K and st["rays"] == want["n_rays"], (name, options, source, st, want["n_rays"])
    # moment2 = NULL: radiance is unchanged
    S1, none, st1 = c["scene"].nee(c[source]["items"], c["mine"], **c["kw"][source])
    assert none is None and S1.tobytes() == S.tobytes()
    assert st1["samples"] == N * K and st1["rays"] == want["n_rays"]


def device_buffer(torch, n):
    return torch.full(((GUARD + n + GUARD) * 12,), FILL, dtype=torch.uint8, device="cuda:0")


def payload(t, n):
    """(payload as float32 [n, 3], guards intact?)"""
    h = t.cpu().numpy()
    g, b = GUARD * 12, n * 12
    return h[g:g + b].copy().view(np.float32).reshape(n, 3), bool((h[:g] == FILL).all() and (h[g + b:] == FILL).all())


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_device_form_on_a_side_stream_equals_the_oracle_and_leaves_the_guards(trt, orc, case, name, options, shape, source):
    import torch
    c = case(name, options, shape)
    want = NC.reference(trt, orc, name, source)
    E = len(c["mine"])
    d_items = torch.from_numpy(c[source]["items"].copy()).to("cuda:0")
    d_table = torch.from_numpy(c["mine"].view(np.uint8).copy()).to("cuda:0")
    side = torch.cuda.Stream()
    d_s, d_m = device_buffer(torch, N), device_buffer(torch, N)
    ctr = torch.full((16,), 3, dtype=torch.int64, device="cuda:0")          # the counters are added to
    torch.cuda.synchronize()
    c["scene"].nee_device(d_items.data_ptr(), N, d_table.data_ptr(), E, d_s.data_ptr() + GUARD * 12, d_m.data_ptr() + GUARD * 12,
                          d_counters_ptr=ctr.data_ptr(), stream_ptr=side.cuda_stream, **c["kw"][source])
    side.synchronize()
    torch.cuda.synchronize()
    got_s, ok_s = payload(d_s, N)
    got_m, ok_m = payload(d_m, N)
    assert ok_s and ok_m, (name, options, "guard bytes were written")
    NC.assert_same_bits(got_s, want["S"], (name, options, source, "radiance"))
    NC.assert_same_bits(got_m, want["M"], (name, options, source, "moment2"))
    assert int(ctr[0]) == 3 + N * K and int(ctr[1]) == 3 + want["n_rays"] and bool((ctr[2:] == 3).all())
    # without moment2 and without counters: the same radiance, the guards intact
    d_s1 = device_buffer(torch, N)
    c["scene"].nee_device(d_items.data_ptr(), N, d_table.data_ptr(), E, d_s1.data_ptr() + GUARD * 12, **c["kw"][source])
    torch.cuda.synchronize()
    got_s1, ok_s1 = payload(d_s1, N)
    assert ok_s1 and got_s1.tobytes() == got_s.tobytes()


@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_split_by_samples_leaves_the_bytes_of_one_pass(trt, orc, case, name, options, shape):
    c = case(name, options, shape)
    want = NC.reference(trt, orc, name, "cosine")
    kw = c["kw"]["cosine"]
    items = c["cosine"]["items"]
    rays3 = int(want["hits"][:, :3].sum() + want["walks"][:, :3].sum())
    S, M = sentinels()
    _, _, st = c["scene"].nee(items, c["mine"], sample_begin=0, sample_end=3, radiance=S, moment2=M, **kw)
    S3, M3 = R.fold(want["cols"], K, 0, 3)
    NC.assert_same_bits(S, S3, (name, options, "radiance [0, 3)"))
    NC.assert_same_bits(M, M3, (name, options, "moment2 [0, 3)"))
    assert st["samples"] == N * 3 and st["rays"] == rays3
    _, _, st = c["scene"].nee(items, c["mine"], sample_begin=3, sample_end=8, accumulate=True, radiance=S, moment2=M, **kw)
    NC.assert_same_bits(S, want["S"], (name, options, "radiance [0, 3) + [3, 8)"))
    NC.assert_same_bits(M, want["M"], (name, options, "moment2 [0, 3) + [3, 8)"))
    assert st["samples"] == N * 5 and st["rays"] == want["n_rays"] - rays3


@pytest.mark.parametrize("source", ("rays", "cone"))
@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_split_by_items_leaves_the_bytes_of_one_call(trt, orc, case, name, options, shape, source):
    c = case(name, options, shape)
    want = NC.reference(trt, orc, name, source)
    kw = dict(c["kw"][source])
    items = c[source]["items"]
    one_s, one_m, _ = c["scene"].nee(items, c["mine"], moment2=True, **kw)
    S, M = sentinels()
    a = 100
    c["scene"].nee(items[:a], c["mine"], radiance=S[:a], moment2=M[:a], **kw)
    assert (S[a:] == 7.5).all() and (M[a:] == 7.5).all()                    # entries outside the call's range are untouched
    kw["first_stream"] = FIRST + a * K
    head_s, head_m = S[:a].copy(), M[:a].copy()
    c["scene"].nee(items[a:], c["mine"], radiance=S[a:], moment2=M[a:], **kw)
    assert S[:a].tobytes() == head_s.tobytes() and M[:a].tobytes() == head_m.tobytes()
    assert S.tobytes() == one_s.tobytes() and M.tobytes() == one_m.tobytes(), (name, options)           # byte for byte
    NC.assert_same_bits(S, want["S"], (name, options, source, "radiance"))
    NC.assert_same_bits(M, want["M"], (name, options, source, "moment2"))


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
            S, M = sentinels()
            _, _, st = c["scene"].nee(items, c["mine"], accumulate=accumulate, radiance=S, moment2=M, **kw)
            want = 7.5 if accumulate else 0.0
            assert (S == want).all() and (M == want).all(), (name, options, accumulate)
            assert st["rays"] == 0 and st["samples"] == 0
            S, _ = sentinels()
            c["scene"].nee(items, c["mine"], accumulate=accumulate, radiance=S, **kw)
            assert (S == want).all()
    d_items = torch.from_numpy(items.copy()).to("cuda:0")
    d_table = torch.from_numpy(c["mine"].view(np.uint8).copy()).to("cuda:0")
    for kw in nothing[:2]:
        for accumulate in (False, True):
            for with_m2 in (True, False):
                d_s, d_m = device_buffer(torch, N), device_buffer(torch, N)
                c["scene"].nee_device(d_items.data_ptr(), N, d_table.data_ptr(), len(c["mine"]), d_s.data_ptr() + GUARD * 12,
                                      d_m.data_ptr() + GUARD * 12 if with_m2 else 0, accumulate=accumulate, **kw)
                torch.cuda.synchronize()
                for t, written in ((d_s, True), (d_m, with_m2)):
                    got, ok = payload(t, N)
                    assert ok, (name, options, "guard bytes were written")
                    assert (got.view(np.uint32) == (0 if written and not accumulate else 0xCDCDCDCD)).all()


@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_a_shadow_end_of_one_half(trt, orc, case, name, options, shape):
    c = case(name, options, shape)
    want = NC.reference(trt, orc, name, "cosine", shadow_end=0.5)
    S, M, st = c["scene"].nee(c["cosine"]["items"], c["mine"], shadow_end=0.5, moment2=True, **c["kw"]["cosine"])
    NC.assert_same_bits(S, want["S"], (name, options, "radiance"))
    NC.assert_same_bits(M, want["M"], (name, options, "moment2"))
    assert st["samples"] == N * K and st["rays"] == want["n_rays"]
    assert NC.differing(want["S"], NC.reference(trt, orc, name, "cosine")["S"]) >= 3          # measured: 7 (prims600) to 161 (cornell) items


@pytest.mark.parametrize("source", ("rays", "cosine"))
@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_a_diffuse_source(trt, orc, case, name, options, shape, source):
    c = case(name, options, shape)
    want = NC.reference(trt, orc, name, source, source_is_diffuse=True)
    S, M, st = c["scene"].nee(c[source]["items"], c["mine"], source_is_diffuse=True, moment2=True, **c["kw"][source])
    NC.assert_same_bits(S, want["S"], (name, options, source, "radiance"))
    NC.assert_same_bits(M, want["M"], (name, options, source, "moment2"))
    assert st["samples"] == N * K and st["rays"] == want["n_rays"]
    if name in ("prims33", "prims600"):                                     # first hits on their lights are hidden now (cornell's 324 rays meet the lamp 0 or 3 times)
        assert NC.differing(want["S"], NC.reference(trt, orc, name, source)["S"]) >= 8


@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_with_one_bounce_the_result_is_the_plain_querys_on_the_device(trt, case, name, options, shape):
    """B == 1, source_is_diffuse == 0: Scene.radiance / Scene.gather byte for byte, stats included."""
    c = case(name, options, shape)
    for source in SOURCES:
        kw = dict(c["kw"][source], max_bounces=1)
        S, M, st = c["scene"].nee(c[source]["items"], c["mine"], moment2=True, **kw)
        plain = {k: v for k, v in kw.items() if k not in ("source", "spread")}
        if source == "rays":
            plain["samples_per_ray"] = plain.pop("samples_per_item")
            S0, M0, st0 = c["scene"].radiance(c[source]["items"], moment2=True, **plain)
        else:
            S0, M0, st0 = c["scene"].gather(c[source]["items"], lobe=source, spread=NC.SPREAD, moment2=True, **plain)
        assert S.tobytes() == S0.tobytes() and M.tobytes() == M0.tobytes(), (name, options, source)
        assert (st["samples"], st["rays"]) == (st0["samples"], st0["rays"])
        assert np.isfinite(S0).any() and (S0[np.isfinite(S0)] != 0).any()


def test_the_scenes_own_table_alone(trt, orc, case):
    """cornell with E = 1: the lamp itself, the table Scene.emitters() returns."""
    name, options = NC.CASES[0]
    assert name == "cornell"
    c = case(name, options, shape_of(name, options))
    table = c["scene"].emitters()
    assert len(table) == 1 and table.tobytes() == D.emitters_of(orc, c["desc"]).tobytes()
    want = NC.finish(NC.nee_paths(orc, c["ow"], c["desc"], c["cosine"]["rays"], table, background=c["bg"]), K)
    assert NC.differing(want["S"], NC.reference(trt, orc, name, "cosine")["S"]) >= 100 and int((want["lit"] > 0).sum()) >= 400
    S, M, st = c["scene"].nee(c["cosine"]["items"], table, moment2=True, **c["kw"]["cosine"])
    NC.assert_same_bits(S, want["S"], "radiance")
    NC.assert_same_bits(M, want["M"], "moment2")
    assert st["samples"] == N * K and st["rays"] == want["n_rays"]
