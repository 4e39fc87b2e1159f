"""Direct-light queries (tinyrt.h trt_direct, trt_direct_device) on the GPU against the CPU oracle, bit for bit and item by item.

Sample s of item i has stream index j = first_stream + i * K + s.  Its emitter, its point on the emitter, its weight and its shadow ray
are restated with the oracle's draws on RNG stream (seed, j, 1), float32 scalars, orc_vec3_dot and orc_ray_new; its answer is the
oracle's World.hit over [0.001, t_max); the fold is radiance_cases.fold (tests/direct_cases.py).

Items, per scene: the 324 surfels of gather_cases.items_of - a full run of 256 for one wave, a ragged one of 68 for the next, with the
NaN, zero, inf and 1e-9 items.  K = 8, seed 5, first_stream = 1000.  The table is the scene's own emitters followed by a virtual quad and
a virtual sphere, so scenes without a light are lit too.  The scenes are test_gpu_queries.DEFAULT_SHAPES plus test_gpu_queries.OTHER_WALKS;
each case asserts the kernel shape Scene.direct_plan reports, so all six instantiations of direct.hip kDirectKernels run.
tests/test_direct_cases.py asserts without a GPU that this reference is not vacuous."""
import numpy as np
import pytest

import direct_cases as D
import gather_cases as GC
import test_gpu_queries as G
import walk_ray_cases as W

pytestmark = pytest.mark.gpu

K, SEED, FIRST = D.K, D.SEED, D.FIRST_STREAM
N = D.N_ITEMS
GUARD = 64                                                                  # entries on either side of a device buffer
FILL = 0xCD
CASES = [(name, {}, shape) for name, shape in G.DEFAULT_SHAPES.items()] + list(G.OTHER_WALKS)
IDS = ["%s-%s" % (name, "-".join("%s=%s" % kv for kv in sorted(options.items())) or "default") for name, options, _ in CASES]
KW = dict(samples_per_item=K, seed=SEED, first_stream=FIRST)


@pytest.fixture(scope="module")
def reference(trt, orc):
    """name -> description, worlds, items, table and the oracle's direct-light query at shadow_end 0.999 and 0.5; computed once per scene,
    shared by every test and never changed."""
    cache = {}

    def get(name):
        if name not in cache:
            desc = W.scene(trt, name)
            ow, _ = orc.world_from_description(desc)
            items, _ = GC.items_of(orc, ow, desc)
            items.setflags(write=False)
            table = D.table_of(orc, desc)
            table.setflags(write=False)
            cache[name] = dict(desc=desc, ow=ow, world=trt.world_from_description(desc)[0], items=items, table=table,
                               ref=D.freeze(D.reference(orc, ow, items, table)), half=D.freeze(D.reference(orc, ow, items, table, shadow_end=0.5)))
        return cache[name]

    return get


@pytest.fixture(scope="module")
def case(trt, reference):
    """(name, options) -> the reference of the scene plus the product scene compiled with the options, its shape asserted, and the
    product's own table, which must be the restatement's byte for byte."""
    cache = {}

    def get(name, options, shape):
        key = (name, tuple(sorted(options.items())))
        if key not in cache:
            ref = reference(name)
            sc = ref["world"].get_bvh(**options)
            q = sc.direct_plan(N)
            assert G.plan_shape(q) == shape, (name, options, q)
            mine = trt.lights.table(sc.emitters(), trt.lights.quad(**D.VIRTUAL_QUAD), trt.lights.sphere(**D.VIRTUAL_SPHERE))
            assert mine.tobytes() == ref["table"].tobytes(), (name, options)
            cache[key] = dict(ref, scene=sc, mine=mine)
        return cache[key]

    return get


def sentinels(n=N):
    return np.full((n, 3), 7.5, np.float32), np.full((n, 3), 7.5, np.float32)


@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_host_form_is_the_oracles_fold(trt, case, name, options, shape):
    c = case(name, options, shape)
    want = c["ref"]
    S, M = sentinels()
    S, M, st = c["scene"].direct(c["items"], c["mine"], radiance=S, moment2=M, **KW)
    D.assert_same_bits(S, want["S"], (name, options, "radiance"))
    D.assert_same_bits(M, want["M"], (name, options, "moment2"))
    assert st["samples"] == N * K and st["rays"] == want["n_walks"], (name, options, st, want["n_walks"])
    # moment2 = NULL: radiance is unchanged
    S1, none, st1 = c["scene"].direct(c["items"], c["mine"], **KW)
    assert none is None and S1.tobytes() == S.tobytes()
    assert st1["samples"] == N * K and st1["rays"] == want["n_walks"]


def device_buffer(torch, n):
    return torch.full(((GUARD + n + GUARD) * 12,), FILL, dtype=torch.uint8, device="cuda:0")


def payload(t, n):
    """(payload as float32 [n, 3], guards intact?)"""
    h = t.cpu().numpy()
    g, b = GUARD * 12, n * 12
    return h[g:g + b].copy().view(np.float32).reshape(n, 3), bool((h[:g] == FILL).all() and (h[g + b:] == FILL).all())


@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_device_form_on_a_side_stream_equals_the_oracle_and_leaves_the_guards(trt, case, name, options, shape):
    import torch
    c = case(name, options, shape)
    want = c["ref"]
    E = len(c["mine"])
    d_items = torch.from_numpy(c["items"].copy()).to("cuda:0")
    d_table = torch.from_numpy(c["mine"].view(np.uint8).copy()).to("cuda:0")
    side = torch.cuda.Stream()
    d_s, d_m = device_buffer(torch, N), device_buffer(torch, N)
    ctr = torch.full((16,), 3, dtype=torch.int64, device="cuda:0")          # the counters are added to
    torch.cuda.synchronize()
    c["scene"].direct_device(d_items.data_ptr(), N, d_table.data_ptr(), E, d_s.data_ptr() + GUARD * 12, d_m.data_ptr() + GUARD * 12,
                             d_counters_ptr=ctr.data_ptr(), stream_ptr=side.cuda_stream, **KW)
    side.synchronize()
    torch.cuda.synchronize()
    got_s, ok_s = payload(d_s, N)
    got_m, ok_m = payload(d_m, N)
    assert ok_s and ok_m, (name, options, "guard bytes were written")
    D.assert_same_bits(got_s, want["S"], (name, options, "radiance"))
    D.assert_same_bits(got_m, want["M"], (name, options, "moment2"))
    assert int(ctr[0]) == 3 + N * K and int(ctr[1]) == 3 + want["n_walks"] and bool((ctr[2:] == 3).all())
    # without moment2 and without counters: the same radiance, the guards intact
    d_s1 = device_buffer(torch, N)
    c["scene"].direct_device(d_items.data_ptr(), N, d_table.data_ptr(), E, d_s1.data_ptr() + GUARD * 12, **KW)
    torch.cuda.synchronize()
    got_s1, ok_s1 = payload(d_s1, N)
    assert ok_s1 and got_s1.tobytes() == got_s.tobytes()


@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_split_by_samples_leaves_the_bytes_of_one_pass(trt, case, name, options, shape):
    c = case(name, options, shape)
    want = c["ref"]
    S, M = sentinels()
    _, _, st = c["scene"].direct(c["items"], c["mine"], sample_begin=0, sample_end=3, radiance=S, moment2=M, **KW)
    S3, M3 = D.fold(want, K, 0, 3)
    D.assert_same_bits(S, S3, (name, options, "radiance [0, 3)"))
    D.assert_same_bits(M, M3, (name, options, "moment2 [0, 3)"))
    assert st["samples"] == N * 3 and st["rays"] == int(want["walked"][:, :3].sum())
    _, _, st = c["scene"].direct(c["items"], c["mine"], sample_begin=3, sample_end=8, accumulate=True, radiance=S, moment2=M, **KW)
    D.assert_same_bits(S, want["S"], (name, options, "radiance [0, 3) + [3, 8)"))
    D.assert_same_bits(M, want["M"], (name, options, "moment2 [0, 3) + [3, 8)"))
    assert st["samples"] == N * 5 and st["rays"] == int(want["walked"][:, 3:].sum())


@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_split_by_items_leaves_the_bytes_of_one_call(trt, case, name, options, shape):
    c = case(name, options, shape)
    kw = dict(KW)
    one_s, one_m, _ = c["scene"].direct(c["items"], c["mine"], moment2=True, **kw)
    S, M = sentinels()
    a = 100
    c["scene"].direct(c["items"][:a], c["mine"], radiance=S[:a], moment2=M[:a], **kw)
    assert (S[a:] == 7.5).all() and (M[a:] == 7.5).all()                    # entries outside the call's range are untouched
    kw["first_stream"] = FIRST + a * K
    assert kw["first_stream"] == 1800
    head_s, head_m = S[:a].copy(), M[:a].copy()
    c["scene"].direct(c["items"][a:], c["mine"], radiance=S[a:], moment2=M[a:], **kw)
    assert S[:a].tobytes() == head_s.tobytes() and M[:a].tobytes() == head_m.tobytes()
    assert S.tobytes() == one_s.tobytes() and M.tobytes() == one_m.tobytes(), (name, options)           # byte for byte
    D.assert_same_bits(S, c["ref"]["S"], (name, options, "radiance"))
    D.assert_same_bits(M, c["ref"]["M"], (name, options, "moment2"))


@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_an_empty_sample_range(trt, case, name, options, shape):
    """An empty sample range zeroes the n entries without accumulate and leaves them with it; through the device form no byte outside
    [0, 12 n) is written."""
    import torch
    c = case(name, options, shape)
    kw = dict(KW, sample_begin=3, sample_end=3)
    for accumulate in (False, True):
        S, M = sentinels()
        _, _, st = c["scene"].direct(c["items"], c["mine"], accumulate=accumulate, radiance=S, moment2=M, **kw)
        want = 7.5 if accumulate else 0.0
        assert (S == want).all() and (M == want).all(), (name, options, accumulate)
        assert st["rays"] == 0 and st["samples"] == 0
        S, _ = sentinels()
        c["scene"].direct(c["items"], c["mine"], accumulate=accumulate, radiance=S, **kw)
        assert (S == want).all()
    d_items = torch.from_numpy(c["items"].copy()).to("cuda:0")
    d_table = torch.from_numpy(c["mine"].view(np.uint8).copy()).to("cuda:0")
    for accumulate in (False, True):
        for with_m2 in (True, False):
            d_s, d_m = device_buffer(torch, N), device_buffer(torch, N)
            c["scene"].direct_device(d_items.data_ptr(), N, d_table.data_ptr(), len(c["mine"]), d_s.data_ptr() + GUARD * 12,
                                     d_m.data_ptr() + GUARD * 12 if with_m2 else 0, accumulate=accumulate, **dict(KW, sample_begin=2, sample_end=2))
            torch.cuda.synchronize()
            for t, written in ((d_s, True), (d_m, with_m2)):
                got, ok = payload(t, N)
                assert ok, (name, options, "guard bytes were written")
                assert (got.view(np.uint32) == (0 if written and not accumulate else 0xCDCDCDCD)).all()


@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_a_shadow_end_of_one_half(trt, case, name, options, shape):
    c = case(name, options, shape)
    want = c["half"]
    S, M, st = c["scene"].direct(c["items"], c["mine"], shadow_end=0.5, moment2=True, **KW)
    D.assert_same_bits(S, want["S"], (name, options, "radiance"))
    D.assert_same_bits(M, want["M"], (name, options, "moment2"))
    assert st["samples"] == N * K and st["rays"] == want["n_walks"]


@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_the_restated_shadow_rays_through_occluded_are_the_oracles_samples(trt, case, name, options, shape):
    """Three-way agreement without the fold: the restatement's shadow rays and t_max through Scene.occluded equal the oracle's
    per-sample answers, which folded equal Scene.direct (above)."""
    c = case(name, options, shape)
    for which in ("ref", "half"):
        want = c[which]
        walked = want["walked"]
        got = c["scene"].occluded(want["rays"][walked], want["t_max"][walked])
        assert (got == want["occ"][walked]).all(), (name, options, which, int((got != want["occ"][walked]).sum()))
        assert 0 < got.sum() < len(got)


def test_the_scenes_own_table_alone(trt, orc, reference):
    """cornell with E = 1: the lamp itself, the table Scene.emitters() returns."""
    ref = reference("cornell")
    sc = ref["world"].get_bvh()
    table = sc.emitters()
    assert len(table) == 1 and table.tobytes() == D.emitters_of(orc, ref["desc"]).tobytes()
    want = D.reference(orc, ref["ow"], ref["items"], table)
    assert D.differing(want["S"], ref["ref"]["S"]) >= 100 and int((want["live"] & ~want["occ"]).sum()) >= 400
    S, M, st = sc.direct(ref["items"], table, moment2=True, **KW)
    D.assert_same_bits(S, want["S"], "radiance")
    D.assert_same_bits(M, want["M"], "moment2")
    assert st["samples"] == N * K and st["rays"] == want["n_walks"]
