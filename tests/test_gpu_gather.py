"""Gather queries (tinyrt.h trt_gather, trt_gather_device) on the GPU against the CPU oracle, bit for bit and item by item.

Sample s of item i has stream index j = first_stream + i * K + s.  Its first ray is drawn from RNG stream (seed, j, 1) by one of the
reference's two scatter rules - restated with the oracle's own material_scatter (cosine lobe) and its random_in_unit_sphere, vector
operations and Ray::new (cone lobe) - and its path runs on stream (seed, j, 0): orc.sample_batch over the n * K drawn rays with one
sample each (tests/gather_cases.py, tests/radiance_cases.py).  The colours are folded in numpy float32 exactly as the contract states.

Items, per scene (gather_cases.items_of): the 324 rays of radiance_cases.rays_of turned into surfels where they hit and kept as probes
where they miss, two thirds of the axes not unit, and four with NaN, zero, inf and 1e-9 axes or points - a full run of 256 for one wave, a
ragged one of 68 for the next.  K = 8, max_bounces = 8, seed 5, first_stream = 1000, both lobes, the cone with spread 0.5.  The scenes
are test_gpu_queries.DEFAULT_SHAPES plus test_gpu_queries.OTHER_WALKS; each case asserts the kernel shape Scene.gather_plan reports, so all
six instantiations of radiance.hip kGatherKernels run.

Before any GPU call the reference itself is asserted not to be vacuous: finite means, enough distinct means, cosine directions in the
hemisphere of the normal, items whose K directions differ, and folds that differ between the two lobes and from trt_radiance of the same
items - an ignored lobe or an ignored draw cannot pass."""
import numpy as np
import pytest

import gather_cases as GC
import radiance_cases as R
import test_gpu_queries as G
import walk_ray_cases as W

pytestmark = pytest.mark.gpu

K, DEPTH, SEED, FIRST, SPREAD = GC.K, GC.MAX_BOUNCES, GC.SEED, GC.FIRST_STREAM, GC.SPREAD
N = GC.N_ITEMS
GUARD = 64                                                                  # entries on either side of a device buffer
FILL = 0xCD
CASES = [(name, {}, shape) for name, shape in G.DEFAULT_SHAPES.items()] + list(G.OTHER_WALKS)
IDS = ["%s-%s" % (name, "-".join("%s=%s" % kv for kv in sorted(options.items())) or "default") for name, options, _ in CASES]
BROKEN_GEOMETRY = ("degenerate", "nonfinite")
LOBES = GC.LOBES


def differing(a, b):
    """Number of items whose bits differ."""
    return int((a.view(np.uint32) != b.view(np.uint32)).any(axis=1).sum())


@pytest.fixture(scope="module")
def reference(trt, orc):
    """name -> description, world, items, and per lobe the oracle's first rays [n, K, 6], per-sample colours [n, K, 3], ray count and
    folds; computed once per scene, shared by every test and never changed."""
    cache = {}

    def get(name):
        if name in cache:
            return cache[name]
        desc = W.scene(trt, name)
        ow, _ = orc.world_from_description(desc)
        items, unit = GC.items_of(orc, ow, desc)
        bg = tuple(desc["background"])
        ref = dict(desc=desc, world=trt.world_from_description(desc)[0], items=items, bg=bg)
        for lobe in LOBES:
            rays, cols, n_rays = GC.oracle_gather(orc, ow, items, lobe, K, DEPTH, bg, SEED, FIRST)
            S, M = R.fold(cols, K)
            ref[lobe] = dict(rays=rays, cols=cols, n_rays=n_rays, S=S, M=M)
        # the trt_radiance of the same items: what an ignored draw would return
        cols_r, _ = R.oracle_samples(orc, ow, items, K, DEPTH, bg, SEED, FIRST)
        S_r, _ = R.fold(cols_r, K)
        # the case is not vacuous
        for lobe in LOBES:
            S, rays = ref[lobe]["S"], ref[lobe]["rays"]
            assert np.isfinite(S).all(), (name, lobe)
            distinct = len({row.tobytes() for row in S})
            assert distinct >= (15 if name in BROKEN_GEOMETRY else 90), (name, lobe, distinct)
            assert int((rays[:, :, 3:6] != rays[:, :1, 3:6]).any(axis=(1, 2)).sum()) >= N - 4, (name, lobe)       # the K directions of an item differ
            assert differing(S, S_r) >= 10, (name, lobe)
        assert differing(ref["cosine"]["S"], ref["cone"]["S"]) >= 10, name
        assert unit.sum() >= (5 if name in BROKEN_GEOMETRY else 30), (name, int(unit.sum()))
        d = ref["cosine"]["rays"][unit][:, :, 3:6].astype(np.float64)
        assert (np.einsum("nkc,nc->nk", d, items[unit, 3:6].astype(np.float64)) >= 0.0).all(), name    # the hemisphere of the normal
        for a in [items] + [ref[lobe][k] for lobe in LOBES for k in ("rays", "cols", "S", "M")]:
            a.setflags(write=False)
        cache[name] = ref
        return ref

    return get


@pytest.fixture(scope="module")
def case(reference):
    """(name, options) -> the reference of the scene plus the product scene compiled with the options, its shape asserted."""
    cache = {}

    def get(name, options, shape):
        key = (name, tuple(sorted(options.items())))
        if key not in cache:
            ref = reference(name)
            sc = ref["world"].get_bvh(**options)
            q = sc.gather_plan(N)
            assert G.plan_shape(q) == shape, (name, options, q)
            kw = dict(samples_per_item=K, max_bounces=DEPTH, background=ref["bg"], seed=SEED, first_stream=FIRST)
            cache[key] = dict(ref, scene=sc, kw={"cosine": dict(kw, lobe="cosine"), "cone": dict(kw, lobe="cone", spread=SPREAD)})
        return cache[key]

    return get


def sentinel(n=N):
    return np.full((n, 3), 7.5, np.float32)


@pytest.mark.parametrize("lobe", LOBES)
@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_host_form_is_the_oracles_fold(trt, case, name, options, shape, lobe):
    c = case(name, options, shape)
    S, M, st = c["scene"].gather(c["items"], radiance=sentinel(), moment2=sentinel(), **c["kw"][lobe])
    R.assert_same_bits(S, c[lobe]["S"], (name, options, lobe, "radiance"))
    R.assert_same_bits(M, c[lobe]["M"], (name, options, lobe, "moment2"))
    assert st["samples"] == N * K
    assert st["rays"] == c[lobe]["n_rays"], (name, options, lobe)
    # moment2 = NULL: radiance is unchanged
    S1, none, _ = c["scene"].gather(c["items"], **c["kw"][lobe])
    assert none is None and S1.tobytes() == S.tobytes()


def device_buffer(torch, n):
    return torch.full(((GUARD + n + GUARD) * 12,), FILL, dtype=torch.uint8, device="cuda:0")


def payload(t, n):
    """(payload as float32 [n, 3], guards intact?)"""
    h = t.cpu().numpy()
    g = GUARD * 12
    return h[g:g + n * 12].copy().view(np.float32).reshape(n, 3), bool((h[:g] == FILL).all() and (h[g + n * 12:] == FILL).all())


@pytest.mark.parametrize("lobe", LOBES)
@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_device_form_on_a_side_stream_equals_the_oracle_and_leaves_the_guards(trt, case, name, options, shape, lobe):
    import torch
    c = case(name, options, shape)
    d_items = torch.from_numpy(c["items"].copy()).to("cuda:0")
    side = torch.cuda.Stream()
    d_s, d_m = device_buffer(torch, N), device_buffer(torch, N)
    ctr = torch.full((16,), 3, dtype=torch.int64, device="cuda:0")          # the counters are added to
    torch.cuda.synchronize()
    c["scene"].gather_device(d_items.data_ptr(), N, d_s.data_ptr() + GUARD * 12, d_m.data_ptr() + GUARD * 12, d_counters_ptr=ctr.data_ptr(),
                             stream_ptr=side.cuda_stream, **c["kw"][lobe])
    side.synchronize()
    torch.cuda.synchronize()
    got_s, ok_s = payload(d_s, N)
    got_m, ok_m = payload(d_m, N)
    assert ok_s and ok_m, (name, options, lobe, "guard bytes were written")
    R.assert_same_bits(got_s, c[lobe]["S"], (name, options, lobe, "radiance"))
    R.assert_same_bits(got_m, c[lobe]["M"], (name, options, lobe, "moment2"))
    assert int(ctr[0]) == 3 + N * K and int(ctr[1]) == 3 + c[lobe]["n_rays"] and bool((ctr[2:] == 3).all())


@pytest.mark.parametrize("lobe", LOBES)
@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_split_by_samples_leaves_the_bytes_of_one_pass(trt, case, name, options, shape, lobe):
    c = case(name, options, shape)
    S, M = sentinel(), sentinel()
    c["scene"].gather(c["items"], sample_begin=0, sample_end=3, radiance=S, moment2=M, **c["kw"][lobe])
    S3, M3 = R.fold(c[lobe]["cols"], K, 0, 3)
    R.assert_same_bits(S, S3, (name, options, lobe, "radiance [0, 3)"))
    R.assert_same_bits(M, M3, (name, options, lobe, "moment2 [0, 3)"))
    _, _, st = c["scene"].gather(c["items"], sample_begin=3, sample_end=8, accumulate=True, radiance=S, moment2=M, **c["kw"][lobe])
    R.assert_same_bits(S, c[lobe]["S"], (name, options, lobe, "radiance [0, 3) + [3, 8)"))
    R.assert_same_bits(M, c[lobe]["M"], (name, options, lobe, "moment2 [0, 3) + [3, 8)"))
    assert st["samples"] == N * 5


@pytest.mark.parametrize("lobe", LOBES)
@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_split_by_items_leaves_the_bytes_of_one_call(trt, case, name, options, shape, lobe):
    c = case(name, options, shape)
    one_s, one_m, _ = c["scene"].gather(c["items"], moment2=True, **c["kw"][lobe])
    S, M = sentinel(), sentinel()
    kw = dict(c["kw"][lobe])
    a = 100
    c["scene"].gather(c["items"][:a], radiance=S[:a], moment2=M[:a], **kw)
    assert (S[a:] == 7.5).all() and (M[a:] == 7.5).all()                    # entries outside the call's range are untouched
    kw["first_stream"] = FIRST + a * K
    assert kw["first_stream"] == 1800
    head_s, head_m = S[:a].copy(), M[:a].copy()
    c["scene"].gather(c["items"][a:], radiance=S[a:], moment2=M[a:], **kw)
    assert S[:a].tobytes() == head_s.tobytes() and M[:a].tobytes() == head_m.tobytes()
    assert S.tobytes() == one_s.tobytes() and M.tobytes() == one_m.tobytes(), (name, options, lobe)       # byte for byte
    R.assert_same_bits(S, c[lobe]["S"], (name, options, lobe, "radiance"))
    R.assert_same_bits(M, c[lobe]["M"], (name, options, lobe, "moment2"))


@pytest.mark.parametrize("lobe", LOBES)
@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_the_drawn_rays_through_radiance_fold_to_the_gather(trt, case, name, options, shape, lobe):
    """Without the oracle's paths: the n * K oracle-drawn first rays through Scene.radiance with one sample each and the same
    first_stream (ray i * K + s has stream first_stream + i * K + s), folded in numpy, equal Scene.gather.  Product against product."""
    c = case(name, options, shape)
    kw = {k: v for k, v in c["kw"][lobe].items() if k not in ("samples_per_item", "lobe", "spread")}
    cols, _, st1 = c["scene"].radiance(c[lobe]["rays"].reshape(-1, 6), 1, **kw)
    want_s, want_m = R.fold(cols.reshape(N, K, 3), K)
    S, M, st = c["scene"].gather(c["items"], moment2=True, **c["kw"][lobe])
    R.assert_same_bits(S, want_s, (name, options, lobe, "radiance"))
    R.assert_same_bits(M, want_m, (name, options, lobe, "moment2"))
    assert st["rays"] == st1["rays"] and st["samples"] == st1["samples"] == N * K


@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_nothing_to_trace_zeroes_or_leaves(trt, case, name, options, shape):
    """max_bounces == 0 and an empty sample range: the n entries are zeroed without accumulate and untouched with it; through the
    device form no byte outside [0, 12 n) is written."""
    import torch
    c = case(name, options, shape)
    for lobe in LOBES:
        for over in (dict(max_bounces=0), dict(sample_begin=3, sample_end=3)):
            kw = dict(c["kw"][lobe], **over)
            for accumulate in (False, True):
                S, M = sentinel(), sentinel()
                _, _, st = c["scene"].gather(c["items"], accumulate=accumulate, radiance=S, moment2=M, **kw)
                want = 7.5 if accumulate else 0.0
                assert (S == want).all() and (M == want).all(), (name, options, lobe, over, accumulate)
                assert st["rays"] == 0 and st["samples"] == 0
                S = sentinel()
                c["scene"].gather(c["items"], accumulate=accumulate, radiance=S, **kw)
                assert (S == want).all()
    d_items = torch.from_numpy(c["items"].copy()).to("cuda:0")
    for accumulate in (False, True):
        d_s, d_m = device_buffer(torch, N), device_buffer(torch, N)
        c["scene"].gather_device(d_items.data_ptr(), N, d_s.data_ptr() + GUARD * 12, d_m.data_ptr() + GUARD * 12, accumulate=accumulate,
                                 **dict(c["kw"]["cone"], max_bounces=0))
        torch.cuda.synchronize()
        for t in (d_s, d_m):
            got, ok = payload(t, N)
            assert ok, (name, options, "guard bytes were written")
            assert (got.view(np.uint32) == (0xCDCDCDCD if accumulate else 0)).all()


LONG_DEPTH, LONG_STRIDE = 2, 997


@pytest.mark.parametrize("lobe", LOBES)
def test_a_batch_with_lengthened_runs(trt, orc, reference, lobe):
    """Cornell, K = 1, max_bounces = 2, the smallest n at which a wave's run grows past 256 items on the device at hand (some millions):
    the 324 items tiled (item i = item i mod 324; every i has a stream of its own, so no two samples repeat).  One call equals two calls
    split at an odd index, byte for byte, and every 997th item equals the oracle - its first ray drawn for stream first_stream + i and
    its path through orc.sample_batch on a list in which every other point only occupies its stream."""
    ref = reference("cornell")
    sc = ref["world"].get_bvh()
    assert G.plan_shape(sc.gather_plan(1)) == G.DEFAULT_SHAPES["cornell"]
    q1 = sc.gather_plan(1)
    assert q1["rays_per_wave"] == 256
    n = 256 * q1["wave_slots"] + 1                                          # ceil(n / 256) exceeds the resident wave slots
    assert sc.gather_plan(n - 1)["rays_per_wave"] == 256 and sc.gather_plan(n)["rays_per_wave"] > 256
    items = np.ascontiguousarray(ref["items"][np.arange(n) % N])
    kw = dict(samples_per_item=1, lobe=lobe, spread=SPREAD, max_bounces=LONG_DEPTH, background=ref["bg"], seed=SEED)
    one_s, one_m, st = sc.gather(items, first_stream=FIRST, moment2=True, **kw)
    assert st["samples"] == n
    a = n // 2 | 1
    S, M = np.full((n, 3), 7.5, np.float32), np.full((n, 3), 7.5, np.float32)
    _, _, st_a = sc.gather(items[:a], first_stream=FIRST, radiance=S[:a], moment2=M[:a], **kw)
    _, _, st_b = sc.gather(items[a:], first_stream=FIRST + a, radiance=S[a:], moment2=M[a:], **kw)
    assert S.tobytes() == one_s.tobytes() and M.tobytes() == one_m.tobytes()
    assert st_a["rays"] + st_b["rays"] == st["rays"]
    # every 997th item against the oracle
    ow, _ = orc.world_from_description(ref["desc"])
    pick = np.arange(0, n, LONG_STRIDE)
    first = GC.first_rays(orc, items, lobe, 1, SPREAD, SEED, FIRST, only=pick)[:, 0, :]
    rays = np.tile(np.array(R.DUMMY, np.float32), (n, 1))
    rays[pick] = first[pick]
    out, _ = orc.sample_batch(ow, R.points_of(orc.SamplePoint, rays, FIRST), LONG_DEPTH, ref["bg"], SEED)
    want = R.colors_of(out, FIRST + n)[FIRST:][pick]
    # two segments in the Cornell box end in few colours - 0, the background seen through the open front, its product with a wall's
    # albedo, the light and its products: the sample is not vacuous if it holds four of them, which a constant answer cannot match
    assert len({row.tobytes() for row in want}) >= 4 and len(pick) >= 256
    R.assert_same_bits(one_s[pick], want, (lobe, "radiance", n))
    with np.errstate(all="ignore"):
        R.assert_same_bits(one_m[pick], want * want, (lobe, "moment2 of one sample", n))
