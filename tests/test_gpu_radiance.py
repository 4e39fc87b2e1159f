"""Radiance queries (tinyrt.h trt_radiance, trt_radiance_device) on the GPU against the CPU oracle, bit for bit and ray by ray.

Sample s of ray i uses RNG stream (seed, first_stream + i * K + s, 0): trt_sample_batch's numbering opened by an offset.  The reference
is therefore orc.sample_batch - the oracle's restatement of that entry point - over first_stream leading dummy points followed by each ray
K times; its colours are folded in numpy float32 exactly as the contract states (tests/radiance_cases.py).  The oracle's `rays` counts
the reference's world.hit calls, which is what stats.rays reports whatever the kernel shares between the samples of a ray.

Rays, per scene: a 20 x 16 pinhole grid of the scene's camera, most directions not unit, and four rays with NaN, inf and zero components:
324 rays - a full run of 256 for one wave, a ragged one of 68 for the next, three refills per lane group.  K = 8, max_bounces = 8, seed 5,
first_stream = 1000.  The scenes are test_gpu_queries.SCENES compiled by default plus test_gpu_queries.OTHER_WALKS; each case asserts the
kernel shape Scene.radiance_plan reports, so all six instantiations of radiance.hip kRadianceKernels run.

Before any GPU call the reference itself is asserted not to be vacuous: finite means, enough distinct means, rays whose samples differ,
rays whose colour changes with first_stream - a constant image, an ignored sample index or an ignored first_stream cannot pass."""
import numpy as np
import pytest

import radiance_cases as R
import test_gpu_queries as G
import walk_ray_cases as W
from denoise_color_cases import restated_variance

pytestmark = pytest.mark.gpu

K, DEPTH, SEED, FIRST = R.K, R.MAX_BOUNCES, R.SEED, R.FIRST_STREAM
N = R.N_RAYS
GUARD = 64                                                                  # entries on either side of a device buffer
FILL = 0xCD
CASES = [(name, {}, shape) for name, shape in G.DEFAULT_SHAPES.items()] + list(G.OTHER_WALKS)
IDS = ["%s-%s" % (name, "-".join("%s=%s" % kv for kv in sorted(options.items())) or "default") for name, options, _ in CASES]
BROKEN_GEOMETRY = ("degenerate", "nonfinite")


@pytest.fixture(scope="module")
def reference(trt, orc):
    """name -> description, world, rays, the oracle's per-sample colours [n, K, 3], its ray count, the folds; computed once per scene,
    shared by every test and never changed."""
    cache = {}

    def get(name):
        if name in cache:
            return cache[name]
        desc = W.scene(trt, name)
        ow, _ = orc.world_from_description(desc)
        rays = R.rays_of(desc)
        bg = tuple(desc["background"])
        cols, n_rays = R.oracle_samples(orc, ow, rays, K, DEPTH, bg, SEED, FIRST)
        cols0, _ = R.oracle_samples(orc, ow, rays, K, DEPTH, bg, SEED, 0)
        S, M = R.fold(cols, K)
        S0, _ = R.fold(cols0, K)
        # the case is not vacuous
        assert np.isfinite(S).all(), name
        distinct = len({row.tobytes() for row in S})
        assert distinct >= (15 if name in BROKEN_GEOMETRY else 90), (name, distinct)
        assert int((cols != cols[:, :1, :]).any(axis=(1, 2)).sum()) >= 10, name
        assert int((S.view(np.uint32) != S0.view(np.uint32)).any(axis=1).sum()) >= 10, name
        for a in (rays, cols, S, M):
            a.setflags(write=False)
        cache[name] = dict(desc=desc, world=trt.world_from_description(desc)[0], rays=rays, bg=bg, cols=cols, n_rays=n_rays, S=S, M=M)
        return cache[name]

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
            q = sc.radiance_plan(N)
            assert G.plan_shape(q) == shape, (name, options, q)
            cache[key] = dict(ref, scene=sc, kw=dict(samples_per_ray=K, max_bounces=DEPTH, background=ref["bg"], seed=SEED, first_stream=FIRST))
        return cache[key]

    return get


def sentinel(n=N):
    return np.full((n, 3), 7.5, np.float32)


@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_host_form_is_the_oracles_fold(trt, case, name, options, shape):
    c = case(name, options, shape)
    S, M, st = c["scene"].radiance(c["rays"], radiance=sentinel(), moment2=sentinel(), **c["kw"])
    R.assert_same_bits(S, c["S"], (name, options, "radiance"))
    R.assert_same_bits(M, c["M"], (name, options, "moment2"))
    assert st["samples"] == N * K
    assert st["rays"] == c["n_rays"], (name, options)
    # moment2 = NULL: radiance is unchanged
    S1, none, _ = c["scene"].radiance(c["rays"], **c["kw"])
    assert none is None and S1.tobytes() == S.tobytes()


def device_buffer(torch, n):
    return torch.full(((GUARD + n + GUARD) * 12,), FILL, dtype=torch.uint8, device="cuda:0")


def payload(t, n):
    """(payload as float32 [n, 3], guards intact?)"""
    h = t.cpu().numpy()
    g = GUARD * 12
    return h[g:g + n * 12].copy().view(np.float32).reshape(n, 3), bool((h[:g] == FILL).all() and (h[g + n * 12:] == FILL).all())


@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_device_form_on_a_side_stream_equals_the_host_form_and_leaves_the_guards(trt, case, name, options, shape):
    import torch
    c = case(name, options, shape)
    d_rays = torch.from_numpy(c["rays"].copy()).to("cuda:0")
    side = torch.cuda.Stream()
    d_s, d_m = device_buffer(torch, N), device_buffer(torch, N)
    ctr = torch.zeros(16, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    c["scene"].radiance_device(d_rays.data_ptr(), N, d_s.data_ptr() + GUARD * 12, d_m.data_ptr() + GUARD * 12, d_counters_ptr=ctr.data_ptr(),
                               stream_ptr=side.cuda_stream, **c["kw"])
    side.synchronize()
    torch.cuda.synchronize()
    got_s, ok_s = payload(d_s, N)
    got_m, ok_m = payload(d_m, N)
    assert ok_s and ok_m, (name, options, "guard bytes were written")
    R.assert_same_bits(got_s, c["S"], (name, options, "radiance"))
    R.assert_same_bits(got_m, c["M"], (name, options, "moment2"))
    assert int(ctr[0]) == N * K and int(ctr[1]) == c["n_rays"] and not bool(ctr[2:].any())


@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_split_by_samples_leaves_the_bytes_of_one_pass(trt, case, name, options, shape):
    c = case(name, options, shape)
    S, M = sentinel(), sentinel()
    c["scene"].radiance(c["rays"], sample_begin=0, sample_end=3, radiance=S, moment2=M, **c["kw"])
    S3, M3 = R.fold(c["cols"], K, 0, 3)
    R.assert_same_bits(S, S3, (name, options, "radiance [0, 3)"))
    R.assert_same_bits(M, M3, (name, options, "moment2 [0, 3)"))
    _, _, st = c["scene"].radiance(c["rays"], sample_begin=3, sample_end=8, accumulate=True, radiance=S, moment2=M, **c["kw"])
    R.assert_same_bits(S, c["S"], (name, options, "radiance [0, 3) + [3, 8)"))
    R.assert_same_bits(M, c["M"], (name, options, "moment2 [0, 3) + [3, 8)"))
    assert st["samples"] == N * 5


@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_split_by_rays_leaves_the_bytes_of_one_call(trt, case, name, options, shape):
    c = case(name, options, shape)
    S, M = sentinel(), sentinel()
    kw = dict(c["kw"])
    a = 100
    kw["first_stream"] = FIRST
    c["scene"].radiance(c["rays"][:a], radiance=S[:a], moment2=M[:a], **kw)
    assert (S[a:] == 7.5).all() and (M[a:] == 7.5).all()                    # entries outside the call's range are untouched
    R.assert_same_bits(S[:a], c["S"][:a], (name, options, "radiance [0, 100)"))
    kw["first_stream"] = FIRST + a * K
    assert kw["first_stream"] == 1800
    head_s, head_m = S[:a].copy(), M[:a].copy()
    c["scene"].radiance(c["rays"][a:], radiance=S[a:], moment2=M[a:], **kw)
    assert S[:a].tobytes() == head_s.tobytes() and M[:a].tobytes() == head_m.tobytes()
    R.assert_same_bits(S, c["S"], (name, options, "radiance"))
    R.assert_same_bits(M, c["M"], (name, options, "moment2"))


@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_one_sample_from_stream_zero_is_sample_batch(trt, case, name, options, shape):
    """K = 1 and first_stream = 0: radiance[i] is trt_sample_batch's out[i].color for the same rays, through its counting kernel and
    through its production walk.  Product against product: no oracle."""
    c = case(name, options, shape)
    kw = dict(c["kw"], samples_per_ray=1, first_stream=0)
    S, M, st = c["scene"].radiance(c["rays"], moment2=True, **kw)
    assert st["samples"] == N
    points = R.points_of(trt.SamplePoint, c["rays"])
    for collect_stats in (False, True):
        out, bst = trt.sample_batch(c["scene"], points, DEPTH, c["bg"], SEED, collect_stats=collect_stats)
        R.assert_same_bits(S, R.colors_of(out, N), (name, options, collect_stats))
        if collect_stats:
            assert st["rays"] == bst["rays"], (name, options)
    with np.errstate(all="ignore"):
        R.assert_same_bits(M, S * S, (name, options, "moment2 of one sample"))


@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_nothing_to_trace_zeroes_or_leaves(trt, case, name, options, shape):
    """max_bounces == 0 and an empty sample range: the n entries are zeroed without accumulate and untouched with it; through the
    device form no byte outside [0, 12 n) is written."""
    import torch
    c = case(name, options, shape)
    for over in (dict(max_bounces=0), dict(sample_begin=3, sample_end=3)):
        kw = dict(c["kw"], **over)
        for accumulate in (False, True):
            S, M = sentinel(), sentinel()
            _, _, st = c["scene"].radiance(c["rays"], accumulate=accumulate, radiance=S, moment2=M, **kw)
            want = 7.5 if accumulate else 0.0
            assert (S == want).all() and (M == want).all(), (name, options, over, accumulate)
            assert st["rays"] == 0
            S = sentinel()
            c["scene"].radiance(c["rays"], accumulate=accumulate, radiance=S, **kw)
            assert (S == want).all()
    d_rays = torch.from_numpy(c["rays"].copy()).to("cuda:0")
    for accumulate in (False, True):
        d_s, d_m = device_buffer(torch, N), device_buffer(torch, N)
        c["scene"].radiance_device(d_rays.data_ptr(), N, d_s.data_ptr() + GUARD * 12, d_m.data_ptr() + GUARD * 12, accumulate=accumulate,
                                   **dict(c["kw"], max_bounces=0))
        torch.cuda.synchronize()
        for t in (d_s, d_m):
            got, ok = payload(t, N)
            assert ok, (name, options, "guard bytes were written")
            assert (got.view(np.uint32) == (0xCDCDCDCD if accumulate else 0)).all()


@pytest.mark.parametrize("name", G.SCENES)
def test_variance_of_the_result(trt, case, name):
    """trt_variance on (radiance, moment2) is its numpy restatement over the reference's S and M: the variance of each ray's estimate."""
    c = case(name, {}, G.DEFAULT_SHAPES[name])
    S, M, _ = c["scene"].radiance(c["rays"], moment2=True, **c["kw"])
    got = trt.variance(S, M, K)
    want = restated_variance(c["S"], c["M"], K)
    assert got.shape == want.shape == (N,)
    R.assert_same_bits(got.reshape(N, 1), want.reshape(N, 1), (name, "variance"))
