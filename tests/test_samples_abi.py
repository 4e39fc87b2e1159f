"""The sample query entry points (tinyrt.h trt_samples, trt_samples_device, trt_samples_launch_plan, trt_samples_params_default) and the
fold of their records (trt_fold_samples, trt_fold_samples_device) at the C boundary, without a GPU: the symbols are declared, exported and
bound, misuse comes back as TRT_ERR_INVALID_ARG with a message before any device work, an empty batch succeeds without a device, and the
launch plan of n items with a range of R samples is the gather queries' plan of n * R items but for the kernel's launch bound.  What the
buffers hold is checked on the GPU (tests/test_gpu_samples.py, tests/test_gpu_samples_fold.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_query_abi import _check_query_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"trt_samples_params_default": (None, 1), "trt_samples": (C.c_int, 7), "trt_samples_device": (C.c_int, 8),
         "trt_samples_launch_plan": (C.c_int, 5), "trt_fold_samples": (C.c_int, 5), "trt_fold_samples_device": (C.c_int, 6)}


def test_the_symbols_are_declared_exported_and_bound(trt):
    text = open(os.path.join(ROOT, "include", "tinyrt.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = C.CDLL(trt._lib.LIB_PATH)
    later = re.search(r"Later under 4[^/]*\*/", text, flags=re.S).group(0)
    for name, (restype, nargs) in NAMES.items():
        ret = "void" if restype is None else "int"
        assert re.search(r"\b" + ret + r"\s+" + name + r"\s*\(", header), name + " is not declared in tinyrt.h"
        assert hasattr(raw, name), name + " is not exported"
        res, args = trt._lib.SIGNATURES[name]
        assert res is restype and len(args) == nargs, name
        assert re.search(r"\b" + name + r"\b", later), name + " is not listed under 'Later under 4'"
    assert "trt_samples_params," in later and "trt_sample_source," in later
    assert re.search(r"enum\s+trt_sample_source\s*\{\s*TRT_SAMPLE_RAYS\s*=\s*0\s*,\s*TRT_SAMPLE_COSINE\s*=\s*1\s*,\s*TRT_SAMPLE_CONE\s*=\s*2\s*,\s*"
                     r"TRT_SAMPLE_SPHERE\s*=\s*3\s*,\s*TRT_SAMPLE_HEMISPHERE\s*=\s*4\s*\}", header)
    L = trt._lib
    assert (L.SAMPLE_RAYS, L.SAMPLE_COSINE, L.SAMPLE_CONE, L.SAMPLE_SPHERE, L.SAMPLE_HEMISPHERE) == (0, 1, 2, 3, 4)
    assert (L.SAMPLE_RAYS, L.SAMPLE_COSINE, L.SAMPLE_CONE) == (L.PASSES_RAYS, L.PASSES_COSINE, L.PASSES_CONE)
    assert trt.lib.trt_abi_version() == 4                                  # new symbols only: the ABI version stays
    P = L.SamplesParams
    assert C.sizeof(P) == 96
    assert (P.path.offset, P.source.offset, P.spread.offset, P.reserved.offset) == (0, 64, 68, 72)
    # no existing struct changed
    R, G = L.RadianceParams, L.GatherParams
    assert C.sizeof(R) == 64 and C.sizeof(G) == 96 and C.sizeof(L.ProbeParams) == 96
    assert (R.samples_per_ray.offset, R.max_bounces.offset, R.background.offset, R.seed.offset, R.sample_begin.offset, R.sample_end.offset,
            R.accumulate.offset, R.first_stream.offset, R.reserved.offset) == (0, 4, 8, 20, 24, 28, 32, 36, 40)
    # the signatures are the gather queries' with the params struct exchanged; the plan takes the range's length
    for name in ("trt_samples", "trt_samples_device"):
        mine, theirs = L.SIGNATURES[name][1], L.SIGNATURES[name.replace("samples", "gather")][1]
        assert mine[3] is C.POINTER(P) and mine[:3] + mine[4:] == theirs[:3] + theirs[4:], name
    plan, gplan = L.SIGNATURES["trt_samples_launch_plan"][1], L.SIGNATURES["trt_gather_launch_plan"][1]
    assert plan == gplan[:2] + [C.c_uint32] + gplan[2:]
    for name in ("samples", "samples_device", "samples_plan"):
        assert callable(getattr(trt.Scene, name))
    assert callable(trt.fold_samples) and callable(trt.fold_samples_device) and callable(trt.sh.project)


def test_the_default_parameters(trt):
    p = trt._lib.SamplesParams()
    C.memset(C.byref(p), 0xCD, C.sizeof(p))
    trt.lib.trt_samples_params_default(C.byref(p))
    want = trt._lib.RadianceParams()
    trt.lib.trt_radiance_params_default(C.byref(want))
    assert bytes(p.path) == bytes(want)
    assert (p.path.samples_per_ray, p.path.max_bounces, p.path.seed, p.path.accumulate) == (1, 50, 1, 0)
    assert p.source == trt._lib.SAMPLE_COSINE and p.spread == 0.0 and list(p.reserved) == [0] * 6
    trt.lib.trt_samples_params_default(None)                               # tolerated


def _scene(trt):
    return trt.world_from_description(trt.scenes.cornell(8, 8))[0].get_bvh()


PATH_FIELDS = ("samples_per_ray", "max_bounces", "seed", "sample_begin", "sample_end", "accumulate", "first_stream")
N, K = 3, 4


def _params(trt, **over):
    """K = 4, depth 4, seed 5, cosine; a keyword that names a field of the path sets it there."""
    p = trt._lib.SamplesParams()
    trt.lib.trt_samples_params_default(C.byref(p))
    p.path.samples_per_ray, p.path.max_bounces, p.path.seed = K, 4, 5
    for k, v in over.items():
        setattr(p.path if k in PATH_FIELDS else p, k, v)
    return p


def _invalid(trt, rc, word=None):
    assert rc == trt._lib.ERR_INVALID_ARG
    msg = trt.lib.trt_last_error().decode()
    assert msg != "" and (word is None or word in msg), msg


def _call(trt, device, s, items, n, p, colors, directions=None):
    if device:
        return trt.lib.trt_samples_device(s, items, n, p, colors, directions, None, None)
    return trt.lib.trt_samples(s, items, n, p, colors, directions, None)


@pytest.mark.parametrize("device", (False, True))
def test_misuse_is_invalid_arg_before_any_device_work(trt, device):
    """(Host pointers are handed to the device form too: every one of these calls must return before anything is dereferenced.)"""
    sc = _scene(trt)
    items = np.zeros((N, 6), np.float32)
    items[:, 4] = 1.0
    cols = np.full((N, K, 3), 7.0, np.float32)
    dirs = np.full((N, K, 3), 7.0, np.float32)
    ip, cp, dp = items.ctypes.data, cols.ctypes.data, dirs.ctypes.data
    p = _params(trt)

    def call(s, r, n, q, a, d=dp):
        return _call(trt, device, s, r, n, C.byref(q) if q is not None else None, a, d)

    # trt_radiance's own errors, applied to p->path, with colors as the required buffer
    _invalid(trt, call(None, ip, N, p, cp))
    _invalid(trt, call(sc._h, ip, N, None, cp))
    _invalid(trt, call(sc._h, None, N, p, cp))
    _invalid(trt, call(sc._h, ip, N, p, None))
    _invalid(trt, call(sc._h, ip, N, _params(trt, samples_per_ray=0), cp))
    _invalid(trt, call(sc._h, ip, N, _params(trt, sample_begin=3, sample_end=2), cp))
    _invalid(trt, call(sc._h, ip, N, _params(trt, sample_end=K + 1), cp))
    _invalid(trt, call(sc._h, ip, N, _params(trt, sample_begin=K + 1), cp))
    for k in range(6):
        q = _params(trt)
        q.path.reserved[k] = 1
        _invalid(trt, call(sc._h, ip, N, q, cp), "reserved")
    # the sample queries' own
    for accumulate in (1, 2, 2 ** 32 - 1):
        _invalid(trt, call(sc._h, ip, N, _params(trt, accumulate=accumulate), cp), "accumulate")
    for source in (5, 6, 2 ** 32 - 1):
        _invalid(trt, call(sc._h, ip, N, _params(trt, source=source), cp), "source")
    for spread in (-1.0, float("inf"), float("nan")):
        _invalid(trt, call(sc._h, ip, N, _params(trt, source=trt._lib.SAMPLE_CONE, spread=spread), cp), "spread")
    for k in range(6):
        q = _params(trt)
        q.reserved[k] = 1
        _invalid(trt, call(sc._h, ip, N, q, cp), "reserved")
    # first_stream + n * K <= 2^32 in 64 bits, and n * R <= 2^32 - 1
    _invalid(trt, call(sc._h, ip, N, _params(trt, first_stream=2 ** 32 - N * K + 1), cp), "2^32")
    _invalid(trt, call(sc._h, ip, 2 ** 32 - 1, _params(trt, samples_per_ray=2 ** 32 - 1, first_stream=2 ** 32 - 1), cp))
    _invalid(trt, call(sc._h, ip, 2 ** 31, _params(trt, samples_per_ray=2), cp), "2^32 - 1 samples")       # n * K = 2^32 streams fit, n * R does not
    want_ok = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE
    if want_ok != trt._lib.TRT_OK:
        # ... while the same batch with a range of one sample less per item is well formed, as are a spread the other sources do not read
        assert call(sc._h, ip, 2 ** 31, _params(trt, samples_per_ray=2, sample_begin=1), cp) == want_ok
        assert call(sc._h, ip, N, _params(trt, first_stream=2 ** 32 - N * K), cp) == want_ok
        for source in range(5):
            if source != trt._lib.SAMPLE_CONE:
                assert call(sc._h, ip, N, _params(trt, source=source, spread=float("nan")), cp) == want_ok
        assert call(sc._h, ip, N, _params(trt, source=trt._lib.SAMPLE_CONE, spread=0.0), cp, None) == want_ok
    # ... and an empty batch is checked too
    _invalid(trt, call(None, None, 0, p, None))
    _invalid(trt, call(sc._h, None, 0, None, None))
    _invalid(trt, call(sc._h, None, 0, _params(trt, samples_per_ray=0), None))
    _invalid(trt, call(sc._h, None, 0, _params(trt, accumulate=1), None))
    _invalid(trt, call(sc._h, None, 0, _params(trt, source=5), None))
    assert (cols == 7.0).all() and (dirs == 7.0).all()


@pytest.mark.parametrize("device", (False, True))
def test_an_empty_batch_succeeds_without_a_device_and_touches_nothing(trt, device):
    sc = _scene(trt)
    cols = np.full((N, K, 3), 7.0, np.float32)
    for source in range(5):
        p = _params(trt, source=source, first_stream=2 ** 32 - 1)           # n * K == 0: any first stream passes
        assert _call(trt, device, sc._h, None, 0, C.byref(p), None) == trt._lib.TRT_OK
        assert _call(trt, device, sc._h, None, 0, C.byref(p), cols.ctypes.data, cols.ctypes.data) == trt._lib.TRT_OK
    assert (cols == 7.0).all()
    got, dirs, st = sc.samples(np.zeros((0, 6), np.float32), 4, source="hemisphere", directions=True)
    assert got.shape == (0, 4, 3) and dirs.shape == (0, 4, 3) and st["samples"] == 0 and st["rays"] == 0
    # the fold
    q = trt._lib.RadianceParams()
    trt.lib.trt_radiance_params_default(C.byref(q))
    q.samples_per_ray = K
    fold = trt.lib.trt_fold_samples_device if device else trt.lib.trt_fold_samples
    extra = (None,) if device else ()
    assert fold(None, 0, C.byref(q), None, None, *extra) == trt._lib.TRT_OK
    assert fold(cols.ctypes.data, 0, C.byref(q), cols.ctypes.data, None, *extra) == trt._lib.TRT_OK
    assert (cols == 7.0).all()
    r, m = trt.fold_samples(np.zeros((0, K, 3), np.float32), K, moment2=True)
    assert r.shape == (0, 3) and m.shape == (0, 3)


@pytest.mark.parametrize("device", (False, True))
def test_misuse_of_the_fold_is_invalid_arg_before_any_device_work(trt, device):
    cols = np.full((N, K, 3), 7.0, np.float32)
    sums = np.full((2, N, 3), 7.0, np.float32)
    cp, rp, mp = cols.ctypes.data, sums[0].ctypes.data, sums[1].ctypes.data
    fold = trt.lib.trt_fold_samples_device if device else trt.lib.trt_fold_samples
    extra = (None,) if device else ()

    def params(**over):
        q = trt._lib.RadianceParams()
        trt.lib.trt_radiance_params_default(C.byref(q))
        q.samples_per_ray = K
        for k, v in over.items():
            setattr(q, k, v)
        return q

    def call(c, n, q, r, m):
        return fold(c, n, C.byref(q) if q is not None else None, r, m, *extra)

    _invalid(trt, call(cp, N, None, rp, mp))
    _invalid(trt, call(cp, N, params(samples_per_ray=0), rp, mp))
    _invalid(trt, call(cp, N, params(sample_begin=3, sample_end=2), rp, mp))
    _invalid(trt, call(cp, N, params(sample_end=K + 1), rp, mp))
    _invalid(trt, call(cp, N, params(sample_begin=K + 1), rp, mp))
    _invalid(trt, call(None, N, params(), rp, mp))
    _invalid(trt, call(cp, N, params(), None, mp))
    for k in range(6):
        q = params()
        q.reserved[k] = 1
        _invalid(trt, call(cp, N, q, rp, mp), "reserved")
    _invalid(trt, call(None, 0, None, None, None))
    _invalid(trt, call(None, 0, params(samples_per_ray=0), None, None))
    if device:
        # the sums must not overlap the 12 n K bytes of the colours: checked from the sizes, before any device work
        _invalid(trt, call(cp, N, params(), cp, None), "overlap")
        _invalid(trt, call(cp, N, params(), cp + 12 * N * K - 4, None), "overlap")
        _invalid(trt, call(cp, N, params(), rp, cp + 12), "overlap")
        _invalid(trt, call(cp + 12 * N - 4, N, params(), cp, None), "overlap")
    want = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE
    if want != trt._lib.TRT_OK:
        # every field of the path but K, the range and accumulate is not read
        assert call(cp, N, params(max_bounces=0, seed=0, first_stream=2 ** 32 - 1, sample_begin=1, accumulate=1), rp, None) == want
        assert "no HIP device" in trt.lib.trt_last_error().decode()
        if device:
            assert call(cp, N, params(), cp + 12 * N * K, cp - 12 * N) == want                     # touching is not overlapping
    assert (cols == 7.0).all() and (sums == 7.0).all()


def test_well_formed_calls_need_a_device(trt):
    """Without a GPU: TRT_ERR_NO_DEVICE - there is no CPU path, for the fold neither.  With one: success."""
    sc = _scene(trt)
    items = np.zeros((N, 6), np.float32)
    items[:, 0:3] = (50.0, 50.0, 50.0)
    items[:, 4] = 1.0
    cols = np.full((N, K, 3), 7.0, np.float32)
    want = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE
    p = _params(trt)
    assert trt.lib.trt_samples(sc._h, items.ctypes.data, N, C.byref(p), cols.ctypes.data, None, None) == want
    if want != trt._lib.TRT_OK:
        assert "no HIP device" in trt.lib.trt_last_error().decode()
        assert (cols == 7.0).all()
        assert trt.lib.trt_samples_device(sc._h, items.ctypes.data, N, C.byref(p), cols.ctypes.data, None, None, None) == want
        with pytest.raises(trt.TinyRTError) as e:
            sc.samples(items, K)
        assert e.value.code == trt._lib.ERR_NO_DEVICE
        with pytest.raises(trt.TinyRTError) as e:
            trt.fold_samples(cols, K)
        assert e.value.code == trt._lib.ERR_NO_DEVICE
    else:
        assert not (cols == 7.0).any()


def test_python_wrappers_check_their_arguments(trt):
    sc = _scene(trt)
    items = np.zeros((2, 6), np.float32)
    with pytest.raises(ValueError):
        sc.samples(np.zeros((2, 5), np.float32), 4)
    with pytest.raises(ValueError):
        sc.samples(items, 4, source="lobe")
    with pytest.raises(AssertionError):
        sc.samples(items, 4, colors=np.zeros((2, 4, 3), np.float64))
    with pytest.raises(AssertionError):
        sc.samples(items, 4, directions=np.zeros((2, 3, 3), np.float32))
    with pytest.raises(ValueError):
        sc.samples(items, 4, sample_end=0)
    with pytest.raises(TypeError):
        sc.samples(items, 4, accumulate=True)                               # a record is written, never added to: the keyword is not offered
    for kw in (dict(samples_per_item=0), dict(samples_per_item=4, source="cone", spread=-1.0)):
        with pytest.raises(trt.TinyRTError) as e:
            sc.samples(items, **kw)
        assert e.value.code == trt._lib.ERR_INVALID_ARG
    p = trt.Scene._samples_params(7, "hemisphere", max_bounces=3, seed=9, first_stream=11)
    assert (p.path.samples_per_ray, p.path.max_bounces, p.path.seed, p.path.first_stream, p.source) == (7, 3, 9, 11, 4)
    d = trt.Scene._samples_params(3)
    assert (d.source, d.spread, d.path.max_bounces, d.path.seed, d.path.accumulate) == (1, 0.0, 50, 1, 0)
    with pytest.raises(ValueError):
        trt.fold_samples(np.zeros((2, 4, 3), np.float32), 5)
    with pytest.raises(ValueError):
        trt.fold_samples(np.zeros((2, 4), np.float32), 4)
    with pytest.raises(ValueError):
        trt.sh.project(np.zeros((2, 4, 3), np.float32), np.zeros((2, 3, 3), np.float32))


def test_the_plan_symbol_checks_its_arguments(trt):
    sc = _scene(trt)
    out = trt._lib.QueryPlan()
    assert trt.lib.trt_samples_launch_plan(None, 1, 1, 256, C.byref(out)) == trt._lib.ERR_INVALID_ARG
    assert trt.lib.trt_samples_launch_plan(sc._h, 1, 1, 256, None) == trt._lib.ERR_INVALID_ARG
    assert trt.lib.trt_samples_launch_plan(sc._h, 2 ** 16, 2 ** 16, 256, C.byref(out)) == trt._lib.ERR_INVALID_ARG      # n * R = 2^32
    assert "2^32 - 1" in trt.lib.trt_last_error().decode()
    assert trt.lib.trt_samples_launch_plan(sc._h, 2 ** 16 + 1, 2 ** 16 - 1, 256, C.byref(out)) == trt._lib.TRT_OK        # 2^32 - 1
    want = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE      # compute_units = 0 asks the current device
    assert trt.lib.trt_samples_launch_plan(sc._h, 1, 1, 0, C.byref(out)) == want
    assert trt.lib.trt_samples_launch_plan(sc._h, 1, 1, 256, C.byref(out)) == trt._lib.TRT_OK and out.compute_units == 256
    assert sc.samples_plan(1, 2, 304)["compute_units"] == 304
    assert sc.samples_plan(7, None, 304) == sc.samples_plan(7, 1, 304)
    # nothing to launch
    assert sc.samples_plan(0, 5, 256)["workgroups"] == 0 and sc.samples_plan(5, 0, 256)["workgroups"] == 0


# (items, range length): n * R walks test_radiance_abi.py's batch sizes, each once as many items of one sample and once split n x R
WORK = ((1, 1), (64, 1), (1, 64), (257, 1), (324, 1), (36, 9), (100003, 1), (1, 100003), (324, 5), (1, 700), (64, 16384), (2 ** 32 - 1, 1),
        (1, 2 ** 32 - 1), (65537, 65535), (2 ** 20, 16))
FROM_THE_BOUND = ("kernel_waves_per_simd", "workgroups_per_cu", "wave_slots")
FROM_THE_SLOTS = ("rays_per_wave", "waves", "workgroups")
# samples.hip kSamplesKernels (profiles/samples_resource_usage.txt): (scene mode, walk, threads) -> launch bound; none is below its sibling
# in radiance.hip kGatherKernels
BOUNDS = {(1, 2, 256): 7, (1, 1, 256): 8, (1, 1, 768): 8, (1, 5, 512): 8, (0, 3, 256): 7, (0, 5, 256): 8}
GATHER_BOUNDS = {(1, 2, 256): 6, (1, 1, 256): 7, (1, 1, 768): 7, (1, 5, 512): 7, (0, 3, 256): 7, (0, 5, 256): 7}


def test_the_samples_plan_is_the_gather_plan_of_n_times_r_but_for_the_kernel_bound(trt):
    """Every (scene, options) of test_gpu_queries.PLAN_CASES at 256 compute units: the plan's invariants with n * R in the place of n, the
    listed kernel shape, every field equal to trt_gather_launch_plan(n * R)'s but the bound and what the launch rule derives from it;
    waves x rays_per_wave covers n * R; and the runs lengthen exactly where n * R passes 256 x wave_slots."""
    import test_gpu_queries as G
    import walk_ray_cases as W
    cus = 256
    r = trt.Renderer(4, 1, 8, False, (0.1, 0.1, 0.1))
    shapes, worlds, bounds = set(), {}, {}
    for name, options, shape in G.PLAN_CASES:
        if name not in worlds:
            worlds[name] = trt.world_from_description(W.scene(trt, name))
        world, cam = worlds[name]
        host_options = {k: v for k, v in options.items() if k != "on_device"}
        sc = world.get_bvh(**host_options) if host_options else world.get_bvh()
        streamed = r.launch_plan(cam, sc)
        for n, rl in WORK:
            work = n * rl
            q, qg = sc.samples_plan(n, rl, cus), sc.gather_plan(work, cus)
            tag = (name, options, n, rl, q, qg)
            _check_query_plan(q, work, cus, streamed, tag)
            assert q == sc.samples_plan(rl, n, cus), tag                    # a function of n * R alone
            assert G.plan_shape(q) == shape, tag
            assert set(q) == set(qg)
            assert 1 <= q["kernel_waves_per_simd"] <= 8
            same_bound = q["kernel_waves_per_simd"] == qg["kernel_waves_per_simd"]
            lengthened = q["rays_per_wave"] > 256 or qg["rays_per_wave"] > 256
            for k in q:
                if same_bound or not (k in FROM_THE_BOUND or (lengthened and k in FROM_THE_SLOTS)):
                    assert q[k] == qg[k], (k, tag)
            per_wave, waves = q["rays_per_wave"], q["waves"]
            assert waves * per_wave >= work and (waves - 1) * per_wave < work, tag
            assert q["workgroups"] == -(-waves // (q["threads_per_workgroup"] // 64)), tag
            assert (per_wave > 256) == (work > 256 * q["wave_slots"]), tag
            shapes.add(shape[:3])
            bounds[shape[:3]] = q["kernel_waves_per_simd"]
        # the threshold itself, as items and as samples of one item
        edge = 256 * sc.samples_plan(1, 1, cus)["wave_slots"]
        for n, rl in ((edge, 1), (1, edge), (edge // 256, 256)):
            assert sc.samples_plan(n, rl, cus)["rays_per_wave"] == 256, (name, options, n, rl)
        for n, rl in ((edge + 1, 1), (1, edge + 1), (edge // 256 + 1, 256)):
            q = sc.samples_plan(n, rl, cus)
            assert q["rays_per_wave"] > 256 and q["rays_per_wave"] % 64 == 0 and q["waves"] <= q["wave_slots"], (name, options, n, rl, q)
    assert len(shapes) == 6, sorted(shapes)                                 # every entry of the table
    assert bounds == BOUNDS, bounds
    assert all(BOUNDS[k] >= GATHER_BOUNDS[k] for k in BOUNDS)
