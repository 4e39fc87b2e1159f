"""The ambient query entry points (tinyrt.h trt_ambient, trt_ambient_device, trt_ambient_launch_plan, trt_ambient_params_default) at the C
boundary, without a GPU: the symbols are declared, exported and bound, misuse comes back as TRT_ERR_INVALID_ARG with a message before any
device work, an empty batch succeeds without a device, and the launch plan is the gather queries' but for the kernel's launch bound.  What
the buffers hold is checked on the GPU (tests/test_gpu_ambient.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_query_abi import _check_query_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"trt_ambient_params_default": (None, 1), "trt_ambient": (C.c_int, 7), "trt_ambient_device": (C.c_int, 8),
         "trt_ambient_launch_plan": (C.c_int, 4)}


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
        assert name in later, name + " is not listed under 'Later under 4'"
    assert "trt_ambient_params," in later
    assert trt.lib.trt_abi_version() == 4                                  # new symbols only: the ABI version stays
    A = trt._lib.AmbientParams
    assert C.sizeof(A) == 128
    assert (A.gather.offset, A.max_distance.offset, A.reserved.offset) == (0, 96, 100) and A.reserved.size == 28
    # trt_gather_params and trt_radiance_params did not change
    G = trt._lib.GatherParams
    assert C.sizeof(G) == 96 and C.sizeof(trt._lib.RadianceParams) == 64
    assert (G.path.offset, G.lobe.offset, G.spread.offset, G.reserved.offset) == (0, 64, 68, 72)
    R = trt._lib.RadianceParams
    assert (R.samples_per_ray.offset, R.max_bounces.offset, R.background.offset, R.seed.offset, R.sample_begin.offset, R.sample_end.offset,
            R.accumulate.offset, R.first_stream.offset, R.reserved.offset) == (0, 4, 8, 20, 24, 28, 32, 36, 40)
    # the signatures are the gather queries' with the other parameter struct; the plan struct is the queries'
    for name in ("trt_ambient", "trt_ambient_device"):
        mine, theirs = trt._lib.SIGNATURES[name][1], trt._lib.SIGNATURES[name.replace("ambient", "gather")][1]
        assert mine[3] is C.POINTER(A) and mine[:3] + mine[4:] == theirs[:3] + theirs[4:], name
    assert trt._lib.SIGNATURES["trt_ambient_launch_plan"][1] == trt._lib.SIGNATURES["trt_gather_launch_plan"][1]
    for name in ("ambient", "ambient_device", "ambient_plan"):
        assert callable(getattr(trt.Scene, name))
    # the struct in the header, field for field
    m = re.search(r"typedef struct \{([^}]*)\}\s*trt_ambient_params\s*;", header)
    assert m and re.findall(r"(\w+)\s+(\w+)(\[\d+\])?\s*;", m.group(1)) == [("trt_gather_params", "gather", ""), ("float", "max_distance", ""),
                                                                           ("uint32_t", "reserved", "[7]")]


def test_the_default_parameters(trt):
    p = trt._lib.AmbientParams()
    C.memset(C.byref(p), 0xCD, C.sizeof(p))
    trt.lib.trt_ambient_params_default(C.byref(p))
    want = trt._lib.GatherParams()
    trt.lib.trt_gather_params_default(C.byref(want))
    assert bytes(p.gather) == bytes(want)
    assert p.gather.lobe == trt._lib.LOBE_COSINE and p.gather.path.samples_per_ray == 1 and p.gather.path.seed == 1
    assert p.max_distance == float("inf") and list(p.reserved) == [0] * 7
    trt.lib.trt_ambient_params_default(None)                               # tolerated


def _scene(trt):
    return trt.world_from_description(trt.scenes.cornell(8, 8))[0].get_bvh()


PATH_FIELDS = ("samples_per_ray", "max_bounces", "seed", "sample_begin", "sample_end", "accumulate", "first_stream")
GATHER_FIELDS = ("lobe", "spread")


def _params(trt, **over):
    """K = 4, seed 5, cosine, +inf; a keyword that names a field of gather or of its path sets it there."""
    p = trt._lib.AmbientParams()
    trt.lib.trt_ambient_params_default(C.byref(p))
    p.gather.path.samples_per_ray, p.gather.path.seed = 4, 5
    for k, v in over.items():
        setattr(p.gather.path if k in PATH_FIELDS else p.gather if k in GATHER_FIELDS else p, k, v)
    return p


def _invalid(trt, rc):
    assert rc == trt._lib.ERR_INVALID_ARG
    assert trt.lib.trt_last_error().decode() != ""


N = 3


def _call(trt, device, s, items, n, p, vis, bent):
    if device:
        return trt.lib.trt_ambient_device(s, items, n, p, vis, bent, None, None)
    return trt.lib.trt_ambient(s, items, n, p, vis, bent, None)


@pytest.mark.parametrize("device", (False, True))
def test_misuse_is_invalid_arg_before_any_device_work(trt, device):
    """(Host pointers are handed to the device form too: every one of these calls must return before anything is dereferenced.)"""
    sc = _scene(trt)
    items = np.zeros((N, 6), np.float32)
    items[:, 4] = 1.0
    vis = np.full(N, 7.0, np.float32)
    bent = np.full((N, 3), 7.0, np.float32)
    ip, vp, bp = items.ctypes.data, vis.ctypes.data, bent.ctypes.data
    p = _params(trt)
    CONE = trt._lib.LOBE_CONE

    def call(s, r, n, q, a, b):
        return _call(trt, device, s, r, n, C.byref(q) if q is not None else None, a, b)

    _invalid(trt, call(None, ip, N, p, vp, bp))
    _invalid(trt, call(sc._h, ip, N, None, vp, bp))
    _invalid(trt, call(sc._h, None, N, p, vp, bp))
    _invalid(trt, call(sc._h, ip, N, p, None, bp))
    # every error trt_gather reports for p->gather
    _invalid(trt, call(sc._h, ip, N, _params(trt, samples_per_ray=0), vp, bp))
    _invalid(trt, call(sc._h, ip, N, _params(trt, sample_begin=3, sample_end=2), vp, bp))
    _invalid(trt, call(sc._h, ip, N, _params(trt, sample_end=5), vp, bp))                          # K + 1
    _invalid(trt, call(sc._h, ip, N, _params(trt, sample_begin=5), vp, bp))                        # past K after the end == 0 rule
    for k in range(6):
        q = _params(trt)
        q.gather.path.reserved[k] = 1
        _invalid(trt, call(sc._h, ip, N, q, vp, bp))
        assert "reserved" in trt.lib.trt_last_error().decode()
        q = _params(trt)
        q.gather.reserved[k] = 1
        _invalid(trt, call(sc._h, ip, N, q, vp, bp))
        assert "reserved" in trt.lib.trt_last_error().decode()
    for lobe in (0, 3, 2 ** 32 - 1):
        _invalid(trt, call(sc._h, ip, N, _params(trt, lobe=lobe), vp, bp))
        assert "lobe" in trt.lib.trt_last_error().decode()
    for spread in (float("nan"), float("inf"), -float("inf"), -1.0):
        _invalid(trt, call(sc._h, ip, N, _params(trt, lobe=CONE, spread=spread), vp, bp))
        assert "spread" in trt.lib.trt_last_error().decode()
    # this struct's own
    _invalid(trt, call(sc._h, ip, N, _params(trt, max_distance=float("nan")), vp, bp))
    assert "max_distance" in trt.lib.trt_last_error().decode()
    for k in range(7):
        q = _params(trt)
        q.reserved[k] = 1
        _invalid(trt, call(sc._h, ip, N, q, vp, bp))
        assert "reserved" in trt.lib.trt_last_error().decode()
    # the RNG stream index must not wrap: first_stream + n * K <= 2^32, computed in 64 bits
    want_ok = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE
    edge = 2 ** 32 - N * 4
    if not device or want_ok != trt._lib.TRT_OK:                            # (the device form is given host pointers: never let it launch)
        assert call(sc._h, ip, N, _params(trt, first_stream=edge), vp, bp) == want_ok
        # there is no path: max_bounces == 0 and a NaN background are accepted, as is any distance that is a number
        q = _params(trt, max_bounces=0)
        q.gather.path.background.x = float("nan")
        assert call(sc._h, ip, N, q, vp, bp) == want_ok
        for dist in (float("inf"), -float("inf"), 0.0, -1.0, 0.001, 1e30):
            assert call(sc._h, ip, N, _params(trt, max_distance=dist), vp, bp) == want_ok
        assert call(sc._h, ip, N, _params(trt, spread=float("nan")), vp, bp) == want_ok            # the cosine lobe ignores the spread
        assert call(sc._h, ip, N, _params(trt, lobe=CONE, spread=0.0), vp, bp) == want_ok
        assert call(sc._h, ip, N, p, vp, None) == want_ok                                          # bent is optional
        vis[:] = 7.0
        bent[:] = 7.0
    _invalid(trt, call(sc._h, ip, N, _params(trt, first_stream=edge + 1), vp, bp))
    assert "2^32" in trt.lib.trt_last_error().decode()
    _invalid(trt, call(sc._h, ip, 2 ** 32 - 1, _params(trt, samples_per_ray=2 ** 32 - 1, first_stream=2 ** 32 - 1), vp, bp))       # n * K needs 64 bits
    _invalid(trt, call(sc._h, ip, 2 ** 31, _params(trt, samples_per_ray=2, first_stream=1), vp, bp))
    # ... and an empty batch is checked too
    _invalid(trt, call(None, None, 0, p, None, None))
    _invalid(trt, call(sc._h, None, 0, None, None, None))
    _invalid(trt, call(sc._h, None, 0, _params(trt, samples_per_ray=0), None, None))
    _invalid(trt, call(sc._h, None, 0, _params(trt, lobe=0), None, None))
    _invalid(trt, call(sc._h, None, 0, _params(trt, max_distance=float("nan")), None, None))
    q = _params(trt)
    q.reserved[6] = 1
    _invalid(trt, call(sc._h, None, 0, q, None, None))
    assert (vis == 7.0).all() and (bent == 7.0).all()


@pytest.mark.parametrize("device", (False, True))
def test_an_empty_batch_succeeds_without_a_device_and_touches_nothing(trt, device):
    sc = _scene(trt)
    vis = np.full(N, 7.0, np.float32)
    for lobe in (trt._lib.LOBE_COSINE, trt._lib.LOBE_CONE):
        p = _params(trt, lobe=lobe, spread=0.25, first_stream=2 ** 32 - 1, max_distance=3.0)      # n * K == 0: any first stream passes
        assert _call(trt, device, sc._h, None, 0, C.byref(p), None, None) == trt._lib.TRT_OK
        assert _call(trt, device, sc._h, None, 0, C.byref(p), vis.ctypes.data, vis.ctypes.data) == trt._lib.TRT_OK
    assert (vis == 7.0).all()
    got, bent, st = sc.ambient(np.zeros((0, 6), np.float32), 4, lobe="cone", spread=0.5, bent=True)
    assert got.shape == (0,) and bent.shape == (0, 3) and st["samples"] == 0 and st["rays"] == 0


def test_well_formed_calls_need_a_device(trt):
    """Without a GPU: TRT_ERR_NO_DEVICE - there is no CPU path.  With one: success."""
    sc = _scene(trt)
    items = np.zeros((N, 6), np.float32)
    items[:, 0:3] = (50.0, 0.0, 50.0)
    items[:, 4] = 1.0
    vis = np.full(N, 7.0, np.float32)
    want = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE
    p = _params(trt)
    assert trt.lib.trt_ambient(sc._h, items.ctypes.data, N, C.byref(p), vis.ctypes.data, None, None) == want
    if want != trt._lib.TRT_OK:
        assert "no HIP device" in trt.lib.trt_last_error().decode()
        assert (vis == 7.0).all()
        assert trt.lib.trt_ambient_device(sc._h, items.ctypes.data, N, C.byref(p), vis.ctypes.data, None, None, None) == want
        with pytest.raises(trt.TinyRTError) as e:
            sc.ambient(items, 4)
        assert e.value.code == trt._lib.ERR_NO_DEVICE
    else:
        assert not (vis == 7.0).any()


def test_python_wrappers_check_their_arguments(trt):
    sc = _scene(trt)
    with pytest.raises(ValueError):
        sc.ambient(np.zeros((2, 5), np.float32), 4)
    with pytest.raises(ValueError):
        sc.ambient(np.zeros((2, 6), np.float32), 4, lobe="glossy")
    with pytest.raises(AssertionError):
        sc.ambient(np.zeros((2, 6), np.float32), 4, visibility=np.zeros(2, np.float64))
    with pytest.raises(AssertionError):
        sc.ambient(np.zeros((2, 6), np.float32), 4, visibility=np.zeros((2, 1), np.float32))
    with pytest.raises(AssertionError):
        sc.ambient(np.zeros((2, 6), np.float32), 4, bent=np.zeros((3, 3), np.float32))
    for kw in (dict(samples_per_item=0), dict(samples_per_item=4, lobe="cone", spread=-0.5), dict(samples_per_item=4, max_distance=float("nan"))):
        with pytest.raises(trt.TinyRTError) as e:
            sc.ambient(np.zeros((2, 6), np.float32), **kw)
        assert e.value.code == trt._lib.ERR_INVALID_ARG
    p = trt.Scene._ambient_params(7, "cone", 0.25, max_distance=2.5, seed=9, first_stream=11, sample_begin=1, sample_end=5, accumulate=True)
    g = p.gather
    assert (g.path.samples_per_ray, g.path.seed, g.path.first_stream, g.lobe, g.spread, p.max_distance) == (7, 9, 11, 2, 0.25, 2.5)
    assert (g.path.sample_begin, g.path.sample_end, g.path.accumulate) == (1, 5, 1)
    d = trt.Scene._ambient_params(3)
    assert (d.gather.lobe, d.max_distance, d.gather.path.sample_end, d.gather.path.seed) == (1, float("inf"), 0, 1)


def test_the_plan_symbol_checks_its_arguments(trt):
    sc = _scene(trt)
    out = trt._lib.QueryPlan()
    assert trt.lib.trt_ambient_launch_plan(None, 1, 256, C.byref(out)) == trt._lib.ERR_INVALID_ARG
    assert trt.lib.trt_ambient_launch_plan(sc._h, 1, 256, None) == trt._lib.ERR_INVALID_ARG
    want = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE      # compute_units = 0 asks the current device
    assert trt.lib.trt_ambient_launch_plan(sc._h, 1, 0, C.byref(out)) == want
    assert trt.lib.trt_ambient_launch_plan(sc._h, 1, 256, C.byref(out)) == trt._lib.TRT_OK and out.compute_units == 256
    assert sc.ambient_plan(1, 304)["compute_units"] == 304


RAY_COUNTS = (1, 64, 257, 324, 100003, 2 ** 32 - 1)                          # test_radiance_abi.py's
# what plan_batch (stream_plan.h) derives from the kernel's launch bound: the resident workgroups and wave slots, and through them the runs
# of a batch too long for 256 items per wave
FROM_THE_BOUND = ("kernel_waves_per_simd", "workgroups_per_cu", "wave_slots")
FROM_THE_SLOTS = ("rays_per_wave", "waves", "workgroups")
# ambient.hip kAmbientKernels (profiles/ambient_resource_usage.txt): (scene mode, walk, threads) -> launch bound
BOUNDS = {(1, 2, 256): 8, (1, 1, 256): 8, (1, 1, 768): 8, (1, 5, 512): 7, (0, 3, 256): 8, (0, 5, 256): 7}


def test_the_ambient_plan_is_the_gather_plan_but_for_the_kernel_bound(trt):
    """Every (scene, options) of test_gpu_queries.PLAN_CASES at 256 compute units and every batch size test_radiance_abi.py walks: the
    plan's invariants, the listed kernel shape, and every field equal to trt_gather_launch_plan's but the bound and what the launch rule
    derives from it, and those obey the rule."""
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
        for n in RAY_COUNTS:
            q, qg = sc.ambient_plan(n, cus), sc.gather_plan(n, cus)
            tag = (name, options, n, q, qg)
            _check_query_plan(q, n, cus, streamed, tag)
            assert G.plan_shape(q) == shape, tag
            assert set(q) == set(qg)
            assert 1 <= q["kernel_waves_per_simd"] <= 8
            same_bound = q["kernel_waves_per_simd"] == qg["kernel_waves_per_simd"]
            lengthened = q["rays_per_wave"] > 256 or qg["rays_per_wave"] > 256
            for k in q:
                if same_bound or not (k in FROM_THE_BOUND or (lengthened and k in FROM_THE_SLOTS)):
                    assert q[k] == qg[k], (k, tag)
            per_wave, waves = q["rays_per_wave"], q["waves"]
            assert (waves - 1) * per_wave < n <= waves * per_wave, tag
            assert q["workgroups"] == -(-waves // (q["threads_per_workgroup"] // 64)), tag
            shapes.add(shape[:3])
            bounds[shape[:3]] = q["kernel_waves_per_simd"]
    assert len(shapes) == 6, sorted(shapes)                                 # every entry of kAmbientKernels
    assert bounds == BOUNDS, bounds
