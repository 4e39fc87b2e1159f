"""The radiance query entry points (tinyrt.h trt_radiance, trt_radiance_device, trt_radiance_launch_plan, trt_radiance_params_default) at
the C boundary, without a GPU: the symbols are declared, exported and bound, misuse comes back as TRT_ERR_INVALID_ARG with a message before
any device work, an empty batch succeeds without a device, and the launch arithmetic holds its invariants for every scene and option the
GPU tests use.  What the buffers hold is checked on the GPU (tests/test_gpu_radiance.py, tests/test_gpu_radiance_long.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_query_abi import QUERY_KERNEL_SHAPES, WALK_LDS_TREE, WALK_LOCK_STEP, _check_query_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"trt_radiance_params_default": (None, 1), "trt_radiance": (C.c_int, 7), "trt_radiance_device": (C.c_int, 8),
         "trt_radiance_launch_plan": (C.c_int, 4)}
# kRadianceKernels (radiance.hip): one instantiation per walk of the sparse render's table, which is the queries'
RADIANCE_KERNEL_SHAPES = QUERY_KERNEL_SHAPES


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
    assert "trt_radiance_params," in later
    assert trt.lib.trt_abi_version() == 4                                  # new symbols only: the ABI version stays
    assert C.sizeof(trt._lib.RadianceParams) == 64
    # the plan struct is the queries' (no new struct)
    assert trt._lib.SIGNATURES["trt_radiance_launch_plan"][1][3] is trt._lib.SIGNATURES["trt_query_launch_plan"][1][3]
    assert C.sizeof(trt._lib.QueryPlan) == 16 * 4 + 2 * 8
    for name in ("radiance", "radiance_device", "radiance_plan"):
        assert callable(getattr(trt.Scene, name))


def test_the_default_parameters(trt):
    p = trt._lib.RadianceParams()
    C.memset(C.byref(p), 0xCD, C.sizeof(p))
    trt.lib.trt_radiance_params_default(C.byref(p))
    assert (p.samples_per_ray, p.max_bounces, p.seed) == (1, 50, 1)
    assert p.background.tolist() == [0.0, 0.0, 0.0]
    assert (p.sample_begin, p.sample_end, p.accumulate, p.first_stream) == (0, 0, 0, 0) and list(p.reserved) == [0] * 6
    trt.lib.trt_radiance_params_default(None)                              # tolerated


def _scene(trt):
    return trt.world_from_description(trt.scenes.cornell(8, 8))[0].get_bvh()


def _params(trt, **over):
    p = trt._lib.RadianceParams()
    trt.lib.trt_radiance_params_default(C.byref(p))
    p.samples_per_ray, p.max_bounces, p.seed = 4, 4, 5
    for k, v in over.items():
        setattr(p, k, v)
    return p


def _invalid(trt, rc):
    assert rc == trt._lib.ERR_INVALID_ARG
    assert trt.lib.trt_last_error().decode() != ""


N = 3


def _call(trt, device, s, rays, n, p, rad, m2):
    if device:
        return trt.lib.trt_radiance_device(s, rays, n, p, rad, m2, None, None)
    return trt.lib.trt_radiance(s, rays, n, p, rad, m2, None)


@pytest.mark.parametrize("device", (False, True))
def test_misuse_is_invalid_arg_before_any_device_work(trt, device):
    """(Host pointers are handed to the device form too: every one of these calls must return before anything is dereferenced.)"""
    sc = _scene(trt)
    rays = np.zeros((N, 6), np.float32)
    rays[:, 5] = 1.0
    rad = np.full((N, 3), 7.0, np.float32)
    m2 = np.full((N, 3), 7.0, np.float32)
    rp, sp, mp = rays.ctypes.data, rad.ctypes.data, m2.ctypes.data
    p = _params(trt)

    def call(s, r, n, q, a, m):
        return _call(trt, device, s, r, n, C.byref(q) if q is not None else None, a, m)

    _invalid(trt, call(None, rp, N, p, sp, mp))
    _invalid(trt, call(sc._h, rp, N, None, sp, mp))
    _invalid(trt, call(sc._h, None, N, p, sp, mp))
    _invalid(trt, call(sc._h, rp, N, p, None, mp))
    _invalid(trt, call(sc._h, rp, N, _params(trt, samples_per_ray=0), sp, mp))
    _invalid(trt, call(sc._h, rp, N, _params(trt, sample_begin=3, sample_end=2), sp, mp))
    _invalid(trt, call(sc._h, rp, N, _params(trt, sample_end=5), sp, mp))                          # K + 1
    _invalid(trt, call(sc._h, rp, N, _params(trt, sample_begin=5), sp, mp))                        # past K after the end == 0 rule
    for k in range(6):
        q = _params(trt)
        q.reserved[k] = 1
        _invalid(trt, call(sc._h, rp, N, q, sp, mp))
        assert "reserved" in trt.lib.trt_last_error().decode()
    # the RNG stream index must not wrap: first_stream + n * K <= 2^32, computed in 64 bits
    want_ok = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE
    edge = 2 ** 32 - N * 4
    if not device or want_ok != trt._lib.TRT_OK:                            # (the device form is given host pointers: never let it launch)
        assert call(sc._h, rp, N, _params(trt, first_stream=edge), sp, mp) == want_ok
        rad[:] = 7.0
        m2[:] = 7.0
    _invalid(trt, call(sc._h, rp, N, _params(trt, first_stream=edge + 1), sp, mp))
    assert "2^32" in trt.lib.trt_last_error().decode()
    _invalid(trt, call(sc._h, rp, 2 ** 32 - 1, _params(trt, samples_per_ray=2 ** 32 - 1, first_stream=2 ** 32 - 1), sp, mp))       # n * K needs 64 bits
    _invalid(trt, call(sc._h, rp, 2 ** 31, _params(trt, samples_per_ray=2, first_stream=1), sp, mp))
    # ... and an empty batch is checked too
    _invalid(trt, call(None, None, 0, p, None, None))
    _invalid(trt, call(sc._h, None, 0, _params(trt, samples_per_ray=0), None, None))
    assert (rad == 7.0).all() and (m2 == 7.0).all()


@pytest.mark.parametrize("device", (False, True))
def test_an_empty_batch_succeeds_without_a_device_and_touches_nothing(trt, device):
    sc = _scene(trt)
    rad = np.full((N, 3), 7.0, np.float32)
    p = _params(trt, first_stream=2 ** 32 - 1)                              # n * K == 0: any first stream passes
    assert _call(trt, device, sc._h, None, 0, C.byref(p), None, None) == trt._lib.TRT_OK
    assert _call(trt, device, sc._h, None, 0, C.byref(p), rad.ctypes.data, rad.ctypes.data) == trt._lib.TRT_OK
    assert (rad == 7.0).all()
    got, m2, st = sc.radiance(np.zeros((0, 6), np.float32), 4, moment2=True)
    assert got.shape == (0, 3) and m2.shape == (0, 3) and st["samples"] == 0 and st["rays"] == 0


def test_well_formed_calls_need_a_device(trt):
    """Without a GPU: TRT_ERR_NO_DEVICE - there is no CPU path.  With one: success."""
    sc = _scene(trt)
    rays = np.zeros((N, 6), np.float32)
    rays[:, 5] = 1.0
    rad = np.full((N, 3), 7.0, np.float32)
    want = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE
    p = _params(trt)
    assert trt.lib.trt_radiance(sc._h, rays.ctypes.data, N, C.byref(p), rad.ctypes.data, None, None) == want
    if want != trt._lib.TRT_OK:
        assert "no HIP device" in trt.lib.trt_last_error().decode()
        assert (rad == 7.0).all()
        assert trt.lib.trt_radiance_device(sc._h, rays.ctypes.data, N, C.byref(p), rad.ctypes.data, None, None, None) == want
        with pytest.raises(trt.TinyRTError) as e:
            sc.radiance(rays, 4)
        assert e.value.code == trt._lib.ERR_NO_DEVICE
    else:
        assert not (rad == 7.0).any()


def test_python_wrappers_check_their_arguments(trt):
    sc = _scene(trt)
    with pytest.raises(ValueError):
        sc.radiance(np.zeros((2, 5), np.float32), 4)
    with pytest.raises(AssertionError):
        sc.radiance(np.zeros((2, 6), np.float32), 4, radiance=np.zeros((2, 3), np.float64))
    with pytest.raises(AssertionError):
        sc.radiance(np.zeros((2, 6), np.float32), 4, moment2=np.zeros((3, 3), np.float32))
    with pytest.raises(ValueError):
        sc.radiance(np.zeros((2, 6), np.float32), 4, sample_end=0)
    with pytest.raises(trt.TinyRTError) as e:
        sc.radiance(np.zeros((2, 6), np.float32), 0)
    assert e.value.code == trt._lib.ERR_INVALID_ARG


def test_the_plan_symbol_checks_its_arguments(trt):
    sc = _scene(trt)
    out = trt._lib.QueryPlan()
    assert trt.lib.trt_radiance_launch_plan(None, 1, 256, C.byref(out)) == trt._lib.ERR_INVALID_ARG
    assert trt.lib.trt_radiance_launch_plan(sc._h, 1, 256, None) == trt._lib.ERR_INVALID_ARG
    want = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE      # compute_units = 0 asks the current device
    assert trt.lib.trt_radiance_launch_plan(sc._h, 1, 0, C.byref(out)) == want
    assert trt.lib.trt_radiance_launch_plan(sc._h, 1, 256, C.byref(out)) == trt._lib.TRT_OK and out.compute_units == 256
    assert sc.radiance_plan(1, 304)["compute_units"] == 304


RAY_COUNTS = (1, 64, 257, 324, 100003, 2 ** 32 - 1)


def test_radiance_launch_plan_invariants_on_every_scene_and_option_of_the_gpu_tests(trt):
    """Every (scene, options) of test_gpu_queries.PLAN_CASES - the cases tests/test_gpu_radiance.py runs - at 256 compute units and every
    batch size of RAY_COUNTS: the invariants tests/test_query_abi.py checks for the queries, and the listed kernel shape; the cases reach
    every entry of kRadianceKernels and every route to the fallback."""
    import test_gpu_queries as G
    import walk_ray_cases as W
    cus = 256
    r = trt.Renderer(4, 1, 8, False, (0.1, 0.1, 0.1))
    shapes, routes, worlds, lengthened = set(), set(), {}, 0
    for name, options, shape in G.PLAN_CASES:
        if name not in worlds:
            worlds[name] = trt.world_from_description(W.scene(trt, name))
        world, cam = worlds[name]
        host_options = {k: v for k, v in options.items() if k != "on_device"}       # (both compilers give the same bytes: tests/test_gpu_scene_build.py)
        sc = world.get_bvh(**host_options) if host_options else world.get_bvh()
        streamed = r.launch_plan(cam, sc)
        for n in RAY_COUNTS:
            q = sc.radiance_plan(n, cus)
            tag = (name, options, n, q)
            _check_query_plan(q, n, cus, streamed, tag)
            assert G.plan_shape(q) == shape, tag
            per_wave, waves = q["rays_per_wave"], q["waves"]
            assert (waves - 1) * per_wave < n <= waves * per_wave, tag
            assert q["workgroups"] == -(-waves // (q["threads_per_workgroup"] // 64)), tag
            lengthened += per_wave > 256
            shapes.add(shape[:3])
            if q["fallback"]:
                routes.add((q["scene_mode"], q["streamed_walk"]))
        # the plan of the sparse render for as many entries is the same kernel shape and LDS layout; the launch bound is this kernel's own
        qp, qr = sc.pixels_plan(324, cus), sc.radiance_plan(324, cus)
        for k in ("scene_mode", "walk", "threads_per_workgroup", "leaf_slots", "stragglers", "lds_bytes", "fallback", "rays_per_wave"):
            assert qp[k] == qr[k], (name, options, k)
        assert 1 <= qr["kernel_waves_per_simd"] <= 8
    assert shapes == RADIANCE_KERNEL_SHAPES, sorted(shapes)
    assert {(1, WALK_LDS_TREE), (1, WALK_LOCK_STEP), (0, WALK_LOCK_STEP)} <= routes, sorted(routes)
    assert lengthened > 0                                                    # 2^32 - 1 rays lengthen the runs of every shape
