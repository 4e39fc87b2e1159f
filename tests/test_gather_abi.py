"""The gather query entry points (tinyrt.h trt_gather, trt_gather_device, trt_gather_launch_plan, trt_gather_params_default) at the C
boundary, and bake.quad_texels, without a GPU: the symbols are declared, exported and bound, misuse comes back as TRT_ERR_INVALID_ARG with
a message before any device work, an empty batch succeeds without a device, and the launch plan is the radiance queries' but for the
kernel's launch bound.  What the buffers hold is checked on the GPU (tests/test_gpu_gather.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_query_abi import _check_query_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"trt_gather_params_default": (None, 1), "trt_gather": (C.c_int, 7), "trt_gather_device": (C.c_int, 8),
         "trt_gather_launch_plan": (C.c_int, 4)}


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
    assert "trt_gather_params," in later and "trt_lobe," in later
    assert re.search(r"enum\s+trt_lobe\s*\{\s*TRT_LOBE_COSINE\s*=\s*1\s*,\s*TRT_LOBE_CONE\s*=\s*2\s*\}", header)
    assert (trt._lib.LOBE_COSINE, trt._lib.LOBE_CONE) == (1, 2)
    assert trt.lib.trt_abi_version() == 4                                  # new symbols only: the ABI version stays
    G = trt._lib.GatherParams
    assert C.sizeof(G) == 96 and C.sizeof(trt._lib.RadianceParams) == 64   # trt_radiance_params itself did not change
    assert (G.path.offset, G.lobe.offset, G.spread.offset, G.reserved.offset) == (0, 64, 68, 72)
    # the signatures are the radiance queries' with the other parameter struct; the plan struct is the queries'
    for name in ("trt_gather", "trt_gather_device"):
        mine, theirs = trt._lib.SIGNATURES[name][1], trt._lib.SIGNATURES[name.replace("gather", "radiance")][1]
        assert mine[3] is C.POINTER(G) and mine[:3] + mine[4:] == theirs[:3] + theirs[4:], name
    assert trt._lib.SIGNATURES["trt_gather_launch_plan"][1] == trt._lib.SIGNATURES["trt_radiance_launch_plan"][1]
    for name in ("gather", "gather_device", "gather_plan"):
        assert callable(getattr(trt.Scene, name))


def test_the_default_parameters(trt):
    p = trt._lib.GatherParams()
    C.memset(C.byref(p), 0xCD, C.sizeof(p))
    trt.lib.trt_gather_params_default(C.byref(p))
    want = trt._lib.RadianceParams()
    trt.lib.trt_radiance_params_default(C.byref(want))
    assert bytes(p.path) == bytes(want)
    assert (p.path.samples_per_ray, p.path.max_bounces, p.path.seed) == (1, 50, 1) and list(p.path.reserved) == [0] * 6
    assert p.lobe == trt._lib.LOBE_COSINE and p.spread == 0.0 and list(p.reserved) == [0] * 6
    trt.lib.trt_gather_params_default(None)                                # tolerated


def _scene(trt):
    return trt.world_from_description(trt.scenes.cornell(8, 8))[0].get_bvh()


PATH_FIELDS = ("samples_per_ray", "max_bounces", "seed", "sample_begin", "sample_end", "accumulate", "first_stream")


def _params(trt, **over):
    """K = 4, depth 4, seed 5, cosine; a keyword that names a field of the path sets it there."""
    p = trt._lib.GatherParams()
    trt.lib.trt_gather_params_default(C.byref(p))
    p.path.samples_per_ray, p.path.max_bounces, p.path.seed = 4, 4, 5
    for k, v in over.items():
        setattr(p.path if k in PATH_FIELDS else p, k, v)
    return p


def _invalid(trt, rc):
    assert rc == trt._lib.ERR_INVALID_ARG
    assert trt.lib.trt_last_error().decode() != ""


N = 3


def _call(trt, device, s, items, n, p, rad, m2):
    if device:
        return trt.lib.trt_gather_device(s, items, n, p, rad, m2, None, None)
    return trt.lib.trt_gather(s, items, n, p, rad, m2, None)


@pytest.mark.parametrize("device", (False, True))
def test_misuse_is_invalid_arg_before_any_device_work(trt, device):
    """(Host pointers are handed to the device form too: every one of these calls must return before anything is dereferenced.)"""
    sc = _scene(trt)
    items = np.zeros((N, 6), np.float32)
    items[:, 4] = 1.0
    rad = np.full((N, 3), 7.0, np.float32)
    m2 = np.full((N, 3), 7.0, np.float32)
    ip, sp, mp = items.ctypes.data, rad.ctypes.data, m2.ctypes.data
    p = _params(trt)
    CONE = trt._lib.LOBE_CONE

    def call(s, r, n, q, a, m):
        return _call(trt, device, s, r, n, C.byref(q) if q is not None else None, a, m)

    # trt_radiance's own errors, applied to p->path
    _invalid(trt, call(None, ip, N, p, sp, mp))
    _invalid(trt, call(sc._h, ip, N, None, sp, mp))
    _invalid(trt, call(sc._h, None, N, p, sp, mp))
    _invalid(trt, call(sc._h, ip, N, p, None, mp))
    _invalid(trt, call(sc._h, ip, N, _params(trt, samples_per_ray=0), sp, mp))
    _invalid(trt, call(sc._h, ip, N, _params(trt, sample_begin=3, sample_end=2), sp, mp))
    _invalid(trt, call(sc._h, ip, N, _params(trt, sample_end=5), sp, mp))                          # K + 1
    _invalid(trt, call(sc._h, ip, N, _params(trt, sample_begin=5), sp, mp))                        # past K after the end == 0 rule
    for k in range(6):
        q = _params(trt)
        q.path.reserved[k] = 1
        _invalid(trt, call(sc._h, ip, N, q, sp, mp))
        assert "reserved" in trt.lib.trt_last_error().decode()
    # the gather's own
    for k in range(6):
        q = _params(trt)
        q.reserved[k] = 1
        _invalid(trt, call(sc._h, ip, N, q, sp, mp))
        assert "reserved" in trt.lib.trt_last_error().decode()
    for lobe in (0, 3, 2 ** 32 - 1):
        _invalid(trt, call(sc._h, ip, N, _params(trt, lobe=lobe), sp, mp))
        assert "lobe" in trt.lib.trt_last_error().decode()
    for spread in (float("nan"), float("inf"), -float("inf"), -1.0):
        _invalid(trt, call(sc._h, ip, N, _params(trt, lobe=CONE, spread=spread), sp, mp))
        assert "spread" in trt.lib.trt_last_error().decode()
    # the RNG stream index must not wrap: first_stream + n * K <= 2^32, computed in 64 bits
    want_ok = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE
    edge = 2 ** 32 - N * 4
    if not device or want_ok != trt._lib.TRT_OK:                            # (the device form is given host pointers: never let it launch)
        assert call(sc._h, ip, N, _params(trt, first_stream=edge), sp, mp) == want_ok
        # the cosine lobe ignores the spread, whatever it holds; the cone lobe takes 0 and any finite positive value
        assert call(sc._h, ip, N, _params(trt, spread=float("nan")), sp, mp) == want_ok
        assert call(sc._h, ip, N, _params(trt, spread=-1.0), sp, mp) == want_ok
        assert call(sc._h, ip, N, _params(trt, lobe=CONE, spread=0.0), sp, mp) == want_ok
        assert call(sc._h, ip, N, _params(trt, lobe=CONE, spread=1e30), sp, mp) == want_ok
        rad[:] = 7.0
        m2[:] = 7.0
    _invalid(trt, call(sc._h, ip, N, _params(trt, first_stream=edge + 1), sp, mp))
    assert "2^32" in trt.lib.trt_last_error().decode()
    _invalid(trt, call(sc._h, ip, 2 ** 32 - 1, _params(trt, samples_per_ray=2 ** 32 - 1, first_stream=2 ** 32 - 1), sp, mp))       # n * K needs 64 bits
    _invalid(trt, call(sc._h, ip, 2 ** 31, _params(trt, samples_per_ray=2, first_stream=1), sp, mp))
    # ... and an empty batch is checked too
    _invalid(trt, call(None, None, 0, p, None, None))
    _invalid(trt, call(sc._h, None, 0, None, None, None))
    _invalid(trt, call(sc._h, None, 0, _params(trt, samples_per_ray=0), None, None))
    _invalid(trt, call(sc._h, None, 0, _params(trt, lobe=0), None, None))
    _invalid(trt, call(sc._h, None, 0, _params(trt, lobe=CONE, spread=-1.0), None, None))
    assert (rad == 7.0).all() and (m2 == 7.0).all()


@pytest.mark.parametrize("device", (False, True))
def test_an_empty_batch_succeeds_without_a_device_and_touches_nothing(trt, device):
    sc = _scene(trt)
    rad = np.full((N, 3), 7.0, np.float32)
    for lobe in (trt._lib.LOBE_COSINE, trt._lib.LOBE_CONE):
        p = _params(trt, lobe=lobe, spread=0.25, first_stream=2 ** 32 - 1)  # n * K == 0: any first stream passes
        assert _call(trt, device, sc._h, None, 0, C.byref(p), None, None) == trt._lib.TRT_OK
        assert _call(trt, device, sc._h, None, 0, C.byref(p), rad.ctypes.data, rad.ctypes.data) == trt._lib.TRT_OK
    assert (rad == 7.0).all()
    got, m2, st = sc.gather(np.zeros((0, 6), np.float32), 4, lobe="cone", spread=0.5, moment2=True)
    assert got.shape == (0, 3) and m2.shape == (0, 3) and st["samples"] == 0 and st["rays"] == 0


def test_well_formed_calls_need_a_device(trt):
    """Without a GPU: TRT_ERR_NO_DEVICE - there is no CPU path.  With one: success."""
    sc = _scene(trt)
    items = np.zeros((N, 6), np.float32)
    items[:, 0:3] = (50.0, 0.0, 50.0)
    items[:, 4] = 1.0
    rad = np.full((N, 3), 7.0, np.float32)
    want = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE
    p = _params(trt)
    assert trt.lib.trt_gather(sc._h, items.ctypes.data, N, C.byref(p), rad.ctypes.data, None, None) == want
    if want != trt._lib.TRT_OK:
        assert "no HIP device" in trt.lib.trt_last_error().decode()
        assert (rad == 7.0).all()
        assert trt.lib.trt_gather_device(sc._h, items.ctypes.data, N, C.byref(p), rad.ctypes.data, None, None, None) == want
        with pytest.raises(trt.TinyRTError) as e:
            sc.gather(items, 4)
        assert e.value.code == trt._lib.ERR_NO_DEVICE
    else:
        assert not (rad == 7.0).any()


def test_python_wrappers_check_their_arguments(trt):
    sc = _scene(trt)
    with pytest.raises(ValueError):
        sc.gather(np.zeros((2, 5), np.float32), 4)
    with pytest.raises(ValueError):
        sc.gather(np.zeros((2, 6), np.float32), 4, lobe="glossy")
    with pytest.raises(AssertionError):
        sc.gather(np.zeros((2, 6), np.float32), 4, radiance=np.zeros((2, 3), np.float64))
    with pytest.raises(AssertionError):
        sc.gather(np.zeros((2, 6), np.float32), 4, moment2=np.zeros((3, 3), np.float32))
    with pytest.raises(ValueError):
        sc.gather(np.zeros((2, 6), np.float32), 4, sample_end=0)
    for kw in (dict(samples_per_item=0), dict(samples_per_item=4, lobe="cone", spread=-0.5)):
        with pytest.raises(trt.TinyRTError) as e:
            sc.gather(np.zeros((2, 6), np.float32), **kw)
        assert e.value.code == trt._lib.ERR_INVALID_ARG
    p = trt.Scene._gather_params(7, "cone", 0.25, max_bounces=3, seed=9, first_stream=11)
    assert (p.path.samples_per_ray, p.path.max_bounces, p.path.seed, p.path.first_stream, p.lobe, p.spread) == (7, 3, 9, 11, 2, 0.25)


def test_the_plan_symbol_checks_its_arguments(trt):
    sc = _scene(trt)
    out = trt._lib.QueryPlan()
    assert trt.lib.trt_gather_launch_plan(None, 1, 256, C.byref(out)) == trt._lib.ERR_INVALID_ARG
    assert trt.lib.trt_gather_launch_plan(sc._h, 1, 256, None) == trt._lib.ERR_INVALID_ARG
    want = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE      # compute_units = 0 asks the current device
    assert trt.lib.trt_gather_launch_plan(sc._h, 1, 0, C.byref(out)) == want
    assert trt.lib.trt_gather_launch_plan(sc._h, 1, 256, C.byref(out)) == trt._lib.TRT_OK and out.compute_units == 256
    assert sc.gather_plan(1, 304)["compute_units"] == 304


RAY_COUNTS = (1, 64, 257, 324, 100003, 2 ** 32 - 1)                          # test_radiance_abi.py's
# what plan_batch (stream_plan.h) derives from the kernel's launch bound: the resident workgroups and wave slots, and through them the runs
# of a batch too long for 256 items per wave
FROM_THE_BOUND = ("kernel_waves_per_simd", "workgroups_per_cu", "wave_slots")
FROM_THE_SLOTS = ("rays_per_wave", "waves", "workgroups")


def test_the_gather_plan_is_the_radiance_plan_but_for_the_kernel_bound(trt):
    """Every (scene, options) of test_gpu_queries.PLAN_CASES at 256 compute units and every batch size test_radiance_abi.py walks: the
    plan's invariants, the listed kernel shape, and every field equal to trt_radiance_launch_plan's - where the two kernels have the same
    launch bound, all of them; where they do not (the lock-step list: 6 against 7), all but the bound and what the launch rule derives
    from it, and those obey the rule."""
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
            q, qr = sc.gather_plan(n, cus), sc.radiance_plan(n, cus)
            tag = (name, options, n, q, qr)
            _check_query_plan(q, n, cus, streamed, tag)
            assert G.plan_shape(q) == shape, tag
            assert set(q) == set(qr)
            assert 1 <= q["kernel_waves_per_simd"] <= 8
            same_bound = q["kernel_waves_per_simd"] == qr["kernel_waves_per_simd"]
            lengthened = q["rays_per_wave"] > 256 or qr["rays_per_wave"] > 256
            for k in q:
                if same_bound or not (k in FROM_THE_BOUND or (lengthened and k in FROM_THE_SLOTS)):
                    assert q[k] == qr[k], (k, tag)
            per_wave, waves = q["rays_per_wave"], q["waves"]
            assert (waves - 1) * per_wave < n <= waves * per_wave, tag
            assert q["workgroups"] == -(-waves // (q["threads_per_workgroup"] // 64)), tag
            shapes.add(shape[:3])
            bounds[shape[:3]] = (q["kernel_waves_per_simd"], qr["kernel_waves_per_simd"])
    assert len(shapes) == 6, sorted(shapes)                                 # every entry of kGatherKernels
    # radiance.hip kGatherKernels: the lock-step list at 6 waves per SIMD, the other five at the radiance kernels' 7
    lock_step = [s for s in shapes if s[:2] == G.DEFAULT_SHAPES["cornell"][:2]]
    assert len(lock_step) == 1 and bounds[lock_step[0]] == (6, 7)
    assert all(b == (7, 7) for s, b in bounds.items() if s != lock_step[0]), bounds


def test_quad_texels(trt):
    """bake.quad_texels: the centres lie on the quad at (i + .5) / nu, (j + .5) / nv, column fastest; the axis is unit, orthogonal to u
    and v, along cross(u, v), and flip negates it; host arithmetic in float64, rounded once."""
    corner, u, v = np.array([1.0, 2.0, 3.0]), np.array([4.0, 0.5, 0.0]), np.array([0.0, 1.0, 5.0])
    nu, nv = 5, 3
    t = trt.bake.quad_texels(corner, u, v, nu, nv)
    assert t.dtype == np.float32 and t.shape == (nv * nu, 6) and t.flags.c_contiguous
    normal = np.cross(u, v)
    normal /= np.linalg.norm(normal)
    for j in range(nv):
        for i in range(nu):
            want = corner + (i + 0.5) / nu * u + (j + 0.5) / nv * v
            row = t[j * nu + i]
            assert row[0:3].tobytes() == want.astype(np.float32).tobytes(), (i, j)
            # on the quad: inside the parallelogram, in its plane (to f32 rounding of coordinates of this size)
            d = row[0:3].astype(np.float64) - corner
            a, b = np.linalg.lstsq(np.stack([u, v], axis=1), d, rcond=None)[0]
            assert 0.0 < a < 1.0 and 0.0 < b < 1.0 and abs(np.dot(d, normal)) < 1e-6
    axis = t[:, 3:6].astype(np.float64)
    assert (t[:, 3:6] == t[0, 3:6]).all() and t[0, 3:6].tobytes() == normal.astype(np.float32).tobytes()
    assert abs(np.linalg.norm(axis[0]) - 1.0) < 1e-6 and abs(np.dot(axis[0], u)) < 1e-5 and abs(np.dot(axis[0], v)) < 1e-5
    f = trt.bake.quad_texels(corner, u, v, nu, nv, flip=True)
    assert f[:, 0:3].tobytes() == t[:, 0:3].tobytes() and (f[:, 3:6] == -t[:, 3:6]).all()
    # the floor of the Cornell box, as examples/bake_lightmap.py lays it out: flipped, the axis points up
    kind, c, fu, fv, _ = trt.scenes.cornell(2, 2)["geometries"][3]
    floor = trt.bake.quad_texels(c, fu, fv, 4, 4, flip=True)
    assert kind == "quad" and (floor[:, 3:6] == (0.0, 1.0, 0.0)).all() and (floor[:, 1] == 0.0).all()
    assert floor[0, 0:3].tolist() == [12.5, 0.0, 12.5] and floor[1, 0:3].tolist() == [37.5, 0.0, 12.5]
    for bad in (dict(nu=0, nv=1), dict(nu=1, nv=0)):
        with pytest.raises(ValueError):
            trt.bake.quad_texels(corner, u, v, **bad)
    with pytest.raises(ValueError):
        trt.bake.quad_texels(corner, u, 2.0 * u, 2, 2)
