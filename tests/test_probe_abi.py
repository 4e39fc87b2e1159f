"""The probe query entry points (tinyrt.h trt_probe, trt_probe_device, trt_probe_launch_plan, trt_probe_params_default) at the C boundary,
without a GPU: the symbols are declared, exported and bound, misuse comes back as TRT_ERR_INVALID_ARG with a message before any device
work, an empty batch succeeds without a device, and the launch plan for every number of bands is the gather queries' but for the
kernel's launch bound.  What the buffers hold is checked on the GPU (tests/test_gpu_probe.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_query_abi import _check_query_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"trt_probe_params_default": (None, 1), "trt_probe": (C.c_int, 6), "trt_probe_device": (C.c_int, 7), "trt_probe_launch_plan": (C.c_int, 5)}


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
    assert "trt_probe_params," in later and "trt_probe_domain," in later
    assert re.search(r"enum\s+trt_probe_domain\s*\{\s*TRT_PROBE_SPHERE\s*=\s*1\s*,\s*TRT_PROBE_HEMISPHERE\s*=\s*2\s*\}", header)
    assert (trt._lib.PROBE_SPHERE, trt._lib.PROBE_HEMISPHERE) == (1, 2)
    # the domains are not new lobes: trt_lobe keeps its two values
    assert re.search(r"enum\s+trt_lobe\s*\{\s*TRT_LOBE_COSINE\s*=\s*1\s*,\s*TRT_LOBE_CONE\s*=\s*2\s*\}", header)
    assert trt.lib.trt_abi_version() == 4                                  # new symbols only: the ABI version stays
    P = trt._lib.ProbeParams
    assert C.sizeof(P) == 96
    assert (P.path.offset, P.domain.offset, P.bands.offset, P.reserved.offset) == (0, 64, 68, 72)
    # trt_radiance_params and trt_gather_params did not change
    R, G = trt._lib.RadianceParams, trt._lib.GatherParams
    assert C.sizeof(R) == 64 and C.sizeof(G) == 96
    assert (G.path.offset, G.lobe.offset, G.spread.offset, G.reserved.offset) == (0, 64, 68, 72)
    assert (R.samples_per_ray.offset, R.max_bounces.offset, R.background.offset, R.seed.offset, R.sample_begin.offset, R.sample_end.offset,
            R.accumulate.offset, R.first_stream.offset, R.reserved.offset) == (0, 4, 8, 20, 24, 28, 32, 36, 40)
    # the signatures are the gather queries' less the second-moment buffer; the plan takes the bands
    for name in ("trt_probe", "trt_probe_device"):
        mine, theirs = trt._lib.SIGNATURES[name][1], trt._lib.SIGNATURES[name.replace("probe", "gather")][1]
        assert mine[3] is C.POINTER(P) and mine[:3] + mine[4:] == theirs[:3] + theirs[4:5] + theirs[6:], name
    plan, gplan = trt._lib.SIGNATURES["trt_probe_launch_plan"][1], trt._lib.SIGNATURES["trt_gather_launch_plan"][1]
    assert plan == gplan[:2] + [C.c_uint32] + gplan[2:]
    for name in ("probe", "probe_device", "probe_plan"):
        assert callable(getattr(trt.Scene, name))
    for name in ("basis", "evaluate", "irradiance"):
        assert callable(getattr(trt.sh, name))


def test_the_default_parameters(trt):
    p = trt._lib.ProbeParams()
    C.memset(C.byref(p), 0xCD, C.sizeof(p))
    trt.lib.trt_probe_params_default(C.byref(p))
    want = trt._lib.RadianceParams()
    trt.lib.trt_radiance_params_default(C.byref(want))
    assert bytes(p.path) == bytes(want)
    assert (p.path.samples_per_ray, p.path.max_bounces, p.path.seed) == (1, 50, 1) and list(p.path.reserved) == [0] * 6
    assert p.domain == trt._lib.PROBE_SPHERE and p.bands == 3 and list(p.reserved) == [0] * 6
    trt.lib.trt_probe_params_default(None)                                 # tolerated


def _scene(trt):
    return trt.world_from_description(trt.scenes.cornell(8, 8))[0].get_bvh()


PATH_FIELDS = ("samples_per_ray", "max_bounces", "seed", "sample_begin", "sample_end", "accumulate", "first_stream")


def _params(trt, **over):
    """K = 4, depth 4, seed 5, sphere, bands 3; a keyword that names a field of the path sets it there."""
    p = trt._lib.ProbeParams()
    trt.lib.trt_probe_params_default(C.byref(p))
    p.path.samples_per_ray, p.path.max_bounces, p.path.seed = 4, 4, 5
    for k, v in over.items():
        setattr(p.path if k in PATH_FIELDS else p, k, v)
    return p


def _invalid(trt, rc):
    assert rc == trt._lib.ERR_INVALID_ARG
    assert trt.lib.trt_last_error().decode() != ""


N = 3


def _call(trt, device, s, items, n, p, sh):
    if device:
        return trt.lib.trt_probe_device(s, items, n, p, sh, None, None)
    return trt.lib.trt_probe(s, items, n, p, sh, None)


@pytest.mark.parametrize("device", (False, True))
def test_misuse_is_invalid_arg_before_any_device_work(trt, device):
    """(Host pointers are handed to the device form too: every one of these calls must return before anything is dereferenced.)"""
    sc = _scene(trt)
    items = np.zeros((N, 6), np.float32)
    items[:, 4] = 1.0
    sh = np.full((N, 9, 3), 7.0, np.float32)
    ip, sp = items.ctypes.data, sh.ctypes.data
    p = _params(trt)
    HEMI = trt._lib.PROBE_HEMISPHERE

    def call(s, r, n, q, a):
        return _call(trt, device, s, r, n, C.byref(q) if q is not None else None, a)

    # trt_radiance's own errors, applied to p->path, with sh as the required buffer
    _invalid(trt, call(None, ip, N, p, sp))
    _invalid(trt, call(sc._h, ip, N, None, sp))
    _invalid(trt, call(sc._h, None, N, p, sp))
    _invalid(trt, call(sc._h, ip, N, p, None))
    _invalid(trt, call(sc._h, ip, N, _params(trt, samples_per_ray=0), sp))
    _invalid(trt, call(sc._h, ip, N, _params(trt, sample_begin=3, sample_end=2), sp))
    _invalid(trt, call(sc._h, ip, N, _params(trt, sample_end=5), sp))                              # K + 1
    _invalid(trt, call(sc._h, ip, N, _params(trt, sample_begin=5), sp))                            # past K after the end == 0 rule
    for k in range(6):
        q = _params(trt)
        q.path.reserved[k] = 1
        _invalid(trt, call(sc._h, ip, N, q, sp))
        assert "reserved" in trt.lib.trt_last_error().decode()
    # the probe's own
    for k in range(6):
        q = _params(trt)
        q.reserved[k] = 1
        _invalid(trt, call(sc._h, ip, N, q, sp))
        assert "reserved" in trt.lib.trt_last_error().decode()
    for domain in (0, 3, 2 ** 32 - 1):
        _invalid(trt, call(sc._h, ip, N, _params(trt, domain=domain), sp))
        assert "domain" in trt.lib.trt_last_error().decode()
    for bands in (0, 4, 9, 2 ** 32 - 1):
        _invalid(trt, call(sc._h, ip, N, _params(trt, bands=bands), sp))
        assert "bands" in trt.lib.trt_last_error().decode()
    # the RNG stream index must not wrap: first_stream + n * K <= 2^32, computed in 64 bits
    want_ok = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE
    edge = 2 ** 32 - N * 4
    if not device or want_ok != trt._lib.TRT_OK:                            # (the device form is given host pointers: never let it launch)
        assert call(sc._h, ip, N, _params(trt, first_stream=edge), sp) == want_ok
        for bands in (1, 2, 3):
            assert call(sc._h, ip, N, _params(trt, bands=bands, domain=HEMI), sp) == want_ok
        sh[:] = 7.0
    _invalid(trt, call(sc._h, ip, N, _params(trt, first_stream=edge + 1), sp))
    assert "2^32" in trt.lib.trt_last_error().decode()
    _invalid(trt, call(sc._h, ip, 2 ** 32 - 1, _params(trt, samples_per_ray=2 ** 32 - 1, first_stream=2 ** 32 - 1), sp))           # n * K needs 64 bits
    _invalid(trt, call(sc._h, ip, 2 ** 31, _params(trt, samples_per_ray=2, first_stream=1), sp))
    # ... and an empty batch is checked too
    _invalid(trt, call(None, None, 0, p, None))
    _invalid(trt, call(sc._h, None, 0, None, None))
    _invalid(trt, call(sc._h, None, 0, _params(trt, samples_per_ray=0), None))
    _invalid(trt, call(sc._h, None, 0, _params(trt, domain=0), None))
    _invalid(trt, call(sc._h, None, 0, _params(trt, bands=4), None))
    assert (sh == 7.0).all()


@pytest.mark.parametrize("device", (False, True))
def test_an_empty_batch_succeeds_without_a_device_and_touches_nothing(trt, device):
    sc = _scene(trt)
    sh = np.full((N, 9, 3), 7.0, np.float32)
    for domain in (trt._lib.PROBE_SPHERE, trt._lib.PROBE_HEMISPHERE):
        for bands in (1, 2, 3):
            p = _params(trt, domain=domain, bands=bands, first_stream=2 ** 32 - 1)      # n * K == 0: any first stream passes
            assert _call(trt, device, sc._h, None, 0, C.byref(p), None) == trt._lib.TRT_OK
            assert _call(trt, device, sc._h, None, 0, C.byref(p), sh.ctypes.data) == trt._lib.TRT_OK
    assert (sh == 7.0).all()
    got, st = sc.probe(np.zeros((0, 6), np.float32), 4, bands=2, domain="hemisphere")
    assert got.shape == (0, 4, 3) and st["samples"] == 0 and st["rays"] == 0


def test_well_formed_calls_need_a_device(trt):
    """Without a GPU: TRT_ERR_NO_DEVICE - there is no CPU path.  With one: success."""
    sc = _scene(trt)
    items = np.zeros((N, 6), np.float32)
    items[:, 0:3] = (50.0, 50.0, 50.0)
    items[:, 4] = 1.0
    sh = np.full((N, 9, 3), 7.0, np.float32)
    want = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE
    p = _params(trt)
    assert trt.lib.trt_probe(sc._h, items.ctypes.data, N, C.byref(p), sh.ctypes.data, None) == want
    if want != trt._lib.TRT_OK:
        assert "no HIP device" in trt.lib.trt_last_error().decode()
        assert (sh == 7.0).all()
        assert trt.lib.trt_probe_device(sc._h, items.ctypes.data, N, C.byref(p), sh.ctypes.data, None, None) == want
        with pytest.raises(trt.TinyRTError) as e:
            sc.probe(items, 4)
        assert e.value.code == trt._lib.ERR_NO_DEVICE
    else:
        assert not (sh[:, 0, :] == 7.0).any()


def test_python_wrappers_check_their_arguments(trt):
    sc = _scene(trt)
    with pytest.raises(ValueError):
        sc.probe(np.zeros((2, 5), np.float32), 4)
    with pytest.raises(ValueError):
        sc.probe(np.zeros((2, 6), np.float32), 4, domain="cosine")
    with pytest.raises(AssertionError):
        sc.probe(np.zeros((2, 6), np.float32), 4, sh=np.zeros((2, 9, 3), np.float64))
    with pytest.raises(AssertionError):
        sc.probe(np.zeros((2, 6), np.float32), 4, bands=2, sh=np.zeros((2, 9, 3), np.float32))
    with pytest.raises(ValueError):
        sc.probe(np.zeros((2, 6), np.float32), 4, sample_end=0)
    for kw in (dict(samples_per_item=0), dict(samples_per_item=4, bands=4), dict(samples_per_item=4, bands=0)):
        with pytest.raises(trt.TinyRTError) as e:
            sc.probe(np.zeros((2, 6), np.float32), **kw)
        assert e.value.code == trt._lib.ERR_INVALID_ARG
    p = trt.Scene._probe_params(7, 2, "hemisphere", max_bounces=3, seed=9, first_stream=11)
    assert (p.path.samples_per_ray, p.path.max_bounces, p.path.seed, p.path.first_stream, p.domain, p.bands) == (7, 3, 9, 11, 2, 2)
    d = trt.Scene._probe_params(3)
    assert (d.domain, d.bands, d.path.max_bounces, d.path.seed) == (1, 3, 50, 1)


def test_the_plan_symbol_checks_its_arguments(trt):
    sc = _scene(trt)
    out = trt._lib.QueryPlan()
    assert trt.lib.trt_probe_launch_plan(None, 1, 3, 256, C.byref(out)) == trt._lib.ERR_INVALID_ARG
    assert trt.lib.trt_probe_launch_plan(sc._h, 1, 3, 256, None) == trt._lib.ERR_INVALID_ARG
    for bands in (0, 4, 2 ** 32 - 1):
        assert trt.lib.trt_probe_launch_plan(sc._h, 1, bands, 256, C.byref(out)) == trt._lib.ERR_INVALID_ARG
        assert "bands" in trt.lib.trt_last_error().decode()
    want = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE      # compute_units = 0 asks the current device
    assert trt.lib.trt_probe_launch_plan(sc._h, 1, 3, 0, C.byref(out)) == want
    assert trt.lib.trt_probe_launch_plan(sc._h, 1, 3, 256, C.byref(out)) == trt._lib.TRT_OK and out.compute_units == 256
    assert sc.probe_plan(1, 2, 304)["compute_units"] == 304


RAY_COUNTS = (1, 64, 257, 324, 100003, 2 ** 32 - 1)                          # test_radiance_abi.py's
# what plan_batch (stream_plan.h) derives from the kernel's launch bound: the resident workgroups and wave slots, and through them the runs
# of a batch too long for 256 items per wave
FROM_THE_BOUND = ("kernel_waves_per_simd", "workgroups_per_cu", "wave_slots")
FROM_THE_SLOTS = ("rays_per_wave", "waves", "workgroups")
# probe.hip kProbeKernels4 / kProbeKernels9 (profiles/probe_resource_usage.txt): (scene mode, walk, threads) -> launch bound
BOUNDS4 = {(1, 2, 256): 5, (1, 1, 256): 5, (1, 1, 768): 5, (1, 5, 512): 6, (0, 3, 256): 5, (0, 5, 256): 6}
BOUNDS9 = {(1, 2, 256): 4, (1, 1, 256): 5, (1, 1, 768): 5, (1, 5, 512): 4, (0, 3, 256): 4, (0, 5, 256): 4}
BOUNDS = {1: BOUNDS4, 2: BOUNDS4, 3: BOUNDS9}                                # bands 1 runs the 4-coefficient kernels


@pytest.mark.parametrize("bands", (1, 2, 3))
def test_the_probe_plan_is_the_gather_plan_but_for_the_kernel_bound(trt, bands):
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
            q, qg = sc.probe_plan(n, bands, cus), sc.gather_plan(n, cus)
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
    assert len(shapes) == 6, sorted(shapes)                                 # every entry of the table
    assert bounds == BOUNDS[bands], bounds
