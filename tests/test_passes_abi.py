"""The passes query entry points (tinyrt.h trt_passes, trt_passes_device, trt_passes_launch_plan, trt_passes_params_default) at the C
boundary, without a GPU: the symbols are declared, exported and bound, misuse comes back as TRT_ERR_INVALID_ARG with a message before any
device work, an empty batch succeeds without a device, and the launch plan for every number of depth bins is the gather queries' but for
the kernel's launch bound.  What the buffers hold is checked on the GPU (tests/test_gpu_passes.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_query_abi import _check_query_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"trt_passes_params_default": (None, 1), "trt_passes": (C.c_int, 7), "trt_passes_device": (C.c_int, 8), "trt_passes_launch_plan": (C.c_int, 5)}


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
    assert "trt_passes_params," in later and "trt_passes_source," in later
    assert re.search(r"enum\s+trt_passes_source\s*\{\s*TRT_PASSES_RAYS\s*=\s*0\s*,\s*TRT_PASSES_COSINE\s*=\s*1\s*,\s*TRT_PASSES_CONE\s*=\s*2\s*\}", header)
    assert (trt._lib.PASSES_RAYS, trt._lib.PASSES_COSINE, trt._lib.PASSES_CONE) == (0, 1, 2)
    assert (trt._lib.PASSES_COSINE, trt._lib.PASSES_CONE) == (trt._lib.LOBE_COSINE, trt._lib.LOBE_CONE)
    # the sources are not new lobes: trt_lobe keeps its two values
    assert re.search(r"enum\s+trt_lobe\s*\{\s*TRT_LOBE_COSINE\s*=\s*1\s*,\s*TRT_LOBE_CONE\s*=\s*2\s*\}", header)
    assert trt.lib.trt_abi_version() == 4                                  # new symbols only: the ABI version stays
    P = trt._lib.PassesParams
    assert C.sizeof(P) == 128
    assert (P.gather.offset, P.depth_bins.offset, P.reserved.offset) == (0, 96, 100)
    # trt_radiance_params and trt_gather_params did not change
    R, G = trt._lib.RadianceParams, trt._lib.GatherParams
    assert C.sizeof(R) == 64 and C.sizeof(G) == 96
    assert (G.path.offset, G.lobe.offset, G.spread.offset, G.reserved.offset) == (0, 64, 68, 72)
    # the signatures are the gather queries' with the spent shares in the place of the second moments; the plan takes the bins
    for name in ("trt_passes", "trt_passes_device"):
        mine, theirs = trt._lib.SIGNATURES[name][1], trt._lib.SIGNATURES[name.replace("passes", "gather")][1]
        assert mine[3] is C.POINTER(P) and mine[:3] + mine[4:] == theirs[:3] + theirs[4:], name
    plan, gplan = trt._lib.SIGNATURES["trt_passes_launch_plan"][1], trt._lib.SIGNATURES["trt_gather_launch_plan"][1]
    assert plan == gplan[:2] + [C.c_uint32] + gplan[2:]
    for name in ("passes", "passes_device", "passes_plan"):
        assert callable(getattr(trt.Scene, name))
    for name in ("slot", "direct", "indirect", "emitters", "sky"):
        assert callable(getattr(trt.passes, name))


def test_the_rust_and_cpp_texts_name_the_symbols():
    """The crates cannot be compiled here: the declarations are kept textually consistent with the header."""
    sys_rs = open(os.path.join(ROOT, "bindings", "rust", "tinyrt-sys", "src", "lib.rs")).read()
    safe_rs = open(os.path.join(ROOT, "bindings", "rust", "tinyrt", "src", "lib.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "tinyrt.hpp")).read()
    for name in NAMES:
        assert re.search(r"pub fn " + name + r"\s*\(", sys_rs), name + " is not declared in tinyrt-sys"
    assert re.search(r"pub struct trt_passes_params\s*\{[^}]*pub gather: trt_gather_params,[^}]*pub depth_bins: u32,[^}]*pub reserved: \[u32; 7\],", sys_rs)
    for k, v in (("TRT_PASSES_RAYS", 0), ("TRT_PASSES_COSINE", 1), ("TRT_PASSES_CONE", 2)):
        assert re.search(r"pub const " + k + r": u32 = %d;" % v, sys_rs), k
    assert re.search(r"pub fn passes\s*\(", safe_rs) and "sys::trt_passes(" in safe_rs
    assert re.search(r"\bpasses\s*\(", hpp) and "trt_passes(" in hpp and "trt_passes_params_default" in hpp


def test_the_default_parameters(trt):
    p = trt._lib.PassesParams()
    C.memset(C.byref(p), 0xCD, C.sizeof(p))
    trt.lib.trt_passes_params_default(C.byref(p))
    want = trt._lib.GatherParams()
    trt.lib.trt_gather_params_default(C.byref(want))
    assert bytes(p.gather) == bytes(want)
    assert (p.gather.path.samples_per_ray, p.gather.path.max_bounces, p.gather.path.seed) == (1, 50, 1)
    assert p.gather.lobe == trt._lib.PASSES_COSINE and p.gather.spread == 0.0 and list(p.gather.reserved) == [0] * 6
    assert p.depth_bins == 3 and list(p.reserved) == [0] * 7
    trt.lib.trt_passes_params_default(None)                                # tolerated


def _scene(trt):
    return trt.world_from_description(trt.scenes.cornell(8, 8))[0].get_bvh()


PATH_FIELDS = ("samples_per_ray", "max_bounces", "seed", "sample_begin", "sample_end", "accumulate", "first_stream")
GATHER_FIELDS = ("lobe", "spread")


def _params(trt, **over):
    """K = 4, depth 4, seed 5, cosine, 3 bins; a keyword that names a field of the path or of the gather sets it there."""
    p = trt._lib.PassesParams()
    trt.lib.trt_passes_params_default(C.byref(p))
    p.gather.path.samples_per_ray, p.gather.path.max_bounces, p.gather.path.seed = 4, 4, 5
    for k, v in over.items():
        setattr(p.gather.path if k in PATH_FIELDS else p.gather if k in GATHER_FIELDS else p, k, v)
    return p


def _invalid(trt, rc):
    assert rc == trt._lib.ERR_INVALID_ARG
    assert trt.lib.trt_last_error().decode() != ""


N = 3


def _call(trt, device, s, items, n, p, passes, spent=None):
    if device:
        return trt.lib.trt_passes_device(s, items, n, p, passes, spent, None, None)
    return trt.lib.trt_passes(s, items, n, p, passes, spent, None)


@pytest.mark.parametrize("device", (False, True))
def test_misuse_is_invalid_arg_before_any_device_work(trt, device):
    """(Host pointers are handed to the device form too: every one of these calls must return before anything is dereferenced.)"""
    sc = _scene(trt)
    items = np.zeros((N, 6), np.float32)
    items[:, 4] = 1.0
    out = np.full((N, 8, 3), 7.0, np.float32)
    spent = np.full(N, 7.0, np.float32)
    ip, op, sp = items.ctypes.data, out.ctypes.data, spent.ctypes.data
    p = _params(trt)
    RAYS, COSINE, CONE = trt._lib.PASSES_RAYS, trt._lib.PASSES_COSINE, trt._lib.PASSES_CONE

    def call(s, r, n, q, a):
        return _call(trt, device, s, r, n, C.byref(q) if q is not None else None, a, sp)

    # trt_radiance's own errors, applied to p->gather.path, with passes as the required buffer
    _invalid(trt, call(None, ip, N, p, op))
    _invalid(trt, call(sc._h, ip, N, None, op))
    _invalid(trt, call(sc._h, None, N, p, op))
    _invalid(trt, call(sc._h, ip, N, p, None))
    _invalid(trt, call(sc._h, ip, N, _params(trt, samples_per_ray=0), op))
    _invalid(trt, call(sc._h, ip, N, _params(trt, sample_begin=3, sample_end=2), op))
    _invalid(trt, call(sc._h, ip, N, _params(trt, sample_end=5), op))                              # K + 1
    _invalid(trt, call(sc._h, ip, N, _params(trt, sample_begin=5), op))                            # past K after the end == 0 rule
    for k in range(6):
        q = _params(trt)
        q.gather.path.reserved[k] = 1
        _invalid(trt, call(sc._h, ip, N, q, op))
        assert "reserved" in trt.lib.trt_last_error().decode()
    # trt_gather's
    for k in range(6):
        q = _params(trt)
        q.gather.reserved[k] = 1
        _invalid(trt, call(sc._h, ip, N, q, op))
        assert "reserved" in trt.lib.trt_last_error().decode()
    for source in (3, 4, 2 ** 32 - 1):
        _invalid(trt, call(sc._h, ip, N, _params(trt, lobe=source), op))
        assert "source" in trt.lib.trt_last_error().decode()
    for spread in (-0.5, float("nan"), float("inf"), -float("inf")):
        _invalid(trt, call(sc._h, ip, N, _params(trt, lobe=CONE, spread=spread), op))
        assert "spread" in trt.lib.trt_last_error().decode()
    # the passes' own
    for k in range(7):
        q = _params(trt)
        q.reserved[k] = 1
        _invalid(trt, call(sc._h, ip, N, q, op))
        assert "reserved" in trt.lib.trt_last_error().decode()
    for bins in (0, 5, 8, 2 ** 32 - 1):
        _invalid(trt, call(sc._h, ip, N, _params(trt, depth_bins=bins), op))
        assert "depth_bins" in trt.lib.trt_last_error().decode()
    # the RNG stream index must not wrap: first_stream + n * K <= 2^32, computed in 64 bits
    want_ok = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE
    edge = 2 ** 32 - N * 4
    if not device or want_ok != trt._lib.TRT_OK:                            # (the device form is given host pointers: never let it launch)
        assert call(sc._h, ip, N, _params(trt, first_stream=edge), op) == want_ok
        for bins in (1, 2, 3, 4):
            for source in (RAYS, COSINE, CONE):
                assert call(sc._h, ip, N, _params(trt, depth_bins=bins, lobe=source, spread=0.25), op) == want_ok
        # a bad spread is an error of the cone only: the other sources do not read it
        for source in (RAYS, COSINE):
            assert call(sc._h, ip, N, _params(trt, lobe=source, spread=float("nan")), op) == want_ok
        assert _call(trt, device, sc._h, ip, N, C.byref(p), op, None) == want_ok          # spent is optional
        out[:] = 7.0
        spent[:] = 7.0
    _invalid(trt, call(sc._h, ip, N, _params(trt, first_stream=edge + 1), op))
    assert "2^32" in trt.lib.trt_last_error().decode()
    _invalid(trt, call(sc._h, ip, 2 ** 32 - 1, _params(trt, samples_per_ray=2 ** 32 - 1, first_stream=2 ** 32 - 1), op))           # n * K needs 64 bits
    _invalid(trt, call(sc._h, ip, 2 ** 31, _params(trt, samples_per_ray=2, first_stream=1), op))
    # ... and an empty batch is checked too
    _invalid(trt, call(None, None, 0, p, None))
    _invalid(trt, call(sc._h, None, 0, None, None))
    _invalid(trt, call(sc._h, None, 0, _params(trt, samples_per_ray=0), None))
    _invalid(trt, call(sc._h, None, 0, _params(trt, lobe=3), None))
    _invalid(trt, call(sc._h, None, 0, _params(trt, depth_bins=5), None))
    _invalid(trt, call(sc._h, None, 0, _params(trt, lobe=CONE, spread=-1.0), None))
    assert (out == 7.0).all() and (spent == 7.0).all()


@pytest.mark.parametrize("device", (False, True))
def test_an_empty_batch_succeeds_without_a_device_and_touches_nothing(trt, device):
    sc = _scene(trt)
    out = np.full((N, 8, 3), 7.0, np.float32)
    spent = np.full(N, 7.0, np.float32)
    for source in (0, 1, 2):
        for bins in (1, 2, 3, 4):
            p = _params(trt, lobe=source, depth_bins=bins, first_stream=2 ** 32 - 1)      # n * K == 0: any first stream passes
            assert _call(trt, device, sc._h, None, 0, C.byref(p), None) == trt._lib.TRT_OK
            assert _call(trt, device, sc._h, None, 0, C.byref(p), out.ctypes.data, spent.ctypes.data) == trt._lib.TRT_OK
    assert (out == 7.0).all() and (spent == 7.0).all()
    got, sp, st = sc.passes(np.zeros((0, 6), np.float32), 4, depth_bins=2, source="rays")
    assert got.shape == (0, 4, 3) and sp.shape == (0,) and st["samples"] == 0 and st["rays"] == 0


def test_well_formed_calls_need_a_device(trt):
    """Without a GPU: TRT_ERR_NO_DEVICE - there is no CPU path.  With one: success."""
    sc = _scene(trt)
    items = np.zeros((N, 6), np.float32)
    items[:, 0:3] = (50.0, 50.0, 50.0)
    items[:, 4] = 1.0
    out = np.full((N, 6, 3), 7.0, np.float32)
    spent = np.full(N, 7.0, np.float32)
    want = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE
    p = _params(trt)
    assert trt.lib.trt_passes(sc._h, items.ctypes.data, N, C.byref(p), out.ctypes.data, spent.ctypes.data, None) == want
    if want != trt._lib.TRT_OK:
        assert "no HIP device" in trt.lib.trt_last_error().decode()
        assert (out == 7.0).all() and (spent == 7.0).all()
        assert trt.lib.trt_passes_device(sc._h, items.ctypes.data, N, C.byref(p), out.ctypes.data, None, None, None) == want
        with pytest.raises(trt.TinyRTError) as e:
            sc.passes(items, 4)
        assert e.value.code == trt._lib.ERR_NO_DEVICE
    else:
        assert not (out == 7.0).any() and not (spent == 7.0).any()


def test_python_wrappers_check_their_arguments(trt):
    sc = _scene(trt)
    z = np.zeros((2, 6), np.float32)
    with pytest.raises(ValueError):
        sc.passes(np.zeros((2, 5), np.float32), 4)
    with pytest.raises(ValueError):
        sc.passes(z, 4, source="sphere")
    with pytest.raises(AssertionError):
        sc.passes(z, 4, passes=np.zeros((2, 6, 3), np.float64))
    with pytest.raises(AssertionError):
        sc.passes(z, 4, depth_bins=2, passes=np.zeros((2, 6, 3), np.float32))
    with pytest.raises(AssertionError):
        sc.passes(z, 4, spent=np.zeros((2, 1), np.float32))
    with pytest.raises(ValueError):
        sc.passes(z, 4, sample_end=0)
    for kw in (dict(samples_per_item=0), dict(samples_per_item=4, depth_bins=5), dict(samples_per_item=4, depth_bins=0),
               dict(samples_per_item=4, source="cone", spread=-1.0)):
        with pytest.raises(trt.TinyRTError) as e:
            sc.passes(z, **kw)
        assert e.value.code == trt._lib.ERR_INVALID_ARG
    p = trt.Scene._passes_params(7, 2, "cone", 0.25, max_bounces=3, seed=9, first_stream=11)
    g = p.gather
    assert (g.path.samples_per_ray, g.path.max_bounces, g.path.seed, g.path.first_stream, g.lobe, g.spread, p.depth_bins) == (7, 3, 9, 11, 2, 0.25, 2)
    d = trt.Scene._passes_params(3)
    assert (d.gather.lobe, d.depth_bins, d.gather.path.max_bounces, d.gather.path.seed) == (1, 3, 50, 1)
    assert trt.Scene._passes_params(3, source="rays").gather.lobe == 0


def test_the_plan_symbol_checks_its_arguments(trt):
    sc = _scene(trt)
    out = trt._lib.QueryPlan()
    assert trt.lib.trt_passes_launch_plan(None, 1, 3, 256, C.byref(out)) == trt._lib.ERR_INVALID_ARG
    assert trt.lib.trt_passes_launch_plan(sc._h, 1, 3, 256, None) == trt._lib.ERR_INVALID_ARG
    for bins in (0, 5, 2 ** 32 - 1):
        assert trt.lib.trt_passes_launch_plan(sc._h, 1, bins, 256, C.byref(out)) == trt._lib.ERR_INVALID_ARG
        assert "depth_bins" in trt.lib.trt_last_error().decode()
    want = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE      # compute_units = 0 asks the current device
    assert trt.lib.trt_passes_launch_plan(sc._h, 1, 3, 0, C.byref(out)) == want
    assert trt.lib.trt_passes_launch_plan(sc._h, 1, 3, 256, C.byref(out)) == trt._lib.TRT_OK and out.compute_units == 256
    assert sc.passes_plan(1, 2, 304)["compute_units"] == 304


RAY_COUNTS = (1, 64, 257, 324, 100003, 2 ** 32 - 1)                          # test_radiance_abi.py's
# what plan_batch (stream_plan.h) derives from the kernel's launch bound: the resident workgroups and wave slots, and through them the runs
# of a batch too long for 256 items per wave
FROM_THE_BOUND = ("kernel_waves_per_simd", "workgroups_per_cu", "wave_slots")
FROM_THE_SLOTS = ("rays_per_wave", "waves", "workgroups")
# passes.hip kPassesKernels2 / kPassesKernels4 (profiles/passes_resource_usage.txt): (scene mode, walk, threads) -> launch bound
BOUNDS2 = {(1, 2, 256): 5, (1, 1, 256): 5, (1, 1, 768): 5, (1, 5, 512): 6, (0, 3, 256): 5, (0, 5, 256): 6}
BOUNDS4 = {(1, 2, 256): 5, (1, 1, 256): 5, (1, 1, 768): 5, (1, 5, 512): 5, (0, 3, 256): 5, (0, 5, 256): 5}
BOUNDS = {1: BOUNDS2, 2: BOUNDS2, 3: BOUNDS4, 4: BOUNDS4}                    # 1 and 2 bins run the kernels that carry 2, 3 and 4 those that carry 4


@pytest.mark.parametrize("bins", (1, 2, 3, 4))
def test_the_passes_plan_is_the_gather_plan_but_for_the_kernel_bound(trt, bins):
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
            q, qg = sc.passes_plan(n, bins, cus), sc.gather_plan(n, cus)
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
    assert bounds == BOUNDS[bins], bounds
