"""The direct-light entry points (tinyrt.h trt_scene_emitters, trt_emitter_init_quad, trt_emitter_init_sphere, trt_direct, trt_direct_device,
trt_direct_launch_plan, trt_direct_params_default) at the C boundary, without a GPU: the symbols are declared, exported and bound, the two
structs have the header's layout, misuse comes back as TRT_ERR_INVALID_ARG with a message before any device work, an empty batch succeeds
without a device, the emitter records equal the numpy restatement (tests/direct_cases.py) bit for bit, and the launch plan is the ambient
queries' but for the kernel's launch bound.  What the buffers hold is checked on the GPU (tests/test_gpu_direct.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import direct_cases as D
from test_query_abi import _check_query_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"trt_scene_emitters": (C.c_int, 4), "trt_emitter_init_quad": (None, 5), "trt_emitter_init_sphere": (None, 4),
         "trt_direct_params_default": (None, 1), "trt_direct": (C.c_int, 9), "trt_direct_device": (C.c_int, 10),
         "trt_direct_launch_plan": (C.c_int, 4)}


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
    assert "trt_emitter," in later and "trt_direct_params," in later
    assert trt.lib.trt_abi_version() == 4                                  # new symbols only: the ABI version stays
    E = trt._lib.Emitter
    assert C.sizeof(E) == 80
    assert (E.kind.offset, E.geometry.offset, E.a.offset, E.b.offset, E.c.offset, E.normal.offset, E.color.offset, E.area.offset,
            E.reserved.offset) == (0, 4, 8, 20, 32, 44, 56, 68, 72) and E.reserved.size == 8
    assert trt.lights.EMITTER_DTYPE == D.EMITTER_DTYPE and D.EMITTER_DTYPE.itemsize == 80
    assert [D.EMITTER_DTYPE.fields[n][1] for n in D.EMITTER_DTYPE.names] == [0, 4, 8, 20, 32, 44, 56, 68, 72]
    P = trt._lib.DirectParams
    assert C.sizeof(P) == 96 and (P.path.offset, P.shadow_end.offset, P.reserved.offset) == (0, 64, 68) and P.reserved.size == 28
    assert C.sizeof(trt._lib.RadianceParams) == 64                          # unchanged
    # the signatures are the gather queries' with the table and its length behind n and the other parameter struct
    for name in ("trt_direct", "trt_direct_device"):
        mine, theirs = trt._lib.SIGNATURES[name][1], trt._lib.SIGNATURES[name.replace("direct", "gather")][1]
        assert mine[5] is C.POINTER(P) and mine[3] is C.c_void_p and mine[4] is C.c_uint32, name
        assert mine[:3] + mine[6:] == theirs[:3] + theirs[4:], name
    assert trt._lib.SIGNATURES["trt_direct_launch_plan"][1] == trt._lib.SIGNATURES["trt_ambient_launch_plan"][1]
    for name in ("emitters", "direct", "direct_device", "direct_plan"):
        assert callable(getattr(trt.Scene, name))
    assert callable(trt.lights.quad) and callable(trt.lights.sphere)
    # the structs in the header, field for field
    m = re.search(r"typedef struct \{([^}]*)\}\s*trt_emitter\s*;", header)
    assert m and re.findall(r"(\w+)\s+([\w, ]+?)(\[\d+\])?\s*;", m.group(1)) == [
        ("uint32_t", "kind", ""), ("uint32_t", "geometry", ""), ("trt_vec3", "a, b, c", ""), ("trt_vec3", "normal", ""), ("trt_vec3", "color", ""),
        ("float", "area", ""), ("uint32_t", "reserved", "[2]")]
    m = re.search(r"typedef struct \{([^}]*)\}\s*trt_direct_params\s*;", header)
    assert m and re.findall(r"(\w+)\s+(\w+)(\[\d+\])?\s*;", m.group(1)) == [("trt_radiance_params", "path", ""), ("float", "shadow_end", ""),
                                                                           ("uint32_t", "reserved", "[7]")]


def test_the_layouts_match_the_c_compiler(trt, tmp_path):
    import subprocess
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tinyrt.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(trt_emitter), offsetof(trt_emitter, normal), offsetof(trt_emitter, color), offsetof(trt_emitter, area), '
                   'offsetof(trt_emitter, reserved), sizeof(trt_direct_params), offsetof(trt_direct_params, shadow_end), '
                   'offsetof(trt_direct_params, reserved)); return 0; }\n')
    exe = str(tmp_path / "sz")
    subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [80, 44, 56, 68, 72, 96, 64, 68]


def test_the_default_parameters(trt):
    p = trt._lib.DirectParams()
    C.memset(C.byref(p), 0xCD, C.sizeof(p))
    trt.lib.trt_direct_params_default(C.byref(p))
    want = trt._lib.RadianceParams()
    trt.lib.trt_radiance_params_default(C.byref(want))
    assert bytes(p.path) == bytes(want)
    assert np.float32(p.shadow_end) == np.float32(0.999) and list(p.reserved) == [0] * 7
    trt.lib.trt_direct_params_default(None)                                # tolerated
    trt.lib.trt_emitter_init_quad(None, trt.Vec3(), trt.Vec3(), trt.Vec3(), trt.Vec3())
    trt.lib.trt_emitter_init_sphere(None, trt.Vec3(), 1.0, trt.Vec3())


def _scene(trt):
    return trt.world_from_description(trt.scenes.cornell(8, 8))[0].get_bvh()


PATH_FIELDS = ("samples_per_ray", "max_bounces", "seed", "sample_begin", "sample_end", "accumulate", "first_stream")


def _params(trt, **over):
    """K = 4, seed 5; a keyword that names a field of the path sets it there."""
    p = trt._lib.DirectParams()
    trt.lib.trt_direct_params_default(C.byref(p))
    p.path.samples_per_ray, p.path.seed = 4, 5
    for k, v in over.items():
        setattr(p.path if k in PATH_FIELDS else p, k, v)
    return p


def _invalid(trt, rc, word=None):
    assert rc == trt._lib.ERR_INVALID_ARG
    msg = trt.lib.trt_last_error().decode()
    assert msg != "" and (word is None or word in msg), msg


N = 3


def _call(trt, device, s, items, n, table, n_emitters, p, rad, m2):
    if device:
        return trt.lib.trt_direct_device(s, items, n, table, n_emitters, p, rad, m2, None, None)
    return trt.lib.trt_direct(s, items, n, table, n_emitters, p, rad, m2, None)


@pytest.mark.parametrize("device", (False, True))
def test_misuse_is_invalid_arg_before_any_device_work(trt, device):
    """(Host pointers are handed to the device form too: every one of these calls must return before anything is dereferenced.)"""
    sc = _scene(trt)
    items = np.zeros((N, 6), np.float32)
    items[:, 4] = 1.0
    rad = np.full((N, 3), 7.0, np.float32)
    m2 = np.full((N, 3), 7.0, np.float32)
    table = trt.lights.table(sc.emitters(), trt.lights.sphere((50.0, 50.0, 50.0), 2.0, (1.0, 1.0, 1.0)))
    E = len(table)
    assert E == 2
    ip, rp, mp, tp = items.ctypes.data, rad.ctypes.data, m2.ctypes.data, table.ctypes.data
    p = _params(trt)

    def call(s, r, n, q, a, b, t=tp, e=E):
        return _call(trt, device, s, r, n, t, e, C.byref(q) if q is not None else None, a, b)

    _invalid(trt, call(None, ip, N, p, rp, mp))
    _invalid(trt, call(sc._h, ip, N, None, rp, mp))
    _invalid(trt, call(sc._h, None, N, p, rp, mp))
    _invalid(trt, call(sc._h, ip, N, p, None, mp))
    # everything trt_radiance reports on the path
    _invalid(trt, call(sc._h, ip, N, _params(trt, samples_per_ray=0), rp, mp))
    _invalid(trt, call(sc._h, ip, N, _params(trt, sample_begin=3, sample_end=2), rp, mp))
    _invalid(trt, call(sc._h, ip, N, _params(trt, sample_end=5), rp, mp))                          # K + 1
    _invalid(trt, call(sc._h, ip, N, _params(trt, sample_begin=5), rp, mp))                        # past K after the end == 0 rule
    for k in range(6):
        q = _params(trt)
        q.path.reserved[k] = 1
        _invalid(trt, call(sc._h, ip, N, q, rp, mp), "reserved")
    # the table
    _invalid(trt, call(sc._h, ip, N, p, rp, mp, t=None), "emitter")
    for e in (0, 2 ** 20 + 1, 2 ** 32 - 1):
        _invalid(trt, call(sc._h, ip, N, p, rp, mp, e=e), "n_emitters")
    if not device:                                                          # the device form cannot read the table
        for kind in (2, 3, 2 ** 32 - 1):
            bad = table.copy()
            bad["kind"][1] = kind
            _invalid(trt, call(sc._h, ip, N, p, rp, mp, t=bad.ctypes.data), "kind")
        for k in range(2):
            bad = table.copy()
            bad["reserved"][0, k] = 1
            _invalid(trt, call(sc._h, ip, N, p, rp, mp, t=bad.ctypes.data), "reserved")
    # this struct's own
    for end in (float("nan"), 0.0, -0.0, -1.0, float(np.nextafter(np.float32(1.0), np.float32(2.0))), 2.0, float("inf"), -float("inf")):
        _invalid(trt, call(sc._h, ip, N, _params(trt, shadow_end=end), rp, mp), "shadow_end")
    for k in range(7):
        q = _params(trt)
        q.reserved[k] = 1
        _invalid(trt, call(sc._h, ip, N, q, rp, mp), "reserved")
    # the RNG stream index must not wrap: first_stream + n * K <= 2^32, computed in 64 bits
    want_ok = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE
    edge = 2 ** 32 - N * 4
    if not device or want_ok != trt._lib.TRT_OK:                            # (the device form is given host pointers: never let it launch)
        assert call(sc._h, ip, N, _params(trt, first_stream=edge), rp, mp) == want_ok
        # there is no path: max_bounces == 0 and a NaN background are accepted, as is every shadow_end in (0, 1]
        q = _params(trt, max_bounces=0)
        q.path.background.x = float("nan")
        assert call(sc._h, ip, N, q, rp, mp) == want_ok
        for end in (1.0, 0.5, 1e-30):
            assert call(sc._h, ip, N, _params(trt, shadow_end=end), rp, mp) == want_ok
        assert call(sc._h, ip, N, p, rp, None) == want_ok                                          # moment2 is optional
        assert call(sc._h, ip, N, p, rp, mp, e=1) == want_ok
        big = np.zeros(2 ** 20, D.EMITTER_DTYPE)
        big[:] = table[1]
        assert call(sc._h, ip, N, p, rp, mp, t=big.ctypes.data, e=2 ** 20) == want_ok              # the largest table
        rad[:] = 7.0
        m2[:] = 7.0
    _invalid(trt, call(sc._h, ip, N, _params(trt, first_stream=edge + 1), rp, mp), "2^32")
    _invalid(trt, call(sc._h, ip, 2 ** 32 - 1, _params(trt, samples_per_ray=2 ** 32 - 1, first_stream=2 ** 32 - 1), rp, mp))       # n * K needs 64 bits
    _invalid(trt, call(sc._h, ip, 2 ** 31, _params(trt, samples_per_ray=2, first_stream=1), rp, mp))
    # ... and an empty batch is checked too, but for the table, which it does not need
    _invalid(trt, call(None, None, 0, p, None, None))
    _invalid(trt, call(sc._h, None, 0, None, None, None))
    _invalid(trt, call(sc._h, None, 0, _params(trt, samples_per_ray=0), None, None))
    _invalid(trt, call(sc._h, None, 0, _params(trt, shadow_end=float("nan")), None, None))
    q = _params(trt)
    q.reserved[6] = 1
    _invalid(trt, call(sc._h, None, 0, q, None, None))
    assert (rad == 7.0).all() and (m2 == 7.0).all()


@pytest.mark.parametrize("device", (False, True))
def test_an_empty_batch_succeeds_without_a_device_and_touches_nothing(trt, device):
    sc = _scene(trt)
    rad = np.full((N, 3), 7.0, np.float32)
    p = _params(trt, first_stream=2 ** 32 - 1, shadow_end=0.5)             # n * K == 0: any first stream passes
    assert _call(trt, device, sc._h, None, 0, None, 0, C.byref(p), None, None) == trt._lib.TRT_OK
    assert _call(trt, device, sc._h, None, 0, None, 7, C.byref(p), rad.ctypes.data, rad.ctypes.data) == trt._lib.TRT_OK
    assert (rad == 7.0).all()
    got, m2, st = sc.direct(np.zeros((0, 6), np.float32), sc.emitters(), 4, moment2=True)
    assert got.shape == (0, 3) and m2.shape == (0, 3) and st["samples"] == 0 and st["rays"] == 0


def test_well_formed_calls_need_a_device(trt):
    """Without a GPU: TRT_ERR_NO_DEVICE - there is no CPU path.  With one: success."""
    sc = _scene(trt)
    items = np.zeros((N, 6), np.float32)
    items[:, 0:3] = (50.0, 0.0, 50.0)
    items[:, 4] = 1.0
    rad = np.full((N, 3), 7.0, np.float32)
    table = sc.emitters()
    want = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE
    p = _params(trt)
    assert trt.lib.trt_direct(sc._h, items.ctypes.data, N, table.ctypes.data, len(table), C.byref(p), rad.ctypes.data, None, None) == want
    if want != trt._lib.TRT_OK:
        assert "no HIP device" in trt.lib.trt_last_error().decode()
        assert (rad == 7.0).all()
        assert trt.lib.trt_direct_device(sc._h, items.ctypes.data, N, table.ctypes.data, len(table), C.byref(p), rad.ctypes.data, None, None, None) == want
        with pytest.raises(trt.TinyRTError) as e:
            sc.direct(items, table, 4)
        assert e.value.code == trt._lib.ERR_NO_DEVICE
    else:
        assert not (rad == 7.0).any()


def test_python_wrappers_check_their_arguments(trt):
    sc = _scene(trt)
    table = sc.emitters()
    with pytest.raises(ValueError):
        sc.direct(np.zeros((2, 5), np.float32), table, 4)
    with pytest.raises(ValueError):
        sc.direct(np.zeros((2, 6), np.float32), np.zeros((1, 20), np.float32), 4)
    with pytest.raises(AssertionError):
        sc.direct(np.zeros((2, 6), np.float32), table, 4, radiance=np.zeros((2, 3), np.float64))
    with pytest.raises(AssertionError):
        sc.direct(np.zeros((2, 6), np.float32), table, 4, moment2=np.zeros((3, 3), np.float32))
    for kw in (dict(samples_per_item=0), dict(samples_per_item=4, shadow_end=0.0), dict(samples_per_item=4, shadow_end=float("nan"))):
        with pytest.raises(trt.TinyRTError) as e:
            sc.direct(np.zeros((2, 6), np.float32), table, **kw)
        assert e.value.code == trt._lib.ERR_INVALID_ARG
    with pytest.raises(trt.TinyRTError) as e:
        sc.direct(np.zeros((2, 6), np.float32), table[:0], 4)               # an empty table
    assert e.value.code == trt._lib.ERR_INVALID_ARG
    p = trt.Scene._direct_params(7, shadow_end=0.25, seed=9, first_stream=11, sample_begin=1, sample_end=5, accumulate=True)
    assert (p.path.samples_per_ray, p.path.seed, p.path.first_stream, p.shadow_end) == (7, 9, 11, 0.25)
    assert (p.path.sample_begin, p.path.sample_end, p.path.accumulate) == (1, 5, 1)
    d = trt.Scene._direct_params(3)
    assert (np.float32(d.shadow_end), d.path.sample_end, d.path.seed) == (np.float32(0.999), 0, 1)


@pytest.mark.parametrize("name", ["cornell", "prims33", "prims600"])
def test_the_emitter_records_equal_the_restatement(trt, orc, name):
    """trt_scene_emitters against tests/direct_cases.py emitters_of - the lights of the description in insertion order, normal and area
    in float32 scalars and orc_ray_new - and the two init functions against quad_record / sphere_record, byte for byte."""
    import walk_ray_cases as W
    desc = W.scene(trt, name)
    sc = trt.world_from_description(desc)[0].get_bvh()
    want = D.emitters_of(orc, desc)
    got = sc.emitters()
    assert len(want) >= 1 and got.dtype == D.EMITTER_DTYPE
    assert got.tobytes() == want.tobytes(), (name, got, want)
    assert (np.diff(got["geometry"].astype(np.int64)) > 0).all() and (got["reserved"] == 0).all()
    kinds = {desc["geometries"][g][0] for g in got["geometry"]}
    assert {("quad", "sphere")[1 - k] for k in got["kind"]} == kinds
    print(name, "emitters", len(got), "kinds", sorted(kinds))
    # cap cuts the copy, never the count; the entries behind cap stay
    count = C.c_uint32(99)
    buf = np.zeros(len(want) + 1, D.EMITTER_DTYPE)
    buf["geometry"] = 12345
    assert trt.lib.trt_scene_emitters(sc._h, buf.ctypes.data, 1, C.byref(count)) == 0 and count.value == len(want)
    assert buf[:1].tobytes() == want[:1].tobytes() and (buf["geometry"][1:] == 12345).all()
    assert trt.lib.trt_scene_emitters(sc._h, None, 0, C.byref(count)) == 0 and count.value == len(want)
    assert trt.lib.trt_scene_emitters(None, None, 0, C.byref(count)) == trt._lib.ERR_INVALID_ARG
    assert trt.lib.trt_scene_emitters(sc._h, None, 0, None) == trt._lib.ERR_INVALID_ARG
    assert trt.lib.trt_scene_emitters(sc._h, None, 1, C.byref(count)) == trt._lib.ERR_INVALID_ARG
    # the init functions on the scene's own lights (as if they were virtual) and on the tests' two
    for e in want:
        w = e.copy()
        w["geometry"] = D.NO_GEOMETRY
        mine = trt.lights.quad(e["a"], e["b"], e["c"], e["color"]) if e["kind"] == 1 else trt.lights.sphere(e["a"], e["b"][0], e["color"])
        assert mine.tobytes() == w.tobytes(), (name, mine, w)
    virt = trt.lights.table(trt.lights.quad(**D.VIRTUAL_QUAD), trt.lights.sphere(**D.VIRTUAL_SPHERE))
    assert virt.tobytes() == D.virtual_emitters(orc).tobytes()
    assert virt["area"].tolist() == [1600.0, float(np.float32(12.566371) * np.float32(4.0))] and virt["normal"][0].tolist() == [0.0, -1.0, 0.0]


def test_the_init_functions_on_awkward_quads(trt, orc):
    """A skewed quad whose cross product rounds, a degenerate one (zero area: the normal is 0 / 0) and a huge one (the area overflows)."""
    rng = np.random.default_rng(3)
    cases = [((0.0, 0.0, 0.0), tuple(rng.normal(size=3)), tuple(rng.normal(size=3))) for _ in range(50)]
    cases += [((1.0, 2.0, 3.0), (1.0, 0.0, 0.0), (2.0, 0.0, 0.0)), ((0.0, 0.0, 0.0), (1e30, 0.0, 0.0), (0.0, 1e30, 0.0)),
              ((0.0, 0.0, 0.0), (1e-30, 0.0, 0.0), (0.0, 1e-30, 0.0))]
    for corner, u, v in cases:
        want = D.quad_record(orc, corner, u, v, (1.0, 2.0, 3.0))
        got = trt.lights.quad(corner, u, v, (1.0, 2.0, 3.0))
        D.assert_same_bits(got["normal"], want["normal"], (corner, u, v, "normal"))
        D.assert_same_bits(got["area"].reshape(1, 1), want["area"].reshape(1, 1), (corner, u, v, "area"))
    for r in (0.0, 1.5, 1e-30, 1e25, float("inf")):
        want, got = D.sphere_record((1.0, 2.0, 3.0), r, (1.0, 1.0, 1.0)), trt.lights.sphere((1.0, 2.0, 3.0), r, (1.0, 1.0, 1.0))
        assert got.tobytes() == want.tobytes(), r


def test_a_scene_without_lights_has_no_emitters(trt):
    import walk_ray_cases as W
    for name in ("grid3000", "random_spheres"):
        sc = trt.world_from_description(W.scene(trt, name))[0].get_bvh()
        assert len(sc.emitters()) == 0
        count = C.c_uint32(99)
        assert trt.lib.trt_scene_emitters(sc._h, None, 0, C.byref(count)) == 0 and count.value == 0


def test_the_plan_symbol_checks_its_arguments(trt):
    sc = _scene(trt)
    out = trt._lib.QueryPlan()
    assert trt.lib.trt_direct_launch_plan(None, 1, 256, C.byref(out)) == trt._lib.ERR_INVALID_ARG
    assert trt.lib.trt_direct_launch_plan(sc._h, 1, 256, None) == trt._lib.ERR_INVALID_ARG
    want = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE      # compute_units = 0 asks the current device
    assert trt.lib.trt_direct_launch_plan(sc._h, 1, 0, C.byref(out)) == want
    assert trt.lib.trt_direct_launch_plan(sc._h, 1, 256, C.byref(out)) == trt._lib.TRT_OK and out.compute_units == 256
    assert sc.direct_plan(1, 304)["compute_units"] == 304


RAY_COUNTS = (1, 64, 257, 324, 100003, 2 ** 32 - 1)                          # test_radiance_abi.py's
# what plan_batch (stream_plan.h) derives from the kernel's launch bound: the resident workgroups and wave slots, and through them the runs
# of a batch too long for 256 items per wave
FROM_THE_BOUND = ("kernel_waves_per_simd", "workgroups_per_cu", "wave_slots")
FROM_THE_SLOTS = ("rays_per_wave", "waves", "workgroups")
# direct.hip kDirectKernels (profiles/direct_resource_usage.txt): (scene mode, walk, threads) -> launch bound
BOUNDS = {(1, 2, 256): 7, (1, 1, 256): 8, (1, 1, 768): 8, (1, 5, 512): 7, (0, 3, 256): 7, (0, 5, 256): 6}


def test_the_direct_plan_is_the_ambient_plan_but_for_the_kernel_bound(trt):
    """Every (scene, options) of test_gpu_queries.PLAN_CASES at 256 compute units and every batch size test_radiance_abi.py walks: the
    plan's invariants, the listed kernel shape, and every field equal to trt_ambient_launch_plan's but the bound and what the launch rule
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
            q, qa = sc.direct_plan(n, cus), sc.ambient_plan(n, cus)
            tag = (name, options, n, q, qa)
            _check_query_plan(q, n, cus, streamed, tag)
            assert G.plan_shape(q) == shape, tag
            assert set(q) == set(qa)
            assert 1 <= q["kernel_waves_per_simd"] <= 8
            same_bound = q["kernel_waves_per_simd"] == qa["kernel_waves_per_simd"]
            lengthened = q["rays_per_wave"] > 256 or qa["rays_per_wave"] > 256
            for k in q:
                if same_bound or not (k in FROM_THE_BOUND or (lengthened and k in FROM_THE_SLOTS)):
                    assert q[k] == qa[k], (k, tag)
            per_wave, waves = q["rays_per_wave"], q["waves"]
            assert (waves - 1) * per_wave < n <= waves * per_wave, tag
            assert q["workgroups"] == -(-waves // (q["threads_per_workgroup"] // 64)), tag
            shapes.add(shape[:3])
            bounds[shape[:3]] = q["kernel_waves_per_simd"]
    assert len(shapes) == 6, sorted(shapes)                                 # every entry of kDirectKernels
    assert bounds == BOUNDS, bounds
