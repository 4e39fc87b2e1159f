"""The second-moment render, the variance kernel and the variance-guided denoiser (tinyrt.h trt_render_moments[_device],
trt_variance[_device], trt_denoise_color_default, trt_denoise_ex[_device]) at the C boundary, without a GPU: the symbols are declared,
exported and bound, trt_denoise_color has the documented layout and defaults, every misuse comes back as TRT_ERR_INVALID_ARG with a
message before any device work (on a machine without a GPU: before TRT_ERR_NO_DEVICE), trt_variance of no pixels succeeds, and
trt_denoise_scratch_bytes is what it was.  What the kernels compute is checked on the GPU (tests/test_gpu_moments.py,
tests/test_gpu_denoise_color.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"trt_render_moments": 6, "trt_render_moments_device": 7, "trt_variance": 5, "trt_variance_device": 6,
         "trt_denoise_color_default": 1, "trt_denoise_ex": 6, "trt_denoise_ex_device": 9}
W, H = 7, 5


def _header():
    text = open(os.path.join(ROOT, "include", "tinyrt.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _invalid(trt, rc):
    assert rc == trt._lib.ERR_INVALID_ARG
    assert trt.lib.trt_last_error().decode() != ""


def test_the_symbols_are_declared_exported_and_bound(trt):
    text, header = _header()
    raw = C.CDLL(trt._lib.LIB_PATH)
    later = re.search(r"Later under 4[^/]*\*/", text, flags=re.S).group(0)
    for name, nargs in NAMES.items():
        assert re.search(r"\b(int|void)\s+" + name + r"\s*\(", header), name + " is not declared in tinyrt.h"
        assert hasattr(raw, name), name + " is not exported"
        res, args = trt._lib.SIGNATURES[name]
        assert len(args) == nargs, name
        assert res is (None if name == "trt_denoise_color_default" else C.c_int), name
        assert name in later, name + " is not listed under 'Later under 4'"
    assert "trt_denoise_color" in later
    assert trt.lib.trt_abi_version() == 4                                  # new symbols only: the ABI version stays
    for name in ("variance", "variance_device", "denoise_color"):
        assert callable(getattr(trt, name)), name
    for name in ("render_moments", "render_moments_device"):
        assert callable(getattr(trt.Renderer, name)), name


def test_denoise_color_layout_and_defaults(trt):
    K = trt._lib.DenoiseColor
    assert C.sizeof(K) == 32
    assert [getattr(K, n).offset for n in ("variance", "sigma_color", "reserved")] == [0, 8, 12]
    _, header = _header()
    decls = [d.strip() for d in re.search(r"typedef struct \{([^}]*)\}\s*trt_denoise_color\s*;", header).group(1).split(";") if d.strip()]
    assert decls == ["const float *variance", "float sigma_color", "uint32_t reserved[5]"]
    k = K(0xDEAD, 9.0, (C.c_uint32 * 5)(9, 9, 9, 9, 9))
    trt.lib.trt_denoise_color_default(C.byref(k))
    assert k.variance is None and list(k.reserved) == [0] * 5
    assert np.float32(k.sigma_color) == np.float32(SIGMA_COLOR_DEFAULT) and k.sigma_color > 0
    trt.lib.trt_denoise_color_default(None)                                # tolerated
    assert trt.denoise_color().sigma_color == k.sigma_color and trt.denoise_color(sigma_color=2.5).sigma_color == 2.5
    # the struct that may not grow did not
    assert C.sizeof(trt._lib.DenoiseParams) == 32 and C.sizeof(trt._lib.DenoiseInputs) == 32


SIGMA_COLOR_DEFAULT = 8.0                                                  # tinyrt.h / DESIGN.md 6.4


def _scene(trt):
    world, cam = trt.world_from_description(trt.scenes.cornell(8, 8))
    return world, world.get_bvh(), cam


@pytest.mark.parametrize("device", (False, True))
def test_render_moments_misuse_is_invalid_arg_before_any_device_work(trt, device):
    """(Host pointers are handed to the device form too: every one of these calls must return before anything is dereferenced.)"""
    world, scene, cam = _scene(trt)
    r = trt.Renderer(4, 1, 8, False, (0.0, 0.0, 0.0), seed=1)
    accum = np.full((8, 8, 3), 7.0, np.float32)
    m2 = np.full((8, 8, 3), 7.0, np.float32)

    def call(s, c, p, a, m):
        ps = None if p is None else C.byref(p)
        pc = None if c is None else C.byref(c.pod)
        if device:
            return trt.lib.trt_render_moments_device(s, pc, ps, a, m, None, None)
        return trt.lib.trt_render_moments(s, pc, ps, a, m, None)

    ok = r.params()
    _invalid(trt, call(scene._h, cam, ok, accum.ctypes.data, None))                        # a NULL moment2
    assert "moment2" in trt.lib.trt_last_error().decode()
    _invalid(trt, call(scene._h, cam, ok, None, m2.ctypes.data))
    _invalid(trt, call(None, cam, ok, accum.ctypes.data, m2.ctypes.data))
    _invalid(trt, call(scene._h, None, ok, accum.ctypes.data, m2.ctypes.data))
    _invalid(trt, call(scene._h, cam, None, accum.ctypes.data, m2.ctypes.data))
    for backend in (trt.BACKEND_MEGAKERNEL, trt.BACKEND_WAVEFRONT, 17):                    # only the streamed backend keeps per-sample records
        _invalid(trt, call(scene._h, cam, r.params(backend=backend), accum.ctypes.data, m2.ctypes.data))
        assert "backend" in trt.lib.trt_last_error().decode()
    assert (accum == 7.0).all() and (m2 == 7.0).all()
    # a valid call: TRT_OK with a device, TRT_ERR_NO_DEVICE without one - there is no CPU path
    if trt.lib.trt_device_count() == 0:
        for backend in (trt.BACKEND_AUTO, trt.BACKEND_STREAMED):
            assert call(scene._h, cam, r.params(backend=backend), accum.ctypes.data, m2.ctypes.data) == trt._lib.ERR_NO_DEVICE
        assert (accum == 7.0).all() and (m2 == 7.0).all()
        if not device:
            with pytest.raises(trt.TinyRTError) as e:
                r.render_moments(cam, world)
            assert e.value.code == trt._lib.ERR_NO_DEVICE


@pytest.mark.parametrize("device", (False, True))
def test_variance_misuse_and_the_empty_call(trt, device):
    s = np.full((H, W, 3), 0.5, np.float32)
    m = np.full((H, W, 3), 0.5, np.float32)
    v = np.full((H, W), 7.0, np.float32)
    n = W * H

    def call(a, b, npix, spp, out):
        if device:
            return trt.lib.trt_variance_device(a, b, npix, spp, out, None)
        return trt.lib.trt_variance(a, b, npix, spp, out)

    _invalid(trt, call(None, m.ctypes.data, n, 4, v.ctypes.data))
    _invalid(trt, call(s.ctypes.data, None, n, 4, v.ctypes.data))
    _invalid(trt, call(s.ctypes.data, m.ctypes.data, n, 4, None))
    _invalid(trt, call(None, None, 1, 0, None))
    # no pixels: succeeds, with or without a device, whatever the pointers
    assert call(None, None, 0, 4, None) == trt._lib.TRT_OK
    assert call(s.ctypes.data, m.ctypes.data, 0, 0, v.ctypes.data) == trt._lib.TRT_OK
    assert (v == 7.0).all()
    if trt.lib.trt_device_count() == 0:
        assert call(s.ctypes.data, m.ctypes.data, n, 4, v.ctypes.data) == trt._lib.ERR_NO_DEVICE
        assert "no HIP device" in trt.lib.trt_last_error().decode() and (v == 7.0).all()
    if not device:
        assert trt.variance(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), 4).shape == (0,)
        with pytest.raises(ValueError):
            trt.variance(s, m[:-1], 4)
        with pytest.raises(ValueError):
            trt.variance(s[..., 0], m[..., 0], 4)


@pytest.mark.parametrize("device", (False, True))
def test_denoise_ex_misuse_is_invalid_arg_before_any_device_work(trt, device):
    color = np.full((H, W, 3), 0.5, np.float32)
    guide3 = np.full((H, W, 3), 0.25, np.float32)
    depth = np.ones((H, W), np.float32)
    var = np.full((H, W), 0.01, np.float32)
    out = np.full((H, W, 3), 7.0, np.float32)
    need = trt.denoise_scratch_bytes(W, H)
    scratch = np.full(need, 0xCD, np.uint8)
    pod = trt._lib.DenoiseInputs()
    pod.color, pod.albedo, pod.normal, pod.depth = color.ctypes.data, guide3.ctypes.data, guide3.ctypes.data, depth.ctypes.data

    def call(col, o, inputs=pod, w=W, h=H, params=None, scratch_ptr=scratch.ctypes.data, scratch_bytes=need):
        pin = None if inputs is None else C.byref(inputs)
        pc = None if col is None else C.byref(col)
        pp = None if params is None else C.byref(params)
        if device:
            return trt.lib.trt_denoise_ex_device(pin, pc, w, h, pp, o, scratch_ptr, scratch_bytes, None)
        return trt.lib.trt_denoise_ex(pin, pc, w, h, pp, o)

    ok = trt.denoise_color(var.ctypes.data)
    _invalid(trt, call(trt.denoise_color(var.ctypes.data, float("nan")), out.ctypes.data))   # a NaN sigma_color
    assert "sigma_color" in trt.lib.trt_last_error().decode()
    _invalid(trt, call(trt.denoise_color(None, float("nan")), out.ctypes.data))              # ... also with the term off
    for k in range(5):                                                                       # a non-zero reserved word
        bad = trt.denoise_color(var.ctypes.data)
        bad.reserved[k] = 1
        _invalid(trt, call(bad, out.ctypes.data))
        assert "reserved" in trt.lib.trt_last_error().decode()
    big = np.zeros(H * W * 3 + 8, np.float32)                                                # the output overlapping `variance`
    for off in (0, 4, W * H * 4 - 4):
        _invalid(trt, call(trt.denoise_color(big.ctypes.data + off), big.ctypes.data))
        assert "overlap" in trt.lib.trt_last_error().decode()
    _invalid(trt, call(trt.denoise_color(big.ctypes.data + W * H * 12 - 4), big.ctypes.data))
    # trt_denoise's own misuse is still refused with the extra argument present
    _invalid(trt, call(ok, out.ctypes.data, inputs=None))
    _invalid(trt, call(ok, None))
    _invalid(trt, call(ok, out.ctypes.data, w=0))
    _invalid(trt, call(ok, color.ctypes.data))
    _invalid(trt, call(ok, out.ctypes.data, params=trt.denoise_params(iterations=9)))
    p = trt.denoise_params()
    p.reserved[3] = 1
    _invalid(trt, call(ok, out.ctypes.data, params=p))
    if device:
        _invalid(trt, call(ok, out.ctypes.data, scratch_ptr=None))
        _invalid(trt, call(ok, out.ctypes.data, scratch_bytes=need - 1))                     # the term on needs no more scratch, and no less
    assert (out == 7.0).all() and (scratch == 0xCD).all() and (color == 0.5).all() and (var == np.float32(0.01)).all()
    if trt.lib.trt_device_count() == 0:
        for col in (None, ok, trt.denoise_color(None), trt.denoise_color(var.ctypes.data, 0.0), trt.denoise_color(var.ctypes.data, -1.0)):
            assert call(col, out.ctypes.data) == trt._lib.ERR_NO_DEVICE
        assert (out == 7.0).all()
        with pytest.raises(trt.TinyRTError) as e:
            trt.denoise(color, variance=var)
        assert e.value.code == trt._lib.ERR_NO_DEVICE
    with pytest.raises(ValueError):
        trt.denoise(color, variance=np.zeros((H, W + 1), np.float32))
    with pytest.raises(trt.TinyRTError) as e:
        trt.denoise(color, variance=var, sigma_color=float("nan"))
    assert e.value.code == trt._lib.ERR_INVALID_ARG


def test_scratch_bytes_are_unchanged(trt):
    """trt_denoise_ex needs no more scratch than trt_denoise: the variance rides in the fourth word of the 16-byte colour records (the
    plain form's two 4-byte images fit into the 64 B per pixel).  The figures: 16 bytes to reach a 16-byte boundary, then four images
    of 16 bytes per pixel, each rounded up to 16 bytes - for the sizes tests/test_denoise_abi.py uses."""
    fn = trt.lib.trt_denoise_scratch_bytes
    sizes = (1, 2, 3, 5, 7, 31, 32, 33, 64, 65, 300, 2048, 3840, 65536)
    for w in sizes:
        for h in sizes:
            assert fn(w, h, None) == 16 + 4 * ((w * h * 16 + 15) // 16 * 16), (w, h)
    assert fn(W, H, None) == 16 + 4 * W * H * 16 == 2256
    for it in range(1, 9):
        assert trt.denoise_scratch_bytes(W, H, iterations=it) == 2256
