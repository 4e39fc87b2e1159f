"""The denoiser's entry points (tinyrt.h trt_denoise_params_default, trt_denoise_scratch_bytes, trt_denoise, trt_denoise_device) at the C
boundary, without a GPU: the symbols are declared, exported and bound, the two structs have the documented layout, the defaults are the
documented ones, the scratch size behaves, and every misuse comes back as TRT_ERR_INVALID_ARG with a message before any device work.
What the filter computes is checked on the GPU (tests/test_gpu_denoise.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"trt_denoise_params_default": 1, "trt_denoise_scratch_bytes": 3, "trt_denoise": 5, "trt_denoise_device": 8}
W, H = 7, 5


def _header():
    text = open(os.path.join(ROOT, "include", "tinyrt.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_the_symbols_are_declared_exported_and_bound(trt):
    text, header = _header()
    raw = C.CDLL(trt._lib.LIB_PATH)
    later = re.search(r"Later under 4[^/]*\*/", text, flags=re.S).group(0)
    for name, nargs in NAMES.items():
        assert re.search(r"\b(int|void|uint64_t)\s+" + name + r"\s*\(", header), name + " is not declared in tinyrt.h"
        assert hasattr(raw, name), name + " is not exported"
        res, args = trt._lib.SIGNATURES[name]
        assert len(args) == nargs, name
        assert name in later, name + " is not listed under 'Later under 4'"
    assert trt._lib.SIGNATURES["trt_denoise_scratch_bytes"][0] is C.c_uint64
    assert trt._lib.SIGNATURES["trt_denoise"][0] is C.c_int and trt._lib.SIGNATURES["trt_denoise_device"][0] is C.c_int
    assert "trt_denoise_params" in later and "trt_denoise_inputs" in later
    assert trt.lib.trt_abi_version() == 4                                  # new symbols only: the ABI version stays
    for name in ("denoise", "denoise_device", "denoise_scratch_bytes", "denoise_params"):
        assert callable(getattr(trt, name)), name


def test_struct_layouts(trt):
    P, I = trt._lib.DenoiseParams, trt._lib.DenoiseInputs
    assert C.sizeof(P) == 32 and C.sizeof(I) == 32
    assert [getattr(P, n).offset for n in ("iterations", "normal_power_log2", "sigma_albedo", "sigma_depth", "reserved")] == [0, 4, 8, 12, 16]
    assert [getattr(I, n).offset for n in ("color", "albedo", "normal", "depth")] == [0, 8, 16, 24]
    # the header declares one field per declaration, in this order
    _, header = _header()
    decls = lambda name: [d.strip() for d in re.search(r"typedef struct \{([^}]*)\}\s*" + name + r"\s*;", header).group(1).split(";")   # noqa: E731
                          if d.strip()]
    assert decls("trt_denoise_params") == ["uint32_t iterations", "uint32_t normal_power_log2", "float sigma_albedo", "float sigma_depth",
                                           "uint32_t reserved[4]"]
    assert decls("trt_denoise_inputs") == ["const float *color", "const float *albedo", "const float *normal", "const float *depth"]


def test_the_defaults(trt):
    p = trt._lib.DenoiseParams(9, 9, 9.0, 9.0, (C.c_uint32 * 4)(9, 9, 9, 9))
    trt.lib.trt_denoise_params_default(C.byref(p))
    assert (p.iterations, p.normal_power_log2, list(p.reserved)) == (4, 7, [0, 0, 0, 0])
    assert np.float32(p.sigma_albedo) == np.float32(0.1) and np.float32(p.sigma_depth) == np.float32(0.05)
    trt.lib.trt_denoise_params_default(None)                               # tolerated
    assert trt.denoise_params().as_dict() == p.as_dict()
    assert trt.denoise_params(iterations=2, sigma_depth=0.0).as_dict() == dict(p.as_dict(), iterations=2, sigma_depth=0.0)
    with pytest.raises(TypeError):
        trt.denoise_params(reserved=1)
    with pytest.raises(TypeError):
        trt.denoise_params(sigma_colour=1.0)


def _bad_params(trt):
    """Every invalid trt_denoise_params the header lists."""
    nan = float("nan")
    out = [trt.denoise_params(iterations=0), trt.denoise_params(iterations=9), trt.denoise_params(iterations=0xFFFFFFFF),
           trt.denoise_params(normal_power_log2=11), trt.denoise_params(sigma_albedo=nan), trt.denoise_params(sigma_depth=nan)]
    for k in range(4):
        p = trt.denoise_params()
        p.reserved[k] = 1
        out.append(p)
    return out


def test_scratch_bytes(trt):
    fn = trt.lib.trt_denoise_scratch_bytes
    assert fn(1, 1, None) > 0 and fn(W, H, None) == fn(W, H, C.byref(trt.denoise_params())) == trt.denoise_scratch_bytes(W, H)
    sizes = (1, 2, 3, 31, 32, 33, 64, 65, 300, 2048, 3840)
    for a in sizes:
        prev_w = prev_h = 1                                               # > 0, and non-decreasing in width and in height
        for b in sizes:
            assert fn(b, a, None) >= prev_w and fn(a, b, None) >= prev_h, (a, b)
            prev_w, prev_h = fn(b, a, None), fn(a, b, None)
    for it in range(1, 9):
        assert trt.denoise_scratch_bytes(W, H, iterations=it) > 0
    assert fn(0, H, None) == 0 and fn(W, 0, None) == 0 and fn(0, 0, None) == 0
    for p in _bad_params(trt):
        assert fn(W, H, C.byref(p)) == 0
    assert fn(65536, 65536, None) > 2 ** 32                               # 64-bit arithmetic


def _invalid(trt, rc):
    assert rc == trt._lib.ERR_INVALID_ARG
    assert trt.lib.trt_last_error().decode() != ""


@pytest.mark.parametrize("device", (False, True))
def test_misuse_is_invalid_arg_before_any_device_work(trt, device):
    """(Host pointers are handed to the device form too: every one of these calls must return before anything is dereferenced.)  On a
    machine without a GPU this is also the proof that misuse is reported before TRT_ERR_NO_DEVICE."""
    color = np.full((H, W, 3), 0.5, np.float32)
    guide3 = np.full((H, W, 3), 0.25, np.float32)
    depth = np.ones((H, W), np.float32)
    out = np.full((H, W, 3), 7.0, np.float32)
    need = trt.denoise_scratch_bytes(W, H)
    scratch = np.full(need, 0xCD, np.uint8)

    def call(inputs, w, h, params, o, scratch_ptr=scratch.ctypes.data, scratch_bytes=need):
        pin = None if inputs is None else C.byref(inputs)
        pp = None if params is None else C.byref(params)
        if device:
            return trt.lib.trt_denoise_device(pin, w, h, pp, o, scratch_ptr, scratch_bytes, None)
        return trt.lib.trt_denoise(pin, w, h, pp, o)

    def inputs(**over):
        pod = trt._lib.DenoiseInputs()
        for k, v in dict(dict(color=color, albedo=guide3, normal=guide3, depth=depth), **over).items():
            setattr(pod, k, None if v is None else (v if isinstance(v, int) else v.ctypes.data))
        return pod

    ok = inputs()
    _invalid(trt, call(None, W, H, None, out.ctypes.data))
    _invalid(trt, call(inputs(color=None), W, H, None, out.ctypes.data))
    _invalid(trt, call(ok, W, H, None, None))
    _invalid(trt, call(ok, 0, H, None, out.ctypes.data))
    _invalid(trt, call(ok, W, 0, None, out.ctypes.data))
    for p in _bad_params(trt):
        _invalid(trt, call(ok, W, H, p, out.ctypes.data))
    _invalid(trt, call(ok, W, H, None, color.ctypes.data))                                   # out == color
    assert "overlap" in trt.lib.trt_last_error().decode()
    _invalid(trt, call(ok, W, H, None, color.ctypes.data + 12))                              # out inside color
    _invalid(trt, call(ok, W, H, None, guide3.ctypes.data))                                  # out == a guide
    if device:
        _invalid(trt, call(ok, W, H, None, out.ctypes.data, scratch_ptr=None))
        _invalid(trt, call(ok, W, H, None, out.ctypes.data, scratch_bytes=need - 1))
        _invalid(trt, call(ok, W, H, None, out.ctypes.data, scratch_bytes=0))
        assert "scratch" in trt.lib.trt_last_error().decode()
    assert (out == 7.0).all() and (scratch == 0xCD).all() and (color == 0.5).all()


def test_a_valid_call_needs_a_device(trt):
    """Without a GPU: TRT_ERR_NO_DEVICE - there is no CPU path.  With one: success, and a constant frame stays what it is."""
    color = np.full((H, W, 3), 0.5, np.float32)
    want = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE
    pod = trt._lib.DenoiseInputs()
    pod.color = color.ctypes.data
    out = np.full((H, W, 3), 7.0, np.float32)
    assert trt.lib.trt_denoise(C.byref(pod), W, H, None, out.ctypes.data) == want
    if want != trt._lib.TRT_OK:
        assert "no HIP device" in trt.lib.trt_last_error().decode()
        assert (out == 7.0).all()
        with pytest.raises(trt.TinyRTError) as e:
            trt.denoise(color, depth=np.ones((H, W), np.float32), iterations=2)
        assert e.value.code == trt._lib.ERR_NO_DEVICE
        # the device form, given valid arguments (host memory stands in: nothing is touched without a device)
        need = trt.denoise_scratch_bytes(W, H)
        scratch = np.zeros(need, np.uint8)
        with pytest.raises(trt.TinyRTError) as e:
            trt.denoise_device(color.ctypes.data, W, H, out.ctypes.data, scratch.ctypes.data, need)
        assert e.value.code == trt._lib.ERR_NO_DEVICE
    else:
        assert not (out == 7.0).any()


def test_python_wrappers_check_their_arguments(trt):
    color = np.zeros((H, W, 3), np.float32)
    with pytest.raises(ValueError):
        trt.denoise(np.zeros((H, W), np.float32))
    with pytest.raises(ValueError):
        trt.denoise(color, depth=np.zeros((H, W, 3), np.float32))
    with pytest.raises(ValueError):
        trt.denoise(color, normal=np.zeros((H, W + 1, 3), np.float32))
    with pytest.raises(TypeError):
        trt.denoise(color, sigma_colour=1.0)
    with pytest.raises(trt.TinyRTError) as e:
        trt.denoise(color, iterations=9)
    assert e.value.code == trt._lib.ERR_INVALID_ARG
