"""The ray-query entry points (tinyrt.h trt_intersect / trt_occluded and their device forms) at the C boundary, without a GPU: the
symbols are declared, exported and bound, trt_hit has the documented layout, and misuse comes back as a code with a message before any
device work.  What the queries answer is checked on the GPU (tests/test_gpu_queries.py); the per-kind to insertion-index table they
report `geometry` through is not reachable from Python and is covered there too (mixed400 interleaves spheres and quads)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("trt_intersect", "trt_occluded", "trt_intersect_device", "trt_occluded_device")


def test_the_four_symbols_are_declared_exported_and_bound(trt):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tinyrt.h")).read(), flags=re.S)
    raw = C.CDLL(trt._lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name + " is not declared in tinyrt.h"
        assert hasattr(raw, name), name + " is not exported"
        assert name in trt._lib.SIGNATURES and trt._lib.SIGNATURES[name][0] is C.c_int
    assert len(trt._lib.SIGNATURES["trt_intersect"][1]) == 5 and len(trt._lib.SIGNATURES["trt_intersect_device"][1]) == 6
    assert len(trt._lib.SIGNATURES["trt_occluded"][1]) == 5 and len(trt._lib.SIGNATURES["trt_occluded_device"][1]) == 6
    assert trt.lib.trt_abi_version() == 4                                  # new symbols only: the ABI version stays
    assert "trt_intersect" in re.search(r"Later under 4[^/]*\*/", open(os.path.join(ROOT, "include", "tinyrt.h")).read(), flags=re.S).group(0)


def test_trt_hit_layout(trt):
    H = trt._lib.Hit
    assert C.sizeof(H) == 28 and H.t.offset == 0 and H.geometry.offset == 4 and H.material.offset == 8 and H.front_face.offset == 12
    assert H.normal.offset == 16
    d = trt.HIT_DTYPE
    assert d.itemsize == 28 and d.fields["normal"][1] == 16 and d.fields["geometry"][1] == 4 and d.names == ("t", "geometry", "material", "front_face", "normal")


def _scene(trt):
    return trt.world_from_description(trt.scenes.cornell(8, 8))[0].get_bvh()


@pytest.mark.parametrize("name", NAMES)
def test_misuse_is_invalid_arg_with_a_message_before_any_device_work(trt, name):
    fn = getattr(trt.lib, name)
    device = name.endswith("_device")
    rays = np.zeros((4, 6), np.float32)
    out = np.zeros(4 * 28, np.uint8)
    tail = (None,) if device else ()

    def call(scene, r, n, o):
        return fn(scene, r, None, n, o, *tail)

    s = _scene(trt)
    # (host pointers are handed to the device forms too: every one of these calls must return before anything is dereferenced)
    for args in ((None, rays.ctypes.data, 4, out.ctypes.data), (s._h, None, 4, out.ctypes.data), (s._h, rays.ctypes.data, 4, None),
                 (None, None, 0, None)):
        assert call(*args) == trt._lib.ERR_INVALID_ARG, args
        assert trt.lib.trt_last_error().decode() != ""


@pytest.mark.parametrize("name", ("trt_intersect", "trt_occluded"))
def test_a_well_formed_call_needs_a_device(trt, name):
    """Without a GPU: TRT_ERR_NO_DEVICE, also for n == 0 (the order of trt_sample_batch) - there is no CPU path.  With one: success."""
    fn = getattr(trt.lib, name)
    s = _scene(trt)
    rays = np.zeros((4, 6), np.float32)
    rays[:, 5] = 1.0
    out = np.full(4 * 28, 0xCD, np.uint8)
    want = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE
    assert fn(s._h, rays.ctypes.data, None, 4, out.ctypes.data) == want
    assert fn(s._h, None, None, 0, None) == want                            # n == 0 touches nothing
    if want != trt._lib.TRT_OK:
        assert "no HIP device" in trt.lib.trt_last_error().decode()
        assert (out == 0xCD).all()
        with pytest.raises(trt.TinyRTError) as e:
            s.intersect(rays)
        assert e.value.code == trt._lib.ERR_NO_DEVICE
        with pytest.raises(trt.TinyRTError):
            s.occluded(rays, t_max=np.ones(4, np.float32))


def test_python_wrappers_check_their_arguments(trt):
    s = _scene(trt)
    with pytest.raises(ValueError):
        s.intersect(np.zeros((4, 5), np.float32))
    with pytest.raises(ValueError):
        s.occluded(np.zeros((4, 6), np.float32), t_max=np.zeros(3, np.float32))
