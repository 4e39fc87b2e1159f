"""The probe fold of sample records (tinyrt.h trt_project_samples, trt_project_samples_device) and the probe query built on it
(trt_probe_parallel, trt_probe_parallel_device, trt_probe_parallel_launch_plan) at the C boundary, without a GPU: the symbols are
declared, exported and bound; trt_probe_params is the struct read; every misuse comes back as TRT_ERR_INVALID_ARG with its message
before any device work, in the documented order; an empty batch succeeds without a device; the device forms refuse overlapping
buffers; a record buffer that holds no item is refused with the bytes one item needs; and the plan is trt_samples_launch_plan's.  What
the buffers hold is checked on the GPU (tests/test_gpu_project.py, test_gpu_project_identity.py, test_gpu_probe_parallel.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"trt_project_samples": (C.c_int, 6), "trt_project_samples_device": (C.c_int, 7), "trt_probe_parallel": (C.c_int, 7),
         "trt_probe_parallel_device": (C.c_int, 9), "trt_probe_parallel_launch_plan": (C.c_int, 5)}
PATH_FIELDS = ("samples_per_ray", "max_bounces", "seed", "sample_begin", "sample_end", "accumulate", "first_stream")
N, K = 3, 4


def test_the_symbols_are_declared_exported_and_bound(trt):
    text = open(os.path.join(ROOT, "include", "tinyrt.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = C.CDLL(trt._lib.LIB_PATH)
    later = re.search(r"Later under 4[^/]*\*/", text, flags=re.S).group(0)
    L = trt._lib
    for name, (restype, nargs) in NAMES.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name + " is not declared in tinyrt.h"
        assert hasattr(raw, name), name + " is not exported"
        res, args = L.SIGNATURES[name]
        assert res is restype and len(args) == nargs, name
        assert re.search(r"\b" + name + r"\b", later), name + " is not listed under 'Later under 4'"
    assert trt.lib.trt_abi_version() == 4                                  # new symbols only: the ABI version stays
    # trt_probe_params is the struct all four read, unchanged
    P = L.ProbeParams
    assert C.sizeof(P) == 96 and (P.path.offset, P.domain.offset, P.bands.offset, P.reserved.offset) == (0, 64, 68, 72)
    for name, at in (("trt_project_samples", 4), ("trt_project_samples_device", 4), ("trt_probe_parallel", 3), ("trt_probe_parallel_device", 3)):
        assert L.SIGNATURES[name][1][at] is C.POINTER(P), name
        assert re.search(name + r"\s*\([^)]*const\s+trt_probe_params\s*\*\s*p\b", header), name
    # trt_probe's signatures with the record buffer's size (and the buffer) added; the plan is trt_samples_launch_plan's
    assert L.SIGNATURES["trt_probe_parallel"][1] == L.SIGNATURES["trt_probe"][1] + [C.c_uint64]
    probe_device = L.SIGNATURES["trt_probe_device"][1]
    assert L.SIGNATURES["trt_probe_parallel_device"][1] == probe_device[:-1] + [C.c_void_p, C.c_uint64] + probe_device[-1:]
    assert L.SIGNATURES["trt_probe_parallel_launch_plan"] == L.SIGNATURES["trt_samples_launch_plan"]
    for name in ("probe_parallel", "probe_parallel_device", "probe_parallel_plan"):
        assert callable(getattr(trt.Scene, name))
    assert callable(trt.project_samples) and callable(trt.project_samples_device) and callable(trt.sh.project)


def _scene(trt):
    return trt.world_from_description(trt.scenes.cornell(8, 8))[0].get_bvh()


def _params(trt, **over):
    """K = 4, depth 4, seed 5, sphere, bands 3; a keyword that names a field of the path sets it there."""
    p = trt._lib.ProbeParams()
    trt.lib.trt_probe_params_default(C.byref(p))
    p.path.samples_per_ray, p.path.max_bounces, p.path.seed = K, 4, 5
    for k, v in over.items():
        if k == "path_reserved":
            p.path.reserved[v] = 1
        elif k == "reserved":
            p.reserved[v] = 1
        else:
            setattr(p.path if k in PATH_FIELDS else p, k, v)
    return p


def _invalid(trt, rc, word):
    assert rc == trt._lib.ERR_INVALID_ARG
    msg = trt.lib.trt_last_error().decode()
    assert word in msg, (word, msg)
    return msg


def _ok_or_no_device(trt):
    return trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE


# ---- trt_project_samples / trt_project_samples_device ----

@pytest.mark.parametrize("device", (False, True))
def test_misuse_of_the_projection_is_invalid_arg_in_order_before_any_device_work(trt, device):
    """(Host pointers are handed to the device form too: every one of these calls must return before anything is dereferenced.)"""
    cols = np.full((N, K, 3), 7.0, np.float32)
    dirs = np.full((N, K, 3), 7.0, np.float32)
    sh = np.full((N, 9, 3), 7.0, np.float32)
    cp, dp, sp = cols.ctypes.data, dirs.ctypes.data, sh.ctypes.data
    fn = trt.lib.trt_project_samples_device if device else trt.lib.trt_project_samples
    extra = (None,) if device else ()

    def call(c, d, n, q, s, items=None):
        return fn(c, d, items, n, C.byref(q) if q is not None else None, s, *extra)

    # each rule alone
    _invalid(trt, call(cp, dp, N, None, sp), "null argument")
    _invalid(trt, call(cp, dp, N, _params(trt, samples_per_ray=0), sp), "samples_per_ray")
    _invalid(trt, call(cp, dp, N, _params(trt, sample_begin=3, sample_end=2), sp), "range")
    _invalid(trt, call(cp, dp, N, _params(trt, sample_end=K + 1), sp), "range")
    _invalid(trt, call(cp, dp, N, _params(trt, sample_begin=K + 1), sp), "range")
    for bands in (0, 4, 9, 2 ** 32 - 1):
        _invalid(trt, call(cp, dp, N, _params(trt, bands=bands), sp), "bands")
    for k in range(6):
        _invalid(trt, call(cp, dp, N, _params(trt, path_reserved=k), sp), "reserved")
        _invalid(trt, call(cp, dp, N, _params(trt, reserved=k), sp), "reserved")
    _invalid(trt, call(None, dp, N, _params(trt), sp), "null buffer")
    _invalid(trt, call(cp, None, N, _params(trt), sp), "null buffer")
    _invalid(trt, call(cp, dp, N, _params(trt), None), "null buffer")
    # the order: the earlier rule's message wins
    _invalid(trt, call(None, None, N, None, None), "null argument")
    _invalid(trt, call(None, dp, N, _params(trt, samples_per_ray=0, bands=0, reserved=0), sp), "samples_per_ray")
    _invalid(trt, call(None, dp, N, _params(trt, sample_begin=3, sample_end=2, bands=0, reserved=0), sp), "range")
    _invalid(trt, call(None, dp, N, _params(trt, bands=4, reserved=0), sp), "bands")
    _invalid(trt, call(None, dp, N, _params(trt, bands=4, path_reserved=5), sp), "bands")
    _invalid(trt, call(None, dp, N, _params(trt, reserved=5), sp), "reserved")
    _invalid(trt, call(None, dp, N, _params(trt, path_reserved=0), cp), "reserved")
    # an empty batch is checked too, but for its buffers
    _invalid(trt, call(None, None, 0, None, None), "null argument")
    _invalid(trt, call(None, None, 0, _params(trt, samples_per_ray=0), None), "samples_per_ray")
    _invalid(trt, call(None, None, 0, _params(trt, bands=0), None), "bands")
    _invalid(trt, call(None, None, 0, _params(trt, reserved=3), None), "reserved")
    if device:
        # sh must overlap neither the 12 n K bytes of the colours nor of the directions: from the sizes, after the other rules
        _invalid(trt, call(cp, dp, N, _params(trt), cp), "overlap")
        _invalid(trt, call(cp, dp, N, _params(trt), dp), "overlap")
        _invalid(trt, call(cp, dp, N, _params(trt), cp + 12 * N * K - 4), "overlap")
        _invalid(trt, call(cp, dp, N, _params(trt), dp + 12 * N * K - 4), "overlap")
        _invalid(trt, call(cp + 12 * 9 * N - 4, dp, N, _params(trt), cp), "overlap")
        _invalid(trt, call(cp, dp + 12 * N - 4, N, _params(trt, bands=1), dp), "overlap")          # C = 1: 12 n bytes of sums
        _invalid(trt, call(cp, dp, N, _params(trt, bands=4), cp), "bands")                         # ... after the other rules
    want = _ok_or_no_device(trt)
    if want != trt._lib.TRT_OK:
        # `domain` and every field of the path but K, the range and accumulate are not read
        q = _params(trt, domain=77, max_bounces=0, seed=0, first_stream=2 ** 32 - 1, sample_begin=1, accumulate=1)
        assert call(cp, dp, N, q, sp) == want
        assert "no HIP device" in trt.lib.trt_last_error().decode()
        assert call(cp, dp, N, _params(trt), sp, items=cp) == want
        if device:
            assert call(cp, dp, N, _params(trt), cp + 12 * N * K) == want                          # touching is not overlapping
            assert call(cp, dp + 12 * N, N, _params(trt, bands=1), dp) == want
    assert (cols == 7.0).all() and (dirs == 7.0).all() and (sh == 7.0).all()


@pytest.mark.parametrize("device", (False, True))
def test_an_empty_batch_of_the_projection_succeeds_without_a_device_and_touches_nothing(trt, device):
    buf = np.full((N, K, 3), 7.0, np.float32)
    fn = trt.lib.trt_project_samples_device if device else trt.lib.trt_project_samples
    extra = (None,) if device else ()
    for bands in (1, 2, 3):
        for accumulate in (0, 1):
            p = _params(trt, bands=bands, accumulate=accumulate)
            assert fn(None, None, None, 0, C.byref(p), None, *extra) == trt._lib.TRT_OK
            assert fn(buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, 0, C.byref(p), buf.ctypes.data, *extra) == trt._lib.TRT_OK
    assert (buf == 7.0).all()
    got = trt.project_samples(np.zeros((0, K, 3), np.float32), np.zeros((0, K, 3), np.float32), bands=2)
    assert got.shape == (0, 4, 3)


def test_python_wrappers_of_the_projection_check_their_arguments(trt):
    c = np.zeros((2, 4, 3), np.float32)
    with pytest.raises(ValueError):
        trt.project_samples(c, np.zeros((2, 3, 3), np.float32))
    with pytest.raises(ValueError):
        trt.project_samples(np.zeros((2, 4), np.float32), np.zeros((2, 4), np.float32))
    with pytest.raises(AssertionError):
        trt.project_samples(c, c, bands=2, sh=np.zeros((2, 9, 3), np.float32))
    with pytest.raises(AssertionError):
        trt.project_samples(c, c, items=np.zeros((3, 6), np.float32))
    with pytest.raises(trt.TinyRTError) as e:
        trt.project_samples(c, c, bands=4, sh=np.zeros((2, 16, 3), np.float32))
    assert e.value.code == trt._lib.ERR_INVALID_ARG
    if trt.lib.trt_device_count() == 0:
        with pytest.raises(trt.TinyRTError) as e:
            trt.project_samples(c, c)
        assert e.value.code == trt._lib.ERR_NO_DEVICE                       # there is no CPU path


# ---- trt_probe_parallel / trt_probe_parallel_device ----

def _probe(trt, device, s, items, n, p, sh):
    if device:
        return trt.lib.trt_probe_device(s, items, n, p, sh, None, None)
    return trt.lib.trt_probe(s, items, n, p, sh, None)


def _parallel(trt, device, s, items, n, p, sh, records, record_bytes):
    if device:
        return trt.lib.trt_probe_parallel_device(s, items, n, p, sh, None, records, record_bytes, None)
    return trt.lib.trt_probe_parallel(s, items, n, p, sh, None, record_bytes)


@pytest.mark.parametrize("device", (False, True))
def test_misuse_of_the_parallel_probe_is_trt_probes_in_trt_probes_order_then_its_own(trt, device):
    sc = _scene(trt)
    items = np.zeros((N, 6), np.float32)
    items[:, 4] = 1.0
    sh = np.full((N, 9, 3), 7.0, np.float32)
    scratch = np.full((N * K * 6 + 64,), 7.0, np.float32)
    ip, sp, rp = items.ctypes.data, sh.ctypes.data, scratch.ctypes.data
    need = 24 * K
    HEMI = trt._lib.PROBE_HEMISPHERE

    def both(s, r, n, q, a, records=rp, record_bytes=0):
        """The parallel call with a record buffer too small for an item - a rule of trt_probe's must win - returns what trt_probe does."""
        qp = C.byref(q) if q is not None else None
        want = _probe(trt, device, s, r, n, qp, a)
        want_msg = trt.lib.trt_last_error().decode()
        got = _parallel(trt, device, s, r, n, qp, a, records, need - 1)
        assert got == want == trt._lib.ERR_INVALID_ARG and trt.lib.trt_last_error().decode() == want_msg != "", (got, want, want_msg)
        return want_msg

    p = _params(trt)
    # each of trt_probe's rules, with the same message
    both(None, ip, N, p, sp)
    both(sc._h, ip, N, None, sp)
    both(sc._h, None, N, p, sp)
    both(sc._h, ip, N, p, None)
    assert "samples_per_ray" in both(sc._h, ip, N, _params(trt, samples_per_ray=0), sp)
    assert "range" in both(sc._h, ip, N, _params(trt, sample_begin=3, sample_end=2), sp)
    assert "range" in both(sc._h, ip, N, _params(trt, sample_end=K + 1), sp)
    for k in range(6):
        assert "reserved" in both(sc._h, ip, N, _params(trt, path_reserved=k), sp)
        assert "reserved" in both(sc._h, ip, N, _params(trt, reserved=k), sp)
    assert "2^32" in both(sc._h, ip, N, _params(trt, first_stream=2 ** 32 - N * K + 1), sp)
    for domain in (0, 3, 2 ** 32 - 1):
        assert "domain" in both(sc._h, ip, N, _params(trt, domain=domain), sp)
    for bands in (0, 4, 2 ** 32 - 1):
        assert "bands" in both(sc._h, ip, N, _params(trt, bands=bands), sp)
    # trt_probe's order: the path before the domain, the domain before the bands, the bands before the reserved words
    assert "null" in both(sc._h, None, N, _params(trt, samples_per_ray=0, domain=0), sp)
    assert "samples_per_ray" in both(sc._h, ip, N, _params(trt, samples_per_ray=0, domain=0, bands=0), sp)
    assert "2^32" in both(sc._h, ip, N, _params(trt, first_stream=2 ** 32 - 1, domain=0), sp)
    assert "domain" in both(sc._h, ip, N, _params(trt, domain=0, bands=0, reserved=0), sp)
    assert "bands" in both(sc._h, ip, N, _params(trt, bands=0, reserved=0), sp)
    # an empty batch is checked too
    both(None, None, 0, p, None)
    both(sc._h, None, 0, None, None)
    assert "domain" in both(sc._h, None, 0, _params(trt, domain=0), None)
    # then its own.  m == 0: the message says how many bytes one item needs
    for q, item in ((_params(trt), need), (_params(trt, samples_per_ray=130, domain=HEMI), 24 * 130), (_params(trt, sample_begin=1, sample_end=2), need),
                    (_params(trt, max_bounces=0), need), (_params(trt, sample_begin=2, sample_end=2, accumulate=1), need)):
        for short in (item - 1, 1) + ((0,) if device else ()):               # (0 is the host form's default)
            msg = _invalid(trt, _parallel(trt, device, sc._h, ip, N, C.byref(q), sp, rp, short), "record_bytes")
            assert (" %d bytes" % item) in msg, msg
    if device:
        _invalid(trt, _parallel(trt, True, sc._h, ip, N, C.byref(p), sp, None, need), "null record buffer")
        # d_sh must not overlap the 24 K m bytes of the record buffer the call uses: m = 1 here, then m = N
        _invalid(trt, _parallel(trt, True, sc._h, ip, N, C.byref(p), rp, rp, need), "overlap")
        _invalid(trt, _parallel(trt, True, sc._h, ip, N, C.byref(p), rp + need - 4, rp, need), "overlap")
        _invalid(trt, _parallel(trt, True, sc._h, ip, N, C.byref(p), rp + N * need - 4, rp, N * need + 40), "overlap")
        _invalid(trt, _parallel(trt, True, sc._h, ip, N, C.byref(p), rp - 12 * 9 * N + 4, rp, need), "overlap")
    want = _ok_or_no_device(trt)
    if want != trt._lib.TRT_OK:
        for bytes_ in (need, need + 1, N * need, 2 ** 40):
            assert _parallel(trt, device, sc._h, ip, N, C.byref(p), sp, rp, bytes_) == want
            assert "no HIP device" in trt.lib.trt_last_error().decode()
        if device:
            assert _parallel(trt, True, sc._h, ip, N, C.byref(p), rp + need, rp, need) == want       # m = 1: behind one item's records is free
            assert _parallel(trt, True, sc._h, ip, N, C.byref(p), rp + N * need, rp, 2 ** 40) == want
        else:
            assert _parallel(trt, False, sc._h, ip, N, C.byref(p), sp, None, 0) == want              # the default holds an item whatever K is
            big = _params(trt, samples_per_ray=2 ** 23, first_stream=0)
            assert _parallel(trt, False, sc._h, ip, N, C.byref(big), sp, None, 0) == want
    assert (sh == 7.0).all() and (scratch == 7.0).all()


@pytest.mark.parametrize("device", (False, True))
def test_an_empty_batch_of_the_parallel_probe_succeeds_without_a_device_and_touches_nothing(trt, device):
    sc = _scene(trt)
    sh = np.full((N, 9, 3), 7.0, np.float32)
    for domain in (trt._lib.PROBE_SPHERE, trt._lib.PROBE_HEMISPHERE):
        for bands in (1, 2, 3):
            p = _params(trt, domain=domain, bands=bands, first_stream=2 ** 32 - 1)      # n * K == 0: any first stream passes
            for record_bytes in (0, 1, 24 * K):                             # no item, so no item's need
                assert _parallel(trt, device, sc._h, None, 0, C.byref(p), None, None, record_bytes) == trt._lib.TRT_OK
                assert _parallel(trt, device, sc._h, None, 0, C.byref(p), sh.ctypes.data, sh.ctypes.data, record_bytes) == trt._lib.TRT_OK
    assert (sh == 7.0).all()
    got, st = sc.probe_parallel(np.zeros((0, 6), np.float32), 4, bands=2, domain="hemisphere")
    assert got.shape == (0, 4, 3) and st["samples"] == 0 and st["rays"] == 0
    stats = trt._lib.Stats()
    C.memset(C.byref(stats), 0xCD, C.sizeof(stats))
    p = _params(trt)
    assert trt.lib.trt_probe_parallel(sc._h, None, 0, C.byref(p), None, C.byref(stats), 0) == trt._lib.TRT_OK
    assert stats.samples == 0 and stats.rays == 0                           # as trt_probe: the stats of an empty batch are zeros


def test_the_plan_is_trt_samples_launch_plans(trt):
    import test_gpu_queries as G
    import walk_ray_cases as W
    out, want = trt._lib.QueryPlan(), trt._lib.QueryPlan()
    sc = _scene(trt)
    assert trt.lib.trt_probe_parallel_launch_plan(None, 1, 1, 256, C.byref(out)) == trt._lib.ERR_INVALID_ARG
    assert trt.lib.trt_probe_parallel_launch_plan(sc._h, 1, 1, 256, None) == trt._lib.ERR_INVALID_ARG
    assert trt.lib.trt_probe_parallel_launch_plan(sc._h, 2 ** 16, 2 ** 16, 256, C.byref(out)) == trt._lib.ERR_INVALID_ARG
    assert "2^32 - 1" in trt.lib.trt_last_error().decode()
    assert trt.lib.trt_probe_parallel_launch_plan(sc._h, 1, 1, 0, C.byref(out)) == _ok_or_no_device(trt)
    worlds = {}
    for name, options, _ in G.PLAN_CASES:
        if name not in worlds:
            worlds[name] = trt.world_from_description(W.scene(trt, name))[0]
        host_options = {k: v for k, v in options.items() if k != "on_device"}
        s = worlds[name].get_bvh(**host_options) if host_options else worlds[name].get_bvh()
        for n, r in ((1, 1), (64, 16384), (324, 8), (7, 130), (2 ** 20, 16), (1, 700), (65537, 65535), (5, 0), (0, 5)):
            for cus in (256, 304):
                assert trt.lib.trt_probe_parallel_launch_plan(s._h, n, r, cus, C.byref(out)) == trt._lib.TRT_OK
                assert trt.lib.trt_samples_launch_plan(s._h, n, r, cus, C.byref(want)) == trt._lib.TRT_OK
                assert bytes(out) == bytes(want), (name, options, n, r, cus)
                assert s.probe_parallel_plan(n, r, cus) == s.samples_plan(n, r, cus)
    assert sc.probe_parallel_plan(7, None, 256) == sc.samples_plan(7, 1, 256)
    # 64 probes of 16 384 samples: 4096 waves, where trt_probe's rule gives the 64 items one
    assert sc.probe_parallel_plan(64, 16384, 256)["waves"] == 4096 and sc.probe_plan(64, 3, 256)["waves"] == 1
