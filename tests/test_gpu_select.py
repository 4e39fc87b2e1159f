"""The selection of the pixels that are still too noisy (trt_select_pixels and its device form) on the GPU, bit for bit against a numpy
restatement of tinyrt.h (tests/adaptive_cases.py restated_select): all float32, one operation per operator, in the header's order.

Inputs: synthetic sums that hit every case of the definition - d < 0 (clamped), a NaN sum, +-inf, v == b exactly (not kept) and one
float above it (kept), zeros; samples_done = 1 and 0 (every candidate kept); random sums of 200 000 pixels; the oracle's Cornell 19 x 13
moments after 4 of 8 samples.  List lengths: 0, 1, 63, 64, 65 (both sides of a wave), 257 (one beyond the 256 candidates a workgroup
scans), 65 537 (one beyond the 256 x 256 candidates one chunk of the second scan level covers) and 196 613 (three chunks: the carry).
Candidate lists: NULL (the pixels 0 .. n-1), a fixed shuffle, and lists with entries past npixels, which are not kept and not read.
The order of the output is the candidates'; the restatement must keep some and drop some wherever that is possible, so no comparison
is between two empty or two full lists.  The host form may select in place (selected == candidates).  Every GPU step is one in-process call."""
import numpy as np
import pytest

import denoise_color_cases as D
import walk_ray_cases as W
from adaptive_cases import restated_select

pytestmark = pytest.mark.gpu

f32 = np.float32
TILE = 256                                                                  # pixels.hip kSelectTile
LENGTHS = [0, 1, 63, 64, 65, TILE + 1, TILE * TILE + 1, 3 * TILE * TILE + 5]
GUARD = 64                                                                  # words


def synthetic():
    """(S, M) float32 [16, 3] for N = done = 2 (k = 1, inv = 1), rel_tol = 1, abs_tol = 0."""
    s, m = np.zeros((16, 3), f32), np.zeros((16, 3), f32)
    s[0], m[0] = (0.5, 0.0, 0.0), (0.5, 0.0, 0.0)                            # d = 0.25 = v; l = 0.5, b = 0.25: v == b exactly -> not kept
    s[1], m[1] = (0.5, 0.0, 0.0), (np.nextafter(f32(0.5), f32(1)), 0.0, 0.0)  # one float above: kept
    s[2], m[2] = (0.7, 0.1, 0.2), (0.1, 0.001, 0.01)                         # M < S*S in every channel: d clamped to 0, not kept
    s[3], m[3] = (np.nan, 0.1, 0.1), (1.0, 1.0, 1.0)                         # NaN sum: l is NaN, b is NaN -> not kept
    s[4], m[4] = (0.1, 0.1, 0.1), (np.nan, 5.0, 5.0)                         # NaN moment: that channel counts 0, the others decide: kept
    s[5], m[5] = (0.1, 0.1, 0.1), (np.inf, 0.0, 0.0)                         # v = inf > b: kept
    s[6], m[6] = (np.inf, 0.1, 0.1), (np.inf, 1.0, 1.0)                      # inf - inf = NaN -> 0; b = inf: not kept
    s[7], m[7] = (-np.inf, 0.1, 0.1), (1.0, 1.0, 1.0)                        # b = inf: not kept
    s[8], m[8] = 0.0, 0.0                                                    # 0 > 0: not kept
    s[9], m[9] = (0.0, 0.0, 0.0), (1e-30, 0.0, 0.0)                          # any variance over a black pixel: kept
    s[10], m[10] = (15.0, 15.0, 15.0), (225.0, 225.0, 225.0)                 # the light itself: constant, not kept
    s[11], m[11] = (0.1, 0.2, 0.3), (0.5, 0.5, 0.5)                          # plainly noisy: kept
    s[12], m[12] = (0.1, 0.2, 0.3), (0.0100001, 0.0400001, 0.0900001)        # plainly converged
    s[13], m[13] = (3e38, 0.0, 0.0), (3e38, 0.0, 0.0)                        # s*s overflows: d = -inf -> 0
    s[14], m[14] = (1e-30, 0.0, 0.0), (1e-30, 0.0, 0.0)                      # s*s underflows to a denormal / 0
    s[15], m[15] = (0.25, 0.25, 0.25), (0.5, 0.5, 0.5)
    return s, m


def host_and_device(trt, s, m, n_cap, done, rel_tol, abs_tol, candidates, n, what):
    """Both forms against the restatement; returns the selection."""
    import torch
    want = restated_select(s, m, n_cap, done, rel_tol, abs_tol, candidates, n)
    import ctypes as C
    cand_arr = None if candidates is None else np.ascontiguousarray(candidates, np.uint32)
    sc, mc = np.ascontiguousarray(s, np.float32), np.ascontiguousarray(m, np.float32)
    out = np.full(n + 1, 0xCDCDCDCD, np.uint32)
    count = C.c_uint32(0xCDCDCDCD)
    trt._lib.check(trt.lib.trt_select_pixels(sc.ctypes.data, mc.ctypes.data, sc.size // 3, n_cap, done,
                                             cand_arr.ctypes.data if cand_arr is not None and n else None, n, rel_tol, abs_tol, out.ctypes.data,
                                             C.byref(count)))
    assert count.value == len(want), (what, "host form", count.value, len(want))
    assert np.array_equal(out[:len(want)], want) and (out[len(want):] == 0xCDCDCDCD).all(), (what, "host form")
    if candidates is not None or n == sc.size // 3:
        assert np.array_equal(trt.select_pixels(s, m, n_cap, done, rel_tol, abs_tol, candidates=candidates), want), (what, "Python wrapper")
    npixels = s.size // 3
    d_s = torch.from_numpy(np.ascontiguousarray(s).reshape(-1)).to("cuda:0") if s.size else torch.zeros(3, device="cuda:0")
    d_m = torch.from_numpy(np.ascontiguousarray(m).reshape(-1)).to("cuda:0") if m.size else torch.zeros(3, device="cuda:0")
    d_cand = None if candidates is None or n == 0 else torch.from_numpy(np.asarray(candidates, np.uint32).astype(np.int64)).to(torch.int32).to("cuda:0")
    side = torch.cuda.Stream()
    scratch_bytes = trt.select_scratch_bytes(n)
    assert scratch_bytes % 4 == 0 and scratch_bytes >= 4 * -(-n // TILE)
    for stream in (None, side):
        d_sel = torch.full((GUARD + n + GUARD,), -0x32323233, dtype=torch.int32, device="cuda:0")          # 0xCDCDCDCD
        d_count = torch.full((1 + GUARD,), -0x32323233, dtype=torch.int32, device="cuda:0")
        d_scratch = torch.full((scratch_bytes // 4 + GUARD,), -0x32323233, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        ptr = 0 if stream is None else stream.cuda_stream
        trt.select_pixels_device(d_s.data_ptr(), d_m.data_ptr(), npixels, n_cap, done, n, rel_tol, abs_tol, d_sel.data_ptr() + GUARD * 4,
                                 d_count.data_ptr(), d_scratch.data_ptr(), scratch_bytes, d_candidates_ptr=0 if d_cand is None else d_cand.data_ptr(),
                                 stream_ptr=ptr)
        (torch.cuda.current_stream() if stream is None else stream).synchronize()
        torch.cuda.synchronize()
        count = d_count.cpu().numpy().view(np.uint32)
        sel = d_sel.cpu().numpy().view(np.uint32)
        assert count[0] == len(want), (what, "device form", int(count[0]), len(want))
        assert (count[1:] == 0xCDCDCDCD).all()
        assert np.array_equal(sel[GUARD:GUARD + len(want)], want), (what, "device form")
        assert (sel[:GUARD] == 0xCDCDCDCD).all() and (sel[GUARD + len(want):] == 0xCDCDCDCD).all(), (what, "written past the selection")
        assert (d_scratch.cpu().numpy().view(np.uint32)[scratch_bytes // 4:] == 0xCDCDCDCD).all(), (what, "written past the scratch")
    return want


def test_every_case_of_the_definition(trt):
    s, m = synthetic()
    want = host_and_device(trt, s, m, 2, 2, 1.0, 0.0, None, 16, "synthetic")
    assert want.tolist() == [1, 4, 5, 9, 11, 14, 15], want.tolist()
    # an absolute floor drops the black pixel with its tiny variance and keeps the plainly noisy ones
    want = host_and_device(trt, s, m, 2, 2, 1.0, 0.01, None, 16, "synthetic with abs_tol")
    assert 9 not in want and 11 in want and 0 not in want
    # other scales: k = 4, inv = 1 / 3; k = 1.6, inv = 0.25
    for n_cap, done in ((16, 4), (8, 5)):
        want = host_and_device(trt, s, m, n_cap, done, 0.5, 0.0, None, 16, ("synthetic", n_cap, done))
        assert 0 < len(want) < 16
    # NaN tolerances keep nothing; samples_done <= 1 keeps every candidate inside the image, in order
    assert len(host_and_device(trt, s, m, 2, 2, float("nan"), 0.0, None, 16, "NaN rel_tol")) == 0
    assert len(host_and_device(trt, s, m, 2, 2, 0.0, float("nan"), None, 16, "NaN abs_tol")) == 0
    for done in (1, 0):
        cand = np.array([3, 16, 0, 15, 99, 7], np.uint32)
        assert host_and_device(trt, s, m, 8, done, 0.5, 0.0, cand, len(cand), ("unknown variance", done)).tolist() == [3, 0, 15, 7]
        assert len(host_and_device(trt, s, m, 8, done, 0.5, 0.0, None, 16, ("unknown variance", done))) == 16


@pytest.fixture(scope="module")
def sums():
    """Random running sums of 200 000 pixels after 4 of 16 samples: S in [0, 1) / 4, M around S*S*4 on either side."""
    rng = np.random.default_rng(11)
    npixels = 200_000
    c = rng.random((npixels, 3), f32)
    s = c * f32(0.25)
    noise = rng.random((npixels, 3), f32) * f32(0.2) - f32(0.05)
    m = (c * c) * f32(0.25) * (f32(1) + noise)
    s.setflags(write=False)
    m.setflags(write=False)
    return s, m


@pytest.mark.parametrize("n", LENGTHS)
def test_list_lengths_around_the_scan_tiles(trt, sums, n):
    s, m = sums
    npixels = len(s)
    rel_tol = 0.02
    rng = np.random.default_rng(n + 1)
    # NULL: the pixels 0 .. n-1 (the last length reaches 3 * 65536 + 5 < npixels)
    want = host_and_device(trt, s, m, 16, 4, rel_tol, 0.0, None, n, ("NULL", n))
    if n >= 63:
        assert 0 < len(want) < n, (n, len(want))
    # a shuffle of distinct pixels
    cand = rng.permutation(npixels).astype(np.uint32)[:n]
    want = host_and_device(trt, s, m, 16, 4, rel_tol, 0.0, cand, n, ("shuffle", n))
    if n >= 63:
        assert 0 < len(want) < n
    # entries past the image: the first, the last, one on either side of a wave and of a tile, and a sprinkle
    bad = cand.copy()
    for i in (0, 63, 64, TILE - 1, TILE, n - 1):
        if 0 <= i < n:
            bad[i] = npixels + (i % 2) * 0x7FFFFFF0
    if n:
        bad[rng.random(n) < 0.01] = 0xFFFFFFFF
    want = host_and_device(trt, s, m, 16, 4, rel_tol, 0.0, bad, n, ("out of range", n))
    assert (want < npixels).all()


def test_selection_of_a_selection_only_shrinks(trt, sums):
    s, m = sums
    first = trt.select_pixels(s, m, 16, 4, 0.02, 0.0)
    again = trt.select_pixels(s, m, 16, 4, 0.02, 0.0, candidates=first)
    assert np.array_equal(first, again)
    tighter = trt.select_pixels(s, m, 16, 4, 0.05, 0.0, candidates=first)
    assert 0 < len(tighter) < len(first) and np.isin(tighter, first).all() and (np.diff(tighter.astype(np.int64)) > 0).all()


def test_the_oracles_cornell_moments(trt, orc):
    desc = W.scene(trt, "cornell")
    desc = dict(desc, camera=dict(desc["camera"], width=19, height=13))
    ow, ocam = orc.world_from_description(desc)
    samples = D.oracle_samples(orc, ow, ocam, 8, 8, desc["background"], 5)
    s, m = D.fold_moments(samples, 8, 0, 4)
    for rel_tol, abs_tol in ((0.1, 0.0), (0.3, 0.01), (0.05, 0.001)):
        want = host_and_device(trt, s, m, 8, 4, rel_tol, abs_tol, None, 19 * 13, ("cornell", rel_tol, abs_tol))
        print(f"\ncornell 19x13 after 4 of 8 samples, rel_tol {rel_tol}, abs_tol {abs_tol}: {len(want)} of {19 * 13} pixels kept")
        assert 0 < len(want) < 19 * 13
        cand = np.random.default_rng(3).permutation(19 * 13).astype(np.uint32)
        host_and_device(trt, s, m, 8, 4, rel_tol, abs_tol, cand, len(cand), ("cornell, shuffled", rel_tol, abs_tol))


def test_the_host_form_may_select_in_place(trt, sums):
    """selected == candidates: the host form works on device copies of its own, so a list may be shrunk in place (the device form refuses
    overlapping lists: tests/test_pixels_abi.py).  Three chunks of the second scan level long, so that many tiles write slots other tiles own."""
    import ctypes as C
    s, m = sums
    cand = np.random.default_rng(5).permutation(len(s)).astype(np.uint32)[:LENGTHS[-1]]
    want = restated_select(s, m, 16, 4, 0.02, 0.0, cand)
    assert 0 < len(want) < len(cand)
    buf = cand.copy()
    count = C.c_uint32(0xCDCDCDCD)
    trt._lib.check(trt.lib.trt_select_pixels(s.ctypes.data, m.ctypes.data, len(s), 16, 4, buf.ctypes.data, len(buf), 0.02, 0.0, buf.ctypes.data,
                                             C.byref(count)))
    assert count.value == len(want) and np.array_equal(buf[:len(want)], want), "selecting in place on the host"
    assert np.array_equal(buf[len(want):], cand[len(want):]), "written behind the selection"
