"""The pieces of the sample queries that need no GPU.

  * csrc/sample_index.h - the work index q -> (item, sample) of samples.hip and the row of the tile fold - compiled alone with
    tests/native/sample_index_check.cpp, a stand-alone program, and held against 64-bit division (R = 1, 2, 3, 5, 63 .. 65, 255 .. 257,
    2^16 -+ 1, 2^31, 2^32 - 1; q = 0, R - 1, R and the multiples of R nearest 2^31 and 2^32 - 1, each -+ 1, clipped to n * R).
  * sh.project over the oracle's probe rays and colours (probe_cases.oracle_probe) is probe_cases.fold, by bits, for both domains and
    bands 1 - 3, over the whole range and over split ranges; the NaN-point rule needs the `points` argument.
  * A numpy fold of the oracle's colours over split ranges is radiance_cases.fold over the whole: the reference the GPU tests of the fold
    use (tests/test_gpu_samples_fold.py), shown not vacuous - the splits matter, the order matters, the colours differ."""
import os
import subprocess

import numpy as np
import pytest

import gather_cases as GC
import probe_cases as PC
import radiance_cases as R
import walk_ray_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = PC.K


def test_the_work_index_against_64_bit_division(tmp_path):
    exe = str(tmp_path / "sample_index_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "tiny-raytracer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "sample_index_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok all" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.fixture(scope="module")
def reference(trt, orc):
    """cornell: the items, and per probe domain / gather lobe the oracle's first rays [n, K, 6] and colours [n, K, 3]; computed once."""
    desc = W.scene(trt, "cornell")
    ow, _ = orc.world_from_description(desc)
    items, _ = GC.items_of(orc, ow, desc)
    bg = tuple(desc["background"])
    ref = dict(items=items)
    for domain in PC.DOMAINS:
        rays, cols, _, _, _ = PC.oracle_probe(orc, ow, items, domain, K, PC.MAX_BOUNCES, bg, PC.SEED, PC.FIRST_STREAM)
        ref[domain] = (rays, cols)
    rays, cols, _ = GC.oracle_gather(orc, ow, items, "cosine", K, GC.MAX_BOUNCES, bg, GC.SEED, GC.FIRST_STREAM)
    ref["cosine"] = (rays, cols)
    for a in [items] + [x for k in ("sphere", "hemisphere", "cosine") for x in ref[k]]:
        a.setflags(write=False)
    return ref


@pytest.mark.parametrize("bands", (1, 2, 3))
@pytest.mark.parametrize("domain", PC.DOMAINS)
def test_project_is_the_probe_fold(trt, reference, domain, bands):
    rays, cols = reference[domain]
    dirs = np.ascontiguousarray(rays[:, :, 3:6])
    points = reference["items"][:, 0:3]
    want = PC.fold(trt.sh.basis, rays, cols, K, bands)
    got = trt.sh.project(cols, dirs, bands, points=points)
    assert got.dtype == np.float32 and got.shape == (len(cols), bands * bands, 3)
    R.assert_same_bits(got.reshape(len(got), -1), want.reshape(len(want), -1), (domain, bands))
    # split ranges, continued from `sh` (which is not changed)
    head = trt.sh.project(cols, dirs, bands, 0, 3, points=points)
    R.assert_same_bits(head.reshape(len(head), -1), PC.fold(trt.sh.basis, rays, cols, K, bands, 0, 3).reshape(len(head), -1), (domain, bands, "[0, 3)"))
    keep = head.copy()
    both = trt.sh.project(cols, dirs, bands, 3, None, sh=head, points=points)
    assert head.tobytes() == keep.tobytes()
    R.assert_same_bits(both.reshape(len(both), -1), want.reshape(len(want), -1), (domain, bands, "[0, 3) + [3, 8)"))
    # not vacuous: the sums are not all zero, a NaN point's item adds nothing only when the points are given, and the order matters
    assert np.count_nonzero(want) > want.size // 4
    nan_point = np.flatnonzero(np.isnan(points).any(axis=1))
    assert len(nan_point) == 1 and (want[nan_point] == 0).all()
    blind = trt.sh.project(cols, dirs, bands)
    assert not (blind[nan_point] == 0).all()
    swapped = trt.sh.project(cols[:, ::-1], dirs[:, ::-1], bands, points=points)
    assert (swapped.view(np.uint32) != want.view(np.uint32)).any()


def numpy_fold(cols, k, ranges):
    """The reference of the GPU tests: radiance_cases.fold range by range, each continuing the sums of the last."""
    s = m = None
    for b, e in ranges:
        s, m = R.fold(cols, k, b, e, s, m)
    return s, m


def test_a_fold_over_split_ranges_is_the_fold_over_the_whole(reference):
    _, cols = reference["cosine"]
    S, M = R.fold(cols, K)
    for ranges in ([(0, 3), (3, 8)], [(0, 1), (1, 2), (2, 8)], [(0, 8), (8, 8)], [(0, 0), (0, 8)]):
        s, m = numpy_fold(cols, K, ranges)
        R.assert_same_bits(s, S, ("radiance", ranges))
        R.assert_same_bits(m, M, ("moment2", ranges))
    # not vacuous: a range left out, ranges in another order or another K change bits
    lit = np.flatnonzero((cols != 0).any(axis=(1, 2)))
    assert len(lit) > len(cols) // 2
    s, _ = numpy_fold(cols, K, [(0, 3), (4, 8)])
    assert (s.view(np.uint32) != S.view(np.uint32)).any()
    s, _ = numpy_fold(cols, K, [(3, 8), (0, 3)])
    assert (s.view(np.uint32) != S.view(np.uint32)).any()
    s, _ = numpy_fold(cols, K + 1, [(0, 8)])
    assert (s.view(np.uint32) != S.view(np.uint32)).any()
    # the samples of an item differ, so a fold that read one record K times would show
    assert (cols[lit, 0] != cols[lit, 1]).any()
