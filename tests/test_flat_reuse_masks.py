"""The reuse schedule of the lock-step leaf walk (tiny-raytracer_amd/csrc/flat_reuse.h), without a GPU: the host derivation compiled
with g++ and driven on synthetic leaf lists (signed zeros, NaN, inf, padding, length limit, switched off) and on Cornell's leaf list."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tiny-raytracer_amd", "csrc")

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "flat_reuse.h"
int main(int, char** argv) {
    std::vector<unsigned char> b;
    if (FILE* f = fopen(argv[1], "rb")) { int c; while ((c = fgetc(f)) != EOF) b.push_back((unsigned char)c); fclose(f); }
    uint32_t m[3];
    trt::flat_reuse_masks(b.empty() ? nullptr : b.data(), (uint32_t)strtoul(argv[2], nullptr, 10), atoi(argv[3]) != 0, m);
    printf("%u %u %u\n", m[0], m[1], m[2]);
    return 0;
}
"""


@pytest.fixture(scope="module")
def masks_of(tmp_path_factory):
    d = tmp_path_factory.mktemp("flat_reuse")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, str(src), "-o", str(exe)], check=True)
    count = [0]

    def run(leaves, n=None, enabled=True):
        """leaves: (k, 6) float32 boxes (lo.x lo.y lo.z hi.x hi.y hi.z) in walk order; n: n_leaves passed (default k)."""
        box = np.asarray(leaves, np.float32).reshape(-1, 6)
        k = len(box)
        words = np.zeros((k, 8), np.uint32)
        words[:, :6] = box.view(np.uint32)
        words[:, 6] = np.arange(1, k + 1)
        words[:, 7] = np.arange(k) | 0x40000000
        count[0] += 1
        f = d / ("leaves%d.bin" % count[0])
        f.write_bytes(words.tobytes())
        out = subprocess.run([str(exe), str(f), str(k if n is None else n), "1" if enabled else "0"], capture_output=True, text=True, check=True)
        return tuple(int(v) for v in out.stdout.split())
    return run


BOX = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]


def test_identical_leaves_reuse_every_axis_but_the_first(masks_of):
    assert masks_of([BOX] * 5) == (0b11110, 0b11110, 0b11110)


def test_bit_zero_is_always_clear_and_one_leaf_has_no_bits(masks_of):
    assert masks_of([BOX]) == (0, 0, 0)
    assert all(m & 1 == 0 for m in masks_of([BOX] * 32))


def test_axes_are_independent_and_need_both_planes(masks_of):
    a = list(BOX)
    b = list(BOX); b[0] = 1.5                    # x: lo differs
    c = list(b); c[4] = 7.0                      # y: hi differs
    assert masks_of([a, b, c]) == (0b100, 0b010, 0b110)


def test_signed_zero_planes_do_not_merge(masks_of):
    p, m = [0.0, 0.0, 0.0, 1.0, 1.0, 1.0], [-0.0, 0.0, 0.0, 1.0, 1.0, 1.0]
    assert masks_of([p, m]) == (0, 0b10, 0b10)
    q = [0.0, 0.0, -1.0, 1.0, 1.0, -0.0]
    r = [0.0, 0.0, -1.0, 1.0, 1.0, 0.0]
    assert masks_of([q, r, r]) == (0b110, 0b110, 0b100)


def test_nan_and_inf_coordinates_are_never_reused(masks_of):
    nan, inf = float("nan"), float("inf")
    for bad in (nan, inf, -inf):
        for axis in range(3):
            for plane in (axis, axis + 3):
                box = list(BOX)
                box[plane] = bad
                got = masks_of([box] * 4)          # bit-identical NaN / inf planes
                want = [0b1110] * 3
                want[axis] = 0
                assert got == tuple(want), (bad, axis, plane)


def test_no_bits_at_or_beyond_n_leaves(masks_of):
    leaves = [BOX] * 9                           # e.g. the list's padding: copies of the last leaf
    assert masks_of(leaves, n=5) == (0b11110, 0b11110, 0b11110)
    assert masks_of(leaves, n=0) == (0, 0, 0)


def test_longer_lists_than_a_mask_holds_get_none(masks_of):
    assert masks_of([BOX] * 33) == (0, 0, 0)
    assert masks_of([BOX] * 32) == (0xFFFFFFFE,) * 3


def test_disabled_gives_zero_masks(masks_of):
    assert masks_of([BOX] * 6, enabled=False) == (0, 0, 0)


def reuse_numpy(box):
    """The schedule restated: bit i of axis k iff leaf i's (lo_k, hi_k) bits equal leaf i-1's, both finite."""
    w = np.asarray(box, np.float32).reshape(-1, 6).view(np.uint32)
    fin = (w & 0x7F800000) != 0x7F800000
    out = []
    for k in range(3):
        m = 0
        for i in range(1, len(w)):
            if w[i, k] == w[i - 1, k] and w[i, k + 3] == w[i - 1, k + 3] and fin[i, k] and fin[i, k + 3]:
                m |= 1 << i
        out.append(m)
    return tuple(out)


def test_cornell_leaf_list(trt, masks_of):
    """Cornell's 18 leaves in walk order (the reference tree's leaves in pre-order, which the packed leaf list holds):
    15 of its 54 per-axis intervals are the previous leaf's."""
    s = trt.Scene(trt.world_from_description(trt.scenes.cornell(64, 64))[0])
    box, prim, _ = s.nodes()
    leaves = box[prim >= 0]
    assert len(leaves) == 18
    m = masks_of(leaves)
    assert m == reuse_numpy(leaves)
    assert sum(bin(v).count("1") for v in m) == 15
