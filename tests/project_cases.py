"""What tests/test_project_cases.py and tests/test_gpu_project.py share, none of it touching a GPU: the synthetic sample records the
projection alone is tested on, the conditions that make them a test, and the numpy reference (tiny-raytracer_amd/sh.py project).

Colours: test_gpu_samples_fold.synthetic - ordinary sizes, -0 and denormals everywhere, NaN / inf / 1e30 in items i % 8 == 5, item 0
all -0 and item 1 all one denormal from eight items on.  Directions: f32-normalised Gaussian vectors; one sample in 16 of items
i % 4 == 2 has one NaN component.  Items i % 8 == 3 have a NaN point (one component, cycling); the others' points and every axis are
ordinary numbers the projection never reads.

The shapes (n, K) walk both regimes of the host rule (project.hip project_by_wave: a wave per item where R >= 64 and n <= 4096, else a
lane per item through LDS tiles of 64 items x 8 samples) and both sides of its two thresholds."""
import numpy as np

import test_gpu_samples_fold as F

f32 = np.float32
SHAPES = [(1, 1), (1, 700), (3, 4096), (70, 63), (70, 64), (70, 65), (65, 17), (130, 33), (324, 8), (5000, 16), (100003, 1), (4096, 64),
          (4097, 64)]
WAVE_MIN_RANGE, WAVE_MAX_ITEMS = 64, 4096                                   # project.hip kProjectWaveMinRange, kProjectWaveMaxItems


def by_wave(n, r):
    return r >= WAVE_MIN_RANGE and n <= WAVE_MAX_ITEMS


def synthetic(n, k):
    """(colours [n, k, 3], directions [n, k, 3], items [n, 6]), float32, read-only."""
    c = F.synthetic(n, k, 1000 * n + k)
    g = np.random.default_rng(7000 * n + k + 1)
    d = g.standard_normal((n, k, 3)).astype(f32)
    d = (d / np.sqrt((d * d).sum(axis=2, dtype=f32), dtype=f32)[:, :, None]).astype(f32)
    item = np.arange(n)
    hit = (g.integers(0, 16, (n, k)) == 0) & (item % 4 == 2)[:, None]
    comp = g.integers(0, 3, (n, k))
    d = np.where(hit[:, :, None] & (comp[:, :, None] == np.arange(3)), f32(np.nan), d).astype(f32)
    items = g.standard_normal((n, 6)).astype(f32)
    dead = np.flatnonzero(item % 8 == 3)
    items[dead, (dead // 8) % 3] = np.nan
    for a in (d, items):
        a.setflags(write=False)
    return c, d, items


_RECORDS = {}


def records(trt, n, k):
    """The records of a shape, the reference over the whole range at bands 3 with the items, and what makes them a test; computed once."""
    if (n, k) not in _RECORDS:
        c, d, items = synthetic(n, k)
        points = items[:, 0:3]
        S = trt.sh.project(c, d, 3, points=points)
        flat = S.reshape(n, 27)
        finite = np.isfinite(flat).all(axis=1)
        assert finite.sum() * 4 >= n * 3, (n, k, int(finite.sum()))        # at least three items in four, all 27 sums
        moved = np.zeros(n, bool)
        if k >= 2:
            Sr = trt.sh.project(np.ascontiguousarray(c[:, ::-1]), np.ascontiguousarray(d[:, ::-1]), 3, points=points)
            moved = (flat.view(np.uint32) != Sr.reshape(n, 27).view(np.uint32)).any(axis=1)
        if k >= 16:
            assert (finite & moved).sum() * 2 >= n, (n, k, int((finite & moved).sum()))
        dead = np.isnan(points).any(axis=1)
        assert dead.sum() == len(np.flatnonzero(np.arange(n) % 8 == 3))
        assert (flat[dead].view(np.uint32) == 0).all()                      # NaN-point items are all +0
        S.setflags(write=False)
        _RECORDS[(n, k)] = dict(c=c, d=d, items=items, S=S, finite=int(finite.sum()), moved=int((finite & moved).sum()), dead=dead)
    return _RECORDS[(n, k)]


def no_sample_folds(rec, begin, end):
    """bool [n]: the items none of whose samples of [begin, end) folds - a NaN point, or a NaN in every direction of the range."""
    return rec["dead"] | np.isnan(rec["d"][:, begin:end]).any(axis=2).all(axis=1)


def prior_sums(n, coeffs, seed):
    """float32 [n, coeffs, 3] to continue: ordinary numbers; item 0 and the items i % 4 == 2 and i % 8 == 3 (the ones with NaN directions
    and NaN points) hold -0, +inf and a NaN with a payload in their first coefficient, cycling over the channels - so that an item no
    sample touches has words to keep."""
    g = np.random.default_rng(seed)
    s = g.random((n, coeffs, 3), f32)
    w = s.view(np.uint32)
    i = np.arange(n)
    i = i[(i == 0) | (i % 4 == 2) | (i % 8 == 3)]
    w[i, 0, i % 3] = 0x80000000                                             # -0
    w[i, 0, (i + 1) % 3] = 0x7F800000                                       # +inf
    w[i, 0, (i + 2) % 3] = 0x7FC12345                                       # a NaN with a payload
    return s
