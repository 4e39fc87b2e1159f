"""The device fold of sample records (tinyrt.h trt_fold_samples, trt_fold_samples_device) on the GPU, bit for bit.

The fold alone: synthetic colours from a seeded generator - finite and order-sensitive in at least three items of four (asserted for
every shape, with the dependence on the sample order and on the records behind the first 64), NaN, +-inf and 1e30 in every eighth item,
-0 and denormals everywhere - against radiance_cases.fold (numpy f32, one IEEE operation per operator), whose fold over split ranges
tests/test_samples_cases.py holds against the fold over the whole.
The shapes (n, K) walk both regimes of the host rule (samples.hip fold_by_wave: a wave per item where R >= 64 and n <= 4096, else a lane
per item through LDS tiles of 64 items x 16 samples) and both sides of its two thresholds: R = 63 | 64 at n = 70, n = 4096 | 4097 at
R = 64; a range [3, K) moves R = K - 3 across the first threshold for K = 64 .. 67.

The identity: fold_samples_device over samples_device's records is Scene.radiance / Scene.gather, for one pass and for two ranges with
accumulate - at K = 8, where a lane folds an item, and at K = 130 for seven items, where a wave does; sh.project of the sphere /
hemisphere records is Scene.probe at bands 3.

Every f32 is compared by its bits through radiance_cases.assert_same_bits, a NaN by NaN-ness: which operand's payload and sign a NaN sum
inherits depends on the operand order the compiler gave the addition, and differs between the two regimes (seen: 0x7FC00000 against
0xFFC00000 for the same records)."""
import numpy as np
import pytest

import gather_cases as GC
import radiance_cases as R
import test_gpu_queries as G
import walk_ray_cases as W

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xCD
SHAPES = [(1, 1), (1, 700), (3, 4096), (70, 64), (70, 65), (324, 8), (5000, 16), (100003, 1),
          (70, 63), (70, 66), (70, 67), (4096, 64), (4097, 64), (65, 17), (130, 33)]


def synthetic(n, k, seed):
    """float32 [n, k, 3]: colours of ordinary size (uniform in [0, 4), one in ten scaled by 1e-3), so that a sum depends on the order of
    its terms and on every record.  One entry in sixteen of every item is -0, +0 or a denormal of either sign, which keep a sum finite.
    Item i with i % 8 == 5 carries the values that do not: one entry in eight of it is NaN, +inf, -inf or 1e30 (whose square overflows) -
    seven items in eight, and every item of a batch of five or fewer, stay finite in both sums.  From eight items on, item 0 is all -0
    and item 1 all one denormal, so that a sum stays -0 or denormal to the end."""
    g = np.random.default_rng(seed)
    c = (g.random((n, k, 3), np.float32) * np.float32(4.0)).astype(np.float32)
    c *= np.where(g.random((n, k, 3)) < 0.1, np.float32(1e-3), np.float32(1.0)).astype(np.float32)
    quiet = np.array([-0.0, 0.0, 1e-41, -3e-42], np.float32)
    pick = g.integers(0, 64, (n, k, 3))
    c = np.where(pick < 4, quiet[pick % 4], c).astype(np.float32)
    loud = np.array([np.nan, np.inf, -np.inf, 1e30], np.float32)
    pick = g.integers(0, 32, (n, k, 3))
    carries = (np.arange(n) % 8 == 5)[:, None, None]
    c = np.where(carries & (pick < 4), loud[pick % 4], c).astype(np.float32)
    if n >= 8:
        c[0], c[1] = np.float32(-0.0), np.float32(1e-41)
    c.setflags(write=False)
    return c


_SYNTH = {}


def colours(n, k):
    """The records of a shape and what makes them a test: most of the reference's channels are finite, and from two samples on the
    reference depends on the order of the samples (a fold that dropped a chunk, repeated a record or walked with another stride would
    show in numbers, not only in NaN-ness)."""
    if (n, k) not in _SYNTH:
        c = synthetic(n, k, 1000 * n + k)
        S, M = R.fold(c, k)
        finite = np.isfinite(S).all(axis=1) & np.isfinite(M).all(axis=1)
        assert finite.sum() * 8 >= n * 6, (n, k, int(finite.sum()))        # at least three items in four, all six channels
        if k >= 2:
            Sr, Mr = R.fold(np.ascontiguousarray(c[:, ::-1]), k)
            moved = (S.view(np.uint32) != Sr.view(np.uint32)).any(axis=1) | (M.view(np.uint32) != Mr.view(np.uint32)).any(axis=1)
            assert (finite & moved).sum() * 2 >= (n if k >= 16 else 1), (n, k, int((finite & moved).sum()))
        if k > 64:
            # the records behind the first 64 matter: without them most finite sums differ
            S64, _ = R.fold(c, k, 0, 64)
            assert ((S.view(np.uint32) != S64.view(np.uint32)).any(axis=1) & finite).sum() * 2 >= n, (n, k)
        _SYNTH[(n, k)] = c
    return _SYNTH[(n, k)]


def same(got, want, what):
    R.assert_same_bits(got, want, what)


@pytest.mark.parametrize("n,k", SHAPES)
def test_the_fold_alone_host_form(trt, n, k):
    c = colours(n, k)
    S, M = R.fold(c, k)
    s, m = trt.fold_samples(c, k, radiance=np.full((n, 3), 7.5, np.float32), moment2=np.full((n, 3), 7.5, np.float32))
    same(s, S, (n, k, "radiance"))
    same(m, M, (n, k, "moment2"))
    s1, none = trt.fold_samples(c, k)                                        # moment2 NULL
    assert none is None
    same(s1, s, (n, k, "without moment2"))
    if k > 3:
        # [3, K) alone, then [0, 3) continuing other sums: the order of the ranges is the caller's, the sums are the numpy fold's
        S3, M3 = R.fold(c, k, 3, k)
        s3, m3 = trt.fold_samples(c, k, 3, k, moment2=True)
        same(s3, S3, (n, k, "[3, K) radiance"))
        same(m3, M3, (n, k, "[3, K) moment2"))
        g = np.random.default_rng(n + k)
        s0, m0 = g.random((n, 3), np.float32), g.random((n, 3), np.float32)
        s0[0, 0], m0[0, 1] = np.float32(-0.0), np.float32(np.inf)
        S03, M03 = R.fold(c, k, 0, 3, s0, m0)
        sa, ma = trt.fold_samples(c, k, 0, 3, radiance=s0.copy(), moment2=m0.copy(), accumulate=True)
        same(sa, S03, (n, k, "prior sums + [0, 3) radiance"))
        same(ma, M03, (n, k, "prior sums + [0, 3) moment2"))
    # an empty range zeroes the entries, or leaves them with accumulate
    b = min(k, 2)
    z, zm = trt.fold_samples(c, k, b, b, radiance=np.full((n, 3), 7.5, np.float32), moment2=np.full((n, 3), 7.5, np.float32))
    assert (z.view(np.uint32) == 0).all() and (zm.view(np.uint32) == 0).all()
    z, zm = trt.fold_samples(c, k, b, b, radiance=np.full((n, 3), 7.5, np.float32), moment2=np.full((n, 3), 7.5, np.float32), accumulate=True)
    assert (z == 7.5).all() and (zm == 7.5).all()


def device_buffer(torch, entries, fill=FILL):
    return torch.full(((GUARD + entries + GUARD) * 12,), fill, dtype=torch.uint8, device="cuda:0")


def payload(t, n):
    h = t.cpu().numpy()
    g, b = GUARD * 12, n * 12
    return h[g:g + b].copy().view(np.float32).reshape(n, 3), bool((h[:g] == FILL).all() and (h[g + b:] == FILL).all())


@pytest.mark.parametrize("n,k", SHAPES)
def test_the_fold_alone_device_form_on_a_side_stream_leaves_the_guards(trt, n, k):
    import torch
    c = colours(n, k)
    d_c = torch.from_numpy(c.copy()).to("cuda:0")
    side = torch.cuda.Stream()
    d_s, d_m, d_s1 = device_buffer(torch, n), device_buffer(torch, n), device_buffer(torch, n)
    torch.cuda.synchronize()
    at = GUARD * 12
    trt.fold_samples_device(d_c.data_ptr(), n, k, d_s.data_ptr() + at, d_m.data_ptr() + at, stream_ptr=side.cuda_stream)
    b = 3 if k > 3 else 0
    trt.fold_samples_device(d_c.data_ptr(), n, k, d_s1.data_ptr() + at, 0, sample_begin=b, sample_end=k, stream_ptr=side.cuda_stream)
    side.synchronize()
    torch.cuda.synchronize()
    S, M = R.fold(c, k)
    s, ok_s = payload(d_s, n)
    m, ok_m = payload(d_m, n)
    s1, ok_1 = payload(d_s1, n)
    assert ok_s and ok_m and ok_1, (n, k, "guard bytes were written")
    same(s, S, (n, k, "radiance"))
    same(m, M, (n, k, "moment2"))
    same(s1, R.fold(c, k, b, k)[0], (n, k, "[3, K) without moment2"))
    assert (d_c.cpu().numpy().view(np.uint32) == c.view(np.uint32)).all()  # the colours are read only
    # accumulate continues what the buffers hold: [0, b) onto the sums of [b, K) is no fold of [0, K) in order, but it is numpy's
    if b:
        trt.fold_samples_device(d_c.data_ptr(), n, k, d_s1.data_ptr() + at, 0, sample_begin=0, sample_end=b, accumulate=True)
        torch.cuda.synchronize()
        s2, ok_2 = payload(d_s1, n)
        assert ok_2
        same(s2, R.fold(c, k, 0, b, s1, np.zeros_like(s1))[0], (n, k, "[3, K) then [0, 3)"))


def test_both_regimes_give_the_same_bytes(trt):
    """The same records on either side of a threshold: n = 4096 | 4097 items of 64 samples share their first 4096 items, R = 63 | 64 share
    the fold of their first 63 samples as a range."""
    c = colours(4097, 64)
    a, am = trt.fold_samples(np.ascontiguousarray(c[:4096]), 64, moment2=True)          # a wave per item
    b, bm = trt.fold_samples(c, 64, moment2=True)                                       # a lane per item
    same(a, np.ascontiguousarray(b[:4096]), "n = 4096 | 4097 radiance")
    same(am, np.ascontiguousarray(bm[:4096]), "n = 4096 | 4097 moment2")
    c = colours(70, 64)
    a, am = trt.fold_samples(c, 64, 0, 63, moment2=True)                                 # R = 63: a lane per item
    S, M = R.fold(c, 64, 0, 63)
    same(a, S, "R = 63")
    a, am = trt.fold_samples(c, 64, 63, 64, radiance=a, moment2=am, accumulate=True)
    b, bm = trt.fold_samples(c, 64, moment2=True)                                       # R = 64: a wave per item
    same(a, b, "R = 63 + 1 | 64 radiance")
    same(am, bm, "R = 63 + 1 | 64 moment2")


K, DEPTH, SEED, FIRST = R.K, R.MAX_BOUNCES, R.SEED, R.FIRST_STREAM
N = R.N_RAYS
IDENTITY_SCENES = ("cornell", "prims33", "random_spheres", "grid3000")


@pytest.fixture(scope="module")
def scene(trt, orc):
    cache = {}

    def get(name):
        if name not in cache:
            desc = W.scene(trt, name)
            ow, _ = orc.world_from_description(desc)
            sc = trt.world_from_description(desc)[0].get_bvh()
            assert G.plan_shape(sc.samples_plan(N, K)) == G.DEFAULT_SHAPES[name]
            cache[name] = dict(scene=sc, bg=tuple(desc["background"]), rays=R.rays_of(desc), items=GC.items_of(orc, ow, desc)[0])
        return cache[name]

    return get


@pytest.mark.parametrize("source", ("rays", "cosine", "cone"))
@pytest.mark.parametrize("name", IDENTITY_SCENES)
def test_the_fold_of_the_records_is_the_folding_query(trt, scene, name, source):
    """fold_samples_device(samples_device(...)) against Scene.radiance / Scene.gather: one pass, and ranges [0, 3) and [3, 8) - traced in
    the other order, into one record buffer - folded in order with accumulate."""
    import torch
    c = scene(name)
    sc = c["scene"]
    path = dict(max_bounces=DEPTH, background=c["bg"], seed=SEED, first_stream=FIRST)
    if source == "rays":
        items = c["rays"]
        want, want2, st = sc.radiance(items, K, moment2=True, **path)
    else:
        items = c["items"]
        want, want2, st = sc.gather(items, K, lobe=source, spread=GC.SPREAD, moment2=True, **path)
    d_items = torch.from_numpy(items.copy()).to("cuda:0")
    d_c = torch.full((N * K * 3,), float("nan"), dtype=torch.float32, device="cuda:0")
    d_s, d_m = device_buffer(torch, N), device_buffer(torch, N)
    ctr = torch.zeros(16, dtype=torch.int64, device="cuda:0")
    at = GUARD * 12
    kw = dict(samples_per_item=K, source=source, spread=GC.SPREAD, **path)
    sc.samples_device(d_items.data_ptr(), N, d_c.data_ptr(), d_counters_ptr=ctr.data_ptr(), **kw)
    trt.fold_samples_device(d_c.data_ptr(), N, K, d_s.data_ptr() + at, d_m.data_ptr() + at)
    torch.cuda.synchronize()
    s, ok_s = payload(d_s, N)
    m, ok_m = payload(d_m, N)
    assert ok_s and ok_m
    same(s, want, (name, source, "radiance"))
    same(m, want2, (name, source, "moment2"))
    assert int(ctr[0]) == st["samples"] == N * K and int(ctr[1]) == st["rays"]
    # two ranges
    d_c2 = torch.full((N * K * 3,), float("nan"), dtype=torch.float32, device="cuda:0")
    sc.samples_device(d_items.data_ptr(), N, d_c2.data_ptr(), sample_begin=3, sample_end=8, **kw)
    sc.samples_device(d_items.data_ptr(), N, d_c2.data_ptr(), sample_begin=0, sample_end=3, **kw)
    d_s2, d_m2 = device_buffer(torch, N), device_buffer(torch, N)
    trt.fold_samples_device(d_c2.data_ptr(), N, K, d_s2.data_ptr() + at, d_m2.data_ptr() + at, sample_begin=0, sample_end=3)
    trt.fold_samples_device(d_c2.data_ptr(), N, K, d_s2.data_ptr() + at, d_m2.data_ptr() + at, sample_begin=3, sample_end=8, accumulate=True)
    torch.cuda.synchronize()
    assert torch.equal(d_c2.view(torch.int32), d_c.view(torch.int32))
    s2, ok_s = payload(d_s2, N)
    m2, ok_m = payload(d_m2, N)
    assert ok_s and ok_m
    same(s2, want, (name, source, "two ranges, radiance"))
    same(m2, want2, (name, source, "two ranges, moment2"))


K_WAVE = 130


@pytest.mark.parametrize("source", ("rays", "cosine"))
@pytest.mark.parametrize("name", ("cornell", "grid3000"))
def test_the_identity_where_a_wave_folds_an_item(trt, scene, name, source):
    """Seven items of K = 130 samples: R >= 64 and n <= 4096, so a wave folds an item, in chunks of 64, 64 and 2 records - and of 64 and 2,
    then 64, for the ranges [0, 66) and [66, 130).  The sums are Scene.radiance / Scene.gather's, the paths' own finite colours."""
    c = scene(name)
    sc = c["scene"]
    path = dict(max_bounces=DEPTH, background=c["bg"], seed=SEED, first_stream=FIRST)
    n = 7
    if source == "rays":
        items = np.ascontiguousarray(c["rays"][40:40 + n])
        want, want2, st = sc.radiance(items, K_WAVE, moment2=True, **path)
    else:
        items = np.ascontiguousarray(c["items"][40:40 + n])
        want, want2, st = sc.gather(items, K_WAVE, lobe=source, moment2=True, **path)
    cols, _, st1 = sc.samples(items, K_WAVE, source=source, **path)
    assert st1["rays"] == st["rays"] and np.isfinite(want).all() and (cols != cols[:, :1]).any()
    s, m = trt.fold_samples(cols, K_WAVE, moment2=True)
    same(s, want, (name, source, "radiance"))
    same(m, want2, (name, source, "moment2"))
    s, m = trt.fold_samples(cols, K_WAVE, 0, 66, moment2=True)
    s, m = trt.fold_samples(cols, K_WAVE, 66, K_WAVE, radiance=s, moment2=m, accumulate=True)
    same(s, want, (name, source, "two ranges, radiance"))
    same(m, want2, (name, source, "two ranges, moment2"))
    # and against numpy over the same records
    S, M = R.fold(cols, K_WAVE)
    same(want, S, (name, source, "numpy"))
    same(want2, M, (name, source, "numpy, moment2"))


@pytest.mark.parametrize("domain", ("sphere", "hemisphere"))
@pytest.mark.parametrize("name", IDENTITY_SCENES)
def test_the_projection_of_the_records_is_the_probe_query(trt, scene, name, domain):
    c = scene(name)
    sc = c["scene"]
    path = dict(max_bounces=DEPTH, background=c["bg"], seed=SEED, first_stream=FIRST)
    want, st = sc.probe(c["items"], K, bands=3, domain=domain, **path)
    cols, dirs, st1 = sc.samples(c["items"], K, source=domain, directions=True, **path)
    got = trt.sh.project(cols, dirs, 3, points=c["items"][:, 0:3])
    same(got.reshape(N, -1), want.reshape(N, -1), (name, domain))
    assert st1["samples"] == st["samples"] and st1["rays"] == st["rays"]
    for bands in (1, 2):
        lead = trt.sh.project(cols, dirs, bands, points=c["items"][:, 0:3])
        same(lead.reshape(N, -1), np.ascontiguousarray(want[:, :bands * bands]).reshape(N, -1), (name, domain, bands))
