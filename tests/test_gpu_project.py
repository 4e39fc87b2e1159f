"""The probe fold of sample records (tinyrt.h trt_project_samples, trt_project_samples_device) on the GPU, bit for bit, on its own.

Synthetic records (project_cases.py: colours of test_gpu_samples_fold.synthetic, f32-normalised Gaussian directions with NaN components
in items i % 4 == 2, NaN points in items i % 8 == 3; finite and order-sensitive in most items, asserted per shape in
tests/test_project_cases.py) against sh.project (numpy f32, one IEEE operation per operator), which tests/test_project_cases.py holds
against probe_cases.fold.  The shapes (n, K) walk both regimes of the host rule (project.hip project_by_wave: a wave per item where
R >= 64 and n <= 4096, else a lane per item through LDS tiles of 64 items x 8 samples) and both sides of its two thresholds:
R = 63 | 64 | 65 at n = 70, n = 4096 | 4097 at R = 64; the range [3, K) moves R = K - 3 across the first threshold for K = 65.

Every f32 is compared by its bits through radiance_cases.assert_same_bits, a NaN by NaN-ness - except where "keeps its prior bits" is
the claim (an item no sample of the range folds into): there the raw words are compared."""
import numpy as np
import pytest

import project_cases as P
import radiance_cases as R

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xCD


def same(got, want, what):
    n = len(want)
    R.assert_same_bits(np.ascontiguousarray(got).reshape(n, -1), np.ascontiguousarray(want).reshape(n, -1), what)


def same_words(got, want, rows, what):
    assert (got[rows].view(np.uint32) == want[rows].view(np.uint32)).all(), what


@pytest.mark.parametrize("n,k", P.SHAPES)
def test_the_projection_alone_host_form(trt, n, k):
    rec = P.records(trt, n, k)
    c, d, items = rec["c"], rec["d"], rec["items"]
    points = items[:, 0:3]
    got = {}
    for bands in (3, 2, 1):
        coeffs = bands * bands
        got[bands] = trt.project_samples(c, d, bands=bands, items=items, sh=np.full((n, coeffs, 3), 7.5, np.float32))
        want = rec["S"] if bands == 3 else trt.sh.project(c, d, bands, points=points)
        same(got[bands], want, (n, k, bands))
        # the bytes of coefficient k do not depend on `bands`
        same(got[bands], np.ascontiguousarray(got[3][:, :coeffs]), (n, k, bands, "against bands 3"))
    same_words(got[3], np.zeros_like(got[3]), rec["dead"], (n, k, "NaN-point items are +0"))
    # without the items the NaN points are not seen
    blind = trt.project_samples(c, d)
    same(blind, trt.sh.project(c, d, 3), (n, k, "items = NULL"))
    if k > 3:
        # [3, K) alone, then [0, 3) continuing other sums that hold -0, inf and a NaN: the order of the ranges is the caller's
        tail = trt.project_samples(c, d, sample_begin=3, sample_end=k, items=items)
        same(tail, trt.sh.project(c, d, 3, 3, k, points=points), (n, k, "[3, K)"))
        for bands in (3, 2):
            prior = P.prior_sums(n, bands * bands, n + k)
            head = trt.project_samples(c, d, bands=bands, sample_begin=0, sample_end=3, sh=prior.copy(), accumulate=True, items=items)
            same(head, trt.sh.project(c, d, bands, 0, 3, sh=prior, points=points), (n, k, bands, "prior sums + [0, 3)"))
            # an item none of whose samples folds keeps the words it had: -0 stays -0, a NaN keeps its payload
            kept = P.no_sample_folds(rec, 0, 3)
            assert kept.sum() >= rec["dead"].sum()
            same_words(head, prior, kept, (n, k, bands, "prior words kept"))
        both = trt.project_samples(c, d, sample_begin=0, sample_end=3, sh=tail.copy(), accumulate=True, items=items)
        same(both, trt.sh.project(c, d, 3, 0, 3, sh=tail, points=points), (n, k, "[3, K) then [0, 3)"))
    else:
        prior = P.prior_sums(n, 9, n + k)
        head = trt.project_samples(c, d, sh=prior.copy(), accumulate=True, items=items)
        same(head, trt.sh.project(c, d, 3, sh=prior, points=points), (n, k, "prior sums + [0, K)"))
        same_words(head, prior, P.no_sample_folds(rec, 0, k), (n, k, "prior words kept"))
    # an empty range zeroes the entries, or leaves them with accumulate
    b = min(k, 2)
    z = trt.project_samples(c, d, sample_begin=b, sample_end=b, sh=np.full((n, 9, 3), 7.5, np.float32), items=items)
    assert (z.view(np.uint32) == 0).all()
    prior = P.prior_sums(n, 4, 3)
    z = trt.project_samples(c, d, bands=2, sample_begin=b, sample_end=b, sh=prior.copy(), accumulate=True, items=items)
    assert z.tobytes() == prior.tobytes()


def device_buffer(torch, entries):
    return torch.full(((GUARD + entries + GUARD) * 12,), FILL, dtype=torch.uint8, device="cuda:0")


def payload(t, n, coeffs):
    h = t.cpu().numpy()
    g, b = GUARD * 12, n * coeffs * 12
    return h[g:g + b].copy().view(np.float32).reshape(n, coeffs, 3), bool((h[:g] == FILL).all() and (h[g + b:] == FILL).all())


@pytest.mark.parametrize("n,k", P.SHAPES)
def test_the_projection_alone_device_form_on_a_side_stream_leaves_the_guards(trt, n, k):
    import torch
    rec = P.records(trt, n, k)
    c, d, items = rec["c"], rec["d"], rec["items"]
    points = items[:, 0:3]
    d_c, d_d, d_i = (torch.from_numpy(a.copy()).to("cuda:0") for a in (c, d, items))
    side = torch.cuda.Stream()
    out = {bands: device_buffer(torch, n * bands * bands) for bands in (1, 2, 3)}
    d_tail, d_blind = device_buffer(torch, n * 9), device_buffer(torch, n * 9)
    torch.cuda.synchronize()
    at = GUARD * 12
    for bands in (1, 2, 3):
        trt.project_samples_device(d_c.data_ptr(), d_d.data_ptr(), n, k, out[bands].data_ptr() + at, bands=bands, d_items_ptr=d_i.data_ptr(),
                                   stream_ptr=side.cuda_stream)
    b = 3 if k > 3 else 0
    trt.project_samples_device(d_c.data_ptr(), d_d.data_ptr(), n, k, d_tail.data_ptr() + at, sample_begin=b, sample_end=k, d_items_ptr=d_i.data_ptr(),
                               stream_ptr=side.cuda_stream)
    trt.project_samples_device(d_c.data_ptr(), d_d.data_ptr(), n, k, d_blind.data_ptr() + at, stream_ptr=side.cuda_stream)      # items = NULL
    side.synchronize()
    torch.cuda.synchronize()
    got3, ok = payload(out[3], n, 9)
    assert ok, (n, k, "guard bytes were written")
    same(got3, rec["S"], (n, k, 3))
    for bands in (1, 2):
        got, ok = payload(out[bands], n, bands * bands)
        assert ok, (n, k, bands, "guard bytes were written")
        same(got, trt.sh.project(c, d, bands, points=points), (n, k, bands))
        same(got, np.ascontiguousarray(got3[:, :bands * bands]), (n, k, bands, "against bands 3"))
    tail, ok_t = payload(d_tail, n, 9)
    blind, ok_b = payload(d_blind, n, 9)
    assert ok_t and ok_b
    same(tail, trt.sh.project(c, d, 3, b, k, points=points), (n, k, "[3, K)"))
    same(blind, trt.sh.project(c, d, 3), (n, k, "items = NULL"))
    # the record buffers and the items are read only
    for dev, host in ((d_c, c), (d_d, d), (d_i, items)):
        assert (dev.cpu().numpy().view(np.uint32) == host.view(np.uint32)).all()
    if b:
        # accumulate continues what the buffer holds
        trt.project_samples_device(d_c.data_ptr(), d_d.data_ptr(), n, k, d_tail.data_ptr() + at, sample_begin=0, sample_end=b, accumulate=True,
                                   d_items_ptr=d_i.data_ptr())
        torch.cuda.synchronize()
        both, ok = payload(d_tail, n, 9)
        assert ok
        same(both, trt.sh.project(c, d, 3, 0, b, sh=tail, points=points), (n, k, "[3, K) then [0, 3)"))
    # an empty range with accumulate touches nothing; without, it zeroes [0, 12 C n) and no byte more
    e = min(k, 2)
    trt.project_samples_device(d_c.data_ptr(), d_d.data_ptr(), n, k, d_blind.data_ptr() + at, sample_begin=e, sample_end=e, accumulate=True)
    trt.project_samples_device(d_c.data_ptr(), d_d.data_ptr(), n, k, out[2].data_ptr() + at, bands=2, sample_begin=e, sample_end=e)
    torch.cuda.synchronize()
    again, ok_a = payload(d_blind, n, 9)
    zero, ok_z = payload(out[2], n, 4)
    assert ok_a and ok_z and again.tobytes() == blind.tobytes() and (zero.view(np.uint32) == 0).all()


def test_both_regimes_give_the_same_bytes(trt):
    """The same records on either side of a threshold: n = 4096 | 4097 items of 64 samples share their first 4096 items, R = 63 | 64 share
    the fold of their first 63 samples as a range."""
    rec = P.records(trt, 4097, 64)
    c, d, items = rec["c"], rec["d"], rec["items"]
    assert P.by_wave(4096, 64) and not P.by_wave(4097, 64) and not P.by_wave(70, 63)
    a = trt.project_samples(np.ascontiguousarray(c[:4096]), np.ascontiguousarray(d[:4096]), items=np.ascontiguousarray(items[:4096]))       # a wave per item
    b = trt.project_samples(c, d, items=items)                                                                                              # a lane per item
    same(a, np.ascontiguousarray(b[:4096]), "n = 4096 | 4097")
    rec = P.records(trt, 70, 64)
    c, d, items = rec["c"], rec["d"], rec["items"]
    for bands in (1, 2, 3):
        a = trt.project_samples(c, d, bands=bands, sample_begin=0, sample_end=63, items=items)      # R = 63: a lane per item
        same(a, trt.sh.project(c, d, bands, 0, 63, points=items[:, 0:3]), ("R = 63", bands))
        a = trt.project_samples(c, d, bands=bands, sample_begin=63, sample_end=64, sh=a, accumulate=True, items=items)
        b = trt.project_samples(c, d, bands=bands, items=items)                                    # R = 64: a wave per item
        same(a, b, ("R = 63 + 1 | 64", bands))
