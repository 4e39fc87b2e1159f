"""The identity of tinyrt.h trt_project_samples on the GPU: project_samples_device over samples_device's colours and directions, with the
items, is Scene.probe - for one pass and for the ranges [0, 3) + [3, K) folded in order with accumulate, on four scenes and both
domains at bands 3 (K = 8: a lane folds an item), and at K = 130 for seven items, one of them with a NaN point, where a wave folds an
item in chunks of 64, 64 and 2 records.  The records are the paths' own: finite colours that differ from sample to sample.

Every f32 is compared by its bits through radiance_cases.assert_same_bits, a NaN by NaN-ness."""
import numpy as np
import pytest

import gather_cases as GC
import project_cases as P
import radiance_cases as R
import test_gpu_queries as G
import walk_ray_cases as W

pytestmark = pytest.mark.gpu

K, DEPTH, SEED, FIRST = R.K, R.MAX_BOUNCES, R.SEED, R.FIRST_STREAM
N = R.N_RAYS
GUARD = 64
FILL = 0xCD
SCENES = ("cornell", "prims33", "random_spheres", "grid3000")
DOMAINS = ("sphere", "hemisphere")


@pytest.fixture(scope="module")
def scene(trt, orc):
    cache = {}

    def get(name):
        if name not in cache:
            desc = W.scene(trt, name)
            ow, _ = orc.world_from_description(desc)
            sc = trt.world_from_description(desc)[0].get_bvh()
            assert G.plan_shape(sc.samples_plan(N, K)) == G.DEFAULT_SHAPES[name]
            items = GC.items_of(orc, ow, desc)[0]
            assert np.isnan(items[:, 0:3]).any(axis=1).sum() == 1
            cache[name] = dict(scene=sc, items=items, path=dict(max_bounces=DEPTH, background=tuple(desc["background"]), seed=SEED, first_stream=FIRST))
        return cache[name]

    return get


def same(got, want, what):
    R.assert_same_bits(np.ascontiguousarray(got).reshape(len(want), -1), np.ascontiguousarray(want).reshape(len(want), -1), what)


def device_buffer(torch, entries):
    return torch.full(((GUARD + entries + GUARD) * 12,), FILL, dtype=torch.uint8, device="cuda:0")


def payload(t, n, coeffs):
    h = t.cpu().numpy()
    g, b = GUARD * 12, n * coeffs * 12
    return h[g:g + b].copy().view(np.float32).reshape(n, coeffs, 3), bool((h[:g] == FILL).all() and (h[g + b:] == FILL).all())


@pytest.mark.parametrize("domain", DOMAINS)
@pytest.mark.parametrize("name", SCENES)
def test_the_projection_of_the_records_is_the_probe_query(trt, scene, name, domain):
    import torch
    c = scene(name)
    sc, items, path = c["scene"], c["items"], c["path"]
    want, st = sc.probe(items, K, bands=3, domain=domain, **path)
    assert np.count_nonzero(want) > 0
    d_items = torch.from_numpy(items.copy()).to("cuda:0")
    d_c = torch.full((N * K * 3,), float("nan"), dtype=torch.float32, device="cuda:0")
    d_d = torch.full((N * K * 3,), float("nan"), dtype=torch.float32, device="cuda:0")
    d_sh = device_buffer(torch, N * 9)
    ctr = torch.zeros(16, dtype=torch.int64, device="cuda:0")
    at = GUARD * 12
    kw = dict(samples_per_item=K, source=domain, **path)
    sc.samples_device(d_items.data_ptr(), N, d_c.data_ptr(), d_d.data_ptr(), d_counters_ptr=ctr.data_ptr(), **kw)
    trt.project_samples_device(d_c.data_ptr(), d_d.data_ptr(), N, K, d_sh.data_ptr() + at, d_items_ptr=d_items.data_ptr())
    torch.cuda.synchronize()
    got, ok = payload(d_sh, N, 9)
    assert ok
    same(got, want, (name, domain))
    assert int(ctr[0]) == st["samples"] == N * K and int(ctr[1]) == st["rays"]
    # two ranges, traced in the other order into one pair of record buffers, folded in order with accumulate
    d_c2, d_d2 = torch.full_like(d_c, float("nan")), torch.full_like(d_d, float("nan"))
    sc.samples_device(d_items.data_ptr(), N, d_c2.data_ptr(), d_d2.data_ptr(), sample_begin=3, sample_end=K, **kw)
    sc.samples_device(d_items.data_ptr(), N, d_c2.data_ptr(), d_d2.data_ptr(), sample_begin=0, sample_end=3, **kw)
    d_sh2 = device_buffer(torch, N * 9)
    trt.project_samples_device(d_c2.data_ptr(), d_d2.data_ptr(), N, K, d_sh2.data_ptr() + at, sample_begin=0, sample_end=3, d_items_ptr=d_items.data_ptr())
    trt.project_samples_device(d_c2.data_ptr(), d_d2.data_ptr(), N, K, d_sh2.data_ptr() + at, sample_begin=3, sample_end=K, accumulate=True,
                               d_items_ptr=d_items.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(d_c2.view(torch.int32), d_c.view(torch.int32)) and torch.equal(d_d2.view(torch.int32), d_d.view(torch.int32))
    got2, ok = payload(d_sh2, N, 9)
    assert ok
    same(got2, want, (name, domain, "two ranges"))
    # ... and sh.project over the same records agrees with both
    cols, dirs = d_c.cpu().numpy().reshape(N, K, 3), d_d.cpu().numpy().reshape(N, K, 3)
    same(trt.sh.project(cols, dirs, 3, points=items[:, 0:3]), want, (name, domain, "numpy"))


K_WAVE = 130


@pytest.mark.parametrize("domain", DOMAINS)
@pytest.mark.parametrize("name", ("cornell", "grid3000"))
def test_the_identity_where_a_wave_folds_an_item(trt, scene, name, domain):
    """Seven items of K = 130 samples: R >= 64 and n <= 4096, so a wave folds an item, in chunks of 64, 64 and 2 records - and of 64 and 2,
    then 64, for the ranges [0, 66) and [66, 130).  One of the seven has a NaN point: its row stays +0, or keeps its prior words."""
    c = scene(name)
    sc, path = c["scene"], c["path"]
    n = 7
    assert P.by_wave(n, K_WAVE) and P.by_wave(n, 66) and P.by_wave(n, K_WAVE - 66)
    items = np.ascontiguousarray(c["items"][40:40 + n]).copy()
    items[4, 1] = np.nan
    want, st = sc.probe(items, K_WAVE, bands=3, domain=domain, **path)
    cols, dirs, st1 = sc.samples(items, K_WAVE, source=domain, directions=True, **path)
    assert st1["rays"] == st["rays"] and st1["samples"] == st["samples"] == n * K_WAVE
    live = np.arange(n) != 4
    assert np.isfinite(want).all() and (cols[live] != cols[live, :1]).any() and (want[4].view(np.uint32) == 0).all()
    assert np.count_nonzero(want[live]) > 0
    got = trt.project_samples(cols, dirs, items=items)
    same(got, want, (name, domain))
    head = trt.project_samples(cols, dirs, sample_begin=0, sample_end=66, items=items)
    both = trt.project_samples(cols, dirs, sample_begin=66, sample_end=K_WAVE, sh=head, accumulate=True, items=items)
    same(both, want, (name, domain, "two ranges"))
    for bands in (1, 2):
        lead = trt.project_samples(cols, dirs, bands=bands, items=items)
        same(lead, np.ascontiguousarray(want[:, :bands * bands]), (name, domain, bands))
    # the NaN-point item keeps prior words; the others continue them as numpy does
    prior = P.prior_sums(n, 9, 130)
    prior.view(np.uint32)[4, 0] = (0x80000000, 0x7FC12345, 0x7F800000)
    cont = trt.project_samples(cols, dirs, sh=prior.copy(), accumulate=True, items=items)
    assert cont[4].tobytes() == prior[4].tobytes()
    same(cont, trt.sh.project(cols, dirs, 3, sh=prior, points=items[:, 0:3]), (name, domain, "prior sums"))
    # and against numpy over the same records
    same(want, trt.sh.project(cols, dirs, 3, points=items[:, 0:3]), (name, domain, "numpy"))
