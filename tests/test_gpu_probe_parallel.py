"""The K-aware probe query (tinyrt.h trt_probe_parallel, trt_probe_parallel_device) on the GPU against Scene.probe: the sums, `samples`
and `rays` are trt_probe's, bit for bit, for the same arguments - whatever the record buffer makes of the chunks.

The 324 items of gather_cases.items_of (a NaN point, a zero axis and an axis with an inf among them), K = 8, max_bounces = 8, seed 5,
first_stream = 1000.  The scenes are the four of the identity tests plus the two compilations that reach the remaining sample-kernel
shapes; each case asserts the shape Scene.probe_parallel_plan reports, so all six instantiations of samples.hip run behind the
projection.  record_bytes gives one item per chunk (324 chunks), three chunks with a ragged last (120, 120, 84) and one chunk.

Every f32 is compared by its bits through radiance_cases.assert_same_bits, a NaN by NaN-ness.

The long cases at the end: chunks past one workgroup of samples (n x R > 256 x 64), folded a wave per item (R = 64) and a lane per item
over more than one workgroup (R = 60, 324 items)."""
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
ITEM = 24 * K                                                               # bytes of records one item needs
CASES = [("cornell", {}), ("prims33", {}), ("random_spheres", {}), ("grid3000", {}), ("prims600", {}), ("grid3000", dict(compact_nodes=0))]
SHAPES = [G.DEFAULT_SHAPES[name] if not options else next(s for n, o, s in G.OTHER_WALKS if n == name and o == options) for name, options in CASES]
assert len({s[:3] for s in SHAPES}) == 6                                    # every entry of samples.hip kSamplesKernels
IDS = ["%s-%s" % (name, "-".join("%s=%s" % kv for kv in sorted(options.items())) or "default") for name, options in CASES]
DOMAINS = ("sphere", "hemisphere")
every_case = pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
RECORD_BYTES = {"one item per chunk": ITEM + 5, "three chunks, ragged": 120 * ITEM + ITEM - 1, "one chunk": N * ITEM, "default": 0}


@pytest.fixture(scope="module")
def case(trt, orc):
    """index, domain -> the compiled scene (its shape asserted), the items, the path keywords and Scene.probe's answer at bands 3: the
    reference, computed once per case and domain and never changed."""
    scenes, cache = {}, {}

    def get(index, domain):
        name, options = CASES[index]
        if index not in scenes:
            desc = W.scene(trt, name)
            ow, _ = orc.world_from_description(desc)
            sc = trt.world_from_description(desc)[0].get_bvh(**options)
            for n, r in ((N, K), (1, K), (120, 5)):
                assert G.plan_shape(sc.probe_parallel_plan(n, r)) == SHAPES[index], (name, options)
            items = GC.items_of(orc, ow, desc)[0]
            assert np.isnan(items[:, 0:3]).any(axis=1).sum() == 1
            items.setflags(write=False)
            scenes[index] = dict(scene=sc, items=items, path=dict(max_bounces=DEPTH, background=tuple(desc["background"]), seed=SEED, first_stream=FIRST))
        if (index, domain) not in cache:
            s = scenes[index]
            want, st = s["scene"].probe(s["items"], K, bands=3, domain=domain, **s["path"])
            assert np.count_nonzero(want) > 0 and st["samples"] == N * K
            want.setflags(write=False)
            cache[(index, domain)] = dict(s, want=want, st=st)
        return cache[(index, domain)]

    return get


def same(got, want, what):
    R.assert_same_bits(np.ascontiguousarray(got).reshape(len(want), -1), np.ascontiguousarray(want).reshape(len(want), -1), what)


@pytest.mark.parametrize("domain", DOMAINS)
@every_case
def test_host_form_is_scene_probe_whatever_the_chunks(trt, case, index, domain):
    c = case(index, domain)
    sc, items, path, want, st = c["scene"], c["items"], c["path"], c["want"], c["st"]
    for what, record_bytes in RECORD_BYTES.items():
        got, st1 = sc.probe_parallel(items, K, domain=domain, record_bytes=record_bytes, sh=np.full((N, 9, 3), 7.5, np.float32), **path)
        same(got, want, (CASES[index], domain, what))
        assert st1["samples"] == st["samples"] and st1["rays"] == st["rays"], (CASES[index], domain, what)
        assert st1["kernel_ms"] > 0.0
    # bands 1 and 2: the leading coefficients
    for bands in (1, 2):
        got, st1 = sc.probe_parallel(items, K, bands=bands, domain=domain, record_bytes=RECORD_BYTES["three chunks, ragged"], **path)
        same(got, np.ascontiguousarray(want[:, :bands * bands]), (CASES[index], domain, bands))
        assert st1["rays"] == st["rays"]


@pytest.mark.parametrize("domain", DOMAINS)
@pytest.mark.parametrize("index", (0, 3), ids=("cornell", "grid3000"))
def test_ranges_accumulate_and_the_split_by_items(trt, case, index, domain):
    c = case(index, domain)
    sc, items, path, want, st = c["scene"], c["items"], c["path"], c["want"], c["st"]
    rb = RECORD_BYTES["three chunks, ragged"]
    # two ranges with accumulate, chunked differently
    head, st0 = sc.probe_parallel(items, K, domain=domain, sample_begin=0, sample_end=3, record_bytes=rb, **path)
    ref_head, rst0 = sc.probe(items, K, domain=domain, sample_begin=0, sample_end=3, **path)
    same(head, ref_head, (domain, "[0, 3)"))
    assert (st0["samples"], st0["rays"]) == (rst0["samples"], rst0["rays"]) and st0["samples"] == N * 3
    both, st1 = sc.probe_parallel(items, K, domain=domain, sample_begin=3, sample_end=K, accumulate=True, sh=head, record_bytes=50 * ITEM, **path)
    same(both, want, (domain, "[0, 3) + [3, K)"))
    assert st0["rays"] + st1["rays"] == st["rays"]
    # prior sums with -0, inf and a NaN: what trt_probe makes of them; the NaN-point item keeps its words
    prior = P.prior_sums(N, 9, 77)
    dead = np.flatnonzero(np.isnan(items[:, 0:3]).any(axis=1))
    prior.view(np.uint32)[dead, 0] = (0x80000000, 0x7FC12345, 0x7F800000)
    cont, _ = sc.probe_parallel(items, K, domain=domain, accumulate=True, sh=prior.copy(), record_bytes=rb, **path)
    ref, _ = sc.probe(items, K, domain=domain, accumulate=True, sh=prior.copy(), **path)
    same(cont, ref, (domain, "prior sums"))
    assert cont[dead].tobytes() == prior[dead].tobytes()
    # the split by items: items [a, n) with first_stream + a K
    a = 100
    tail, _ = sc.probe_parallel(np.ascontiguousarray(items[a:]), K, domain=domain, record_bytes=rb, **dict(path, first_stream=FIRST + a * K))
    same(tail, np.ascontiguousarray(want[a:]), (domain, "items [100, n)"))
    # nothing to trace: zero unless accumulate, nothing counted, no sample launch
    for kw in (dict(max_bounces=0), dict(sample_begin=2, sample_end=2)):
        z, stz = sc.probe_parallel(items, K, domain=domain, record_bytes=ITEM, sh=np.full((N, 9, 3), 7.5, np.float32), **dict(path, **kw))
        assert (z.view(np.uint32) == 0).all() and stz["samples"] == 0 and stz["rays"] == 0
        z, stz = sc.probe_parallel(items, K, domain=domain, record_bytes=ITEM, accumulate=True, sh=prior.copy(), **dict(path, **kw))
        assert z.tobytes() == prior.tobytes() and stz["samples"] == 0 and stz["rays"] == 0
    # a record buffer one byte short of an item is refused, with the bytes an item needs
    with pytest.raises(trt.TinyRTError) as e:
        sc.probe_parallel(items, K, domain=domain, record_bytes=ITEM - 1, **path)
    assert e.value.code == trt._lib.ERR_INVALID_ARG and (" %d bytes" % ITEM) in str(e.value)


def device_bytes(torch, nbytes):
    return torch.full((GUARD * 12 + nbytes + GUARD * 12,), FILL, dtype=torch.uint8, device="cuda:0")


def guards_intact(t, nbytes):
    h = t.cpu().numpy()
    g = GUARD * 12
    return bool((h[:g] == FILL).all() and (h[g + nbytes:] == FILL).all())


def sums_of(t, n, coeffs):
    g = GUARD * 12
    return t.cpu().numpy()[g:g + n * coeffs * 12].copy().view(np.float32).reshape(n, coeffs, 3)


@pytest.mark.parametrize("domain", DOMAINS)
@every_case
def test_device_form_on_a_side_stream_leaves_the_guards_and_adds_to_the_counters(trt, case, index, domain):
    import torch
    c = case(index, domain)
    sc, items, path, want, st = c["scene"], c["items"], c["path"], c["want"], c["st"]
    d_items = torch.from_numpy(items.copy()).to("cuda:0")
    side = torch.cuda.Stream()
    at = GUARD * 12
    runs = []
    for what, record_bytes in (("one item per chunk", ITEM), ("three chunks, ragged", 120 * ITEM + 7), ("one chunk", N * ITEM)):
        d_sh, d_rec = device_bytes(torch, N * 9 * 12), device_bytes(torch, record_bytes)
        ctr = torch.full((16,), 3, dtype=torch.int64, device="cuda:0")      # the counters are added to
        runs.append((what, record_bytes, d_sh, d_rec, ctr))
    torch.cuda.synchronize()
    for what, record_bytes, d_sh, d_rec, ctr in runs:
        sc.probe_parallel_device(d_items.data_ptr(), N, d_sh.data_ptr() + at, d_rec.data_ptr() + at, record_bytes, d_counters_ptr=ctr.data_ptr(),
                                 stream_ptr=side.cuda_stream, samples_per_item=K, domain=domain, **path)
    side.synchronize()
    torch.cuda.synchronize()
    for what, record_bytes, d_sh, d_rec, ctr in runs:
        assert guards_intact(d_sh, N * 9 * 12) and guards_intact(d_rec, record_bytes), (CASES[index], domain, what, "guard bytes were written")
        same(sums_of(d_sh, N, 9), want, (CASES[index], domain, what))
        assert int(ctr[0]) == 3 + st["samples"] and int(ctr[1]) == 3 + st["rays"] and bool((ctr[2:] == 3).all()), (CASES[index], domain, what)
        # no byte of the record buffer beyond the chunk size's 24 K m is touched
        m = min(N, record_bytes // ITEM)
        rec = d_rec.cpu().numpy()[at:at + record_bytes]
        assert (rec[m * ITEM:] == FILL).all(), (CASES[index], domain, what)
    assert (d_items.cpu().numpy().view(np.uint32) == items.view(np.uint32)).all()
    # two ranges with accumulate through the device form, and scratch one byte short of an item
    what, record_bytes, d_sh, d_rec, ctr = runs[1]
    d_sh2 = device_bytes(torch, N * 9 * 12)
    kw = dict(samples_per_item=K, domain=domain, **path)
    sc.probe_parallel_device(d_items.data_ptr(), N, d_sh2.data_ptr() + at, d_rec.data_ptr() + at, record_bytes, sample_begin=0, sample_end=3, **kw)
    sc.probe_parallel_device(d_items.data_ptr(), N, d_sh2.data_ptr() + at, d_rec.data_ptr() + at, record_bytes, sample_begin=3, sample_end=K,
                             accumulate=True, **kw)
    with pytest.raises(trt.TinyRTError) as e:
        sc.probe_parallel_device(d_items.data_ptr(), N, d_sh2.data_ptr() + at, d_rec.data_ptr() + at, ITEM - 1, **kw)
    assert e.value.code == trt._lib.ERR_INVALID_ARG and (" %d bytes" % ITEM) in str(e.value)
    with pytest.raises(trt.TinyRTError) as e:                               # the sums inside the record buffer
        sc.probe_parallel_device(d_items.data_ptr(), N, d_rec.data_ptr() + at + 12, d_rec.data_ptr() + at, record_bytes, **kw)
    assert e.value.code == trt._lib.ERR_INVALID_ARG and "overlap" in str(e.value)
    torch.cuda.synchronize()
    assert guards_intact(d_sh2, N * 9 * 12) and guards_intact(d_rec, record_bytes)
    same(sums_of(d_sh2, N, 9), want, (CASES[index], domain, "two ranges"))


# ---- long cases: chunks past one workgroup of samples; the projection's lane regime over more than one workgroup ----

LONG_DEPTH = 4


@pytest.mark.parametrize("k,r", ((64, 64), (64, 60)), ids=("wave-per-item", "lane-per-item"))
@pytest.mark.parametrize("index", (0, 3), ids=("cornell", "grid3000"))
def test_chunks_past_one_workgroup_of_samples(trt, case, index, k, r):
    c = case(index, "hemisphere")
    sc, items = c["scene"], c["items"]
    path = dict(c["path"], max_bounces=LONG_DEPTH)
    assert N * r > 256 * 64 and P.by_wave(N, r) == (r == 64) and (r == 64 or N > 256)
    assert sc.probe_parallel_plan(N, r)["workgroups"] > 1
    want, st = sc.probe(items, k, domain="hemisphere", sample_begin=0, sample_end=r, **path)
    one, st1 = sc.probe_parallel(items, k, domain="hemisphere", sample_begin=0, sample_end=r, record_bytes=N * 24 * k, **path)
    same(one, want, (CASES[index], k, r, "one chunk"))
    assert (st1["samples"], st1["rays"]) == (st["samples"], st["rays"]) and st["samples"] == N * r
    two, st2 = sc.probe_parallel(items, k, domain="hemisphere", sample_begin=0, sample_end=r, record_bytes=300 * 24 * k, **path)
    same(two, want, (CASES[index], k, r, "chunks of 300 and 24"))
    assert st2["rays"] == st["rays"]
    assert np.count_nonzero(want) > 0
