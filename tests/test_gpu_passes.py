"""Passes queries (tinyrt.h trt_passes, trt_passes_device) on the GPU against the CPU oracle, bit for bit and item by item.

Sample s of item i has stream index j = first_stream + i * K + s.  Its first ray is the item itself (source "rays":
radiance_cases.rays_of) or trt_gather's draw from RNG stream (seed, j, 1) (sources "cosine" and "cone": gather_cases.first_rays), and its
path runs on stream (seed, j, 0), restated from the oracle's pieces WITH the class of the sample - which line of cpu.rs:39-65 ended it and
after how many scatters (tests/passes_cases.py oracle_paths; tests/test_passes_cases.py pins it to the oracle's own loop and asserts that
the inputs reach every slot).  The colours are folded per slot in numpy float32 exactly as the contract states.

Items, per scene: 324, a full run of 256 for one wave and a ragged one of 68 for the next, four of them rays or surfels with NaN, inf
and zero components.  K = 8, max_bounces = 5, seed 5, first_stream = 1000, every source, 1 to 4 depth bins.  The scenes are one per kernel
shape (passes_cases.CASES); each case asserts the shape Scene.passes_plan reports for every number of bins, so all six instantiations of
both tables of passes.hip run."""
import numpy as np
import pytest

import passes_cases as P
import radiance_cases as R
import test_gpu_queries as G

pytestmark = pytest.mark.gpu

K, DEPTH, SEED, FIRST = P.K, P.MAX_BOUNCES, P.SEED, P.FIRST_STREAM
N = P.N_ITEMS
GUARD = 64                                                                  # floats of 7.5 on either side of a device buffer
SOURCES, BINS = P.SOURCES, P.BINS


def shape_of(name, options):
    if not options:
        return G.DEFAULT_SHAPES[name]
    return [s for n, o, s in G.OTHER_WALKS if n == name and o == options][0]


CASES = [(name, options, shape_of(name, options)) for name, options in P.CASES]
IDS = ["%s-%s" % (name, "-".join("%s=%s" % kv for kv in sorted(options.items())) or "default") for name, options, _ in CASES]


def same_bits(got, want, what):
    R.assert_same_bits(got.reshape(len(got), -1), want.reshape(len(want), -1), what)


@pytest.fixture(scope="module")
def case(trt, orc):
    """(name, options) -> the reference of the scene (passes_cases.reference: computed once, never changed), per source and number of bins
    the oracle's fold, and the product scene compiled with the options, its shape asserted for both tables."""
    cache, folds = {}, {}

    def get(name, options, shape):
        key = (name, tuple(sorted(options.items())))
        if key not in cache:
            ref = P.reference(trt, orc, name)
            if name not in folds:
                folds[name] = {(src, b): P.fold(ref[src]["cols"], ref[src]["kinds"], ref[src]["depths"], K, b) for src in SOURCES for b in BINS}
            sc = trt.world_from_description(ref["desc"])[0].get_bvh(**options)
            for bins in BINS:
                q = sc.passes_plan(N, bins)
                assert G.plan_shape(q) == shape, (name, options, bins, q)
            kw = dict(samples_per_item=K, max_bounces=DEPTH, background=ref["bg"], seed=SEED, first_stream=FIRST, spread=P.SPREAD)
            cache[key] = dict(ref, scene=sc, fold=folds[name], kw={s: dict(kw, source=s) for s in SOURCES})
        return cache[key]

    return get


def sentinels(bins, n=N):
    return np.full((n, 2 * bins, 3), 7.5, np.float32), np.full(n, 7.5, np.float32)


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_host_form_is_the_oracles_fold_for_every_number_of_bins(trt, case, name, options, shape, source):
    """B = 1 and 2 run the kernels that carry 2 bins, B = 3 and 4 those that carry 4.  Identity 2 of tinyrt.h follows on the device's own
    results: the slots at depth d < B - 1 do not depend on B."""
    c = case(name, options, shape)
    got = {}
    for bins in BINS:
        passes, spent = sentinels(bins)
        _, _, st = c["scene"].passes(c[source]["items"], depth_bins=bins, passes=passes, spent=spent, **c["kw"][source])
        want_p, want_s = c["fold"][(source, bins)]
        same_bits(passes, want_p, (name, options, source, bins, "passes"))
        same_bits(spent, want_s, (name, options, source, bins, "spent"))
        assert st["samples"] == N * K
        assert st["rays"] == c[source]["n_rays"], (name, options, source, bins)
        got[bins] = passes
    for b in BINS:
        for b2 in BINS:
            for d in range(min(b, b2) - 1):
                assert got[b][:, d].tobytes() == got[b2][:, d].tobytes() and got[b][:, b + d].tobytes() == got[b2][:, b2 + d].tobytes()


def device_buffer(torch, floats):
    return torch.full((GUARD + floats + GUARD,), 7.5, dtype=torch.float32, device="cuda:0")


def payload(t, floats):
    """(payload as float32 [floats], guards intact?)"""
    h = t.cpu().numpy()
    return h[GUARD:GUARD + floats].copy(), bool((h[:GUARD] == 7.5).all() and (h[GUARD + floats:] == 7.5).all())


@pytest.mark.parametrize("bins", BINS)
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_device_form_on_a_side_stream_equals_the_oracle_and_leaves_the_guards(trt, case, name, options, shape, source, bins):
    """The device form gives the bytes of the host form (both equal the oracle's), adds to the counters and writes nothing outside
    [0, 24 B n) and [0, 4 n); without a spent buffer `passes` is the same."""
    import torch
    c = case(name, options, shape)
    want_p, want_s = c["fold"][(source, bins)]
    d_items = torch.from_numpy(c[source]["items"].copy()).to("cuda:0")
    side = torch.cuda.Stream()
    d_p, d_s = device_buffer(torch, N * 6 * bins), device_buffer(torch, N)
    d_p2 = device_buffer(torch, N * 6 * bins)
    ctr = torch.full((16,), 3, dtype=torch.int64, device="cuda:0")          # the counters are added to
    torch.cuda.synchronize()
    c["scene"].passes_device(d_items.data_ptr(), N, d_p.data_ptr() + GUARD * 4, d_s.data_ptr() + GUARD * 4, d_counters_ptr=ctr.data_ptr(),
                             stream_ptr=side.cuda_stream, depth_bins=bins, **c["kw"][source])
    c["scene"].passes_device(d_items.data_ptr(), N, d_p2.data_ptr() + GUARD * 4, 0, stream_ptr=side.cuda_stream, depth_bins=bins,
                             **c["kw"][source])
    side.synchronize()
    torch.cuda.synchronize()
    got_p, ok_p = payload(d_p, N * 6 * bins)
    got_s, ok_s = payload(d_s, N)
    got_p2, ok_p2 = payload(d_p2, N * 6 * bins)
    assert ok_p and ok_s and ok_p2, (name, options, source, bins, "guard floats were written")
    same_bits(got_p.reshape(N, 2 * bins, 3), want_p, (name, options, source, bins, "passes"))
    same_bits(got_s, want_s, (name, options, source, bins, "spent"))
    assert got_p2.tobytes() == got_p.tobytes()
    assert int(ctr[0]) == 3 + N * K and int(ctr[1]) == 3 + c[source]["n_rays"] and bool((ctr[2:] == 3).all())


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_without_spent_the_passes_are_the_same(trt, case, name, options, shape, source):
    c = case(name, options, shape)
    for bins in (4, 1):
        passes, _ = sentinels(bins)
        got, none, st = c["scene"].passes(c[source]["items"], depth_bins=bins, passes=passes, spent=False, **c["kw"][source])
        assert none is None and got is passes
        same_bits(passes, c["fold"][(source, bins)][0], (name, options, source, bins))
        assert st["rays"] == c[source]["n_rays"]


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_with_a_black_sky_and_one_bin_slot_0_is_the_gather(trt, case, name, options, shape, source):
    """Identity 1 of tinyrt.h, product against product: background 0, B = 1 - slot 0 is Scene.gather's (source "rays":
    Scene.radiance's) radiance byte for byte, the SKY slot is +0, and the ray counts agree."""
    c = case(name, options, shape)
    kw = dict(c["kw"][source], background=(0.0, 0.0, 0.0))
    passes, spent, st = c["scene"].passes(c[source]["items"], depth_bins=1, **kw)
    kw.pop("source")
    if source == "rays":
        kw.pop("spread")
        want, _, st1 = c["scene"].radiance(c[source]["items"], kw.pop("samples_per_item"), **kw)
    else:
        want, _, st1 = c["scene"].gather(c[source]["items"], kw.pop("samples_per_item"), lobe=source, **kw)
    assert np.ascontiguousarray(passes[:, 0]).tobytes() == want.tobytes(), (name, options, source)
    assert not passes[:, 1].view(np.uint32).any()
    assert st["rays"] == st1["rays"] and st["samples"] == st1["samples"] == N * K
    assert (want != 0.0).any() or name in ("random_spheres", "grid3000")    # (those two scenes have no emitter)


@pytest.mark.parametrize("bins", (4, 2))
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_split_by_samples_leaves_the_bytes_of_one_pass(trt, case, name, options, shape, source, bins):
    c = case(name, options, shape)
    r = c[source]
    passes, spent = sentinels(bins)
    c["scene"].passes(r["items"], sample_begin=0, sample_end=3, depth_bins=bins, passes=passes, spent=spent, **c["kw"][source])
    p3, s3 = P.fold(r["cols"], r["kinds"], r["depths"], K, bins, 0, 3)
    same_bits(passes, p3, (name, options, source, bins, "[0, 3)"))
    same_bits(spent, s3, (name, options, source, bins, "[0, 3) spent"))
    _, _, st = c["scene"].passes(r["items"], sample_begin=3, sample_end=8, accumulate=True, depth_bins=bins, passes=passes, spent=spent,
                                 **c["kw"][source])
    same_bits(passes, c["fold"][(source, bins)][0], (name, options, source, bins, "[0, 3) + [3, 8)"))
    same_bits(spent, c["fold"][(source, bins)][1], (name, options, source, bins, "[0, 3) + [3, 8) spent"))
    assert st["samples"] == N * 5


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_accumulate_leaves_the_slots_no_sample_reaches(trt, case, name, options, shape, source):
    """Not adding is not adding 0: sums that start at -0 keep their sign bit wherever no sample of the item reached the slot, and the
    reached ones are the oracle's fold continued from -0."""
    c = case(name, options, shape)
    r = c[source]
    start_p, start_s = np.full((N, 8, 3), -0.0, np.float32), np.full(N, -0.0, np.float32)
    want_p, want_s = P.fold(r["cols"], r["kinds"], r["depths"], K, 4, passes=start_p, spent=start_s)
    passes, spent = start_p.copy(), start_s.copy()
    c["scene"].passes(r["items"], depth_bins=4, accumulate=True, passes=passes, spent=spent, **c["kw"][source])
    assert passes.tobytes() == want_p.tobytes() and spent.tobytes() == want_s.tobytes(), (name, options, source)
    slots = P.slots_of(r["kinds"], r["depths"], 4)
    unreached = np.ones((N, 8), bool)
    for s in range(K):
        live = slots[:, s] >= 0
        unreached[np.arange(N)[live], slots[live, s]] = False
    assert unreached.any() and (passes.view(np.uint32)[unreached] == 0x80000000).all()


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_split_by_items_leaves_the_bytes_of_one_call(trt, case, name, options, shape, source):
    c = case(name, options, shape)
    items = c[source]["items"]
    bins = 3
    one_p, one_s, st = c["scene"].passes(items, depth_bins=bins, **c["kw"][source])
    passes, spent = sentinels(bins)
    kw = dict(c["kw"][source], depth_bins=bins)
    a = 100
    _, _, st_a = c["scene"].passes(items[:a], passes=passes[:a], spent=spent[:a], **kw)
    assert (passes[a:] == 7.5).all() and (spent[a:] == 7.5).all()           # entries outside the call's range are untouched
    kw["first_stream"] = FIRST + a * K
    assert kw["first_stream"] == 1800
    head_p, head_s = passes[:a].copy(), spent[:a].copy()
    _, _, st_b = c["scene"].passes(items[a:], passes=passes[a:], spent=spent[a:], **kw)
    assert passes[:a].tobytes() == head_p.tobytes() and spent[:a].tobytes() == head_s.tobytes()
    assert passes.tobytes() == one_p.tobytes() and spent.tobytes() == one_s.tobytes(), (name, options, source)        # byte for byte
    same_bits(passes, c["fold"][(source, bins)][0], (name, options, source))
    assert st_a["rays"] + st_b["rays"] == st["rays"] == c[source]["n_rays"]


@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_nothing_to_trace_zeroes_or_leaves(trt, case, name, options, shape):
    """max_bounces == 0 and an empty sample range: the 24 B n bytes of `passes` and the 4 n of `spent` are zeroed without accumulate and
    untouched with it; through the device form no byte outside them is written."""
    import torch
    c = case(name, options, shape)
    for source, bins in (("rays", 4), ("cosine", 3), ("cone", 1)):
        for over in (dict(max_bounces=0), dict(sample_begin=3, sample_end=3)):
            kw = dict(c["kw"][source], depth_bins=bins, **over)
            for accumulate in (False, True):
                passes, spent = sentinels(bins)
                _, _, st = c["scene"].passes(c[source]["items"], accumulate=accumulate, passes=passes, spent=spent, **kw)
                want = 7.5 if accumulate else 0.0
                assert (passes == want).all() and (spent == want).all(), (name, options, source, bins, over, accumulate)
                assert st["rays"] == 0 and st["samples"] == 0
                passes, _ = sentinels(bins)
                c["scene"].passes(c[source]["items"], accumulate=accumulate, passes=passes, spent=False, **kw)
                assert (passes == want).all()
    d_items = torch.from_numpy(c["cosine"]["items"].copy()).to("cuda:0")
    for bins in (4, 1):
        for accumulate in (False, True):
            for with_spent in (True, False):
                d_p, d_s = device_buffer(torch, N * 6 * bins), device_buffer(torch, N)
                c["scene"].passes_device(d_items.data_ptr(), N, d_p.data_ptr() + GUARD * 4, d_s.data_ptr() + GUARD * 4 if with_spent else 0,
                                         accumulate=accumulate, depth_bins=bins, **dict(c["kw"]["cosine"], max_bounces=0))
                torch.cuda.synchronize()
                got_p, ok_p = payload(d_p, N * 6 * bins)
                got_s, ok_s = payload(d_s, N)
                assert ok_p and ok_s, (name, options, bins, "guard floats were written")
                assert (got_p == (7.5 if accumulate else 0.0)).all()
                assert (got_s == (7.5 if accumulate or not with_spent else 0.0)).all()


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_items_with_a_nan_land_in_the_first_sky_slot_with_the_background(trt, case, name, options, shape, source):
    """A first ray with a NaN component hits nothing: SKY at depth 0.  Slot B holds K times background / K folded, every other slot of
    the item and its spent share stay +0, and each sample counts one world.hit."""
    c = case(name, options, shape)
    items = c[source]["items"]
    nan_items = np.flatnonzero(np.isnan(items).any(axis=1))
    assert len(nan_items) >= 1
    bg = np.array(c["bg"], np.float32)
    want = np.zeros(3, np.float32)
    for _ in range(K):
        want = want + bg * (np.float32(1.0) / np.float32(K))
    for bins in (2, 3):
        passes, spent, st = c["scene"].passes(np.ascontiguousarray(items[nan_items]), depth_bins=bins, **c["kw"][source])
        assert (passes[:, bins].view(np.uint32) == want.view(np.uint32)).all(), (name, options, source, bins)
        others = np.delete(passes, bins, axis=1)
        assert not others.view(np.uint32).any() and not spent.view(np.uint32).any()
        assert st["rays"] == st["samples"] == len(nan_items) * K
