"""Sample-parallel next-event queries (tinyrt.h trt_nee_samples, trt_nee_samples_device) on the GPU against the CPU oracle, bit for bit
and sample by sample, and their records folded by trt_fold_samples_device against the four folding queries on the same device buffers.

The references are the restatements of the folding queries, which already return every sample's colour (`cols`): tests/nee_cases.py
(trt_nee), tests/nee_mis_cases.py (trt_nee_mis), tests/nee_pick_cases.py (trt_nee_pick, trt_nee_mis_pick).  Items, streams, tables and
scenes are tests/test_gpu_nee_pick.py's: 324 rays or surfels per scene and source, K = 8, seed 5, first_stream 1000, B = 5, one scene per
kernel shape, with the shape and launch bound of the plan asserted against profiles/nee_samples_resource_usage.txt, so all six shapes of
the four tables of nee_samples.hip run.  Every comparison is by bits; nothing here has a tolerance."""
import numpy as np
import pytest

import gather_cases as GC
import nee_cases as NC
import nee_mis_cases as NM
import nee_pick_cases as NP
import radiance_cases as R
import test_gpu_nee_pick as T
import test_gpu_queries as G
import test_gpu_samples as GS
import test_nee_samples_abi as SA

pytestmark = pytest.mark.gpu

K, DEPTH, SEED, FIRST = NP.K, NP.MAX_BOUNCES, NP.SEED, NP.FIRST_STREAM
N = NP.N_ITEMS
GUARD, FILL = GS.GUARD, GS.FILL
SOURCES = NP.SOURCES
CASES, IDS = T.CASES, T.IDS
CUT = T.CUT
# name -> (mis, pick): the sibling whose sample is written
VARIANTS = {"plain": (None, False), "balance": ("balance", False), "power": ("power", False), "pick": (None, True), "pick-balance": ("balance", True)}
BY_VARIANT = [(c, v) for c in CASES for v in VARIANTS]
BV_IDS = ["%s-%s" % (i, v) for i in IDS for v in VARIANTS]
same_bits = NP.assert_same_bits


pick_case = T.case                                                          # test_gpu_nee_pick's fixture, under a name of its own here


@pytest.fixture(scope="module")
def case(pick_case):
    """test_gpu_nee_pick's fixtures per (name, options), with the shape and the bound of the four sample plans asserted."""
    get = pick_case
    bounds = SA.bounds_of_the_profile()
    seen = set()

    def checked(name, options, shape):
        c = get(name, options, shape)
        key = (name, tuple(sorted(options.items())))
        if key not in seen:
            for mis, pick in VARIANTS.values():
                q = c["scene"].nee_samples_plan(N, K, mis=mis, pick=pick)
                assert G.plan_shape(q) == shape, (name, options, q)
                assert q["kernel_waves_per_simd"] == bounds[(mis is not None, pick, shape[:3])], (name, options, mis, pick, q)
            seen.add(key)
        return c

    return checked


def want_of(trt, orc, name, source, mis, pick, **kw):
    """The restatement of the sibling that (mis, pick) selects; `pick` may be the records of a table of the caller's."""
    if pick is not False and pick is not None:
        return NP.reference(trt, orc, name, source, heuristic=None if mis is None else NP.HEURISTICS[mis],
                            **(kw if pick is True else dict(kw, pick=pick)))
    if mis is None:
        return NC.reference(trt, orc, name, source, **kw)
    return NM.reference(trt, orc, name, source, heuristic=NM.HEURISTICS[mis], **kw)


def pick_arg(c, mis, pick):
    return T.pick_arg(c, mis) if pick else None


def sentinel(n=N, k=K):
    return np.full((n, k, 3), 7.5, np.float32)


def first_directions(c, source):
    return np.ascontiguousarray(c[source]["rays"][:, :, 3:6])


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("cse,variant", BY_VARIANT, ids=BV_IDS)
def test_host_form_is_the_restatements_colour_and_first_direction_of_every_sample(trt, orc, case, cse, variant, source):
    name, options, shape = cse
    mis, pick = VARIANTS[variant]
    c = case(name, options, shape)
    want = want_of(trt, orc, name, source, mis, pick)
    cols, dirs, st = c["scene"].nee_samples(c[source]["items"], c["mine"], mis=mis, pick=pick_arg(c, mis, pick), colors=sentinel(), directions=sentinel(),
                                            **c["kw"][source])
    same_bits(cols, want["cols"], (name, options, source, variant, "colours"))
    same_bits(dirs, first_directions(c, source), (name, options, source, variant, "directions"))
    assert st["samples"] == N * K == want["n_samples"] and st["rays"] == want["n_rays"], (name, options, source, variant, st, want["n_rays"])
    # directions = None: the colours are unchanged
    cols1, none, st1 = c["scene"].nee_samples(c[source]["items"], c["mine"], mis=mis, pick=pick_arg(c, mis, pick), **c["kw"][source])
    assert none is None and cols1.tobytes() == cols.tobytes() and (st1["samples"], st1["rays"]) == (st["samples"], st["rays"])


def on_device(torch, c, source, mis, pick, table=None, side=None, counters=None, with_dirs=True, n=N, items=None, d_cols=None, **over):
    """(colours [n, K, 3], directions [n, K, 3], guards intact?) of the device form on guarded buffers of the fill byte, both tables padded
    as test_gpu_nee_pick pads them.  `pick`: None, or the records."""
    table = c["mine"] if table is None else table
    d_items = torch.from_numpy(np.ascontiguousarray(c[source]["items"] if items is None else items).copy()).to("cuda:0")
    d_table = T.padded(torch, table)
    d_pick = None if pick is None else T.padded(torch, pick)
    d_c = GS.device_buffer(torch, n * K) if d_cols is None else d_cols
    d_d = GS.device_buffer(torch, n * K)
    torch.cuda.synchronize()
    arg = None if pick is None else d_pick.data_ptr() if mis is None else (d_pick.data_ptr(), c["total"])
    c["scene"].nee_samples_device(d_items.data_ptr(), n, d_table.data_ptr(), len(table), d_c.data_ptr() + GUARD * 12,
                                  d_d.data_ptr() + GUARD * 12 if with_dirs else 0, d_counters_ptr=0 if counters is None else counters.data_ptr(),
                                  stream_ptr=0 if side is None else side.cuda_stream, mis=mis, pick=arg, **dict(c["kw"][source], **over))
    if side is not None:
        side.synchronize()
    torch.cuda.synchronize()
    cols, ok_c = GS.payload(d_c, n, K)
    dirs, ok_d = GS.payload(d_d, n, K)
    if not with_dirs:
        ok_d = ok_d and bool((dirs.view(np.uint32) == 0xCDCDCDCD).all())
    return cols, dirs, ok_c and ok_d


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("cse,variant", BY_VARIANT, ids=BV_IDS)
def test_device_form_on_a_side_stream_equals_the_restatement_and_leaves_the_guards(trt, orc, case, cse, variant, source):
    import torch
    name, options, shape = cse
    mis, pick = VARIANTS[variant]
    c = case(name, options, shape)
    want = want_of(trt, orc, name, source, mis, pick)
    ctr = torch.full((16,), 3, dtype=torch.int64, device="cuda:0")          # the counters are added to
    cols, dirs, ok = on_device(torch, c, source, mis, c["pick"] if pick else None, side=torch.cuda.Stream(), counters=ctr)
    assert ok, (name, options, variant, "guard bytes were written")
    same_bits(cols, want["cols"], (name, options, source, variant, "colours"))
    same_bits(dirs, first_directions(c, source), (name, options, source, variant, "directions"))
    assert int(ctr[0]) == 3 + N * K and int(ctr[1]) == 3 + want["n_rays"] and bool((ctr[2:] == 3).all())
    # without directions and without counters: the same colours, the guards intact, the second buffer untouched
    cols1, _, ok1 = on_device(torch, c, source, mis, c["pick"] if pick else None, with_dirs=False)
    assert ok1 and cols1.tobytes() == cols.tobytes()


@pytest.mark.parametrize("cse,variant", BY_VARIANT, ids=BV_IDS)
def test_ranges_and_a_split_by_items_leave_the_bytes_of_one_call(trt, orc, case, cse, variant):
    name, options, shape = cse
    mis, pick = VARIANTS[variant]
    c = case(name, options, shape)
    source = SOURCES[(CASES.index(cse) + list(VARIANTS).index(variant)) % len(SOURCES)]
    want = want_of(trt, orc, name, source, mis, pick)
    kw = dict(c["kw"][source], mis=mis, pick=pick_arg(c, mis, pick))
    items = c[source]["items"]
    first = first_directions(c, source)
    rays3 = int(want["hits"][:, :3].sum() + want["walks"][:, :3].sum())
    # [0, 3) alone leaves the records of [3, K) as the prefill
    cols, dirs = sentinel(), sentinel()
    _, _, st = c["scene"].nee_samples(items, c["mine"], sample_begin=0, sample_end=3, colors=cols, directions=dirs, **kw)
    assert (cols[:, 3:] == 7.5).all() and (dirs[:, 3:] == 7.5).all()
    same_bits(cols[:, :3], want["cols"][:, :3], (name, options, source, variant, "colours [0, 3)"))
    same_bits(dirs[:, :3], first[:, :3], (name, options, source, variant, "directions [0, 3)"))
    assert st["samples"] == N * 3 and st["rays"] == rays3
    # [3, K) into the same buffers: the bytes of one call
    _, _, st = c["scene"].nee_samples(items, c["mine"], sample_begin=3, sample_end=K, colors=cols, directions=dirs, **kw)
    same_bits(cols, want["cols"], (name, options, source, variant, "colours [0, 3) + [3, K)"))
    same_bits(dirs, first, (name, options, source, variant, "directions [0, 3) + [3, K)"))
    assert st["samples"] == N * (K - 3) and st["rays"] == want["n_rays"] - rays3
    # items [0, 65), then [65, 324) on their own streams
    cols, dirs = sentinel(), sentinel()
    c["scene"].nee_samples(items[:CUT], c["mine"], colors=cols[:CUT], directions=dirs[:CUT], **kw)
    assert (cols[CUT:] == 7.5).all() and (dirs[CUT:] == 7.5).all()         # records outside the call's items are untouched
    c["scene"].nee_samples(items[CUT:], c["mine"], colors=cols[CUT:], directions=dirs[CUT:], **dict(kw, first_stream=FIRST + CUT * K))
    same_bits(cols, want["cols"], (name, options, source, variant, "colours by items"))
    same_bits(dirs, first, (name, options, source, variant, "directions by items"))


@pytest.mark.parametrize("source", ("rays", "cosine"))
@pytest.mark.parametrize("cse,variant", BY_VARIANT, ids=BV_IDS)
def test_a_diffuse_source(trt, orc, case, cse, variant, source):
    """source_is_diffuse = 1: the first hit is hidden in full, weighted or not."""
    name, options, shape = cse
    mis, pick = VARIANTS[variant]
    c = case(name, options, shape)
    want = want_of(trt, orc, name, source, mis, pick, source_is_diffuse=True)
    cols, _, st = c["scene"].nee_samples(c[source]["items"], c["mine"], source_is_diffuse=True, mis=mis, pick=pick_arg(c, mis, pick), colors=sentinel(),
                                         **c["kw"][source])
    same_bits(cols, want["cols"], (name, options, source, variant, "colours"))
    assert st["samples"] == N * K and st["rays"] == want["n_rays"]


def sums_on_device(torch, n):
    return torch.full(((GUARD + n + GUARD) * 12,), FILL, dtype=torch.uint8, device="cuda:0")


@pytest.mark.parametrize("cse,variant", BY_VARIANT, ids=BV_IDS)
def test_the_identity_folded_records_are_the_folding_querys_bytes(trt, orc, case, cse, variant):
    """trt_fold_samples_device over the records of trt_nee_samples_device equals trt_nee_device / its mis / pick forms on the same device
    buffers and the oracle's fold: sums, second moments and counters, for the whole range and for a two-call split with accumulate."""
    import torch
    name, options, shape = cse
    mis, pick = VARIANTS[variant]
    c = case(name, options, shape)
    source = SOURCES[(CASES.index(cse) + list(VARIANTS).index(variant) + 1) % len(SOURCES)]
    want = want_of(trt, orc, name, source, mis, pick)
    kw = c["kw"][source]
    d_items = torch.from_numpy(np.ascontiguousarray(c[source]["items"]).copy()).to("cuda:0")
    d_table, d_pick = T.padded(torch, c["mine"]), T.padded(torch, c["pick"])
    arg = None if not pick else d_pick.data_ptr() if mis is None else (d_pick.data_ptr(), c["total"])
    for ranges in (((0, K),), ((0, 3), (3, K))):
        d_cols = GS.device_buffer(torch, N * K)
        d_s, d_m, d_s0, d_m0 = (sums_on_device(torch, N) for _ in range(4))
        ctr, ctr0 = torch.zeros(16, dtype=torch.int64, device="cuda:0"), torch.zeros(16, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        for k, (b, e) in enumerate(ranges):
            c["scene"].nee_samples_device(d_items.data_ptr(), N, d_table.data_ptr(), len(c["mine"]), d_cols.data_ptr() + GUARD * 12,
                                          d_counters_ptr=ctr.data_ptr(), mis=mis, pick=arg, sample_begin=b, sample_end=e, **kw)
            trt.fold_samples_device(d_cols.data_ptr() + GUARD * 12, N, K, d_s.data_ptr() + GUARD * 12, d_m.data_ptr() + GUARD * 12, sample_begin=b,
                                    sample_end=e, accumulate=k > 0)
            c["scene"].nee_device(d_items.data_ptr(), N, d_table.data_ptr(), len(c["mine"]), d_s0.data_ptr() + GUARD * 12, d_m0.data_ptr() + GUARD * 12,
                                  d_counters_ptr=ctr0.data_ptr(), mis=mis, pick=arg, sample_begin=b, sample_end=e, accumulate=k > 0, **kw)
            torch.cuda.synchronize()
            assert ctr.tolist() == ctr0.tolist(), (name, options, variant, ranges, k)          # range by range
        got = [T.TM.payload(t, N) for t in (d_s, d_m, d_s0, d_m0)]
        assert all(ok for _, ok in got) and GS.payload(d_cols, N, K)[1], (name, options, variant, "guard bytes were written")
        (s, _), (m, _), (s0, _), (m0, _) = got
        assert s.tobytes() == s0.tobytes() and m.tobytes() == m0.tobytes(), (name, options, source, variant, ranges)
        same_bits(s, want["S"], (name, options, source, variant, ranges, "radiance"))
        same_bits(m, want["M"], (name, options, source, variant, ranges, "moment2"))
        assert int(ctr[0]) == N * K and int(ctr[1]) == want["n_rays"] and not bool(ctr[2:].any())


@pytest.mark.parametrize("variant", VARIANTS)
def test_nothing_to_trace(trt, case, variant):
    """An empty range touches nothing.  max_bounces == 0: exactly the colours of the range become +0, the directions and the other records
    stay, nothing is counted.  n == 0 succeeds and touches nothing."""
    import torch
    name, options, shape = CASES[0]
    mis, pick = VARIANTS[variant]
    c = case(name, options, shape)
    items = c["cosine"]["items"]
    kw = dict(c["kw"]["cosine"], mis=mis, pick=pick_arg(c, mis, pick))
    cols, dirs = sentinel(), sentinel()
    _, _, st = c["scene"].nee_samples(items, c["mine"], sample_begin=3, sample_end=3, colors=cols, directions=dirs, **kw)
    assert (cols == 7.5).all() and (dirs == 7.5).all() and st["samples"] == 0 and st["rays"] == 0
    _, _, st = c["scene"].nee_samples(items, c["mine"], sample_begin=3, sample_end=K, colors=cols, directions=dirs, **dict(kw, max_bounces=0))
    assert (cols[:, :3] == 7.5).all() and (cols[:, 3:].view(np.uint32) == 0).all() and (dirs == 7.5).all()
    assert st["samples"] == 0 and st["rays"] == 0
    got, d, st = c["scene"].nee_samples(items[:0], c["mine"], directions=True, **kw)
    assert got.shape == (0, K, 3) and d.shape == (0, K, 3) and st["samples"] == 0 and st["rays"] == 0
    # through the device form no byte outside the range's colours is written
    ctr = torch.full((16,), 3, dtype=torch.int64, device="cuda:0")
    got, untouched, ok = on_device(torch, c, "cosine", mis, c["pick"] if pick else None, counters=ctr, max_bounces=0, sample_begin=3, sample_end=K)
    assert ok and (got[:, :3].view(np.uint32) == 0xCDCDCDCD).all() and (got[:, 3:].view(np.uint32) == 0).all()
    assert (untouched.view(np.uint32) == 0xCDCDCDCD).all() and bool((ctr == 3).all())
    got, untouched, ok = on_device(torch, c, "cosine", mis, c["pick"] if pick else None, counters=ctr, sample_begin=K, sample_end=K)
    assert ok and (got.view(np.uint32) == 0xCDCDCDCD).all() and (untouched.view(np.uint32) == 0xCDCDCDCD).all() and bool((ctr == 3).all())
    got, untouched, ok = on_device(torch, c, "cosine", mis, c["pick"] if pick else None, counters=ctr, n=0, items=items[:0])
    assert ok and bool((ctr == 3).all())


@pytest.mark.parametrize("wrong", ("q_nan", "prob_0", "alias_E", "alias_E_plus_1"))
@pytest.mark.parametrize("cse,mis", T.BY_QUERY[:2 * len(CASES)], ids=T.BQ_IDS[:2 * len(CASES)])
def test_device_form_with_a_wrong_pick_table_returns_the_restatements_bytes(trt, orc, case, cse, mis, wrong):
    """The device form checks only what the siblings' check.  Both tables lie on the device with two records of 0xCD bytes behind them,
    so a missing clamp shows as wrong bytes; no address outside an allocation is ever handed over.  The host form refuses the table."""
    import torch
    name, options, shape = cse
    c = case(name, options, shape)
    pick = T.wrong_tables(c["pick"])[wrong]
    want = want_of(trt, orc, name, "cosine", mis, pick)
    with pytest.raises(Exception):
        c["scene"].nee_samples(c["cosine"]["items"], c["mine"], mis=mis, pick=T.pick_arg(c, mis, pick), **c["kw"]["cosine"])
    cols, dirs, ok = on_device(torch, c, "cosine", mis, pick)
    assert ok and len(pick) == len(c["mine"])
    same_bits(cols, want["cols"], (name, options, mis, wrong, "colours"))
    same_bits(dirs, first_directions(c, "cosine"), (name, options, mis, wrong, "directions"))


def test_one_item_over_three_waves(trt, orc, case):
    """Cornell, the weighted PICK form, one surfel with K = R = 2 x rays_per_wave + 1: its samples are the runs of three waves, where the
    folding query gives them one lane.  Every record against nee_pick_cases.pick_paths for that one item."""
    name, options, shape = CASES[0]
    assert name == "cornell"
    c = case(name, options, shape)
    per_wave = c["scene"].nee_samples_plan(1, 1, mis="balance", pick=True)["rays_per_wave"]
    k_one = 2 * per_wave + 1
    q = c["scene"].nee_samples_plan(1, k_one, mis="balance", pick=True)
    assert q["waves"] == 3 and q["rays_per_wave"] == per_wave == 256
    item = np.ascontiguousarray(c["cosine"]["items"][7:8])
    first = GC.first_rays(orc, item, "cosine", k_one, NP.SPREAD, SEED, FIRST)
    ref = NP.finish(NP.pick_paths(orc, c["ow"], c["desc"], first, c["nee_table"], c["nee_pick"], background=c["bg"], heuristic=NP.HEURISTICS["balance"],
                                  total_power=c["nee_total"]), k_one)
    assert ref["walks"].sum() >= ref["lit"].sum() > 0
    cols, dirs, st = c["scene"].nee_samples(item, c["mine"], mis="balance", pick=(c["pick"], c["total"]), colors=sentinel(1, k_one),
                                            directions=sentinel(1, k_one), **dict(c["kw"]["cosine"], samples_per_item=k_one))
    same_bits(cols, ref["cols"], (name, "colours"))
    same_bits(dirs, np.ascontiguousarray(first[:, :, 3:6]), (name, "directions"))
    assert st["samples"] == k_one and st["rays"] == ref["n_rays"]
    S, M = trt.fold_samples(cols, k_one, moment2=True)
    same_bits(S, ref["S"], (name, "folded"))
    same_bits(M, ref["M"], (name, "folded second moments"))
