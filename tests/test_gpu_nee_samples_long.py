"""Sample-parallel next-event queries past one workgroup: the weighted PICK form (BALANCE) with the cosine source over the 324 surfels of
tests/passes_cases.py through the device form, on Cornell at depth 4 and on grid3000 at depth 2, as the other _long files.

n * R at: the first sample of workgroup 1; 100 003 samples - a prime, so K = 309 with the range cut to fit: 323 surfels over [0, 309) and
the last over [0, 196) in a second call with first_stream advanced by 323 * K; and, on Cornell only, the smallest count at which
nee_samples_plan lengthens a wave's run past 256, rounded up to whole surfels.

The reference is the folding query: trt_fold_samples_device over the records against trt_nee_mis_pick_device on the same buffers, call by
call - every sum, every second moment and the counters, by bits.  trt_nee_mis_pick_device is pinned at these sizes by
tests/test_gpu_nee_pick_long.py; the oracle restatement in Python cannot cover 10^5 paths in seconds.  The records of the first 64 and
the last 64 work indices are compared with the restatement directly (tests/nee_pick_cases.py), the records no call owns keep their fill,
and the guards stay intact."""
import numpy as np
import pytest

import gather_cases as GC
import nee_pick_cases as NP
import test_gpu_nee_pick as T
import test_gpu_queries as G

pytestmark = pytest.mark.gpu

SEED, FIRST = NP.SEED, NP.FIRST_STREAM
GUARD, FILL = T.GUARD, T.FILL
DEPTH = {"cornell": 4, "grid3000": 2}
N = NP.N_ITEMS
MIS = "balance"
EDGE = 64
CASE_OF = {name: next(c for c in T.CASES if c[0] == name) for name in DEPTH}

case = T.case


def calls_of(sc, which):
    """(K, samples, [(first item, items, sample_begin, sample_end)]): the calls that trace the wanted number of samples of the 324 items."""
    q = sc.nee_samples_plan(1, 1, mis=MIS, pick=True)
    assert q["rays_per_wave"] == 256
    if which == "workgroup1":
        total = 256 * (q["threads_per_workgroup"] // 64) + 1
    elif which == "100003":
        total = 100003
    else:
        total = 256 * q["wave_slots"] + 1                                   # ceil(n * R / 256) exceeds the resident wave slots
        assert sc.nee_samples_plan(total - 1, 1, mis=MIS, pick=True)["rays_per_wave"] == 256
        assert sc.nee_samples_plan(1, total, mis=MIS, pick=True)["rays_per_wave"] > 256
    k = -(-total // N)                                                      # the smallest K at which the 324 items hold that many samples
    if which == "100003":
        full = total // k                                                   # items traced over the whole range; the next one over the rest
        calls = [(0, full, 0, k), (full, 1, 0, total - full * k)]
        assert full + 1 == N
    else:
        calls = [(0, -(-total // k), 0, k)]                                 # whole items: a few samples more than asked
        total = calls[0][1] * k
    assert sum(n * (e - b) for _, n, b, e in calls) == total and calls[0][1] * k >= total - k
    return k, total, calls


def guarded(torch, entries):
    return torch.full(((GUARD + entries + GUARD) * 12,), FILL, dtype=torch.uint8, device="cuda:0")


def payload(t, entries):
    h = t.cpu().numpy()
    g, b = GUARD * 12, entries * 12
    assert (h[:g] == FILL).all() and (h[g + b:] == FILL).all(), "guard bytes were written"
    return h[g:g + b].copy().view(np.float32).reshape(entries, 3)


@pytest.mark.parametrize("which,name", [("workgroup1", "cornell"), ("workgroup1", "grid3000"), ("100003", "cornell"), ("100003", "grid3000"),
                                        ("longer_runs", "cornell")])
def test_long_batches_fold_to_the_folding_query_and_their_edges_equal_the_restatement(trt, orc, case, name, which):
    import torch
    c = case(*CASE_OF[name])
    sc, depth = c["scene"], DEPTH[name]
    k, total, calls = calls_of(sc, which)
    if which == "100003":
        assert k == 309 and calls == [(0, 323, 0, 309), (323, 1, 0, 196)]
    q = sc.nee_samples_plan(calls[0][1], k, mis=MIS, pick=True)
    assert G.plan_shape(q) == CASE_OF[name][2]
    assert q["workgroups"] >= 2 and q["waves"] * q["rays_per_wave"] >= calls[0][1] * k
    if which == "longer_runs":
        assert q["rays_per_wave"] > 256 and sc.nee_samples_plan(calls[0][1] - 1, k, mis=MIS, pick=True)["rays_per_wave"] == 256
    items = np.ascontiguousarray(c["cosine"]["items"])
    d_items = torch.from_numpy(items.copy()).to("cuda:0")
    d_table, d_pick = T.padded(torch, c["mine"]), T.padded(torch, c["pick"])
    d_cols = guarded(torch, N * k)
    d_s, d_m, d_s0, d_m0 = (guarded(torch, N) for _ in range(4))
    ctr, ctr0 = torch.zeros(16, dtype=torch.int64, device="cuda:0"), torch.zeros(16, dtype=torch.int64, device="cuda:0")
    kw = dict(samples_per_item=k, source="cosine", spread=NP.SPREAD, max_bounces=depth, background=c["bg"], seed=SEED, mis=MIS,
              pick=(d_pick.data_ptr(), c["total"]))
    torch.cuda.synchronize()
    for first, n, b, e in calls:
        at = dict(kw, first_stream=FIRST + first * k, sample_begin=b, sample_end=e)
        sc.nee_samples_device(d_items.data_ptr() + first * 24, n, d_table.data_ptr(), len(c["mine"]), d_cols.data_ptr() + (GUARD + first * k) * 12,
                              d_counters_ptr=ctr.data_ptr(), **at)
        trt.fold_samples_device(d_cols.data_ptr() + (GUARD + first * k) * 12, n, k, d_s.data_ptr() + (GUARD + first) * 12,
                                d_m.data_ptr() + (GUARD + first) * 12, sample_begin=b, sample_end=e)
        sc.nee_device(d_items.data_ptr() + first * 24, n, d_table.data_ptr(), len(c["mine"]), d_s0.data_ptr() + (GUARD + first) * 12,
                      d_m0.data_ptr() + (GUARD + first) * 12, d_counters_ptr=ctr0.data_ptr(), **at)
    torch.cuda.synchronize()
    # every sum, every second moment, the counters: the folding query's, by bits
    traced_items = sum(n for _, n, _, _ in calls)
    s, m, s0, m0 = (payload(t, N) for t in (d_s, d_m, d_s0, d_m0))
    assert s.tobytes() == s0.tobytes(), (name, which, "radiance")
    assert m.tobytes() == m0.tobytes(), (name, which, "moment2")
    assert (s[traced_items:].view(np.uint32) == 0xCDCDCDCD).all() and np.isfinite(s[:traced_items]).any() and (s[:traced_items] != 0).any()
    assert ctr.tolist() == ctr0.tolist() and int(ctr[0]) == total and total <= int(ctr[1]) <= 2 * depth * total and not bool(ctr[2:].any())
    # the records: the traced ones are a prefix in record order; the rest keep their fill
    got = payload(d_cols, N * k)
    assert (got[total:].view(np.uint32) == 0xCDCDCDCD).all(), (name, which, "a record outside the calls' ranges was written")
    assert not (got[:total].view(np.uint32) == 0xCDCDCDCD).all(axis=1).any(), (name, which, "a record of the calls' ranges was not written")
    # the first 64 and the last 64 work indices against the restatement
    edge = np.concatenate([np.arange(EDGE), np.arange(total - EDGE, total)])
    chosen = np.unique(edge // k)
    rays6 = np.zeros((len(chosen), k, 6), np.float32)
    for r, i in enumerate(chosen):
        rays6[r] = GC.first_rays(orc, items[i:i + 1], "cosine", k, NP.SPREAD, SEED, FIRST + int(i) * k)[0]
    ref = NP.pick_paths(orc, c["ow"], c["desc"], rays6, c["nee_table"], c["nee_pick"], max_bounces=depth, background=c["bg"], item_index=chosen,
                        heuristic=NP.HEURISTICS[MIS], total_power=c["nee_total"])
    row = {int(i): r for r, i in enumerate(chosen)}
    want = np.stack([ref["cols"][row[int(q_ // k)], int(q_ % k)] for q_ in edge])
    NP.assert_same_bits(np.ascontiguousarray(got[edge]), want, (name, which, total, "the first and the last 64 records"))
