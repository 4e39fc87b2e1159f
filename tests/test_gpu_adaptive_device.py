"""The adaptive loop with everything resident on the device: trt_render_moments_device, then trt_select_pixels_device handing its list
and its count to trt_render_pixels_device (d_count) round after round on ONE stream, with no synchronisation and no host read between
the calls - the hand-off the kernels' volatile read of the count exists for, which the host driver (tests/test_gpu_adaptive.py) never makes.

Cases: those of tests/test_gpu_adaptive.py - Cornell 16 x 16 at rel_tol 0.2, random_spheres 19 x 13 at 0.1 / 0.01, and random_spheres at
0.2 / 0.02, which runs out of active pixels after 24 samples.  Cap N = 32, min 4, step 4, max_bounces 8, seed 5.  The reference is
adaptive_cases.restated_adaptive over the oracle's exact samples; as there, the restatement must leave some pixels at 4 samples and take
some to the cap (or end early), so the comparison is never between two trivial runs.

The loop.  render_moments_device for samples [0, 4); select_pixels_device with candidates NULL and n = npixels into list A / count A; then
for each of the seven rounds the cap allows, WHETHER OR NOT anything is still active: render_pixels_device(current list, n = npixels,
d_count = current count, accumulate = 1, the next four samples), a fill of the OTHER list with 0xFFFFFFFF on the same stream, and
select_pixels_device(candidates = current list, n = npixels) into the other list and count; swap.  In the case that ends early the later
rounds launch with a count of 0 and must do nothing.

The fill is what a caller of this loop must do: the selection takes no device-resident candidate count, so it scans all n = npixels words
of the current list, and without the fill the words behind its count would be valid pixel indices left there two rounds earlier - pixels
already dropped, selected again.  Entries >= npixels are "not kept and not read" (tinyrt.h), which 0xFFFFFFFF is for every image.

Lists A and B are distinct buffers (the device form refuses overlapping lists), with two counts and one scratch; every buffer carries
guards.  One synchronisation at the end; then accum and moment2 equal the restatement's S and M bit for bit over every pixel, the final
count is len(history[-1]), the first `count` entries of the final list are history[-1], and every guard is intact.  A second test runs
the same loop on the default stream, and with a host read of the count each round passed as n: the same bytes.
Every GPU step is one in-process call."""
import numpy as np
import pytest

import adaptive_cases as A
import denoise_color_cases as D
import test_gpu_pixels as P
from test_gpu_adaptive import BOUNCES, CASE_IDS, CASES, MIN_SPP, N_CAP, SEED, STEP_SPP, world_of  # noqa: F401  (world_of: the fixture)

pytestmark = pytest.mark.gpu

GUARD = 64                                                                  # words around the lists, the counts and the scratch
MARK = -0x32323233                                                          # 0xCDCDCDCD as int32
ROUNDS = -(-(N_CAP - MIN_SPP) // STEP_SPP)


@pytest.fixture(scope="module")
def restated(world_of):
    """case index -> (S, M, history) of the restated loop, its non-triviality asserted as tests/test_gpu_adaptive.py does."""
    cache = {}

    def get(k):
        if k not in cache:
            name, size, rel_tol, abs_tol, reaches_cap = CASES[k]
            c = world_of(name, size)
            _, s, m, count, history = A.restated_adaptive(c["samples"], MIN_SPP, STEP_SPP, rel_tol, abs_tol)
            hist = dict(zip(*[a.tolist() for a in np.unique(count, return_counts=True)]))
            print(f"\n{name} {size[0]}x{size[1]}: samples -> pixels {hist}; active per round {[len(a) for a in history]}")
            assert hist.get(MIN_SPP, 0) >= 20 and (count > MIN_SPP).sum() >= 20
            assert (hist.get(N_CAP, 0) >= 10) if reaches_cap else (count.max() < N_CAP and len(history[-1]) == 0)
            assert len(set(len(a) for a in history)) >= 3                   # the count handed over changes from round to round
            cache[k] = (s, m, history)
        return cache[k]

    return get


def device_loop(trt, c, rel_tol, abs_tol, stream, host_count=False):
    """The loop of the module docstring on `stream` (None: the default stream); host_count: read the count back every round and pass it as
    n instead of d_count.  Returns (accum, moment2, final count, final list, guards intact?)."""
    import torch
    size = c["cam"].get_image_size()
    npix, shape = size[0] * size[1], (size[1], size[0], 3)
    sc = c["world"].get_bvh()
    renderer = trt.Renderer(N_CAP, 1, BOUNCES, False, c["desc"]["background"], seed=SEED)
    dev = torch.device("cuda:0")
    d_s, d_m = P.device_frame(torch, npix), P.device_frame(torch, npix)
    s_ptr, m_ptr = d_s.data_ptr() + P.GUARD * 12, d_m.data_ptr() + P.GUARD * 12
    lists = [torch.full((GUARD + npix + GUARD,), MARK, dtype=torch.int32, device=dev) for _ in range(2)]
    counts = [torch.full((GUARD + 1 + GUARD,), MARK, dtype=torch.int32, device=dev) for _ in range(2)]
    scratch_bytes = trt.select_scratch_bytes(npix)
    scratch = torch.full((GUARD + scratch_bytes // 4 + GUARD,), MARK, dtype=torch.int32, device=dev)
    lists[0][GUARD:GUARD + npix] = -1
    assert len({t.data_ptr() for t in lists + counts + [scratch]}) == 5
    list_ptr = lambda i: lists[i].data_ptr() + GUARD * 4                    # noqa: E731
    count_ptr = lambda i: counts[i].data_ptr() + GUARD * 4                  # noqa: E731
    torch.cuda.synchronize()                                                # the buffers are ready; from here on: one stream, no waiting
    ptr = 0 if stream is None else stream.cuda_stream
    ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream())

    def select(done, cand, n, out):
        trt.select_pixels_device(s_ptr, m_ptr, npix, N_CAP, done, n, rel_tol, abs_tol, list_ptr(out), count_ptr(out),
                                 scratch.data_ptr() + GUARD * 4, scratch_bytes, d_candidates_ptr=0 if cand is None else list_ptr(cand), stream_ptr=ptr)

    def n_of(i):
        return int(counts[i][GUARD].item()) if host_count else npix       # (.item() waits for the stream: the variant with a host round trip)

    renderer.render_moments_device(c["cam"], sc, s_ptr, m_ptr, stream_ptr=ptr, sample_begin=0, sample_end=MIN_SPP)
    select(MIN_SPP, None, npix, 0)
    cur, done = 0, MIN_SPP
    for _ in range(ROUNDS):
        nxt = min(done + STEP_SPP, N_CAP)
        n = n_of(cur)
        renderer.render_pixels_device(c["cam"], sc, list_ptr(cur), n, s_ptr, m_ptr, d_count_ptr=0 if host_count else count_ptr(cur), stream_ptr=ptr,
                                      sample_begin=done, sample_end=nxt, accumulate=1)
        with ctx:
            lists[1 - cur][GUARD:GUARD + npix].fill_(-1)
        select(nxt, cur, n, 1 - cur)
        cur, done = 1 - cur, nxt
    assert done == N_CAP
    (torch.cuda.current_stream() if stream is None else stream).synchronize()
    torch.cuda.synchronize()
    got_s, ok_s = P.frame_of(d_s, npix, shape)
    got_m, ok_m = P.frame_of(d_m, npix, shape)
    intact = ok_s and ok_m
    for t, k in [(lists[0], npix), (lists[1], npix), (counts[0], 1), (counts[1], 1), (scratch, scratch_bytes // 4)]:
        h = t.cpu().numpy()
        intact = intact and bool((h[:GUARD] == MARK).all() and (h[GUARD + k:] == MARK).all())
    final = lists[cur].cpu().numpy().view(np.uint32)[GUARD:GUARD + npix]
    return got_s, got_m, int(counts[cur].cpu().numpy().view(np.uint32)[GUARD]), final, intact


def check_against_the_restatement(got, want, what):
    got_s, got_m, count, final, intact = got
    s, m, history = want
    assert intact, (what, "a guard was written")
    D.assert_same(got_s, s, (what, "sums"))
    D.assert_same(got_m, m, (what, "second moments"))
    assert count == len(history[-1]), (what, "final count", count, len(history[-1]))
    assert np.array_equal(final[:count], history[-1]), (what, "final list")
    assert (final[count:] == 0xFFFFFFFF).all(), (what, "written behind the count")


@pytest.mark.parametrize("k", range(len(CASES)), ids=CASE_IDS)
def test_the_loop_on_one_side_stream_without_a_host_round_trip_equals_the_restatement(trt, world_of, restated, k):
    import torch
    name, size, rel_tol, abs_tol, _ = CASES[k]
    got = device_loop(trt, world_of(name, size), rel_tol, abs_tol, torch.cuda.Stream())
    check_against_the_restatement(got, restated(k), (name, "side stream"))


@pytest.mark.parametrize("k", range(len(CASES)), ids=CASE_IDS)
def test_the_default_stream_and_a_host_read_of_the_count_give_the_same_bytes(trt, world_of, restated, k):
    name, size, rel_tol, abs_tol, _ = CASES[k]
    c = world_of(name, size)
    default = device_loop(trt, c, rel_tol, abs_tol, None)
    check_against_the_restatement(default, restated(k), (name, "default stream"))
    hosted = device_loop(trt, c, rel_tol, abs_tol, None, host_count=True)
    check_against_the_restatement(hosted, restated(k), (name, "host read of the count"))
    assert default[0].tobytes() == hosted[0].tobytes() and default[1].tobytes() == hosted[1].tobytes() and default[2] == hosted[2]
