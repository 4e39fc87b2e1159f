"""The sparse render (trt_render_pixels_device) on lists long enough that a wave's run grows beyond 256 entries - the lists of its real
use, 1080p and 4K frames - against a whole-frame render on the same device and, around the run boundaries, against the CPU oracle.

plan_batch gives a wave 256 list entries until the list has more than n0 = 256 x wave_slots entries; one entry more and a run is 320
entries: wave w begins at 320 w, no multiple of 256, the refill cursor runs five rounds and the last wave owns a ragged rest.  wave_slots
is read from Scene.pixels_plan(1) for the device at hand (compute_units = 0), never assumed; at 256 compute units n0 + 1 is 3 145 729
(random_spheres: LDS tree, 768 lanes), 4 194 305 (prims600: register slots, 512 lanes) and 5 242 881 (grid3000: 16-byte nodes from global
memory, 256 lanes).  The plan is asserted first: 256 entries per wave at n0, ((ceil((n0 + 1) / wave_slots) + 63) & ~63) > 256 at n0 + 1.

Image: 2048 wide, ceil((n0 + 1) / 2048) + 1 rows, so the list is shorter than the image and a tail of pixels is unlisted.  N = 2,
max_bounces 4, seed 5.  Device form only, both buffers with 64 pixels of guard on either side and filled with the sentinel.  Lists:
arange(n0 + 1), and arange(n0): the boundary on the 256 side, every wave slot used four times over.

References.  (i) trt_render_moments_device of the same frame on the same device, compared there on int32 views: every listed pixel equal
in both buffers, every unlisted pixel and every guard still the sentinel, counter[0] == 2 x len(list).  (ii) The oracle's orc.render of
single image rows: the rows that hold the entries rays_per_wave x w - 1 and rays_per_wave x w for w = 1, a wave in the middle and the last
wave, and the row of entry n0; `accum` bit for bit.  Negative controls: the list with two entries swapped across a run boundary gives the
same bytes everywhere; a reference frame rendered with seed + 1 differs from it, through the same comparison.

Measured on one MI355X (256 compute units, where n0 + 1 is as above: runs of 320 entries in 9831 / 13 108 / 16 385 waves): one sparse
render of the list takes 2 ms (random_spheres), 9 ms (prims600) and 4 ms (grid3000); the whole case - compilation, five device renders
of 3 to 5 million pixels, the comparisons and the oracle's four or five rows - 1.7 s for the first (it warms the device up), 0.1 s and 0.2 s
for the others.  So N and max_bounces stay as the cases were specified.  Every GPU step is one in-process call."""
import time

import numpy as np
import pytest

import test_gpu_pixels as P
import test_gpu_queries as G
import walk_ray_cases as W

pytestmark = pytest.mark.gpu

SCENES = ["random_spheres", "prims600", "grid3000"]
WIDTH, N, BOUNCES = 2048, 2, 4
G12 = P.GUARD * 12
SENTINEL = -0x32323233                                                      # 0xCDCDCDCD as int32


def payload(t, npix):
    """The frame inside a guarded device buffer as int32 [npix, 3]."""
    import torch
    return t[G12:G12 + npix * 12].view(torch.int32).view(npix, 3)


def first_mismatches(got, want, listed):
    """Indices (at most 5, copied back only on a mismatch) of the pixels among the first `listed` whose three words differ."""
    import torch
    if torch.equal(got[:listed], want[:listed]):
        return []
    return (got[:listed] != want[:listed]).any(dim=1).nonzero().flatten()[:5].cpu().tolist()


def untouched(t, npix, listed):
    """Every unlisted pixel of the frame is still the sentinel and both guards still hold their fill."""
    return bool((payload(t, npix)[listed:] == SENTINEL).all()) and bool((t[:G12] == P.FILL).all()) and bool((t[G12 + npix * 12:] == P.FILL).all())


@pytest.mark.parametrize("name", SCENES)
def test_runs_longer_than_256_entries(trt, orc, name):
    import torch
    t_start = time.perf_counter()
    desc = W.scene(trt, name)
    slots = trt.world_from_description(desc)[0].get_bvh().pixels_plan(1)["wave_slots"]
    n0 = 256 * slots
    height = -(-(n0 + 1) // WIDTH) + 1
    npix = WIDTH * height
    desc = dict(desc, camera=dict(desc["camera"], width=WIDTH, height=height))
    world, cam = trt.world_from_description(desc)
    sc = world.get_bvh()
    at, past = sc.pixels_plan(n0), sc.pixels_plan(n0 + 1)
    assert G.plan_shape(past) == G.DEFAULT_SHAPES[name] and past["wave_slots"] == slots, past
    assert at["rays_per_wave"] == 256 and at["waves"] == slots, at
    per_wave, waves = past["rays_per_wave"], past["waves"]
    assert per_wave == ((-(-(n0 + 1) // slots) + 63) & ~63) and per_wave > 256, past
    assert (waves - 1) * per_wave < n0 + 1 <= waves * per_wave and waves <= slots, past
    assert n0 + 1 < npix
    print(f"\n{name}: {past['compute_units']} CUs, {past['threads_per_workgroup']} lanes, wave slots {slots}: n0 = {n0}, image {WIDTH} x {height}; "
          f"n0 + 1 entries: {per_wave} per wave, {waves} waves, the last owns {n0 + 1 - (waves - 1) * per_wave}")

    renderer = trt.Renderer(N, 1, BOUNCES, False, desc["background"], seed=P.SEED)
    dev = torch.device("cuda:0")

    def whole_frame(r):
        s = torch.zeros(npix * 3, dtype=torch.float32, device=dev)
        m = torch.zeros(npix * 3, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        r.render_moments_device(cam, sc, s.data_ptr(), m.data_ptr())
        torch.cuda.synchronize()
        return s.view(torch.int32).view(npix, 3), m.view(torch.int32).view(npix, 3)

    def sparse(d_px, n):
        d_s, d_m = P.device_frame(torch, npix), P.device_frame(torch, npix)
        ctr = torch.zeros(16, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        renderer.render_pixels_device(cam, sc, d_px.data_ptr(), n, d_s.data_ptr() + G12, d_m.data_ptr() + G12, d_counters_ptr=ctr.data_ptr())
        torch.cuda.synchronize()
        print(f"{name}: sparse render of {n} entries: {time.perf_counter() - t0:.3f} s")
        return d_s, d_m, ctr

    ref_s, ref_m = whole_frame(renderer)
    d_px = torch.arange(n0 + 1, dtype=torch.int32, device=dev)
    long_s, long_m = None, None
    for n in (n0 + 1, n0):
        d_s, d_m, ctr = sparse(d_px, n)
        for got, want, tag in ((d_s, ref_s, "accum"), (d_m, ref_m, "moment2")):
            bad = first_mismatches(payload(got, npix), want, n)
            assert not bad, (name, n, tag, "first differing entries", bad, "(wave, entry of its run)", [divmod(i, per_wave if n > n0 else 256) for i in bad])
            assert untouched(got, npix, n), (name, n, tag, "an unlisted pixel or a guard was written")
        assert int(ctr[0]) == N * n and int(ctr[1]) >= int(ctr[0]) and not bool(ctr[2:].any()), (name, n, ctr.tolist())
        if n == n0 + 1:
            long_s, long_m = d_s, d_m
    del d_s, d_m

    # negative controls: two entries swapped across the boundary of the first two runs change no byte; a frame of another seed is seen
    swapped = d_px.clone()
    swapped[per_wave - 1], swapped[per_wave] = per_wave, per_wave - 1
    sw_s, sw_m, ctr = sparse(swapped, n0 + 1)
    assert torch.equal(sw_s, long_s) and torch.equal(sw_m, long_m), (name, "the order of the list changed the frame")
    assert int(ctr[0]) == N * (n0 + 1)
    del sw_s, sw_m, swapped
    other_s, other_m = whole_frame(trt.Renderer(N, 1, BOUNCES, False, desc["background"], seed=P.SEED + 1))
    assert first_mismatches(payload(long_s, npix), other_s, n0 + 1) and first_mismatches(payload(long_m, npix), other_m, n0 + 1), \
        (name, "the comparison cannot tell a frame of another seed")
    del other_s, other_m, ref_s, ref_m

    # the oracle around the run boundaries of the long list (entry i is pixel i)
    entries = sorted({e for w in (1, waves // 2, waves - 1) for e in (per_wave * w - 1, per_wave * w)} | {n0})
    assert 5 <= len(entries) <= 7 and entries[-1] == n0 and 1 < waves // 2 < waves - 1
    rows = sorted({e // WIDTH for e in entries})
    ow, ocam = orc.world_from_description(desc)
    frame = np.zeros((height, WIDTH, 3), np.float32)
    got = payload(long_s, npix).view(height, WIDTH, 3)
    seen = []
    for row in rows:
        orc.render(ow, ocam, N, BOUNCES, desc["background"], seed=P.SEED, nthreads=4, row_begin=row, row_end=row + 1, accum=frame)
        listed = min(WIDTH, n0 + 1 - row * WIDTH)
        assert listed >= 1
        g = got[row].cpu().numpy().view(np.float32)
        bad = np.flatnonzero((g[:listed].view(np.uint32) != frame[row, :listed].view(np.uint32)).any(axis=1))
        assert len(bad) == 0, (name, "row", row, "first differing entries", (row * WIDTH + bad[:5]).tolist(), g[bad[0]], frame[row, bad[0]])
        seen.append(frame[row, :listed].view(np.uint32))
    assert len(np.unique(np.concatenate(seen), axis=0)) >= 20, (name, rows, "the oracle's rows are nearly constant")
    print(f"{name}: oracle rows {rows}; the whole case took {time.perf_counter() - t_start:.1f} s")
