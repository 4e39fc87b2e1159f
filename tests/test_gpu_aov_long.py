"""The feature buffers (trt_render_aov_device) and the primary-ray export (trt_primary_rays_device) at frame size: images of more pixels
than 256 x wave_slots, where a wave's run of pixels grows beyond 256 (stream_plan.h plan_batch) - wave w no longer begins at a multiple of
256, the refill cursor of the resumable walks and the `base += 64` loop of the others run more than four rounds, and the last wave owns a
ragged rest - against the same frame folded on the device from the exported rays and trt_intersect_device, and, around the run
boundaries, against the CPU oracle.

Scenes (default compilation, shape asserted): cornell (lock-step list, 256 lanes), random_spheres (LDS tree, 768 lanes), prims600
(register slots through the fallback, 512 lanes), grid3000 (16-byte nodes from global memory, 256 lanes): both loops that run to their end
and both resumable ones.  Sizes (tests/aov_long_cases.py; read from Scene.aov_plan of the device at hand, never assumed; the same
arithmetic runs without a GPU in tests/test_aov_long_cases.py): with n0 = 256 x wave_slots, the long image is int(sqrt(n0 x 131 / 70)) | 1
wide - odd, so runs begin at every column - and n0 // width + 1 high: runs of 320.  2 samples per pixel, seed 5, device forms only, all
six buffers, the ray buffer and the record buffer with 64 pixels of 0xCD on either side, looked at after every call.

References.  (i) Per sample: trt_primary_rays_device, trt_intersect_device, then the imager's rule in float32 as separate torch
operations (acc = acc + value * inv; depth and coverage only where the sample hit; albedo from the description's material table or the
background; the indices of sample 0).  Every pixel of every buffer on int32 views, a NaN of the reference by NaN-ness; at most five
mismatches come back, each as (wave, entry of its run, row, column).  The queries at this length are pinned to the oracle by their own
suite; this pins fold, ownership and addressing.  (ii) The oracle at the 32 pixels either side of 96 run boundaries and the last 64 of
the image: the exported rays are the restated rays (tests/test_gpu_aov.py), the six buffers the numpy fold of the oracle's first hits; the
oracle's hit share there lies in [0.05, 0.95] with at least 7 geometries, sample 0 with hits and misses.  (iii) The image of exactly n0
pixels, 2048 wide - runs of 256, every wave slot used - against (i).

Also on the long image: sample ranges [0, 1) then [1, 2) with accumulate give the one-pass bytes and leave the indices alone; a render
with seed + 1 and reference (i) rolled by one pixel are both seen to differ, in every buffer, by the comparison that passes above.  On
the image of twice the rows (cornell, random_spheres; runs of 576, compared with (i) as well): the first of two shards of 16-row bands
owns more than n0 pixels and equals those rows of the full image, buffers and exported rays.

Measured on one MI355X (256 compute units).  The long images are 3707 x 1981 (cornell), 3431 x 1834 (random_spheres), 2801 x 1498
(prims600) and 3963 x 2117 (grid3000): 4.2 to 8.4 million pixels in runs of 320 over 13 113 to 26 218 waves, the last of which owns 207,
294, 58 and 231 pixels; the doubled images have 14.7 and 12.6 million pixels in runs of 576, their shards runs of 320.  One render of
the six buffers takes 1 to 2 ms at every size.  A long-image case - five renders, the device fold, the controls and the oracle's 6208
pixels - takes 0.9 s for the first (it warms the device up) and 0.1 to 0.2 s for the others; an n0 case and a band case take less than
0.05 s each; the module's ten cases 3.5 s.  All comparisons of whole frames stay on the device.
Every GPU step is one in-process call; nothing is built here and no child process is started."""
import time

import numpy as np
import pytest

import aov_long_cases as L
import test_gpu_aov as A

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xCD
SPP, SEED = L.SPP, L.SEED
FLOAT_CHANNELS = ("albedo", "normal", "depth", "coverage")


@pytest.fixture(scope="module")
def scene(trt):
    """name -> (description, compiled scene), compiled once."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = L.scene_and_description(trt, name)
        return cache[name]

    return get


def guarded(n, item):
    """uint8 on the device: n items of `item` bytes between two guards of 64 items, all filled with 0xCD."""
    import torch
    return torch.full(((GUARD + n + GUARD) * item,), FILL, dtype=torch.uint8, device="cuda:0")


def inside(t, n, item):
    """What lies between the guards, as int32 [n, item / 4]."""
    import torch
    return t[GUARD * item:(GUARD + n) * item].view(torch.int32).view(n, item // 4)


def guards_intact(t, n, item):
    return bool((t[:GUARD * item] == FILL).all()) and bool((t[(GUARD + n) * item:] == FILL).all())


def new_buffers(trt, n):
    return {ch: guarded(n, 4 * k) for ch, (_, k) in trt.AOV_CHANNELS.items()}


def views(trt, bufs, n):
    return {ch: inside(t, n, 4 * trt.AOV_CHANNELS[ch][1]) for ch, t in bufs.items()}


def render(trt, renderer, cam, sc, n, bufs=None, **over):
    """One trt_render_aov_device into guarded buffers (fresh ones unless given); every guard is looked at.  Returns (buffers, seconds)."""
    import torch
    bufs = new_buffers(trt, n) if bufs is None else bufs
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    renderer.render_aov_device(cam, sc, {ch: t.data_ptr() + GUARD * 4 * trt.AOV_CHANNELS[ch][1] for ch, t in bufs.items()}, **over)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    for ch, t in bufs.items():
        assert guards_intact(t, n, 4 * trt.AOV_CHANNELS[ch][1]), (ch, over, "a guard was written")
    return bufs, seconds


def device_reference(desc, cam, sc, n, **bands):
    """Reference (i) for the local image of n pixels: (channel -> int32 [n, k], the exported rays of each sample as int32 [n, 6])."""
    import torch
    dev, f32 = torch.device("cuda:0"), torch.float32
    mats = torch.tensor([list(m[2]) for m in desc["materials"]], dtype=f32, device=dev)
    background = torch.tensor(list(desc["background"]), dtype=f32, device=dev)
    inv = torch.tensor(float(L.INV), dtype=f32, device=dev)
    one = torch.ones((), dtype=f32, device=dev)
    albedo, normal = torch.zeros((n, 3), dtype=f32, device=dev), torch.zeros((n, 3), dtype=f32, device=dev)
    depth, coverage = torch.zeros(n, dtype=f32, device=dev), torch.zeros(n, dtype=f32, device=dev)
    geometry = material = None
    exported = []
    for s in range(SPP):
        rays, hits = guarded(n, 24), guarded(n, 28)
        cam.primary_rays_device(s, SPP, rays.data_ptr() + GUARD * 24, seed=SEED, **bands)
        sc.intersect_device(rays.data_ptr() + GUARD * 24, n, hits.data_ptr() + GUARD * 28)
        torch.cuda.synchronize()
        assert guards_intact(rays, n, 24) and guards_intact(hits, n, 28), (s, "a guard of the rays or of the records was written")
        rec = inside(hits, n, 28)                                           # trt_hit: t, geometry, material, front_face, normal
        hit = rec[:, 1] != -1
        t = rec[:, 0].view(f32)
        value = torch.where(hit[:, None], mats[torch.where(hit, rec[:, 2], 0).long()], background[None, :])
        albedo = albedo + value * inv
        normal = normal + rec[:, 4:7].view(f32) * inv
        depth = torch.where(hit, depth + t * inv, depth)
        coverage = torch.where(hit, coverage + one * inv, coverage)
        if s == 0:
            geometry, material = rec[:, 1].clone(), rec[:, 2].clone()
        exported.append(inside(rays, n, 24))
        del hits, rec
    i32 = torch.int32
    want = dict(albedo=albedo.view(i32), normal=normal.view(i32), depth=depth.view(i32).view(n, 1), coverage=coverage.view(i32).view(n, 1),
                geometry=geometry.view(n, 1), material=material.view(n, 1))
    return want, exported


def first_mismatches(got, want, is_float):
    """Indices (at most 5, copied back only on a mismatch) of the pixels at which int32 [n, k] `got` is not `want`: bits, or, where a
    float of `want` is NaN, NaN-ness."""
    import torch
    assert got.shape == want.shape and got.dtype == want.dtype == torch.int32, (got.shape, want.shape)
    if torch.equal(got, want):
        return []
    same = got == want
    if is_float:
        same = torch.where(torch.isnan(want.view(torch.float32)), torch.isnan(got.view(torch.float32)), same)
    return (~same).any(dim=1).nonzero().flatten()[:5].cpu().tolist()


def differences(got, want):
    """channel -> first mismatches, for the channels that have any."""
    out = {}
    for ch in want:
        bad = first_mismatches(got[ch], want[ch], ch in FLOAT_CHANNELS)
        if bad:
            out[ch] = bad
    return out


def assert_frames_equal(got, want, im, what):
    for ch, bad in differences(got, want).items():
        located = [divmod(i, im["per_wave"]) + divmod(i, im["width"]) for i in bad]
        raise AssertionError((what, ch, "first differing pixels as (wave, entry of its run, row, column)", located,
                              got[ch][bad[0]].cpu().tolist(), want[ch][bad[0]].cpu().tolist()))


def as_numpy(trt, ch, t):
    """int32 [k, c] from the device as the channel's numpy type, [k, 3] or [k]."""
    dtype, c = trt.AOV_CHANNELS[ch]
    a = t.cpu().numpy().view(dtype)
    return a if c == 3 else a.reshape(-1)


@pytest.mark.parametrize("name", L.SCENES)
def test_an_image_whose_runs_are_longer_than_256_pixels(trt, orc, scene, name):
    import torch
    t_start = time.perf_counter()
    desc, sc = scene(name)
    im = L.sizes(sc, name)["long"]
    n = im["n"]
    assert im["per_wave"] > 256 and n % im["per_wave"] != 0
    desc = L.with_camera(desc, im["width"], im["height"])
    cam = trt.Camera(**desc["camera"])
    renderer = trt.Renderer(SPP, 1, 50, False, desc["background"], seed=SEED)
    print("\n" + L.describe(name, "long", im))

    bufs, seconds = render(trt, renderer, cam, sc, n)
    got = views(trt, bufs, n)
    want, exported = device_reference(desc, cam, sc, n)
    assert_frames_equal(got, want, im, (name, "against the fold of trt_intersect_device on the exported rays"))
    print(f"{name}: one render of the six buffers: {seconds:.3f} s")

    # split sample ranges: the one-pass bytes, guards included; the second pass leaves the indices as the first wrote them
    split, _ = render(trt, renderer, cam, sc, n, sample_begin=0, sample_end=1)
    first_pass = {ch: split[ch].clone() for ch in ("geometry", "material")}
    assert not torch.equal(split["coverage"], bufs["coverage"])             # (one of two samples: not the frame yet)
    render(trt, renderer, cam, sc, n, bufs=split, sample_begin=1, sample_end=2, accumulate=1)
    for ch in trt.AOV_CHANNELS:
        assert torch.equal(split[ch], bufs[ch]), (name, ch, "two passes differ from one", differences(views(trt, split, n), got))
    assert torch.equal(split["geometry"], first_pass["geometry"]) and torch.equal(split["material"], first_pass["material"])
    del split, first_pass

    # negative controls, through the comparison that passed above: another seed, and the reference off by one pixel
    other, _ = render(trt, trt.Renderer(SPP, 1, 50, False, desc["background"], seed=SEED + 1), cam, sc, n)
    assert set(differences(views(trt, other, n), want)) == set(trt.AOV_CHANNELS), (name, "a frame of another seed goes unseen")
    del other
    rolled = {ch: torch.roll(w, 1, 0) for ch, w in want.items()}
    assert set(differences(got, rolled)) == set(trt.AOV_CHANNELS), (name, "a frame that is off by one pixel goes unseen")
    del rolled

    # the oracle around the run boundaries
    picked = L.picked_pixels(im)
    o = L.oracle_at(orc, desc, picked)
    print(f"{name}: {len(picked)} picked pixels: oracle hit share {o['share']:.2f}, {o['geometries']} geometries")
    L.assert_not_vacuous(name, o)
    idx = torch.from_numpy(picked).to("cuda:0")
    for s in range(SPP):
        rays = exported[s][idx].cpu().numpy().view(np.float32)
        assert not np.isnan(o["rays"][s]).any()
        A.assert_same(rays, o["rays"][s], (name, "exported rays of sample", s, "index into the picked pixels"))
    for ch in trt.AOV_CHANNELS:
        A.assert_same(as_numpy(trt, ch, got[ch][idx]), o["buffers"][ch], (name, ch, "against the oracle, index into the picked pixels"))
    print(f"{name}: the whole case took {time.perf_counter() - t_start:.1f} s")


@pytest.mark.parametrize("name", L.SCENES)
def test_an_image_of_exactly_256_pixels_per_wave_slot(trt, scene, name):
    t_start = time.perf_counter()
    desc, sc = scene(name)
    im = L.sizes(sc, name)["at_n0"]
    n = im["n"]
    assert im["per_wave"] == 256 and im["width"] == 2048 and sc.aov_plan(n)["waves"] == sc.aov_plan(n)["wave_slots"]
    desc = L.with_camera(desc, im["width"], im["height"])
    cam = trt.Camera(**desc["camera"])
    print("\n" + L.describe(name, "at n0", im))
    bufs, seconds = render(trt, trt.Renderer(SPP, 1, 50, False, desc["background"], seed=SEED), cam, sc, n)
    want, _ = device_reference(desc, cam, sc, n)
    assert_frames_equal(views(trt, bufs, n), want, im, (name, "n0", "against the fold of trt_intersect_device on the exported rays"))
    print(f"{name}: one render: {seconds:.3f} s; the whole case took {time.perf_counter() - t_start:.1f} s")


@pytest.mark.parametrize("name", L.BAND_SCENES)
def test_a_band_shard_of_more_than_n0_pixels_is_its_rows_of_the_full_image(trt, scene, name):
    import torch
    t_start = time.perf_counter()
    desc, sc = scene(name)
    z = L.sizes(sc, name)
    full, shard, long = z["doubled"], z["shard"], z["long"]
    assert shard["n"] > z["n0"] and shard["per_wave"] > 256 and full["per_wave"] > long["per_wave"] and full["height"] == 2 * long["height"]
    desc = L.with_camera(desc, full["width"], full["height"])
    cam = trt.Camera(**desc["camera"])
    renderer = trt.Renderer(SPP, 1, 50, False, desc["background"], seed=SEED)
    print("\n" + L.describe(name, "doubled", full) + "\n" + L.describe(name, "shard", shard))

    whole, seconds = render(trt, renderer, cam, sc, full["n"])
    whole = views(trt, whole, full["n"])
    want, exported = device_reference(desc, cam, sc, full["n"])
    assert_frames_equal(whole, want, full, (name, "doubled", "against the fold of trt_intersect_device on the exported rays"))
    del want

    rows = torch.tensor(shard["rows"], dtype=torch.long, device="cuda:0")
    assert len(rows) == shard["height"]
    rows_of = lambda t: t.view(full["height"], full["width"], -1)[rows].reshape(shard["n"], -1)        # noqa: E731
    part, part_seconds = render(trt, renderer, cam, sc, shard["n"], **shard["bands"])
    assert_frames_equal(views(trt, part, shard["n"]), {ch: rows_of(t) for ch, t in whole.items()}, shard, (name, "shard against the full image's rows"))
    rays = guarded(shard["n"], 24)
    cam.primary_rays_device(1, SPP, rays.data_ptr() + GUARD * 24, seed=SEED, **shard["bands"])
    torch.cuda.synchronize()
    assert guards_intact(rays, shard["n"], 24)
    bad = first_mismatches(inside(rays, shard["n"], 24), rows_of(exported[1]), False)
    assert not bad, (name, "exported rays of the shard, (local row, column)", [divmod(i, shard["width"]) for i in bad])
    # the comparison sees a shard that is one row off
    assert first_mismatches(inside(rays, shard["n"], 24), torch.roll(rows_of(exported[1]), shard["width"], 0), False)
    print(f"{name}: full render {seconds:.3f} s, shard render {part_seconds:.3f} s; the whole case took {time.perf_counter() - t_start:.1f} s")
