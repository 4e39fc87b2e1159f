"""Sparse rendering of listed pixels (trt_render_pixels and its device form) on the GPU, bit for bit against the CPU oracle.

The checker.  The frame a list is compared with is orc.render's for the same sample range; the second moments are the numpy fold of the
oracle's per-sample colours, recovered exactly at power-of-two spp the way tests/test_gpu_moments.py does it: for N a power of two the
oracle's render of the single sample s at samples_per_pixel = N is c_s * (1/N), times N that is c_s (denoise_color_cases.oracle_samples
asserts the condition), and numpy folds S = S + c * (1/N), M.ch = M.ch + (c.ch * c.ch) * (1/N) in float32 in sample order
(denoise_color_cases.fold_moments).  The same fold continued from given prior contents is what an accumulating pass must leave.

Scenes (tests/walk_ray_cases.py), one per walk: cornell (lock-step list), prims33 (LDS tree, 256 lanes), random_spheres and mixed400 (LDS
trees, 768 lanes), prims600 (register slots through the launch plan's fallback), grid3000 (16-byte nodes from global memory); every case
asserts the kernel shape Scene.pixels_plan reports.  Images: 2 x 2 (the smallest there is), 8 x 8, 19 x 13 (ragged) and 40 x 30 (1200
pixels: more than the 1024 entries the four waves of a 256-lane workgroup own, so two workgroups).  N = 4 and 8, max_bounces 8, seed 5.

Lists: empty, one pixel, 63 / 64 / 65 pixels (both sides of a wave; cut to the image where it is smaller), all pixels ascending and
descending, a fixed shuffle, every third pixel.  Every comparison is over every byte of both buffers: the listed pixels against the
restatement, every other pixel and - in the device form - 64 pixels of guard on either side against the sentinel they were filled with.
Every GPU step is one in-process call."""
import numpy as np
import pytest

import denoise_color_cases as D
import test_gpu_queries as G
import walk_ray_cases as W

pytestmark = pytest.mark.gpu

SEED = 5
SCENES = ["cornell", "prims33", "random_spheres", "mixed400", "prims600", "grid3000"]
SIZES = [(2, 2), (8, 8), (19, 13), (40, 30)]
SPPS = [4, 8]
BOUNCES = 8
GUARD = 64                                                                  # pixels on either side of a device buffer
FILL = 0xCD


def sentinel(shape):
    return np.full(shape, 0xCDCDCDCD, np.uint32).view(np.float32)


def is_sentinel(a):
    return a.view(np.uint32) == 0xCDCDCDCD


def lists_of(npix):
    """name -> uint32 list of distinct local pixel indices."""
    rng = np.random.default_rng(1234)
    shuffle = rng.permutation(npix).astype(np.uint32)
    out = {"empty": np.zeros(0, np.uint32), "one": np.array([npix // 2], np.uint32)}
    for k in (63, 64, 65):
        out[str(k)] = np.sort(shuffle[:min(k, npix)])[::-1].copy() if k == 64 else shuffle[:min(k, npix)].copy()
    out["ascending"] = np.arange(npix, dtype=np.uint32)
    out["descending"] = np.arange(npix, dtype=np.uint32)[::-1].copy()
    out["shuffle"] = shuffle
    out["third"] = np.arange(0, npix, 3, dtype=np.uint32)
    return out


@pytest.fixture(scope="module")
def case(trt, orc):
    """(scene, (width, height), N) -> description, product world / camera / scene / renderer, the oracle's exact samples, the restated S
    and M of the whole range and the oracle's own frame; computed once on first use, shared, never changed."""
    cache = {}

    def get(name, size, n):
        key = (name, size, n)
        if key not in cache:
            desc = W.scene(trt, name)
            desc = dict(desc, camera=dict(desc["camera"], width=size[0], height=size[1]))
            ow, ocam = orc.world_from_description(desc)
            world, cam = trt.world_from_description(desc)
            sc = world.get_bvh()
            npix = size[0] * size[1]
            plan = sc.pixels_plan(npix)
            assert G.plan_shape(plan) == G.DEFAULT_SHAPES[name], (name, plan)
            assert plan["rays_per_wave"] == 256 and plan["workgroups"] == -(-(-(-npix // 256)) // (plan["threads_per_workgroup"] // 64)), plan
            if size == (40, 30) and plan["threads_per_workgroup"] == 256:
                assert plan["workgroups"] == 2
            samples = D.oracle_samples(orc, ow, ocam, n, BOUNCES, desc["background"], SEED)
            s, m = D.fold_moments(samples, n)
            frame, _ = orc.render(ow, ocam, n, BOUNCES, desc["background"], seed=SEED, nthreads=4)
            D.assert_same(s, frame, (name, size, n, "the restated fold is not the oracle's frame"))
            for a in (samples, s, m):
                a.setflags(write=False)
            renderer = trt.Renderer(n, 1, BOUNCES, False, desc["background"], seed=SEED)
            cache[key] = dict(desc=desc, ow=ow, ocam=ocam, world=world, cam=cam, scene=sc, renderer=renderer, samples=samples, S=s, M=m, n=n,
                              size=size, npix=npix)
        return cache[key]

    return get


CASES = [(name, size, n) for name in SCENES for size in SIZES for n in SPPS]
CASE_IDS = ["%s-%dx%d-%dspp" % (name, w, h, n) for name, (w, h), n in CASES]
SMALL = [(name, (19, 13), 8) for name in SCENES]
SMALL_IDS = [name for name in SCENES]


def check_frames(accum, m2, px, want_s, want_m, what, rest_s=None, rest_m=None):
    """The listed pixels hold want_*; every other pixel holds rest_* (None: the sentinel)."""
    h, w, _ = accum.shape
    listed = np.zeros(h * w, bool)
    listed[px] = True
    for got, want, rest, tag in ((accum, want_s, rest_s, "accum"), (m2, want_m, rest_m, "moment2")):
        if got is None:
            continue
        g, wv = got.reshape(-1, 3), want.reshape(-1, 3)
        D.assert_same(np.ascontiguousarray(g[listed]), np.ascontiguousarray(wv[listed]), (what, tag, "listed pixels"))
        if rest is None:
            assert is_sentinel(g[~listed]).all(), (what, tag, "an unlisted pixel was written")
        else:
            assert g[~listed].tobytes() == rest.reshape(-1, 3)[~listed].tobytes(), (what, tag, "an unlisted pixel was written")


@pytest.mark.parametrize("name,size,n", CASES, ids=CASE_IDS)
def test_listed_pixels_equal_the_oracle_and_nothing_else_is_written(trt, case, name, size, n):
    c = case(name, size, n)
    shape = (size[1], size[0], 3)
    for lname, px in lists_of(c["npix"]).items():
        accum, m2 = sentinel(shape), sentinel(shape)
        st = c["renderer"].render_pixels(c["cam"], c["scene"], px, accum, m2)
        check_frames(accum, m2, px, c["S"], c["M"], (name, size, n, lname))
        assert st["samples"] == len(px) * n, (lname, st)
        assert st["rays"] >= st["samples"] and st["node_tests"] == 0
        # without a second-moment buffer: the same frame
        only = sentinel(shape)
        c["renderer"].render_pixels(c["cam"], c["scene"], px, only, None)
        assert only.tobytes() == accum.tobytes(), (name, size, n, lname, "moment2 = NULL changes the frame")


@pytest.mark.parametrize("name,size,n", CASES, ids=CASE_IDS)
def test_all_pixels_equal_render_moments_byte_for_byte(trt, case, name, size, n):
    c = case(name, size, n)
    shape = (size[1], size[0], 3)
    want_s, want_m, want_st = c["renderer"].render_moments(c["cam"], c["scene"])
    for lname in ("ascending", "descending", "shuffle"):
        accum, m2 = sentinel(shape), sentinel(shape)
        st = c["renderer"].render_pixels(c["cam"], c["scene"], lists_of(c["npix"])[lname], accum, m2)
        assert accum.tobytes() == want_s.tobytes() and m2.tobytes() == want_m.tobytes(), (name, size, n, lname)
        assert st["samples"] == want_st["samples"] and st["rays"] == want_st["rays"], (st, want_st)


@pytest.mark.parametrize("name,size,n", SMALL, ids=SMALL_IDS)
def test_split_sample_ranges_with_accumulate_equal_one_pass(trt, case, name, size, n):
    c = case(name, size, n)
    r, cam, sc = c["renderer"], c["cam"], c["scene"]
    shape = (size[1], size[0], 3)
    lists = lists_of(c["npix"])
    for lname in ("65", "third", "shuffle"):
        px = lists[lname]
        accum, m2 = sentinel(shape), sentinel(shape)
        r.render_pixels(cam, sc, px, accum, m2, sample_begin=0, sample_end=3)
        s3, m3 = D.fold_moments(c["samples"], n, 0, 3)
        check_frames(accum, m2, px, s3, m3, (name, lname, "[0, 3)"))
        r.render_pixels(cam, sc, px, accum, m2, sample_begin=3, sample_end=n, accumulate=1)
        check_frames(accum, m2, px, c["S"], c["M"], (name, lname, "[0, 3) + [3, n)"))
    # the same prior contents: an accumulating pass continues whatever the buffers hold, as the fold from that start does
    rng = np.random.default_rng(7)
    prior_s, prior_m = rng.random(shape, np.float32), rng.random(shape, np.float32)
    want_s, want_m = D.fold_moments(c["samples"], n, 2, 7, start=(prior_s, prior_m))
    accum, m2 = prior_s.copy(), prior_m.copy()
    r.render_pixels(cam, sc, lists["third"], accum, m2, sample_begin=2, sample_end=7, accumulate=1)
    check_frames(accum, m2, lists["third"], want_s, want_m, (name, "prior contents"), rest_s=prior_s, rest_m=prior_m)
    # a sparse pass refines a frame of render_moments: the listed pixels are the full render's, the others keep the shorter range
    a0, b0, _ = r.render_moments(cam, sc, sample_begin=0, sample_end=4)
    keep_s, keep_m = a0.copy(), b0.copy()
    r.render_pixels(cam, sc, lists["third"], a0, b0, sample_begin=4, sample_end=n, accumulate=1)
    check_frames(a0, b0, lists["third"], c["S"], c["M"], (name, "refined"), rest_s=keep_s, rest_m=keep_m)


@pytest.mark.parametrize("name,size,n", [(name, size, 8) for name in SCENES for size in ((19, 13), (40, 30))],
                         ids=["%s-%dx%d" % (name, w, h) for name in SCENES for (w, h) in ((19, 13), (40, 30))])
def test_a_band_shard_of_eight_rows(trt, case, name, size, n):
    c = case(name, size, n)
    width, height = size
    seen = np.zeros(height, np.int32)
    for rank in range(2):
        rows = np.array([y for y in range(height) if (y // 8) % 2 == rank])
        local = len(rows) * width
        shape = (len(rows), width, 3)
        for px in (np.arange(local, dtype=np.uint32), np.arange(1, local, 3, dtype=np.uint32)[::-1].copy()):
            accum, m2 = sentinel(shape), sentinel(shape)
            c["renderer"].render_pixels(c["cam"], c["scene"], px, accum, m2, band_rows=8, band_stride=2, band_offset=rank, rows_local=len(rows))
            check_frames(accum, m2, px, np.ascontiguousarray(c["S"][rows]), np.ascontiguousarray(c["M"][rows]), (name, size, "shard", rank))
        seen[rows] += 1
    assert (seen == 1).all()


def device_frame(torch, npix):
    return torch.full(((GUARD + npix + GUARD) * 12,), FILL, dtype=torch.uint8, device="cuda:0")


def frame_of(t, npix, shape):
    """(payload as float32 [shape], guards intact?)"""
    h = t.cpu().numpy()
    g = GUARD * 12
    return h[g:g + npix * 12].copy().view(np.float32).reshape(shape), bool((h[:g] == FILL).all() and (h[g + npix * 12:] == FILL).all())


@pytest.mark.parametrize("name,size,n", CASES, ids=CASE_IDS)
def test_device_form_on_a_side_stream_equals_the_host_form_and_leaves_the_guards(trt, case, name, size, n):
    import torch
    c = case(name, size, n)
    npix, shape = c["npix"], (size[1], size[0], 3)
    side = torch.cuda.Stream()
    lists = lists_of(npix)
    for lname in ("one", "65", "descending", "shuffle", "third"):
        px = lists[lname]
        host_s, host_m = sentinel(shape), sentinel(shape)
        c["renderer"].render_pixels(c["cam"], c["scene"], px, host_s, host_m)
        for stream in (None, side):
            d_s, d_m = device_frame(torch, npix), device_frame(torch, npix)
            d_px = torch.from_numpy(px.astype(np.int64)).to(torch.int32).to("cuda:0") if len(px) else torch.zeros(1, dtype=torch.int32, device="cuda:0")
            ctr = torch.zeros(16, dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()
            ptr = 0 if stream is None else stream.cuda_stream
            c["renderer"].render_pixels_device(c["cam"], c["scene"], d_px.data_ptr(), len(px), d_s.data_ptr() + GUARD * 12, d_m.data_ptr() + GUARD * 12,
                                               stream_ptr=ptr, d_counters_ptr=ctr.data_ptr())
            (torch.cuda.current_stream() if stream is None else stream).synchronize()
            torch.cuda.synchronize()
            got_s, ok_s = frame_of(d_s, npix, shape)
            got_m, ok_m = frame_of(d_m, npix, shape)
            assert ok_s and ok_m, (name, size, n, lname, "guard bytes were written")
            assert got_s.tobytes() == host_s.tobytes() and got_m.tobytes() == host_m.tobytes(), (name, size, n, lname, stream is not None)
            assert int(ctr[0]) == len(px) * n and int(ctr[1]) >= int(ctr[0]) and not bool(ctr[2:].any())


@pytest.mark.parametrize("name,size,n", [(name, size, 8) for name in SCENES for size in ((19, 13), (40, 30))],
                         ids=["%s-%dx%d" % (name, w, h) for name in SCENES for (w, h) in ((19, 13), (40, 30))])
def test_device_count_and_an_entry_past_the_image(trt, case, name, size, n):
    """d_count smaller than n traces only the prefix (also when it is larger than n: then n entries).  An entry equal to rows * width is
    skipped: were it traced it would land in the guard behind the buffer, which is checked - the test cannot fault anything."""
    import torch
    c = case(name, size, n)
    npix, shape = c["npix"], (size[1], size[0], 3)
    px = lists_of(npix)["shuffle"]
    d_px = torch.from_numpy(px.astype(np.int64)).to(torch.int32).to("cuda:0")
    for count, used in ((npix // 3, npix // 3), (0, 0), (65, 65), (npix + 1000, npix)):
        d_s, d_m = device_frame(torch, npix), device_frame(torch, npix)
        d_count = torch.tensor([count], dtype=torch.int32, device="cuda:0")
        ctr = torch.zeros(16, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        c["renderer"].render_pixels_device(c["cam"], c["scene"], d_px.data_ptr(), npix, d_s.data_ptr() + GUARD * 12, d_m.data_ptr() + GUARD * 12,
                                           d_count_ptr=d_count.data_ptr(), d_counters_ptr=ctr.data_ptr())
        torch.cuda.synchronize()
        got_s, ok_s = frame_of(d_s, npix, shape)
        got_m, ok_m = frame_of(d_m, npix, shape)
        assert ok_s and ok_m
        check_frames(got_s, got_m, px[:used], c["S"], c["M"], (name, size, "d_count", count))
        assert int(ctr[0]) == used * n
    # one entry past the image among 130 good ones (in the second wave's lanes), and a list of nothing but such entries
    good = px[:130]
    for bad in (np.concatenate([good[:70], [npix], good[70:]]).astype(np.uint32), np.full(70, npix, np.uint32)):
        d_bad = torch.from_numpy(bad.astype(np.int64)).to(torch.int32).to("cuda:0")
        d_s, d_m = device_frame(torch, npix), device_frame(torch, npix)
        ctr = torch.zeros(16, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        c["renderer"].render_pixels_device(c["cam"], c["scene"], d_bad.data_ptr(), len(bad), d_s.data_ptr() + GUARD * 12, d_m.data_ptr() + GUARD * 12,
                                           d_counters_ptr=ctr.data_ptr())
        torch.cuda.synchronize()
        got_s, ok_s = frame_of(d_s, npix, shape)
        got_m, ok_m = frame_of(d_m, npix, shape)
        assert ok_s and ok_m, (name, size, "the entry past the image was written")
        kept = bad[bad < npix]
        check_frames(got_s, got_m, kept, c["S"], c["M"], (name, size, "entry past the image"))
        assert int(ctr[0]) == len(kept) * n


@pytest.mark.parametrize("name,size,n", SMALL, ids=SMALL_IDS)
def test_nothing_to_trace_zeroes_the_listed_pixels_unless_accumulate(trt, case, name, size, n):
    c = case(name, size, n)
    shape = (size[1], size[0], 3)
    px = lists_of(c["npix"])["third"]
    zero = np.zeros(shape, np.float32)
    for r, over in ((trt.Renderer(n, 1, 0, False, c["desc"]["background"], seed=SEED), {}),             # max_bounces == 0
                    (c["renderer"], dict(sample_begin=3, sample_end=3))):                                # an empty sample range
        accum, m2 = sentinel(shape), sentinel(shape)
        st = r.render_pixels(c["cam"], c["scene"], px, accum, m2, **over)
        check_frames(accum, m2, px, zero, zero, (name, over))
        assert st["samples"] == 0 and st["rays"] == 0
        accum, m2 = sentinel(shape), sentinel(shape)
        r.render_pixels(c["cam"], c["scene"], px, accum, m2, accumulate=1, **over)
        assert is_sentinel(accum).all() and is_sentinel(m2).all(), (name, over)


@pytest.mark.parametrize("name,size,n", SMALL, ids=SMALL_IDS)
def test_the_device_compiled_scene_gives_the_same_bytes(trt, case, name, size, n):
    c = case(name, size, n)
    shape = (size[1], size[0], 3)
    other = trt.Scene(c["world"], on_device=True)
    assert G.plan_shape(other.pixels_plan(c["npix"])) == G.DEFAULT_SHAPES[name]
    px = lists_of(c["npix"])["shuffle"][:100]
    accum, m2 = sentinel(shape), sentinel(shape)
    c["renderer"].render_pixels(c["cam"], other, px, accum, m2)
    check_frames(accum, m2, px, c["S"], c["M"], (name, "device-compiled scene"))


def test_misuse_on_a_device(trt, case):
    c = case("cornell", (8, 8), 4)
    accum = sentinel((8, 8, 3))
    for bad in ([64], [3, 3]):
        with pytest.raises(trt.TinyRTError) as e:
            c["renderer"].render_pixels(c["cam"], c["scene"], np.array(bad, np.uint32), accum)
        assert e.value.code == trt._lib.ERR_INVALID_ARG
    with pytest.raises(trt.TinyRTError) as e:
        c["renderer"].render_pixels(c["cam"], c["scene"], np.array([1], np.uint32), accum, collect_stats=1)
    assert e.value.code == trt._lib.ERR_INVALID_ARG
    assert is_sentinel(accum).all()
