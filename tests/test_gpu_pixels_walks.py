"""The sparse render (trt_render_pixels and its device form) on every kernel shape the default compilations of tests/test_gpu_pixels.py do
not launch, bit for bit against the CPU oracle.

Cases: test_gpu_queries.OTHER_WALKS - each scene compiled with another placement option or by the device compiler, listed with the kernel
shape it is there to run - plus the two scenes made to break walks, `degenerate` and `nonfinite`.  Among them: pixels_kernel<MODE_GLOBAL,
WALK_REGS, 256> (grid3000 with 32-byte nodes), which no default compilation reaches; the LDS tree at 256 lanes on Cornell (stragglers parked
with axis quads in the scene); the lock-step list with more than 32 leaves (prims33, flat_walk=1); the LDS register-slot walk as the
streamed plan's own walk (prims600, flat_walk=1: no fallback).  Every case asserts the shape Scene.pixels_plan reports; with
test_gpu_pixels.SCENES the cases reach all six instantiations of kPixelsKernels (tests/test_pixels_abi.py checks that without a GPU).

Images: 19 x 13 (ragged) and 40 x 30 (1200 pixels, the smallest image that takes a 256-lane shape to two workgroups).  N = 8, max_bounces
8, seed 5.  The reference is the oracle as in tests/test_gpu_pixels.py: denoise_color_cases.oracle_samples -> fold_moments, cross-checked
against orc.render.  No case is vacuous: on the CPU the oracle's 19 x 13 frames of all eight scenes have no NaN and no all-zero pixel, and
between 36 (nonfinite) and 198 (prims600) distinct pixel values (degenerate: 70); at least 20 distinct pixels are asserted, so a constant image
cannot pass.

Per case and image: the lists `one`, `65`, `shuffle` and `third` of test_gpu_pixels.lists_of through the host form; `shuffle` through the
device form on a side stream with 64-pixel guards; one split range, [0, 3) then [3, 8) with accumulate = 1.  Every byte of both buffers
is compared (test_gpu_pixels.check_frames); samples == len(list) * N and rays >= samples.  Every GPU step is one in-process call."""
import numpy as np
import pytest

import denoise_color_cases as D
import test_gpu_pixels as P
import test_gpu_queries as G
import walk_ray_cases as W

pytestmark = pytest.mark.gpu

N = 8
SIZES = [(19, 13), (40, 30)]
CASES = G.OTHER_WALKS + [(name, {}, G.DEFAULT_SHAPES[name]) for name in ("degenerate", "nonfinite")]
PARAMS = [(k, size) for k in range(len(CASES)) for size in SIZES]
IDS = ["%s-%s-%dx%d" % (CASES[k][0], ",".join("%s=%s" % kv for kv in sorted(CASES[k][1].items())) or "default", w, h) for k, (w, h) in PARAMS]


@pytest.fixture(scope="module")
def reference(trt, orc):
    """(scene, (width, height)) -> description, product world and camera, the oracle's exact samples and the restated S and M of the
    whole range; computed once on first use, shared among the cases of a scene, never changed."""
    cache = {}

    def get(name, size):
        if (name, size) not in cache:
            desc = W.scene(trt, name)
            desc = dict(desc, camera=dict(desc["camera"], width=size[0], height=size[1]))
            ow, ocam = orc.world_from_description(desc)
            world, cam = trt.world_from_description(desc)
            samples = D.oracle_samples(orc, ow, ocam, N, P.BOUNCES, desc["background"], P.SEED)
            s, m = D.fold_moments(samples, N)
            frame, _ = orc.render(ow, ocam, N, P.BOUNCES, desc["background"], seed=P.SEED, nthreads=4)
            D.assert_same(s, frame, (name, size, "the restated fold is not the oracle's frame"))
            distinct = len(np.unique(frame.reshape(-1, 3).view(np.uint32), axis=0))
            print(f"\n{name} {size[0]}x{size[1]}: {distinct} distinct pixel values, {int(np.isnan(frame).any(axis=2).sum())} pixels with a NaN")
            assert distinct >= 20, (name, size, distinct)
            for a in (samples, s, m):
                a.setflags(write=False)
            renderer = trt.Renderer(N, 1, P.BOUNCES, False, desc["background"], seed=P.SEED)
            cache[(name, size)] = dict(desc=desc, world=world, cam=cam, renderer=renderer, samples=samples, S=s, M=m, npix=size[0] * size[1])
        return cache[(name, size)]

    return get


@pytest.fixture(scope="module")
def compiled(trt, reference):
    """(case index, size) -> the reference of the scene with the scene compiled with the case's options, its plan asserted."""
    cache = {}

    def get(k, size):
        if (k, size) not in cache:
            name, options, shape = CASES[k]
            c = reference(name, size)
            sc = c["world"].get_bvh(**options)
            plan = sc.pixels_plan(c["npix"])
            assert G.plan_shape(plan) == shape, (name, options, plan)
            assert plan["rays_per_wave"] == 256 and plan["workgroups"] == -(-(-(-c["npix"] // 256)) // (plan["threads_per_workgroup"] // 64)), plan
            if size == (40, 30) and plan["threads_per_workgroup"] == 256:
                assert plan["workgroups"] == 2
            cache[(k, size)] = dict(c, scene=sc, name=name, options=options)
        return cache[(k, size)]

    return get


@pytest.mark.parametrize("k,size", PARAMS, ids=IDS)
def test_listed_pixels_equal_the_oracle_and_nothing_else_is_written(trt, compiled, k, size):
    c = compiled(k, size)
    shape = (size[1], size[0], 3)
    lists = P.lists_of(c["npix"])
    for lname in ("one", "65", "shuffle", "third"):
        px = lists[lname]
        accum, m2 = P.sentinel(shape), P.sentinel(shape)
        st = c["renderer"].render_pixels(c["cam"], c["scene"], px, accum, m2)
        P.check_frames(accum, m2, px, c["S"], c["M"], (c["name"], c["options"], size, lname))
        assert st["samples"] == len(px) * N, (lname, st)
        assert st["rays"] >= st["samples"], (lname, st)


@pytest.mark.parametrize("k,size", PARAMS, ids=IDS)
def test_device_form_on_a_side_stream_equals_the_oracle_and_leaves_the_guards(trt, compiled, k, size):
    import torch
    c = compiled(k, size)
    npix, shape = c["npix"], (size[1], size[0], 3)
    px = P.lists_of(npix)["shuffle"]
    side = torch.cuda.Stream()
    d_s, d_m = P.device_frame(torch, npix), P.device_frame(torch, npix)
    d_px = torch.from_numpy(px.astype(np.int64)).to(torch.int32).to("cuda:0")
    ctr = torch.zeros(16, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    c["renderer"].render_pixels_device(c["cam"], c["scene"], d_px.data_ptr(), len(px), d_s.data_ptr() + P.GUARD * 12, d_m.data_ptr() + P.GUARD * 12,
                                       stream_ptr=side.cuda_stream, d_counters_ptr=ctr.data_ptr())
    side.synchronize()
    torch.cuda.synchronize()
    got_s, ok_s = P.frame_of(d_s, npix, shape)
    got_m, ok_m = P.frame_of(d_m, npix, shape)
    assert ok_s and ok_m, (c["name"], c["options"], size, "guard bytes were written")
    P.check_frames(got_s, got_m, px, c["S"], c["M"], (c["name"], c["options"], size, "device form"))
    assert int(ctr[0]) == len(px) * N and int(ctr[1]) >= int(ctr[0]) and not bool(ctr[2:].any())


@pytest.mark.parametrize("k,size", PARAMS, ids=IDS)
def test_a_split_sample_range_with_accumulate_equals_one_pass(trt, compiled, k, size):
    c = compiled(k, size)
    shape = (size[1], size[0], 3)
    px = P.lists_of(c["npix"])["third"]
    accum, m2 = P.sentinel(shape), P.sentinel(shape)
    st = c["renderer"].render_pixels(c["cam"], c["scene"], px, accum, m2, sample_begin=0, sample_end=3)
    s3, m3 = D.fold_moments(c["samples"], N, 0, 3)
    P.check_frames(accum, m2, px, s3, m3, (c["name"], c["options"], size, "[0, 3)"))
    assert st["samples"] == len(px) * 3 and st["rays"] >= st["samples"], st
    st = c["renderer"].render_pixels(c["cam"], c["scene"], px, accum, m2, sample_begin=3, sample_end=N, accumulate=1)
    P.check_frames(accum, m2, px, c["S"], c["M"], (c["name"], c["options"], size, "[0, 3) + [3, 8)"))
    assert st["samples"] == len(px) * (N - 3) and st["rays"] >= st["samples"], st
