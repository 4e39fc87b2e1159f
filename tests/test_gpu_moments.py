"""Per-pixel second moments out of the streamed fold (trt_render_moments and its device form) and the variance of the pixel estimate
(trt_variance and its device form) on the GPU, bit for bit against the CPU oracle.

The checker.  For N a power of two the oracle's render of the single sample s at samples_per_pixel = N is c_s * (1/N); times N that is
c_s exactly, provided no value is denormal (every non-zero magnitude >= 2^-100: asserted by denoise_color_cases.oracle_samples, a
condition on the inputs, not a tolerance).  From the exact c_s numpy folds S = S + c * (1/N) and M.ch = M.ch + (c.ch * c.ch) * (1/N) in
float32 in sample order (denoise_color_cases.fold_moments): what tinyrt.h says the two buffers hold.

Scenes (tests/walk_ray_cases.py): cornell and random_spheres.  Images: 19 x 13 (edge tiles with off-image lanes in both axes, six
tiles), 8 x 8 (exactly one tile) and 2 x 2 - the smallest image there is: a camera needs two pixels each way (pointgen.rs:41-42 divides
by width - 1 and height - 1; trt_render refuses less), so 2 x 2 stands where a 1 x 1 image would, and a one-row band of it is the
smallest local image.  N = 4 and 8 at max_bounces 8; 16 x 9 at N = 512 and max_bounces 4 is two tracing / fold launch pairs per call
(at most 256 samples per launch), the second fold continuing both buffers.

Every comparison is over every element: bits, and NaN by NaN-ness.  Every GPU step is one in-process call."""
import numpy as np
import pytest

import denoise_color_cases as D
import walk_ray_cases as W

pytestmark = pytest.mark.gpu

SEED = 5
SCENES = ["cornell", "random_spheres"]
SIZES = [(19, 13), (8, 8), (2, 2)]
SPPS = [4, 8]
GUARD = 100                                                                 # bytes: a multiple of 4, not of 16


@pytest.fixture(scope="module")
def case(trt, orc):
    """(scene, (width, height), N, max_bounces) -> description, product world / camera / renderer, the oracle's exact samples and the
    restated S and M; computed once on first use, shared, never changed."""
    cache = {}

    def get(name, size, n, bounces=8):
        key = (name, size, n, bounces)
        if key not in cache:
            desc = W.scene(trt, name)
            desc = dict(desc, camera=dict(desc["camera"], width=size[0], height=size[1]))
            ow, ocam = orc.world_from_description(desc)
            world, cam = trt.world_from_description(desc)
            samples = D.oracle_samples(orc, ow, ocam, n, bounces, desc["background"], SEED)
            s, m = D.fold_moments(samples, n)
            for a in (samples, s, m):
                a.setflags(write=False)
            renderer = trt.Renderer(n, 1, bounces, False, desc["background"], seed=SEED)
            cache[key] = dict(desc=desc, world=world, cam=cam, scene=world.get_bvh(), renderer=renderer, samples=samples, S=s, M=m, n=n)
        return cache[key]

    return get


CASES = [(name, size, n) for name in SCENES for size in SIZES for n in SPPS]
CASE_IDS = ["%s-%dx%d-%dspp" % (name, w, h, n) for name, (w, h), n in CASES]


@pytest.mark.parametrize("name,size,n", CASES, ids=CASE_IDS)
def test_frame_and_moments_against_the_oracle(trt, case, name, size, n):
    c = case(name, size, n)
    accum, m2, stats = c["renderer"].render_moments(c["cam"], c["scene"])
    frame = c["renderer"].render(c["cam"], c["scene"]).data
    assert accum.tobytes() == frame.tobytes(), "the frame is not trt_render's"
    D.assert_same(accum, c["S"], (name, size, n, "frame"))
    D.assert_same(m2, c["M"], (name, size, n, "moment2"))
    assert stats["samples"] == size[0] * size[1] * n
    assert (m2 >= 0).all() and (m2 > 0).any()
    # collect_stats = 1 (the counting kernels on the reference tree): the same buffers
    a1, m1, st1 = c["renderer"].render_moments(c["cam"], c["scene"], collect_stats=True)
    assert a1.tobytes() == accum.tobytes() and m1.tobytes() == m2.tobytes()
    assert st1["node_tests"] > 0 and st1["samples"] == stats["samples"]


def test_the_variance_is_not_trivially_zero(trt, case):
    """On Cornell at N = 8 more than a tenth of the pixels have variance > 0 - in the restatement and so in the product."""
    c = case("cornell", (19, 13), 8)
    want = D.restated_variance(c["S"], c["M"], 8)
    share = float((want > 0).mean())
    print(f"\ncornell 19x13, 8 spp: variance > 0 on {share:.3f} of the pixels")
    assert share > 0.1
    accum, m2, _ = c["renderer"].render_moments(c["cam"], c["scene"])
    got = trt.variance(accum, m2, 8)
    D.assert_same(got, want, "variance")
    assert float((got > 0).mean()) > 0.1


@pytest.mark.parametrize("name", SCENES)
def test_a_split_sample_range_gives_the_same_result(trt, case, name):
    c = case(name, (19, 13), 8)
    r, cam, sc = c["renderer"], c["cam"], c["scene"]
    accum, m2, _ = r.render_moments(cam, sc, sample_begin=0, sample_end=3)
    D.assert_same(accum, D.fold_moments(c["samples"], 8, 0, 3)[0], (name, "S of [0, 3)"))
    D.assert_same(m2, D.fold_moments(c["samples"], 8, 0, 3)[1], (name, "M of [0, 3)"))
    accum, m2, _ = r.render_moments(cam, sc, accum=accum, moment2=m2, sample_begin=3, sample_end=8, accumulate=1)
    D.assert_same(accum, c["S"], (name, "S of [0, 3) + [3, 8)"))
    D.assert_same(m2, c["M"], (name, "M of [0, 3) + [3, 8)"))
    # without `accumulate` the buffers' contents are ignored
    junk = np.full_like(c["S"], 9.0)
    a2, m2b, _ = r.render_moments(cam, sc, accum=junk.copy(), moment2=junk.copy())
    D.assert_same(a2, c["S"], (name, "S over junk"))
    D.assert_same(m2b, c["M"], (name, "M over junk"))


@pytest.mark.parametrize("name", SCENES)
def test_two_band_shards_equal_the_whole_frame(trt, case, name):
    c = case(name, (19, 13), 8)
    seen = np.zeros(13, np.int32)
    for rank in range(2):                                                   # bands of 4 rows dealt round-robin: rows 0-3, 8-11 | 4-7, 12
        rows = np.array([y for y in range(13) if (y // 4) % 2 == rank])
        accum, m2, _ = c["renderer"].render_moments(c["cam"], c["scene"], band_rows=4, band_stride=2, band_offset=rank, rows_local=len(rows))
        assert accum.shape == (len(rows), 19, 3)
        D.assert_same(accum, np.ascontiguousarray(c["S"][rows]), (name, "S of shard", rank))
        D.assert_same(m2, np.ascontiguousarray(c["M"][rows]), (name, "M of shard", rank))
        seen[rows] += 1
    assert (seen == 1).all()
    # the smallest local image: one row of the 2 x 2 frame
    c = case(name, (2, 2), 4)
    for row in range(2):
        accum, m2, _ = c["renderer"].render_moments(c["cam"], c["scene"], band_rows=1, band_stride=2, band_offset=row, rows_local=1)
        D.assert_same(accum, np.ascontiguousarray(c["S"][row:row + 1]), (name, "S of row", row))
        D.assert_same(m2, np.ascontiguousarray(c["M"][row:row + 1]), (name, "M of row", row))


def test_two_fold_launches_per_call(trt, case):
    """16 x 9 at 512 spp, max_bounces 4: the streamed backend traces at most 256 samples per launch, so the call is two tracing / fold
    launch pairs and the second fold continues both buffers."""
    c = case("cornell", (16, 9), 512, bounces=4)
    plan = c["renderer"].launch_plan(c["cam"], c["scene"])
    assert plan["chunk_spp"] <= 256, plan
    accum, m2, _ = c["renderer"].render_moments(c["cam"], c["scene"])
    D.assert_same(accum, c["S"], "S at 512 spp")
    D.assert_same(m2, c["M"], "M at 512 spp")
    assert accum.tobytes() == c["renderer"].render(c["cam"], c["scene"]).data.tobytes()
    want = D.restated_variance(c["S"], c["M"], 512)
    assert float((want > 0).mean()) > 0.1
    D.assert_same(trt.variance(accum, m2, 512), want, "variance at 512 spp")


def test_nothing_to_trace_zeroes_both_buffers_unless_accumulate(trt, case):
    c = case("cornell", (8, 8), 4)
    cam, sc = c["cam"], c["scene"]
    junk = np.full((8, 8, 3), 9.0, np.float32)
    for r, over in ((trt.Renderer(4, 1, 0, False, c["desc"]["background"], seed=SEED), {}),             # max_bounces == 0
                    (c["renderer"], dict(sample_begin=3, sample_end=3)),                                 # an empty sample range
                    (c["renderer"], dict(band_rows=4, band_stride=2, band_offset=0, rows_local=0))):     # no rows
        shape = (0, 8, 3) if "rows_local" in over else (8, 8, 3)
        a, m, _ = r.render_moments(cam, sc, accum=junk[:shape[0]].copy(), moment2=junk[:shape[0]].copy(), **over)
        assert a.shape == shape and not a.any() and not m.any(), over
        a, m, _ = r.render_moments(cam, sc, accum=junk[:shape[0]].copy(), moment2=junk[:shape[0]].copy(), accumulate=1, **over)
        assert (a == 9.0).all() and (m == 9.0).all(), over


def guarded(torch, payload_bytes, fill=0xCD):
    return torch.full((GUARD + payload_bytes + GUARD,), fill, dtype=torch.uint8, device="cuda:0")


def guards_intact(t, payload_bytes, fill=0xCD):
    h = t.cpu().numpy()
    return bool((h[:GUARD] == fill).all() and (h[GUARD + payload_bytes:] == fill).all())


def payload(t, nbytes, shape):
    return t.cpu().numpy()[GUARD:GUARD + nbytes].copy().view(np.float32).reshape(shape)


@pytest.mark.parametrize("name", SCENES)
def test_device_form_with_guard_bytes_and_a_side_stream(trt, case, name):
    import torch
    c = case(name, (19, 13), 8)
    nbytes = 19 * 13 * 12
    side = torch.cuda.Stream()
    for stream in (None, side):
        d_accum, d_m2 = guarded(torch, nbytes), guarded(torch, nbytes)
        ctr = torch.zeros(16, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        ptr = 0 if stream is None else stream.cuda_stream
        c["renderer"].render_moments_device(c["cam"], c["scene"], d_accum.data_ptr() + GUARD, d_m2.data_ptr() + GUARD, stream_ptr=ptr,
                                            d_counters_ptr=ctr.data_ptr())
        d_var = guarded(torch, 19 * 13 * 4)
        trt.variance_device(d_accum.data_ptr() + GUARD, d_m2.data_ptr() + GUARD, 19 * 13, 8, d_var.data_ptr() + GUARD, stream_ptr=ptr)
        (torch.cuda.current_stream() if stream is None else stream).synchronize()
        torch.cuda.synchronize()
        D.assert_same(payload(d_accum, nbytes, (13, 19, 3)), c["S"], (name, "device S", stream is not None))
        D.assert_same(payload(d_m2, nbytes, (13, 19, 3)), c["M"], (name, "device M", stream is not None))
        D.assert_same(payload(d_var, 19 * 13 * 4, (13, 19)), D.restated_variance(c["S"], c["M"], 8), (name, "device variance"))
        assert guards_intact(d_accum, nbytes) and guards_intact(d_m2, nbytes) and guards_intact(d_var, 19 * 13 * 4)
        assert int(ctr[0]) == 19 * 13 * 8
    # the device form continues buffers too: [0, 3) then [3, 8)
    d_accum, d_m2 = guarded(torch, nbytes), guarded(torch, nbytes)
    c["renderer"].render_moments_device(c["cam"], c["scene"], d_accum.data_ptr() + GUARD, d_m2.data_ptr() + GUARD, sample_begin=0, sample_end=3)
    c["renderer"].render_moments_device(c["cam"], c["scene"], d_accum.data_ptr() + GUARD, d_m2.data_ptr() + GUARD, sample_begin=3, sample_end=8,
                                        accumulate=1)
    torch.cuda.synchronize()
    D.assert_same(payload(d_accum, nbytes, (13, 19, 3)), c["S"], (name, "device S, split"))
    D.assert_same(payload(d_m2, nbytes, (13, 19, 3)), c["M"], (name, "device M, split"))
    assert guards_intact(d_accum, nbytes) and guards_intact(d_m2, nbytes)


def test_variance_forms_against_the_restatement(trt, case):
    """Host and device form on buffers with every case of the definition: real moments, a constant pixel (M == S*S up to cancellation:
    the clamp), M < S*S, a NaN sum, inf, zeros; N = 1 writes +inf everywhere, N = 0 too; 2^-23 * M is the size of the cancellation."""
    import torch
    c = case("cornell", (19, 13), 8)
    s, m = c["S"].reshape(-1, 3).copy(), c["M"].reshape(-1, 3).copy()
    s[0], m[0] = (0.3, 0.3, 0.3), np.float32(0.3) * np.float32(0.3)          # constant pixel
    s[1], m[1] = (0.7, 0.1, 0.2), (0.1, 0.001, 0.01)                         # M < S*S: clamped to 0 per channel
    s[2], m[2] = (np.nan, 0.5, 0.5), (1.0, 1.0, 1.0)                         # a NaN sum: that channel counts 0
    s[3], m[3] = (0.5, 0.5, 0.5), (np.nan, np.nan, np.nan)
    s[4], m[4] = (1.0, 1.0, 1.0), (np.inf, 2.0, 2.0)
    s[5], m[5] = (np.inf, 1.0, 1.0), (np.inf, 2.0, 2.0)                      # inf - inf = NaN -> 0
    s[6], m[6] = 0.0, 0.0
    s[7], m[7] = (15.0, 15.0, 15.0), (225.0, 225.0, 225.0)                   # the light itself
    n = len(s)
    for spp in (8, 2, 4096, 1, 0):
        want = D.restated_variance(s, m, spp)
        got = trt.variance(s, m, spp)
        D.assert_same(got, want, ("host form", spp))
        d_s, d_m = torch.from_numpy(s).to("cuda:0"), torch.from_numpy(m).to("cuda:0")
        d_v = guarded(torch, n * 4)
        trt.variance_device(d_s.data_ptr(), d_m.data_ptr(), n, spp, d_v.data_ptr() + GUARD)
        torch.cuda.synchronize()
        D.assert_same(payload(d_v, n * 4, (n,)), want, ("device form", spp))
        assert guards_intact(d_v, n * 4)
        if spp <= 1:
            assert np.isposinf(got).all()
        else:
            assert got[0] == 0 and got[1] == 0 and got[6] == 0 and got[7] == 0
            assert got[2] > 0 and got[3] == 0 and np.isposinf(got[4]) and np.isfinite(got[5])
            assert not np.isnan(got).any()
