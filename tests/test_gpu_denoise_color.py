"""The variance-guided colour stop of the denoiser (trt_denoise_ex and its device form) on the GPU, bit for bit.

The checker is denoise_color_cases.restated: the numpy restatement of the definition in tinyrt.h in np.float32 - one IEEE
operation per operator, nothing fused, denormals kept; with the term off it is the restatement tests/test_gpu_denoise.py checks
trt_denoise with (asserted below, on the CPU side of a GPU test).  Every comparison is over every element: bits, and NaN by NaN-ness.

 1. term off - a NULL trt_denoise_color, a NULL variance, sigma_color 0 or negative - gives trt_denoise's bytes;
 2. real buffers: the 8-spp frame, second moments and variance (trt_render_moments, trt_variance) and the feature buffers of cornell and
    random_spheres at 67 x 35, iterations 1, 2, 4;
 3. synthetic buffers in the style of tests/test_gpu_denoise.py at 1 x 1, 5 x 3, 33 x 33 and 70 x 40 with 8 iterations, the variance map
    holding 0, +inf, NaN, denormals and 1e30 beside ordinary values;
 4. the three consequences the header states, as exact statements: variance +inf everywhere gives trt_denoise's bytes; variance 0
    everywhere leaves every pixel at (w*c) * (1/w) per pass, w = 0.375 * 0.375; a NaN variance does the same to the 3 x 3 pixels its
    prefilter reaches (each with the condition under which it is exact: see the tests);
 5. all 16 subsets of the four terms;
 6. the device form with guard bytes, a scratch of exactly trt_denoise_scratch_bytes at an odd alignment, a side stream, inputs unchanged;
    the plain, packed and LDS forms of the kernel (TRT_DENOISE_VARIANT) give equal bytes with the term on;
 7. consistency, the point of the feature: see test_the_filter_backs_off_as_the_frame_converges.

Every GPU step is one in-process call; nothing is built here and no child process is started."""
import ctypes as C

import numpy as np
import pytest

import denoise_color_cases as D
import test_gpu_denoise as T
import walk_ray_cases as W

pytestmark = pytest.mark.gpu
f32 = np.float32
SIGMA = 4.0                                                                 # an explicit sigma_color for the bit-for-bit cases
GUARD = T.GUARD


def test_the_restatement_with_the_term_off_is_the_one_trt_denoise_is_checked_with():
    color, albedo, normal, depth = T.synthetic(33, 21, seed=3)
    for kw in (dict(), dict(iterations=2, sigma_albedo=0.0), dict(iterations=3, normal_power_log2=0)):
        D.assert_same(D.restated(color, albedo, normal, depth, **kw), T.restated(color, albedo, normal, depth, **kw), kw)
    var = np.ones((21, 33), np.float32)
    D.assert_same(D.restated(color, albedo, normal, depth, var, 0.0), T.restated(color, albedo, normal, depth), "sigma 0")
    D.assert_same(D.restated(color, albedo, normal, depth, var, -1.0), T.restated(color, albedo, normal, depth), "sigma < 0")


def synthetic_variance(width, height, seed):
    """float32 [height, width]: ordinary values between 0.002 and 2 (the colours of T.synthetic are uniform in [0, 2): with SIGMA = 4 the
    stop is shut for some neighbours, open for others and in between for most), and, each on about one per cent of the pixels (at least
    one where the image has the pixels for it), 0, +inf, NaN, a denormal, 1e30 and -0.0."""
    rng = np.random.default_rng(seed)
    v = (f32(0.002) + rng.random((height, width), dtype=np.float32) ** 3 * f32(2)).astype(np.float32)
    n = width * height
    order = rng.permutation(n)
    share = max(1, n // 100)
    for k, value in enumerate((0.0, np.inf, np.nan, 1e-40, 1e30, -0.0)):
        at = np.unravel_index(order[(k * share) % n:(k * share) % n + share], (height, width))
        v[at] = f32(value)
    v.setflags(write=False)
    return v


SHAPES = [(1, 1), (5, 3), (33, 33), (70, 40)]


@pytest.fixture(scope="module")
def synth():
    """(width, height) -> (color, albedo, normal, depth, variance) and the restatement's result with all terms, SIGMA and 8 iterations."""
    cache = {}

    def get(width, height):
        if (width, height) not in cache:
            bufs = T.synthetic(width, height, seed=2000 + width * 7 + height) + (synthetic_variance(width, height, 3000 + width * 7 + height),)
            want = D.restated(*bufs, sigma_color=SIGMA, iterations=8)
            want.setflags(write=False)
            cache[(width, height)] = (bufs, want)
        return cache[(width, height)]

    return get


# ------------------------------------------------------------------------------------------------------------------
# 1. term off
# ------------------------------------------------------------------------------------------------------------------
def test_term_off_gives_the_bytes_of_trt_denoise(trt, synth):
    (color, albedo, normal, depth, var), _ = synth(70, 40)
    base = trt.denoise(color, albedo, normal, depth)
    T.assert_same(base, T.restated(color, albedo, normal, depth), "trt_denoise")
    pod = trt._lib.DenoiseInputs()
    pod.color, pod.albedo, pod.normal, pod.depth = color.ctypes.data, albedo.ctypes.data, normal.ctypes.data, depth.ctypes.data
    for what, col in (("NULL struct", None), ("NULL variance", trt.denoise_color(None, SIGMA)), ("sigma 0", trt.denoise_color(var.ctypes.data, 0.0)),
                      ("sigma -0.0", trt.denoise_color(var.ctypes.data, -0.0)), ("sigma < 0", trt.denoise_color(var.ctypes.data, -2.0))):
        out = np.full((40, 70, 3), 7.0, np.float32)
        trt._lib.check(trt.lib.trt_denoise_ex(C.byref(pod), None if col is None else C.byref(col), 70, 40, None, out.ctypes.data))
        assert out.tobytes() == base.tobytes(), what
    assert trt.denoise(color, albedo, normal, depth, variance=var, sigma_color=0.0).tobytes() == base.tobytes()
    assert trt.denoise(color, albedo, normal, depth, variance=var, sigma_color=SIGMA).tobytes() != base.tobytes()


# ------------------------------------------------------------------------------------------------------------------
# 2. real buffers
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def real(trt):
    """scene -> the 8-spp frame, its variance and the feature buffers of the product at 67 x 35; rendered once, never changed."""
    cache = {}

    def get(name):
        if name not in cache:
            desc = W.scene(trt, name)
            desc = dict(desc, camera=dict(desc["camera"], width=67, height=35))
            world, cam = trt.world_from_description(desc)
            r = trt.Renderer(8, 1, 50, False, desc["background"], seed=5)
            frame, m2, _ = r.render_moments(cam, world)
            var = trt.variance(frame, m2, 8)
            D.assert_same(var, D.restated_variance(frame, m2, 8), (name, "variance"))
            assert float((var > 0).mean()) > 0.1 and np.isfinite(var).all()
            aov = r.render_aov(cam, world, channels=("albedo", "normal", "depth"))
            for a in (frame, var, *aov.values()):
                a.setflags(write=False)
            cache[name] = (frame, var, aov)
        return cache[name]

    return get


@pytest.mark.parametrize("iterations", (1, 2, 4))
@pytest.mark.parametrize("name", ("cornell", "random_spheres"))
def test_real_buffers_against_the_restatement(trt, real, name, iterations):
    frame, var, aov = real(name)
    for sigma in (None, SIGMA):
        got = trt.denoise(frame, aov["albedo"], aov["normal"], aov["depth"], variance=var, sigma_color=sigma, iterations=iterations)
        want = D.restated(frame, aov["albedo"], aov["normal"], aov["depth"], var, trt.denoise_color().sigma_color if sigma is None else sigma,
                          iterations=iterations)
        D.assert_same(got, want, (name, iterations, sigma))
        assert not np.array_equal(got, frame)
        assert not np.array_equal(got, trt.denoise(frame, aov["albedo"], aov["normal"], aov["depth"], iterations=iterations))     # the term does something


# ------------------------------------------------------------------------------------------------------------------
# 3. synthetic buffers, adversarial variance maps
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,height", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_shapes_and_adversarial_variances(trt, synth, width, height):
    (color, albedo, normal, depth, var), want = synth(width, height)
    got = trt.denoise(color, albedo, normal, depth, variance=var, sigma_color=SIGMA, iterations=8)
    D.assert_same(got, want, (width, height))
    if width * height >= 33 * 33:
        # the values are there, and the stop is neither shut nor open everywhere: the result is neither the guides-only one nor the frame
        for value in (0.0, np.inf, 1e30):
            assert (var == f32(value)).any()
        assert np.isnan(var).any() and (var == f32(1e-40)).any() and f32(1e-40) > 0
        off = T.restated(color, albedo, normal, depth, iterations=8)
        finite = np.isfinite(want).all(axis=2) & np.isfinite(off).all(axis=2)
        assert finite.mean() > 0.2
        assert (want[finite] != off[finite]).any() and (want[finite] != color[finite]).any()


# ------------------------------------------------------------------------------------------------------------------
# 4. the consequences, as exact statements
# ------------------------------------------------------------------------------------------------------------------
def finite_synthetic(width, height, seed):
    """T.synthetic with the non-finite and the huge colours replaced (the statements below are about finite e = |c_p - c_q|^2)."""
    color, albedo, normal, depth = T.synthetic(width, height, seed)
    color = np.where(np.isfinite(color) & (np.abs(color) < 1e10), color, f32(0.5)).astype(np.float32)
    return color, albedo, normal, depth


def kept(color, iterations):
    """A pixel whose every neighbour weighs 0: acc = w*c, ws = w, out = (w*c) * (1/w) per pass, w = 0.375 * 0.375."""
    w = f32(0.375) * f32(0.375)
    c = color.astype(np.float32)
    for _ in range(iterations):
        c = (f32(0) + w * c) * (f32(1) / w)
    return c


def test_infinite_variance_gives_the_guides_only_result(trt):
    """v = +inf (what trt_variance writes at 1 spp): inv_c = 0, every m = 1 for a finite e, the term multiplies by 1 - the pass gives
    trt_denoise's bytes, whatever the guides hold.  Over several passes the same is exact as long as v stays +inf, i.e. as long as no
    taken tap's w*w underflows to 0 (0 * inf is NaN, and a NaN v keeps the pixel from the next pass on): without guides the weights are
    h*h >= 2^-8, so four passes give trt_denoise's bytes; with the adversarial guides (half-length normals: w = 2^-128 h*h) they do not,
    and the result is still the restatement's bit for bit."""
    color, albedo, normal, depth = finite_synthetic(70, 40, seed=11)
    var = trt.variance(color, color * color, 1).reshape(40, 70)
    assert np.isposinf(var).all()
    got = trt.denoise(color, albedo, normal, depth, variance=var, sigma_color=SIGMA, iterations=1)
    assert got.tobytes() == trt.denoise(color, albedo, normal, depth, iterations=1).tobytes()
    D.assert_same(got, D.restated(color, albedo, normal, depth, var, SIGMA, iterations=1), "one pass")
    got = trt.denoise(color, variance=var, sigma_color=SIGMA, iterations=4)
    assert got.tobytes() == trt.denoise(color, iterations=4).tobytes()
    D.assert_same(got, D.restated(color, variance=var, sigma_color=SIGMA, iterations=4), "four passes, no guides")
    got = trt.denoise(color, albedo, normal, depth, variance=var, sigma_color=SIGMA, iterations=4)
    D.assert_same(got, D.restated(color, albedo, normal, depth, var, SIGMA, iterations=4), "four passes, adversarial guides")


def test_zero_variance_keeps_every_pixel(trt):
    """v = 0: inv_c = inf, every neighbour's m is -inf or NaN, then 0: a converged pixel is left alone, to the rounding of (w*c) * (1/w)."""
    color, albedo, normal, depth = finite_synthetic(70, 40, seed=12)
    var = np.zeros((40, 70), np.float32)
    for it in (1, 4):
        got = trt.denoise(color, albedo, normal, depth, variance=var, sigma_color=SIGMA, iterations=it)
        D.assert_same(got, kept(color, it), ("kept", it))
        D.assert_same(got, D.restated(color, albedo, normal, depth, var, SIGMA, iterations=it), it)
        assert np.allclose(got, color, rtol=1e-6, atol=1e-37)


def test_a_nan_variance_keeps_the_pixels_its_prefilter_reaches(trt):
    color, albedo, normal, depth = finite_synthetic(70, 40, seed=13)
    var = np.full((40, 70), 0.05, np.float32)
    var[20, 30] = np.nan
    var[0, 69] = np.nan                                                     # a corner: the prefilter has four taps there
    for it in (1, 4):
        got = trt.denoise(color, albedo, normal, depth, variance=var, sigma_color=SIGMA, iterations=it)
        D.assert_same(got, D.restated(color, albedo, normal, depth, var, SIGMA, iterations=it), it)
        want = kept(color, it)
        D.assert_same(got[19:22, 29:32], want[19:22, 29:32], ("round the NaN", it))
        D.assert_same(got[0:2, 68:70], want[0:2, 68:70], ("the corner", it))
        assert np.isfinite(got).all()
        assert not np.array_equal(got[5:15, 5:15], want[5:15, 5:15])        # elsewhere the filter filters


# ------------------------------------------------------------------------------------------------------------------
# 5. every subset of the four terms
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subset", range(16))
def test_every_term_subset(trt, synth, subset):
    (color, albedo, normal, depth, var), _ = synth(33, 33)
    kw = dict(albedo=albedo if subset & 1 else None, normal=normal if subset & 2 else None, depth=depth if subset & 4 else None,
              variance=var if subset & 8 else None)
    got = trt.denoise(color, iterations=3, sigma_color=SIGMA if subset & 8 else None, **kw)
    D.assert_same(got, D.restated(color, iterations=3, sigma_color=SIGMA, **kw), sorted(k for k, v in kw.items() if v is not None))


# ------------------------------------------------------------------------------------------------------------------
# 6. device form, kernel forms
# ------------------------------------------------------------------------------------------------------------------
def test_device_form_with_guards_and_exact_scratch(trt, synth):
    import torch
    width, height = 70, 40
    (color, albedo, normal, depth, var), want = synth(width, height)
    n = width * height
    need = trt.denoise_scratch_bytes(width, height, iterations=8)
    assert need == 16 + 4 * n * 16                                          # what trt_denoise needs: the term costs no scratch
    host = dict(color=color, albedo=albedo, normal=normal, depth=depth, variance=var)
    side = torch.cuda.Stream()
    for stream in (None, side):
        dev = {k: torch.from_numpy(v.copy()).to("cuda:0") for k, v in host.items()}
        out = T.guarded(torch, n * 12)
        scratch = T.guarded(torch, need)
        assert (scratch.data_ptr() + GUARD) % 16 != 0                       # an odd alignment: the library rounds up inside the scratch
        torch.cuda.synchronize()
        trt.denoise_device(dev["color"].data_ptr(), width, height, out.data_ptr() + GUARD, scratch.data_ptr() + GUARD, need,
                           d_albedo_ptr=dev["albedo"].data_ptr(), d_normal_ptr=dev["normal"].data_ptr(), d_depth_ptr=dev["depth"].data_ptr(),
                           stream_ptr=0 if stream is None else stream.cuda_stream, d_variance_ptr=dev["variance"].data_ptr(),
                           sigma_color=SIGMA, iterations=8)
        (torch.cuda.current_stream() if stream is None else stream).synchronize()
        torch.cuda.synchronize()
        got = out.cpu().numpy()[GUARD:GUARD + n * 12].copy().view(np.float32).reshape(height, width, 3)
        D.assert_same(got, want, ("device form", stream is not None))
        assert T.guards_intact(out, n * 12), "bytes round d_out were written"
        assert T.guards_intact(scratch, need), "bytes round d_scratch were written"
        for k, v in host.items():
            assert dev[k].cpu().numpy().tobytes() == v.tobytes(), k + " was changed"


@pytest.mark.parametrize("variant", ("plain", "packed", "lds"))
def test_kernel_forms_give_equal_bytes_with_the_term_on(trt, synth, monkeypatch, variant):
    for width, height in ((70, 40), (33, 33), (1, 1)):
        (color, albedo, normal, depth, var), want = synth(width, height)
        monkeypatch.setenv("TRT_DENOISE_VARIANT", variant)
        got = trt.denoise(color, albedo, normal, depth, variance=var, sigma_color=SIGMA, iterations=8)
        monkeypatch.delenv("TRT_DENOISE_VARIANT")
        D.assert_same(got, want, (variant, width, height))
    (color, albedo, normal, depth, var), _ = synth(70, 40)
    monkeypatch.setenv("TRT_DENOISE_VARIANT", variant)
    got = trt.denoise(color, None, None, None, variance=var, sigma_color=SIGMA, iterations=3)
    monkeypatch.delenv("TRT_DENOISE_VARIANT")
    D.assert_same(got, D.restated(color, variance=var, sigma_color=SIGMA, iterations=3), (variant, "colour term only"))


# ------------------------------------------------------------------------------------------------------------------
# 7. consistency
# ------------------------------------------------------------------------------------------------------------------
N_HI, REF_SPP = 2048, 65536


def test_the_filter_backs_off_as_the_frame_converges(trt):
    """Cornell 64 x 64, max_bounces 8, seed 5, against the 65536-spp frame of seed 77; errors are tonemapped mean squared errors.
    N_HI = 2048 is the lowest power-of-two sample count at which the guides-only filter already makes the frame WORSE: found on the CPU
    with the restatement over the oracle's frames and first hits (at 1024 spp noisy 1.745e-3, guides-only 1.112e-3; at
    2048 spp noisy 8.155e-4, guides-only 9.774e-4, variance-guided with the default sigma_color 2.209e-4; at 4096 spp 4.053e-4,
    9.259e-4, 1.374e-4).  The product's frames, moments and feature buffers equal the oracle's bit for bit and the device filter equals
    the restatement bit for bit, so the two inequalities hold here as they did there: no margin is added.
      - with the default sigma_color the variance-guided result is at most as far from the reference as the noisy frame;
      - the guides-only result is farther: the frame is one on which the term has something to do."""
    desc = trt.scenes.cornell(64, 64)
    world, cam = trt.world_from_description(desc)
    r = trt.Renderer(N_HI, 1, 8, False, desc["background"], seed=5)
    noisy, m2, _ = r.render_moments(cam, world)
    var = trt.variance(noisy, m2, N_HI)
    aov = r.render_aov(cam, world, channels=("albedo", "normal", "depth"))
    ref = trt.Renderer(REF_SPP, 1, 8, False, desc["background"], seed=77).render(cam, world).data
    guides_only = trt.denoise(noisy, aov["albedo"], aov["normal"], aov["depth"])
    guided = trt.denoise(noisy, aov["albedo"], aov["normal"], aov["depth"], variance=var)
    e_noisy, e_guides, e_guided = (D.tonemapped_mse(a, ref) for a in (noisy, guides_only, guided))
    print(f"\ncornell 64x64, {N_HI} spp: tonemapped MSE noisy {e_noisy:.4e}, guides-only {e_guides:.4e}, variance-guided {e_guided:.4e}")
    assert np.isfinite(guided).all()
    assert e_guided <= e_noisy, (e_noisy, e_guides, e_guided)
    assert e_guides > e_noisy, (e_noisy, e_guides, e_guided)
