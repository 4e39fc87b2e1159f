"""The feature-guided a-trous denoiser (trt_denoise and its device form) on the GPU, bit for bit.

The checker is `restated`: the numpy restatement of the filter's definition (tinyrt.h) in np.float32 - one IEEE operation
per operator, nothing fused, denormals kept.  Every comparison is over every element: bits, and NaN by NaN-ness (assert_same, as in
tests/test_gpu_aov.py).

 1. real buffers: a 4-spp render and the feature buffers of the product for cornell and random_spheres (tests/walk_ray_cases.py) at
    67 x 35 and 131 x 70, iterations 1, 2, 4, 8; the coverage buffer must hold both 0 and > 0.9 pixels;
 2. shapes where a tile kernel goes wrong: synthetic buffers at 1 x 1, 3 x 2, 5 x 70, 70 x 5, 64 x 64, 65 x 33 and 300 x 260 with 8
    iterations (taps at step 128 land inside the image both ways; more than two tiles of every kernel form each way);
 3. adversarial values in those buffers: exact zeros, -0.0, denormals, 1e30, NaN and inf colours, NaN guides, zero normals, depth 0,
    normals of length 0.5 (d^128 = 2^-128: a denormal weight) - the w > 0 skip, NaN containment, the centre-tap rule, denormal weights;
 4. all 8 guide subsets, and sigma_albedo = 0, sigma_depth = 0, normal_power_log2 = 0;
 5. independent of the restatement: an impulse under constant guides after two passes is the integer convolution of the two B3 kernels;
 6. the device form equals the host form, with guard bytes round `d_out` and `d_scratch`, a scratch of exactly
    trt_denoise_scratch_bytes at an odd alignment, a side stream, inputs unchanged; the plain, packed and LDS forms of the kernel
    (TRT_DENOISE_VARIANT, read at every call) give the bytes of the default;
 7. it denoises: tonemapped mean squared error against a high-spp frame falls to at most 0.5 of the noisy frame's.

Every GPU step is one in-process call; nothing is built here and no child process is started."""
import numpy as np
import pytest

import walk_ray_cases as W

pytestmark = pytest.mark.gpu

H5 = np.array([0.0625, 0.25, 0.375, 0.25, 0.0625], np.float32)
f32 = np.float32


def restated(color, albedo=None, normal=None, depth=None, iterations=4, normal_power_log2=7, sigma_albedo=0.1, sigma_depth=0.05):
    """The specification."""
    Hh, Ww, _ = color.shape
    c = color.astype(np.float32).copy()
    yy, xx = np.mgrid[0:Hh, 0:Ww]
    use_a = albedo is not None and sigma_albedo > 0
    use_z = depth is not None and sigma_depth > 0
    if use_a:
        inv_a = f32(1) / (f32(sigma_albedo) * f32(sigma_albedo))
    with np.errstate(all="ignore"):
        for it in range(iterations):
            step = 1 << it
            if use_z:
                s = (f32(sigma_depth) * depth) * f32(step)
                inv_z = f32(1) / (s * s)
            acc = np.zeros_like(c)
            ws = np.zeros((Hh, Ww), np.float32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qy = yy + dy * step
                    qx = xx + dx * step
                    ok = (qy >= 0) & (qy < Hh) & (qx >= 0) & (qx < Ww)
                    qyc = np.clip(qy, 0, Hh - 1)
                    qxc = np.clip(qx, 0, Ww - 1)
                    w = np.full((Hh, Ww), H5[dy + 2] * H5[dx + 2], np.float32)
                    if dx or dy:
                        if normal is not None:
                            nq = normal[qyc, qxc]
                            d = (normal[..., 0] * nq[..., 0] + normal[..., 1] * nq[..., 1]) + normal[..., 2] * nq[..., 2]
                            d = np.where(d > 0, d, f32(0))
                            for _ in range(normal_power_log2):
                                d = d * d
                            w = w * d
                        if use_a:
                            da = albedo - albedo[qyc, qxc]
                            e = (da[..., 0] * da[..., 0] + da[..., 1] * da[..., 1]) + da[..., 2] * da[..., 2]
                            m = f32(1) - e * inv_a
                            m = np.where(m > 0, m, f32(0))
                            w = w * (m * m)
                        if use_z:
                            dz = depth - depth[qyc, qxc]
                            m = f32(1) - ((dz * dz) * inv_z) * (f32(1) / f32(dx * dx + dy * dy))
                            m = np.where(m > 0, m, f32(0))
                            w = w * (m * m)
                    take = ok & (w > 0)
                    acc = np.where(take[..., None], acc + w[..., None] * c[qyc, qxc], acc)
                    ws = np.where(take, ws + w, ws)
            c = acc * (f32(1) / ws)[..., None]
    assert c.dtype == np.float32
    return c


def assert_same(got, want, what):
    """Bits; a component that is NaN in `want` by NaN-ness.  Every element is compared."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape)
    same = np.where(np.isnan(want), np.isnan(got), got.view(np.uint32) == want.view(np.uint32))
    bad = np.argwhere(~same)
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


# ------------------------------------------------------------------------------------------------------------------
# 1. real buffers
# ------------------------------------------------------------------------------------------------------------------
REAL_SCENES = ["cornell", "random_spheres"]
REAL_SIZES = [(67, 35), (131, 70)]


@pytest.fixture(scope="module")
def real(trt):
    """(scene, (width, height)) -> the 4-spp frame and the feature buffers of the product, rendered once, never changed."""
    cache = {}

    def get(name, size):
        if (name, size) not in cache:
            desc = W.scene(trt, name)
            desc = dict(desc, camera=dict(desc["camera"], width=size[0], height=size[1]))
            world, cam = trt.world_from_description(desc)
            r = trt.Renderer(4, 1, 50, False, desc["background"], seed=5)
            frame = r.render(cam, world).data
            aov = r.render_aov(cam, world, channels=("albedo", "normal", "depth", "coverage"))
            cov = aov["coverage"]
            assert (cov == 0).any() and (cov > 0.9).any(), (name, size, float(cov.mean()))     # no case runs on an all-hit image
            for a in (frame, *aov.values()):
                a.setflags(write=False)
            cache[(name, size)] = (frame, aov)
        return cache[(name, size)]

    return get


@pytest.mark.parametrize("iterations", (1, 2, 4, 8))
@pytest.mark.parametrize("size", REAL_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", REAL_SCENES)
def test_real_buffers_against_the_restatement(trt, real, name, size, iterations):
    frame, aov = real(name, size)
    got = trt.denoise(frame, aov["albedo"], aov["normal"], aov["depth"], iterations=iterations)
    want = restated(frame, aov["albedo"], aov["normal"], aov["depth"], iterations=iterations)
    assert_same(got, want, (name, size, iterations))
    assert not np.array_equal(got, frame)


# ------------------------------------------------------------------------------------------------------------------
# 2., 3. synthetic buffers with adversarial values
# ------------------------------------------------------------------------------------------------------------------
AXES = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, -1)], np.float32)
PALETTE = np.array([(0.73, 0.73, 0.73), (0.65, 0.05, 0.05), (0.12, 0.45, 0.15), (0.70, 0.72, 0.73)], np.float32)   # the last: 0.03 from the first


def synthetic(width, height, seed):
    """color, albedo, normal, depth: regions of 11 x 9 pixels with one axis normal, one palette albedo and a depth plane each, so that
    taps inside a region weigh and taps across do not; then, each on a few per cent of the pixels (at least one where the image has the
    pixels for it), the adversarial values of the module docstring."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:height, 0:width]
    region = (yy // 9) * 1000 + xx // 11
    normal = AXES[(region * 7 + region // 1000) % 4].copy()
    albedo = PALETTE[(region * 5 + region // 1000) % 4].copy()
    depth = (f32(2) + f32(0.5) * ((region * 3) % 5).astype(np.float32) + f32(0.004) * xx.astype(np.float32)
             + f32(0.003) * yy.astype(np.float32)).astype(np.float32)
    color = rng.random((height, width, 3), dtype=np.float32) * f32(2)
    n = width * height
    order = rng.permutation(n)
    share, few = max(1, n // 40), max(1, n // 2000)                        # `few` for what spreads: NaN and inf colours
    starts = np.cumsum([0] + [few if k in (4, 5, 6) else share for k in range(16)])
    at = lambda k: np.unravel_index(order[starts[k] % n:starts[k] % n + (starts[k + 1] - starts[k])], (height, width))     # noqa: E731
    color[at(0)] = 0.0
    color[at(1)] = -0.0
    color[at(2)] = f32(1e-40)                                              # denormal
    color[at(3)] = f32(1e30)
    color[at(4)] = np.nan
    color[at(5)] = np.inf
    y, x = at(6)
    color[y, x, 1] = -np.inf
    normal[at(7)] = np.nan
    albedo[at(8)] = np.nan
    depth[at(9)] = np.nan
    normal[at(10)] = 0.0                                                   # every sample missed: the pixel keeps its colour
    depth[at(11)] = 0.0
    normal[at(12)] *= f32(0.5)                                             # d = 0.5 against a unit neighbour: 0.5^128 is a denormal weight
    normal[at(13)] *= f32(0.5)
    albedo[at(14)] += f32(0.05)                                            # inside sigma_albedo: a weight strictly between 0 and 1
    y, x = at(15)
    normal[y, x] = (normal[y, x] + rng.normal(0, 0.05, (len(y), 3)).astype(np.float32)).astype(np.float32)
    for a in (color, albedo, normal, depth):
        assert a.dtype == np.float32
        a.setflags(write=False)
    return color, albedo, normal, depth


SHAPES = [(1, 1, 4), (3, 2, 4), (5, 70, 4), (70, 5, 4), (64, 64, 4), (65, 33, 4), (300, 260, 8)]


@pytest.fixture(scope="module")
def synth():
    """(width, height, iterations) -> buffers and the restatement's result with all guides and default parameters; computed once."""
    cache = {}

    def get(width, height, iterations):
        key = (width, height, iterations)
        if key not in cache:
            bufs = synthetic(width, height, seed=1000 + width * 7 + height)
            want = restated(*bufs, iterations=iterations)
            want.setflags(write=False)
            cache[key] = (bufs, want)
        return cache[key]

    return get


@pytest.mark.parametrize("width,height,iterations", SHAPES, ids=["%dx%d-it%d" % s for s in SHAPES])
def test_shapes_and_adversarial_values(trt, synth, width, height, iterations):
    (color, albedo, normal, depth), want = synth(width, height, iterations)
    got = trt.denoise(color, albedo, normal, depth, iterations=iterations)
    assert_same(got, want, (width, height, iterations))
    if width * height >= 64 * 64:
        # the cases the values are there for do occur: weights that are denormal, NaN pixels that stayed contained, pixels kept as they were
        assert np.isnan(want).any() and not np.isnan(want).all(axis=2).all()
        assert (np.isfinite(want).all(axis=2)).mean() > 0.2


def test_the_adversarial_weights_occur():
    """What test_shapes_and_adversarial_values relies on, shown on the restatement's own terms: in the 65 x 33 buffers there are taps
    whose normal weight is the denormal 2^-128, taps removed by a NaN guide next to pixels that stay finite, and a zero-normal pixel that
    keeps its colour (to the rounding of w * c / w) after all passes."""
    color, albedo, normal, depth = synthetic(65, 33, seed=1000 + 65 * 7 + 33)
    with np.errstate(all="ignore"):
        d = (normal[:, :-1] * normal[:, 1:]).sum(axis=2, dtype=np.float32)
        w = d.copy()
        for _ in range(7):
            w = w * w
    assert (w == f32(2.0) ** f32(-128)).any() and f32(2.0) ** f32(-128) > 0
    zero = np.argwhere((normal == 0).all(axis=2) & np.isfinite(color).all(axis=2))
    assert len(zero) > 0
    out = restated(color, albedo, normal, depth, iterations=4)
    for y, x in zero:                                                      # (h*h * c) * (1 / (h*h)) per pass: the colour to rounding
        assert np.allclose(out[y, x], color[y, x], rtol=2e-6, atol=0.0)
    nan_guides = np.isnan(normal).any(axis=2) | np.isnan(albedo).any(axis=2) | np.isnan(depth)
    assert nan_guides.any() and np.isfinite(out[nan_guides & np.isfinite(color).all(axis=2)]).any()


# ------------------------------------------------------------------------------------------------------------------
# 4. guide subsets and switches
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subset", range(8))
def test_every_guide_subset(trt, synth, subset):
    (color, albedo, normal, depth), _ = synth(65, 33, 4)
    guides = dict(albedo=albedo if subset & 1 else None, normal=normal if subset & 2 else None, depth=depth if subset & 4 else None)
    assert_same(trt.denoise(color, iterations=3, **guides), restated(color, iterations=3, **guides), sorted(k for k, v in guides.items() if v is not None))


@pytest.mark.parametrize("over", (dict(sigma_albedo=0.0), dict(sigma_depth=0.0), dict(normal_power_log2=0), dict(sigma_albedo=-1.0, sigma_depth=-0.0),
                                  dict(normal_power_log2=10, sigma_albedo=0.02, sigma_depth=0.5)), ids=str)
def test_switches(trt, synth, over):
    (color, albedo, normal, depth), _ = synth(65, 33, 4)
    assert_same(trt.denoise(color, albedo, normal, depth, iterations=3, **over), restated(color, albedo, normal, depth, iterations=3, **over), over)


# ------------------------------------------------------------------------------------------------------------------
# 5. independent of the restatement
# ------------------------------------------------------------------------------------------------------------------
def test_impulse_is_the_integer_convolution_of_the_two_kernels(trt):
    """One pixel 1, the rest 0, on 41 x 37 under constant guides: every stop is exactly 1, all terms are dyadic, so after two passes
    out * 65536 is the integer convolution of [1,4,6,4,1] x [1,4,6,4,1] at step 1 with the same at step 2, exactly, and the sum is 1.
    (Within 10 pixels of the impulse every tap is inside the image, so ws = 1 there; elsewhere the numerator is 0.)"""
    width, height, cx, cy = 41, 37, 20, 18
    color = np.zeros((height, width, 3), np.float32)
    color[cy, cx] = 1.0
    normal = np.zeros((height, width, 3), np.float32)
    normal[..., 2] = 1.0
    albedo = np.full((height, width, 3), 0.5, np.float32)
    depth = np.full((height, width), 2.0, np.float32)
    got = trt.denoise(color, albedo, normal, depth, iterations=2)
    k = np.array([1, 4, 6, 4, 1], np.int64)
    want = np.zeros((height, width), np.int64)
    for dy1 in range(-2, 3):
        for dx1 in range(-2, 3):
            for dy2 in range(-2, 3):
                for dx2 in range(-2, 3):
                    want[cy + dy1 + 2 * dy2, cx + dx1 + 2 * dx2] += k[dy1 + 2] * k[dx1 + 2] * k[dy2 + 2] * k[dx2 + 2]
    assert want.sum() == 65536
    scaled = got.astype(np.float64) * 65536.0
    for ch in range(3):
        assert np.array_equal(scaled[..., ch], want.astype(np.float64)), ch
    assert float(got[..., 0].astype(np.float64).sum()) == 1.0


# ------------------------------------------------------------------------------------------------------------------
# 6. device form, kernel forms
# ------------------------------------------------------------------------------------------------------------------
GUARD = 100                                                                 # bytes: a multiple of 4, not of 16


def guarded(torch, payload_bytes, fill=0xCD):
    return torch.full((GUARD + payload_bytes + GUARD,), fill, dtype=torch.uint8, device="cuda:0")


def guards_intact(t, payload_bytes, fill=0xCD):
    h = t.cpu().numpy()
    return bool((h[:GUARD] == fill).all() and (h[GUARD + payload_bytes:] == fill).all())


@pytest.mark.parametrize("width,height,iterations", [(65, 33, 4), (300, 260, 8)], ids=["65x33-it4", "300x260-it8"])
def test_device_form_equals_host_form(trt, synth, width, height, iterations):
    import torch
    (color, albedo, normal, depth), want = synth(width, height, iterations)
    n = width * height
    need = trt.denoise_scratch_bytes(width, height, iterations=iterations)
    assert need > 0
    host = dict(color=color, albedo=albedo, normal=normal, depth=depth)
    side = torch.cuda.Stream()
    for stream in (None, side):
        dev = {k: torch.from_numpy(v.copy()).to("cuda:0") for k, v in host.items()}
        out = guarded(torch, n * 12)
        scratch = guarded(torch, need)
        torch.cuda.synchronize()
        trt.denoise_device(dev["color"].data_ptr(), width, height, out.data_ptr() + GUARD, scratch.data_ptr() + GUARD, need,
                           d_albedo_ptr=dev["albedo"].data_ptr(), d_normal_ptr=dev["normal"].data_ptr(), d_depth_ptr=dev["depth"].data_ptr(),
                           stream_ptr=0 if stream is None else stream.cuda_stream, iterations=iterations)
        (torch.cuda.current_stream() if stream is None else stream).synchronize()
        torch.cuda.synchronize()
        got = out.cpu().numpy()[GUARD:GUARD + n * 12].copy().view(np.float32).reshape(height, width, 3)
        assert_same(got, want, (width, height, "device form", stream is not None))
        assert guards_intact(out, n * 12), "bytes round d_out were written"
        assert guards_intact(scratch, need), "bytes round d_scratch were written"
        for k, v in host.items():
            assert dev[k].cpu().numpy().tobytes() == v.tobytes(), k + " was changed"


@pytest.mark.parametrize("variant", ("plain", "packed", "lds"))
def test_kernel_forms_give_equal_bytes(trt, synth, monkeypatch, variant):
    """The plain partner (dword loads, no packing, no LDS), the packed records from global memory at every step and the LDS tile at
    every step it can serve (1, 2, 4) against the shipped choice - and so against the restatement."""
    for width, height, iterations in ((65, 33, 4), (300, 260, 8)):
        (color, albedo, normal, depth), want = synth(width, height, iterations)
        monkeypatch.setenv("TRT_DENOISE_VARIANT", variant)
        got = trt.denoise(color, albedo, normal, depth, iterations=iterations)
        monkeypatch.delenv("TRT_DENOISE_VARIANT")
        assert_same(got, want, (variant, width, height))
    (color, albedo, normal, depth), _ = synth(65, 33, 4)
    monkeypatch.setenv("TRT_DENOISE_VARIANT", variant)
    got = trt.denoise(color, None, normal, None, iterations=3)
    monkeypatch.delenv("TRT_DENOISE_VARIANT")
    assert_same(got, restated(color, None, normal, None, iterations=3), (variant, "normal only"))


# ------------------------------------------------------------------------------------------------------------------
# 7. it denoises
# ------------------------------------------------------------------------------------------------------------------
def tonemapped_mse(a, ref):
    g = lambda v: np.clip(v.astype(np.float64), 0.0, 1.0) ** (1.0 / 2.2)     # noqa: E731
    return float(np.mean((g(a) - g(ref)) ** 2))


@pytest.mark.parametrize("name", ("cornell", "dummy_spheres"))
def test_it_denoises(trt, name):
    """4 spp, max_bounces 50, seed 5, the scene's own background, against the product's render at 1024 / 512 spp, seed 77: with the
    default parameters the tonemapped mean squared error falls to at most 0.5 of the noisy frame's (the definition, run on the CPU over
    the oracle's frames, gives 0.145 and 0.18: the bound leaves room for nothing but an implementation that does not follow it)."""
    desc, ref_spp = (trt.scenes.cornell(96, 96), 1024) if name == "cornell" else (trt.scenes.dummy_spheres(width=128, height=96), 512)
    world, cam = trt.world_from_description(desc)
    noisy_r = trt.Renderer(4, 1, 50, False, desc["background"], seed=5)
    noisy = noisy_r.render(cam, world).data
    aov = noisy_r.render_aov(cam, world, channels=("albedo", "normal", "depth"))
    ref = trt.Renderer(ref_spp, 1, 50, False, desc["background"], seed=77).render(cam, world).data
    out = trt.denoise(noisy, aov["albedo"], aov["normal"], aov["depth"])
    e_noisy, e_out = tonemapped_mse(noisy, ref), tonemapped_mse(out, ref)
    print(f"\n{name}: tonemapped MSE noisy {e_noisy:.6f}, denoised {e_out:.6f}, ratio {e_out / e_noisy:.4f}")
    assert np.isfinite(out).all()
    assert e_out <= 0.5 * e_noisy, (name, e_noisy, e_out)
