"""The primary ray's image coordinates, (x + u) / (W - 1) and (y + v) / (H - 1), on the device (rt_device.h pixel_uv: one refined reciprocal
per denominator instead of two divisions per ray) through trt_primary_rays, against the reference's arithmetic restated with the CPU
oracle's random draws and numpy's float32 division, bit for bit: the smallest images there are (2 x 2: denominators 1; 3 x 2), a ragged
one (17 x 5) and a band of 8 rows of a 2048-wide image (the benchmark's width; rows 800..807 of 2048).  Column 0 and row 0 are in every
whole image, the 2048-wide band has all the numerators up to 2048.  A 1-wide or 1-high image - the division by zero that keeps the plain
division in pixel_uv - is refused at the C boundary before any device work; tests/test_unit_math.py covers that branch on the CPU."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 9
SPP = 2
CAMERA = dict(focus_distance=10.0, defocus_angle=0.6, position=(13.0, 2.0, 3.0), look_at=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), vertical_fov=20.0)
BAND = dict(band_rows=8, band_stride=256, band_offset=100, rows_local=8)        # the one band of 8 rows that starts at row 800


def restated_rays(orc, ocam, s, rows):
    """float32 [len(rows), W, 6]: pointgen.rs:41-43 and camera.rs:58-66 for sample s of the pixels of `rows`; the draws are the oracle's, in
    the reference's order (u, v, the unit disk), the arithmetic numpy's float32 (one IEEE operation per operator), Ray::new the oracle's."""
    width, height = ocam.width, ocam.height
    n = len(rows) * width
    ru, rv, px, py, xs, ys = (np.zeros(n, np.float32) for _ in range(6))
    rng = (C.c_uint32 * 2)()
    i = 0
    for y in rows:
        for x in range(width):
            orc.lib.orc_rng_seed(SEED, y * width + x, s, rng)
            ru[i] = orc.lib.orc_rng_random(rng)
            rv[i] = orc.lib.orc_rng_random(rng)
            p = orc.lib.orc_random_in_unit_disk(rng)
            px[i], py[i], xs[i], ys[i] = p.x, p.y, x, y
            i += 1
    u = ((xs + ru) / np.float32(width - 1))[:, None]
    v = ((ys + rv) / np.float32(height - 1))[:, None]
    vec = lambda name: np.array(getattr(ocam, name).tolist(), np.float32)[None, :]          # noqa: E731
    origin = (vec("position") + px[:, None] * vec("defocus_disk_u")) + py[:, None] * vec("defocus_disk_v")
    target = (vec("viewport_upper_left") + u * vec("horizontal")) - v * vec("vertical")
    direction = target - origin
    assert origin.dtype == direction.dtype == u.dtype == np.float32
    out = np.zeros((n, 6), np.float32)
    for i in range(n):
        r = orc.lib.orc_ray_new(orc.Vec3(*origin[i]), orc.Vec3(*direction[i]))
        out[i, :3] = r.origin.tolist()
        out[i, 3:] = r.direction.tolist()
    return out.reshape(len(rows), width, 6)


@pytest.mark.parametrize("width,height,bands", [(2, 2, {}), (3, 2, {}), (17, 5, {}), (2048, 2048, BAND)],
                         ids=["2x2", "3x2", "17x5", "2048-wide-band-of-8-rows"])
def test_primary_rays_equal_the_restated_reference_rays(trt, orc, width, height, bands):
    cam = trt.Camera(width=width, height=height, **CAMERA)
    ocam = orc.camera(width=width, height=height, **CAMERA)
    rows = list(range(800, 808)) if bands else list(range(height))
    for s in range(SPP):
        got = cam.primary_rays(s, SPP, seed=SEED, **bands)
        want = restated_rays(orc, ocam, s, rows)
        assert got.shape == want.shape == (len(rows), width, 6) and got.dtype == want.dtype
        differ = int((got.view(np.uint32) != want.view(np.uint32)).sum())
        print(f"{width}x{height} sample {s}: {differ} of {got.size} values differ")
        assert not np.isnan(want).any()
        assert differ == 0


@pytest.mark.parametrize("width,height", [(1, 4), (4, 1)])
def test_a_one_wide_or_one_high_image_is_refused(trt, width, height):
    cam = trt.Camera(width=4, height=4, **CAMERA)
    cam.pod.width, cam.pod.height = width, height
    with pytest.raises(trt.TinyRTError) as e:
        cam.primary_rays(0, SPP, seed=SEED)
    assert e.value.code == trt._lib.ERR_INVALID_ARG
