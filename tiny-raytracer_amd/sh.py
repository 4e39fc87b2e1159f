"""Real spherical harmonics as the probe queries use them (tinyrt.h trt_probe): the basis in the graphics convention - no Condon-Shortley
sign, coefficient index k = l (l + 1) + m, bands l = 0 .. 2 - and what a caller does with the coefficients Scene.probe returns: evaluate
the projected radiance in a direction, or the irradiance about a normal.  Host arithmetic only (numpy)."""
import numpy as np

f32 = np.float32
C0, C1, C2, C3, C4 = f32(0.282094792), f32(0.488602512), f32(1.092548431), f32(0.315391565), f32(0.546274215)
BAND_OF = (0, 1, 1, 1, 2, 2, 2, 2, 2)                                       # l of coefficient k
# the cosine lobe's zonal coefficients (Ramamoorthi & Hanrahan 2001): irradiance = sum_k A_l(k) L_k Y_k(n)
COSINE_LOBE = (np.pi, 2.0 * np.pi / 3.0, np.pi / 4.0)
# the solid angle the draws of a domain cover: 4 pi sh[k] (sphere) or 2 pi sh[k] (hemisphere) estimates the integral of L Y_k
SOLID_ANGLE = {"sphere": 4.0 * np.pi, "hemisphere": 2.0 * np.pi}


def _bands_of(coeffs):
    bands = {1: 1, 4: 2, 9: 3}.get(int(coeffs))
    if bands is None:
        raise ValueError("1, 4 or 9 coefficients (bands 1, 2 or 3)")
    return bands


def basis(d, bands=3):
    """float32 [..., bands ** 2]: the basis at directions d [..., 3], evaluated as the device evaluates it - in f32, one IEEE operation per
    operator, nothing fused, in the parenthesisation of tinyrt.h.  d is used as given (the device passes unit vectors)."""
    if bands not in (1, 2, 3):
        raise ValueError("bands must be 1, 2 or 3")
    d = np.asarray(d, f32)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    with np.errstate(all="ignore"):
        b = [np.full(x.shape, C0, f32)]
        if bands >= 2:
            b += [C1 * y, C1 * z, C1 * x]
        if bands >= 3:
            b += [C2 * (x * y), C2 * (y * z), C3 * ((f32(3.0) * (z * z)) - f32(1.0)), C2 * (x * z), C4 * ((x * x) - (y * y))]
    out = np.stack(b, axis=-1)
    assert out.dtype == f32
    return out


def evaluate(coeffs, d):
    """float64 [..., 3]: sum_k coeffs[..., k, :] * Y_k(d) - the projected function in directions d [..., 3] (broadcast against the leading
    axes of coeffs [..., C, 3]).  Of Scene.probe's sums this is the radiance divided by the domain's solid angle (SOLID_ANGLE)."""
    coeffs = np.asarray(coeffs, np.float64)
    y = basis(d, _bands_of(coeffs.shape[-2])).astype(np.float64)
    return (coeffs * y[..., None]).sum(axis=-2)


def irradiance(coeffs, normal, domain="sphere"):
    """float64 [..., 3]: the irradiance about unit normals [..., 3] from Scene.probe's sums coeffs [..., C, 3] drawn over `domain`:
    sum_k A_l(k) * (omega * coeffs[k]) * Y_k(normal), with A = pi, 2 pi / 3, pi / 4 and omega = 4 pi (sphere) or 2 pi (hemisphere).  Exact
    for the bands kept; three bands hold irradiance to about 1 % for any lighting."""
    if domain not in SOLID_ANGLE:
        raise ValueError("domain must be 'sphere' or 'hemisphere'")
    coeffs = np.asarray(coeffs, np.float64)
    count = coeffs.shape[-2]
    a = np.array([COSINE_LOBE[BAND_OF[k]] for k in range(count)])
    y = basis(normal, _bands_of(count)).astype(np.float64)
    return SOLID_ANGLE[domain] * (coeffs * (a * y)[..., None]).sum(axis=-2)


def project(colors, directions, bands=3, begin=0, end=None, sh=None, points=None):
    """float32 [n, bands ** 2, 3]: the probe fold of tinyrt.h over Scene.samples()'s records - colors and directions float32 [n, K, 3] of
    source "sphere" or "hemisphere" - in numpy f32, one IEEE operation per operator: for samples [begin, end) in order (None: K)
    t = b_k(d) * inv_K; sh[k].ch = sh[k].ch + c.ch * t, inv_K = 1 / K, from `sh` (not changed) or from 0.  A sample whose direction has a
    NaN adds nothing; with `points` float32 [n, 3] (the items' points) neither does a sample of an item whose point has one - the rule
    under which the result is Scene.probe()'s, byte for byte."""
    colors, directions = np.asarray(colors, f32), np.asarray(directions, f32)
    if colors.ndim != 3 or colors.shape[2] != 3 or directions.shape != colors.shape:
        raise ValueError("colors and directions must have the same shape [n, K, 3]")
    n, k = colors.shape[0], colors.shape[1]
    end = k if end is None else end
    inv = f32(1.0) / f32(k)
    out = np.zeros((n, bands * bands, 3), f32) if sh is None else np.array(sh, f32)
    dead = np.zeros(n, bool) if points is None else np.isnan(np.asarray(points, f32)).any(axis=-1)
    with np.errstate(all="ignore"):
        for s in range(begin, end):
            t = basis(directions[:, s, :], bands) * inv                     # [n, C]
            added = out + colors[:, s, None, :] * t[:, :, None]
            folds = ~(np.isnan(directions[:, s, :]).any(axis=1) | dead)
            out = np.where(folds[:, None, None], added, out)
    assert out.dtype == f32
    return out
