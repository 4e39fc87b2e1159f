"""What tests/test_gpu_denoise_color.py and tests/test_gpu_moments.py share, none of it touching a GPU: the numpy restatement of
trt_denoise_ex's definition (tinyrt.h) and of trt_variance, the oracle's exact per-sample colours, and the error measure.
Everything is np.float32, one IEEE operation per operator, nothing fused, denormals kept."""
import numpy as np

f32 = np.float32
H5 = np.array([0.0625, 0.25, 0.375, 0.25, 0.0625], np.float32)
B3 = np.array([0.25, 0.5, 0.25], np.float32)


def restated_variance(accum, moment2, n):
    """tinyrt.h trt_variance: float32 [...]: ((d.r + d.g) + d.b) * (1 / (N - 1)), d = max(M - S*S, 0) per channel, NaN -> 0; N <= 1: +inf."""
    s, m = accum.astype(np.float32), moment2.astype(np.float32)
    if n <= 1:
        return np.full(s.shape[:-1], np.inf, np.float32)
    with np.errstate(all="ignore"):
        d = m - s * s
        d = np.where(d > 0, d, f32(0))
        out = ((d[..., 0] + d[..., 1]) + d[..., 2]) * (f32(1) / f32(n - 1))
    assert out.dtype == np.float32
    return out


def restated_prefilter(variance):
    """v_0: the 3 x 3 average of the variance, weights {0.25, 0.5, 0.25} per axis, dy outer, dx inner, over the taps inside the image,
    divided by the sum of the weights used through one reciprocal."""
    Hh, Ww = variance.shape
    yy, xx = np.mgrid[0:Hh, 0:Ww]
    sv = np.zeros((Hh, Ww), np.float32)
    sw = np.zeros((Hh, Ww), np.float32)
    with np.errstate(all="ignore"):
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                qy, qx = yy + dy, xx + dx
                ok = (qy >= 0) & (qy < Hh) & (qx >= 0) & (qx < Ww)
                k = B3[dy + 1] * B3[dx + 1]
                vq = variance[np.clip(qy, 0, Hh - 1), np.clip(qx, 0, Ww - 1)]
                sv = np.where(ok, sv + k * vq, sv)
                sw = np.where(ok, sw + k, sw)
        out = sv * (f32(1) / sw)
    assert out.dtype == np.float32
    return out


def restated(color, albedo=None, normal=None, depth=None, variance=None, sigma_color=0.0, iterations=4, normal_power_log2=7, sigma_albedo=0.1,
             sigma_depth=0.05, return_variance=False):
    """The specification of trt_denoise_ex; with variance None or sigma_color <= 0, of trt_denoise."""
    Hh, Ww, _ = color.shape
    c = color.astype(np.float32).copy()
    yy, xx = np.mgrid[0:Hh, 0:Ww]
    use_a = albedo is not None and sigma_albedo > 0
    use_z = depth is not None and sigma_depth > 0
    use_c = variance is not None and sigma_color > 0
    if use_a:
        inv_a = f32(1) / (f32(sigma_albedo) * f32(sigma_albedo))
    v = None
    with np.errstate(all="ignore"):
        if use_c:
            v = restated_prefilter(variance.astype(np.float32))
            sc2 = f32(sigma_color) * f32(sigma_color)
        for it in range(iterations):
            step = 1 << it
            if use_z:
                s = (f32(sigma_depth) * depth) * f32(step)
                inv_z = f32(1) / (s * s)
            if use_c:
                inv_c = f32(1) / (sc2 * v)
                va = np.zeros((Hh, Ww), np.float32)
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
                        if use_c:
                            dc = c - c[qyc, qxc]
                            e = (dc[..., 0] * dc[..., 0] + dc[..., 1] * dc[..., 1]) + dc[..., 2] * dc[..., 2]
                            m = f32(1) - e * inv_c
                            m = np.where(m > 0, m, f32(0))
                            w = w * (m * m)
                    take = ok & (w > 0)
                    acc = np.where(take[..., None], acc + w[..., None] * c[qyc, qxc], acc)
                    ws = np.where(take, ws + w, ws)
                    if use_c:
                        va = np.where(take, va + (w * w) * v[qyc, qxc], va)
            r = f32(1) / ws
            c = acc * r[..., None]
            if use_c:
                v = va * (r * r)
    assert c.dtype == np.float32
    return (c, v) if return_variance else c


def assert_same(got, want, what):
    """Bits; a component that is NaN in `want` by NaN-ness.  Every element is compared."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape, got.dtype)
    same = np.where(np.isnan(want), np.isnan(got), got.view(np.uint32) == want.view(np.uint32))
    bad = np.argwhere(~same)
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def tonemapped_mse(a, ref):
    g = lambda v: np.clip(v.astype(np.float64), 0.0, 1.0) ** (1.0 / 2.2)     # noqa: E731
    return float(np.mean((g(a) - g(ref)) ** 2))


def oracle_samples(orc, ow, ocam, n, max_bounces, background, seed, nthreads=4):
    """float32 [n, H, W, 3]: the colour of every sample, exactly.  For n a power of two the oracle's render of the one sample s at
    samples_per_pixel = n is c_s * (1/n), and multiplying by n gives c_s back bit for bit provided no value is denormal: every
    non-zero magnitude must be at least 2^-100 (a condition on the inputs, asserted here, not a tolerance)."""
    assert n >= 1 and n & (n - 1) == 0, n
    out = np.zeros((n, ocam.height, ocam.width, 3), np.float32)
    for s in range(n):
        one, _ = orc.render(ow, ocam, n, max_bounces, background, seed=seed, nthreads=nthreads, sample_begin=s, sample_end=s + 1)
        mag = np.abs(one[np.isfinite(one) & (one != 0)])
        assert mag.size == 0 or mag.min() >= f32(2.0) ** f32(-100), (s, float(mag.min()))
        out[s] = one * f32(n)
    return out


def fold_moments(samples, n, begin=0, end=None, start=None):
    """(S, M): the imager's fold of the samples [begin, end) of `samples` (as oracle_samples returns them) and of their squares, in
    sample order: S = S + c * (1/n), M.ch = M.ch + (c.ch * c.ch) * (1/n); `start`: the (S, M) of earlier passes to continue."""
    inv = f32(1) / f32(n)
    end = len(samples) if end is None else end
    s = np.zeros(samples.shape[1:], np.float32) if start is None else start[0].copy()
    m = np.zeros(samples.shape[1:], np.float32) if start is None else start[1].copy()
    with np.errstate(all="ignore"):
        for k in range(begin, end):
            c = samples[k]
            s = s + c * inv
            m = m + (c * c) * inv
    assert s.dtype == m.dtype == np.float32
    return s, m
