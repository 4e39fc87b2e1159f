"""What tests/test_gpu_radiance.py and tests/test_gpu_radiance_long.py share, none of it touching a GPU: the rays of a scene, the oracle's
per-sample colours through orc.sample_batch (the restatement of the entry point whose RNG numbering trt_radiance continues), and the fold
of tinyrt.h in numpy float32 - one IEEE operation per operator, nothing fused."""
import numpy as np

f32 = np.float32
K, MAX_BOUNCES, SEED, FIRST_STREAM = 8, 8, 5, 1000
GRID_W, GRID_H = 20, 16
N_RAYS = GRID_W * GRID_H + 4
SCALES = (1.0, 0.25, 3.0)
DUMMY = (1e6, 1e6, 1e6, 1.0, 0.0, 0.0)                                      # origin, direction of a leading point that only occupies a stream
# trt_sample_point / orc.SamplePoint as a numpy record (32 bytes)
POINT_DTYPE = np.dtype([("x", np.uint32), ("y", np.uint32), ("ray", np.float32, (6,))])
COLOR_DTYPE = np.dtype([("x", np.uint32), ("y", np.uint32), ("color", np.float32, (3,))])
assert POINT_DTYPE.itemsize == 32 and COLOR_DTYPE.itemsize == 20


def rays_of(desc):
    """324 rays float32 [n, 6]: a 20 x 16 pinhole grid through the pixel centres of the description's camera (position, look_at, up,
    vertical_fov; float64, rounded once to f32), directions normalised and then scaled by (1, 0.25, 3)[k % 3]; then four rays at the camera
    position: NaN origin.x, direction (inf, 0, 1), direction (0, 0, 0), direction (NaN, 1, 0)."""
    cam = desc["camera"]
    pos, at, up = (np.array(cam[k], np.float64) for k in ("position", "look_at", "up"))
    fwd = (at - pos) / np.linalg.norm(at - pos)
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    upv = np.cross(right, fwd)
    half_h = np.tan(np.radians(float(cam["vertical_fov"])) / 2.0)
    half_w = half_h * GRID_W / GRID_H
    y, x = np.mgrid[0:GRID_H, 0:GRID_W]
    u = ((x.reshape(-1) + 0.5) / GRID_W * 2.0 - 1.0) * half_w
    v = (1.0 - (y.reshape(-1) + 0.5) / GRID_H * 2.0) * half_h
    d = fwd[None, :] + u[:, None] * right[None, :] + v[:, None] * upv[None, :]
    d /= np.linalg.norm(d, axis=1)[:, None]
    d *= np.array(SCALES, np.float64)[np.arange(len(d)) % 3][:, None]
    rays = np.concatenate([np.broadcast_to(pos, d.shape), d], axis=1)
    odd = np.array([[np.nan, pos[1], pos[2], 0.0, 0.0, 1.0], [*pos, np.inf, 0.0, 1.0], [*pos, 0.0, 0.0, 0.0], [*pos, np.nan, 1.0, 0.0]], np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        out = np.ascontiguousarray(np.concatenate([rays, odd]).astype(np.float32))
    assert out.shape == (N_RAYS, 6)
    return out


def points_of(struct, rays, dummies=0):
    """A ctypes array of `struct` (trt.SamplePoint or orc.SamplePoint): `dummies` leading points, then ray j at point dummies + j.  Built
    from a numpy record array; the ctypes array shares its memory."""
    rec = np.zeros(dummies + len(rays), POINT_DTYPE)
    rec["ray"][:dummies] = np.array(DUMMY, np.float32)
    rec["ray"][dummies:] = rays
    return (struct * max(len(rec), 1)).from_buffer(rec if len(rec) else np.zeros(1, POINT_DTYPE))


def colors_of(out, n):
    """float32 [n, 3] of a SampledColor array."""
    return np.frombuffer(out, COLOR_DTYPE, count=n)["color"].copy()


def oracle_samples(orc, ow, rays, k, max_bounces, background, seed, first_stream):
    """(colours float32 [n, k, 3] of samples 0..k of every ray under trt_radiance's numbering, the oracle's world.hit calls for them):
    orc.sample_batch over first_stream dummy points followed by each ray k times; the dummies' own rays are taken off by a second call
    over the dummies alone (the same streams, hence the same paths)."""
    rep = np.repeat(rays, k, axis=0)
    out, st = orc.sample_batch(ow, points_of(orc.SamplePoint, rep, first_stream), max_bounces, background, seed)
    cols = colors_of(out, first_stream + len(rep))[first_stream:].reshape(len(rays), k, 3)
    n_rays = st["rays"]
    if first_stream:
        _, st0 = orc.sample_batch(ow, points_of(orc.SamplePoint, rep[:0], first_stream), max_bounces, background, seed)
        n_rays -= st0["rays"]
    return cols, n_rays


def fold(cols, k, begin=0, end=None, s=None, m=None):
    """tinyrt.h trt_radiance: S.ch = S.ch + c.ch * inv_K; M.ch = M.ch + (c.ch * c.ch) * inv_K over samples [begin, end) in order, from
    (s, m) or from 0."""
    end = cols.shape[1] if end is None else end
    inv = f32(1.0) / f32(k)
    S = np.zeros((cols.shape[0], 3), np.float32) if s is None else s.copy()
    M = np.zeros((cols.shape[0], 3), np.float32) if m is None else m.copy()
    with np.errstate(all="ignore"):
        for i in range(begin, end):
            c = cols[:, i, :]
            S = S + c * inv
            M = M + (c * c) * inv
    assert S.dtype == np.float32 and M.dtype == np.float32
    return S, M


def assert_same_bits(got, want, what):
    """Every f32 by its bits; a channel whose reference is NaN by NaN-ness."""
    nan = np.isnan(want)
    same = np.where(nan, np.isnan(got), got.view(np.uint32) == want.view(np.uint32))
    bad = np.flatnonzero(~same.reshape(len(want), -1).all(axis=1))
    assert len(bad) == 0, (what, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
