"""Surfel lists for Scene.gather (tinyrt.h trt_gather): host arithmetic only, nothing here touches the library."""
import numpy as np


def quad_texels(corner, u, v, nu, nv, flip=False):
    """The texels of a lightmap over the quad (corner, u, v) as surfels float32 [nv * nu, 6], row j (along v) by row, column i (along u)
    fastest: the point is the texel centre corner + (i + .5) / nu * u + (j + .5) / nv * v, the axis the unit normal cross(u, v) / |cross(u, v)|
    - its negative with flip - the same for every texel.  Computed in float64 and rounded once."""
    corner, u, v = (np.asarray(a, np.float64).reshape(3) for a in (corner, u, v))
    nu, nv = int(nu), int(nv)
    if nu < 1 or nv < 1:
        raise ValueError("a lightmap has at least one texel each way")
    normal = np.cross(u, v)
    length = np.linalg.norm(normal)
    if not (np.isfinite(length) and length > 0.0):
        raise ValueError("u and v span no plane")
    axis = normal / length * (-1.0 if flip else 1.0)
    a = (np.arange(nu, dtype=np.float64) + 0.5) / nu
    b = (np.arange(nv, dtype=np.float64) + 0.5) / nv
    out = np.empty((nv, nu, 6), np.float64)
    out[..., 0:3] = corner + a[None, :, None] * u + b[:, None, None] * v
    out[..., 3:6] = axis
    return np.ascontiguousarray(out.reshape(nv * nu, 6).astype(np.float32))
