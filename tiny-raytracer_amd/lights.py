"""Emitter tables for the direct-light queries (tinyrt.h trt_direct): numpy records of trt_emitter.

A table is a record array of EMITTER_DTYPE.  Scene.emitters() lists a scene's own lights; quad() and sphere() make the record of a light
that is no geometry of the scene - a virtual lamp - through the library's own init functions, so `normal` and `area` carry the bits the
library computes.  Tables are plain arrays: index, slice and np.concatenate them; table() joins records and tables into one.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import Vec3, lib

# tinyrt.h trt_emitter as a numpy record (80 bytes, no padding)
EMITTER_DTYPE = np.dtype([("kind", np.uint32), ("geometry", np.uint32), ("a", np.float32, (3,)), ("b", np.float32, (3,)), ("c", np.float32, (3,)),
                          ("normal", np.float32, (3,)), ("color", np.float32, (3,)), ("area", np.float32), ("reserved", np.uint32, (2,))])
assert EMITTER_DTYPE.itemsize == C.sizeof(_lib.Emitter) == 80
# tinyrt.h trt_emitter_pick as a numpy record (16 bytes)
PICK_DTYPE = np.dtype([("q", np.float32), ("alias", np.uint32), ("prob", np.float32), ("reserved", np.uint32)])
assert PICK_DTYPE.itemsize == C.sizeof(_lib.EmitterPick) == 16
SPHERE, QUAD = _lib.EMITTER_SPHERE, _lib.EMITTER_QUAD
NO_GEOMETRY = _lib.NO_GEOMETRY


def _record(pod):
    return np.frombuffer(bytes(pod), EMITTER_DTYPE).copy()


def quad(corner, u, v, color):
    """trt_emitter_init_quad: the one-record table of a quad lamp (corner, u, v as in Quad::new) that emits `color` from both faces."""
    e = _lib.Emitter()
    lib.trt_emitter_init_quad(C.byref(e), Vec3(*corner), Vec3(*u), Vec3(*v), Vec3(*color))
    return _record(e)


def sphere(centre, radius, color):
    """trt_emitter_init_sphere: the one-record table of a sphere lamp."""
    e = _lib.Emitter()
    lib.trt_emitter_init_sphere(C.byref(e), Vec3(*centre), float(radius), Vec3(*color))
    return _record(e)


def table(*parts):
    """One contiguous table from records and tables, in the order given."""
    parts = [np.ascontiguousarray(p, EMITTER_DTYPE).reshape(-1) for p in parts]
    return np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros(0, EMITTER_DTYPE)


def pick_table(table, weights=None):
    """trt_emitter_pick_build: (records, total) - the alias table (PICK_DTYPE, one record per emitter) through which direct(pick=...)
    chooses emitter e with probability weights[e] / total, and that total.  weights=None: each emitter's power (luminance of its colour
    x area), the table direct(mis=..., pick=...) needs; else float32 [E], finite and non-negative with a positive sum (direct() without
    mis only).  Host only, deterministic."""
    t = np.ascontiguousarray(table)
    if t.dtype != EMITTER_DTYPE or t.ndim != 1:
        raise ValueError("table must be a one-dimensional record array of lights.EMITTER_DTYPE")
    w = None
    if weights is not None:
        w = np.ascontiguousarray(weights, np.float32)
        if w.shape != (len(t),):
            raise ValueError("weights must be float32 [len(table)]")
    out = np.zeros(len(t), PICK_DTYPE)
    total = C.c_float(0.0)
    _lib.check(lib.trt_emitter_pick_build(t.ctypes.data if len(t) else None, len(t), w.ctypes.data if w is not None and len(w) else None,
                                          out.ctypes.data if len(t) else None, C.byref(total)))
    return out, np.float32(total.value)
