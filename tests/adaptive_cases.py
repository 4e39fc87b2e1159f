"""Numpy restatements shared by tests/test_gpu_adaptive.py and tools/adaptive_quality.py: tinyrt.h trt_select_pixels and the loop of
Renderer.render_adaptive (api.py), driven over the CPU oracle's exact per-sample colours.  Nothing here touches a GPU."""
import numpy as np

import denoise_color_cases as D

f32 = np.float32


def restated_select(accum, moment2, n_cap, done, rel_tol, abs_tol, candidates=None, n=None):
    """uint32 array: tinyrt.h trt_select_pixels - all float32, one operation per operator, in the header's order; candidate order kept.
    candidates None: the pixels 0 .. n-1 (n None: all)."""
    s_all, m_all = accum.reshape(-1, 3), moment2.reshape(-1, 3)
    npixels = len(s_all)
    cand = np.arange(npixels if n is None else n, dtype=np.uint32) if candidates is None else np.asarray(candidates, np.uint32)
    inside = cand < npixels
    if done <= 1:
        return cand[inside].copy()
    k = f32(n_cap) / f32(done)
    inv = f32(1.0) / f32(done - 1)
    rel2 = f32(rel_tol) * f32(rel_tol)
    abs2 = f32(abs_tol) * f32(abs_tol)
    idx = np.where(inside, cand, 0)
    with np.errstate(all="ignore"):
        s = s_all[idx] * k
        q = m_all[idx] * k
        d = q - s * s
        d = np.where(d > 0, d, f32(0))
        v = ((d[:, 0] + d[:, 1]) + d[:, 2]) * inv
        lum = (s[:, 0] + s[:, 1]) + s[:, 2]
        b = rel2 * (lum * lum)
        b = b + abs2
        keep = (v > b) & inside
    assert v.dtype == b.dtype == np.float32
    return cand[keep].copy()


def restated_adaptive(samples, min_spp, step_spp, rel_tol, abs_tol, render_range=None):
    """The loop of Renderer.render_adaptive over `samples` (float32 [N, H, W, 3], exact, as denoise_color_cases.oracle_samples returns
    them; N is the cap): (frame, S, M, count, history).  Each range is folded for the WHOLE frame from the current state and only the
    active pixels' results are kept.  `render_range(begin, end, state)`: a whole-frame render of that range that continues `state`
    (orc.render with accum): when given, the sums it returns must be the fold's, bit for bit.  history: the active set of every round."""
    n_cap, h, w, _ = samples.shape
    assert 2 <= min_spp <= n_cap and step_spp >= 1

    def advance(begin, end, s, m):
        s2, m2 = D.fold_moments(samples, n_cap, begin, end, start=(s, m))
        if render_range is not None:
            D.assert_same(render_range(begin, end, s.copy()), s2, ("oracle render of", begin, end))
        return s2, m2

    s, m = advance(0, min_spp, np.zeros((h, w, 3), f32), np.zeros((h, w, 3), f32))
    count = np.full(h * w, min_spp, np.uint32)
    done = min_spp
    active = restated_select(s, m, n_cap, done, rel_tol, abs_tol)
    history = [active]
    while len(active) and done < n_cap:
        nxt = min(done + step_spp, n_cap)
        s2, m2 = advance(done, nxt, s, m)
        s, m = s.copy(), m.copy()
        s.reshape(-1, 3)[active] = s2.reshape(-1, 3)[active]
        m.reshape(-1, 3)[active] = m2.reshape(-1, 3)[active]
        count[active] = nxt
        done = nxt
        active = restated_select(s, m, n_cap, done, rel_tol, abs_tol, candidates=active)
        history.append(active)
    count = count.reshape(h, w)
    frame = s * (f32(n_cap) / count.astype(f32))[..., None]
    assert frame.dtype == np.float32
    return frame, s, m, count, history
