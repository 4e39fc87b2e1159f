"""What tests/test_draw_cases.py (CPU) and tests/test_gpu_draws.py (GPU) share, none of it touching a GPU: the case list of the two
functions that draw a sample's first ray on the device (csrc/gather_draw.h gather_ray and probe_ray), the oracle's expectation of every
case, a second float32 restatement of the two draws with ten mutants, and the files of tests/native/draw_cases.hip.

A case is (kind, spread, item, stream j): the first ray drawn about item = (point, axis) from RNG stream (SEED, j, 1).  kind: the two
lobes of trt_gather / trt_ambient / trt_passes ("cosine", "cone") and the two domains of trt_probe ("sphere", "hemisphere").  The
expectation is what gather_cases.first_rays / probe_cases.first_rays make of the oracle's pieces for that item and stream, and the
generator state after the three draws (orc_rng_seed, three orc_rng_next_u32).

Classes (tests/README_draws.md has the counts):
  generic                  random items x consecutive streams per kind; axis scales 1 / 0.25 / 3, the four special items of
                           gather_cases.items_of (NaN point, zero axis, inf component, axis of length 1e-9) every 250th item
  cos_near_zero_taken      cosine, axis = -u_j exactly, and -u_j with one component nudged by the LARGEST number of whole floats for which
                           the oracle still takes near_zero (direction == normalized(axis))
  cos_near_zero_not_taken  the next nudge: the oracle does not take the branch
  cos_u_zero, cone_u_zero, sphere_u_zero, hemi_u_zero
                           the streams of golden/draw_edge_streams.json (u1, u2 or u3 exactly 0) with ordinary finite items
  cone_zero_sum            cone, axis = -(spread * v_j) exactly (spread 0: a zero axis of either sign): Ray::new of the zero vector
  cone_tiny_sum            cone, that axis nudged by one to three floats in one or in all components, and for spread 0 axes of 2^-39-sized
                           and subnormal components: both sides of normalized()'s 2^-39 switch
  hemi_dot_zero            hemisphere, axis = (-u.y, u.x, 0), its rotations, negations and power-of-two multiples: dot(u, axis) is exactly 0
  hemi_dot_subnormal       hemisphere, axis = +-c u_j with c = 2^-130 .. 2^-140, and (-u.y, u.x, +-2^-130): the dot is a subnormal of either sign
  probe_renormalised, probe_not_renormalised
                           sphere and hemisphere with an ordinary item: Ray::new's second normalisation changes the bits of u_j / does not

Mutants of the restatement (restate(mut=k)); test_draw_cases.py prints which classes tell each from the oracle:
   1 near_zero eps 1e-8          2 near_zero eps 1e-6           3 near_zero fallback omitted     4 fallback to +u instead of the axis
   5 hemisphere keeps with >=    6 hemisphere flip omitted      7 probe: second normalisation omitted (the gather lobes normalise once)
   8 spread applied after the sum                               9 subnormal dot flushed to zero  10 stream sample word 0 for 1
"""
import ctypes as C
import json
import os
import struct

import numpy as np

import gather_cases as GC
import probe_cases as PC
import shade_cases as S

F = np.float32
SEED = 5
KINDS = ("cosine", "cone", "sphere", "hemisphere")
GENERIC_PER_KIND = 4000
GENERIC_STREAM0 = {"cosine": 100000, "cone": 200000, "sphere": 300000, "hemisphere": 400000}
CONE_SPREADS = (0.5, 0.0, 1.0, 0.3)
LO = S.LO                                                                    # 2^-39: normalized()'s switch (rt_device.h)
MIN_NORMAL = F(2.0 ** -126)
CASE_WORDS, OUT_WORDS = 9, 8
N_MUTANTS = 10
MUTANT_NAMES = {1: "near_zero eps 1e-8", 2: "near_zero eps 1e-6", 3: "near_zero fallback omitted", 4: "fallback to +u instead of the axis",
                5: "hemisphere keeps with >=", 6: "hemisphere flip omitted", 7: "probe: second normalisation omitted",
                8: "spread applied after the sum", 9: "subnormal dot flushed", 10: "stream sample word 0 for 1"}
# classes whose rows may hold NaN words although the item is finite (0/0 of a zero draw or a zero sum; inf from a subnormal length)
NAN_CLASSES = {"cos_u_zero", "sphere_u_zero", "hemi_u_zero", "cone_zero_sum", "cone_tiny_sum"}
ORDINARY_ITEMS = np.array([[0.5, -1.25, 2.0, 0.36, 0.48, -0.8], [-3.0, 0.125, 0.75, -1.5, 2.0, 2.5]], F)

bits, nextf = S.bits, S.nextf


def edge_streams():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "draw_edge_streams.json")) as f:
        doc = json.load(f)
    assert doc["seed"] == SEED and doc["sample"] == 1
    return {k: [int(j) for j in doc[k]] for k in ("u1_zero", "u2_zero", "u3_zero")}


def seed_key(seed=SEED):
    """kernels.h rng_seed_key: what the device's rng_seed takes in the place of the seed."""
    x = (seed + 0x9E3779B9) & S.MASK
    x ^= x >> 16
    x = (x * 0x7FEB352D) & S.MASK
    x ^= x >> 15
    x = (x * 0x846CA68B) & S.MASK
    return x ^ (x >> 16)


def nudge(x, k):
    """x moved k floats away from zero (k < 0: towards it); finite non-zero x, |k| less than its distance from zero."""
    b = int(bits(F(x))[0])
    m = (b & 0x7FFFFFFF) + k
    assert 0 < m < 0x7F800000, (x, k)
    return np.array([(b & 0x80000000) | m], np.uint32).view(F)[0]


# ------------------------------------------------------------------------------------------------------------------
# the oracle's pieces
# ------------------------------------------------------------------------------------------------------------------
def _vec(v):
    return np.array([v.x, v.y, v.z], F)


def _V(orc, a):
    return orc.Vec3(float(a[0]), float(a[1]), float(a[2]))


def stream_state(orc, j, sample=1):
    rng = (C.c_uint32 * 2)()
    orc.lib.orc_rng_seed(SEED, j & S.MASK, sample, C.byref(rng))
    return rng


def stream_draws(orc, j):
    rng = stream_state(orc, j)
    return [F(orc.lib.orc_rng_random(C.byref(rng))) for _ in range(3)]


def in_sphere_of(orc, j):
    return _vec(orc.lib.orc_random_in_unit_sphere(C.byref(stream_state(orc, j))))


def unit_of(orc, j):
    return _vec(orc.lib.orc_random_unit_vector(C.byref(stream_state(orc, j))))


def state_after(orc, j):
    rng = stream_state(orc, j)
    for _ in range(3):
        orc.lib.orc_rng_next_u32(C.byref(rng))
    return int(rng[0]), int(rng[1])


def oracle_dot(orc, a, b):
    return F(orc.lib.orc_vec3_dot(_V(orc, a), _V(orc, b)))


def oracle_normalized(orc, a):
    return _vec(orc.lib.orc_ray_new(orc.Vec3(), _V(orc, a)).direction)


def oracle_rays(orc, kind, spread, items, j0):
    """float32 [n, 6]: the first ray of item i on stream (SEED, j0 + i, 1), from the two modules that state the draws for the GPU tests."""
    items = np.ascontiguousarray(items, F).reshape(-1, 6)
    if kind in GC.LOBES:
        return GC.first_rays(orc, items, kind, k=1, spread=float(spread), seed=SEED, first_stream=j0)[:, 0]
    return PC.first_rays(orc, items, kind, k=1, seed=SEED, first_stream=j0)[0][:, 0]


def oracle_ray(orc, c):
    return oracle_rays(orc, c["kind"], c["spread"], c["item"], c["j"])[0]


def expectations(orc, cases):
    """uint32 [n, 8]: the six words of the ray and the generator state after the three draws.  Runs of cases with one kind, one spread
    and consecutive streams go through first_rays in one call."""
    out = np.zeros((len(cases), OUT_WORDS), np.uint32)
    i = 0
    while i < len(cases):
        c, e = cases[i], i + 1
        while e < len(cases) and cases[e]["kind"] == c["kind"] and bits(cases[e]["spread"]) == bits(c["spread"]) and cases[e]["j"] == c["j"] + (e - i):
            e += 1
        out[i:e, 0:6] = bits(oracle_rays(orc, c["kind"], c["spread"], np.stack([x["item"] for x in cases[i:e]]), c["j"]))
        i = e
    for i, c in enumerate(cases):
        out[i, 6:8] = state_after(orc, c["j"])
    return out


# ------------------------------------------------------------------------------------------------------------------
# the second restatement: numpy float32 scalars (every operation rounds once, nothing contracts), over orc_random_in_unit_sphere
# ------------------------------------------------------------------------------------------------------------------
def normalized(a):
    return a / np.sqrt(S.dot(a, a))


def restate(orc, c, mut=0, tr=None):
    """uint32 [8] as `expectations`; tr: dict that receives intermediate values."""
    tr = {} if tr is None else tr
    with np.errstate(all="ignore"):
        rng = stream_state(orc, c["j"], 0 if mut == 10 else 1)
        v = _vec(orc.lib.orc_random_in_unit_sphere(C.byref(rng)))
        point, axis, spread = c["item"][0:3], c["item"][3:6], F(c["spread"])
        tr.update(in_sphere=v)
        if c["kind"] == "cosine":
            u = normalized(v)
            d = axis + u
            eps = F(1e-8) if mut == 1 else F(1e-6) if mut == 2 else F(1e-7)
            nz = bool((np.abs(d) < eps).all())
            tr.update(unit=u, sum=d, near_zero=nz)
            if nz and mut != 3:
                d = u if mut == 4 else axis
        elif c["kind"] == "cone":
            d = (axis + v) * spread if mut == 8 else axis + spread * v
            tr.update(sum=d)
        else:
            u = normalized(v)
            d = u
            tr.update(unit=u)
            if c["kind"] == "hemisphere":
                dt = S.dot(u, axis)
                tr.update(dot=dt)
                if mut == 9 and np.abs(dt) < MIN_NORMAL:
                    dt = F(0.0)
                keep = bool(dt >= F(0.0)) if mut == 5 else bool(dt > F(0.0))
                tr.update(flipped=not keep)
                if not keep and mut != 6:
                    d = -u
            if mut == 7:
                return np.concatenate([bits(point), bits(d), np.array([rng[0], rng[1]], np.uint32)])
        return np.concatenate([bits(point), bits(normalized(d)), np.array([rng[0], rng[1]], np.uint32)])


# ------------------------------------------------------------------------------------------------------------------
# the case list
# ------------------------------------------------------------------------------------------------------------------
def _case(cls, kind, spread, item, j, **kw):
    assert kind in KINDS and 0 <= j < (1 << 32)
    return dict(cls=cls, kind=kind, spread=F(spread), item=np.array(item, F), j=int(j), **kw)


def generic_items(n, g):
    """float32 [n, 6]: random points, random unit axes times 1 / 0.25 / 3 (item k: AXIS_SCALES[k % 3], in f32), and every 250th item one of
    the four special items of gather_cases.items_of."""
    axis = g.normal(size=(n, 3))
    axis = (axis / np.linalg.norm(axis, axis=1, keepdims=True)).astype(F)
    axis *= np.array(GC.AXIS_SCALES, F)[np.arange(n) % 3][:, None]
    items = np.concatenate([g.uniform(-5.0, 5.0, (n, 3)).astype(F), axis], axis=1)
    special = np.array([[np.nan, 1.0, 2.0, 0.0, 0.0, 1.0], [1.0, 2.0, 3.0, 0.0, 0.0, 0.0], [1.0, 2.0, 3.0, np.inf, 0.0, 1.0], [1.0, 2.0, 3.0, 0.0, 1e-9, 0.0]], F)
    where = np.arange(125, n, 250)
    items[where] = special[np.arange(len(where)) % 4]
    return np.ascontiguousarray(items, F)


def cosine_taken(orc, item, j):
    got = bits(oracle_rays(orc, "cosine", 0.0, item, j)[0, 3:6])
    return np.array_equal(got, bits(oracle_normalized(orc, item[3:6])))


def near_zero_edge(orc, point, u, j, comp, sign):
    """The smallest k >= 1 for which the oracle does NOT take near_zero when component `comp` of axis = -u is moved sign * k floats (the
    sum is exact there, so the branch is monotone in k: doubling, then bisection)."""
    def taken(k):
        axis = -u
        axis[comp] = nudge(axis[comp], sign * k)
        return cosine_taken(orc, np.concatenate([point, axis]).astype(F), j)
    lo, hi = 0, 1                                                            # taken(lo) (k = 0 is the exact case), looking for not taken(hi)
    while taken(hi):
        lo, hi = hi, hi * 2
        assert hi < (1 << 22)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if taken(mid) else (lo, mid)
    return hi


def case_list(orc):
    g = np.random.default_rng([SEED, 7])
    cases = []
    # ---- generic ----
    for kind in KINDS:
        items = generic_items(GENERIC_PER_KIND, g)
        for i, item in enumerate(items):
            spread = CONE_SPREADS[i // (GENERIC_PER_KIND // len(CONE_SPREADS))] if kind == "cone" else GC.SPREAD
            cases.append(_case("generic", kind, spread, item, GENERIC_STREAM0[kind] + i))
    # ---- cosine: near_zero taken, on its edge, just past it ----
    for n, j in enumerate(range(5000, 5008)):
        u, point = unit_of(orc, j), ORDINARY_ITEMS[n % 2, 0:3]
        cases.append(_case("cos_near_zero_taken", "cosine", 0.5, np.concatenate([point, -u]), j, nudged=None, k=0))
        for comp in range(3):
            for sign in (1, -1):
                k = near_zero_edge(orc, point, u, j, comp, sign)
                for kk in sorted({1, k - 1, k} - {0}):
                    axis = -u
                    axis[comp] = nudge(axis[comp], sign * kk)
                    cls = "cos_near_zero_taken" if kk < k else "cos_near_zero_not_taken"
                    cases.append(_case(cls, "cosine", 0.5, np.concatenate([point, axis]), j, nudged=comp, k=sign * kk, edge=k))
    # ---- zero draws ----
    for name, streams in edge_streams().items():
        for j in streams:
            for item in ORDINARY_ITEMS:
                cases.append(_case("cos_u_zero", "cosine", 0.5, item, j, zero=name))
                cases.append(_case("sphere_u_zero", "sphere", 0.5, item, j, zero=name))
                cases.append(_case("hemi_u_zero", "hemisphere", 0.5, item, j, zero=name))
                for spread in (0.5, 0.3, 1.0):
                    cases.append(_case("cone_u_zero", "cone", spread, item, j, zero=name))
    # ---- cone: axis + spread * v exactly zero, or tiny ----
    for n, j in enumerate(range(6000, 6006)):
        v, point = in_sphere_of(orc, j), ORDINARY_ITEMS[n % 2, 0:3]
        for spread in (0.0, 1.0, 0.5, 0.3):
            sv = _vec(orc.lib.orc_vec3_scale(0, _V(orc, v), spread))
            cases.append(_case("cone_zero_sum", "cone", spread, np.concatenate([point, -sv]), j))
            if spread == 0.0:
                cases.append(_case("cone_zero_sum", "cone", spread, np.concatenate([point, sv]), j))
                continue
            for k in (1, -1, 2, 3):
                for comps in ((0,), (1,), (2,), (0, 1, 2)):
                    axis = -sv
                    for cc in comps:
                        axis[cc] = nudge(axis[cc], k)
                    cases.append(_case("cone_tiny_sum", "cone", spread, np.concatenate([point, axis]), j))
    sub = np.array([1e-45, 1e-40, 1e-39], np.float64).astype(F)
    tiny_axes = [[LO, LO, LO], [-LO, LO, -LO], [nextf(LO, -1), LO, LO], [LO, nextf(LO, 1), -nextf(LO, -1)], [nextf(LO, -1)] * 3, [nextf(LO, 1)] * 3,
                 [sub[0], 0.0, 0.0], [0.0, -sub[0], 0.0], [sub[1], -sub[1], sub[2]], [sub[2], sub[2], sub[2]], [MIN_NORMAL, 0.0, -MIN_NORMAL],
                 [F(1e-30), F(2e-30), F(-3e-30)], [F(1e-10), F(-2e-10), F(3e-10)]]
    for n, axis in enumerate(tiny_axes):
        cases.append(_case("cone_tiny_sum", "cone", 0.0, np.concatenate([ORDINARY_ITEMS[n % 2, 0:3], np.array(axis, F)]), 6100 + n))
    # ---- hemisphere: the dot exactly zero, and subnormal ----
    for n, j in enumerate(range(7000, 7008)):
        u, point = unit_of(orc, j), ORDINARY_ITEMS[n % 2, 0:3]
        z = F(0.0)
        for perp in ([-u[1], u[0], z], [z, -u[2], u[1]], [u[2], z, -u[0]]):
            for scale in (1.0, -1.0, 0.25, -4.0):
                cases.append(_case("hemi_dot_zero", "hemisphere", 0.5, np.concatenate([point, np.array(perp, F) * F(scale)]), j))
        for e in (-130, -135, -140):
            for sign in (1.0, -1.0):
                cases.append(_case("hemi_dot_subnormal", "hemisphere", 0.5, np.concatenate([point, u * F(sign * 2.0 ** e)]), j))
        for sign in (1.0, -1.0):
            cases.append(_case("hemi_dot_subnormal", "hemisphere", 0.5, np.concatenate([point, np.array([-u[1], u[0], F(sign * 2.0 ** -130)], F)]), j))
    # ---- probes: the second normalisation changes the bits, or does not ----
    for kind in ("sphere", "hemisphere"):
        for n in range(192):
            j, item = 8000 + n, ORDINARY_ITEMS[n % 2]
            u = unit_of(orc, j)
            ray = oracle_rays(orc, kind, 0.5, item, j)[0]
            same = np.array_equal(bits(np.abs(ray[3:6])), bits(np.abs(u)))
            cases.append(_case("probe_not_renormalised" if same else "probe_renormalised", kind, 0.5, item, j))
    return cases


def nan_words_allowed(c):
    """A NaN word in the oracle's ray is legitimate only for these (the last: the zero-axis special item in the cone of spread 0, which is
    a cone_zero_sum among the generic rows)."""
    zero_cone = c["kind"] == "cone" and c["spread"] == 0 and (c["item"][3:6] == 0).all()
    return c["cls"] in NAN_CLASSES or not np.isfinite(c["item"]).all() or bool(zero_cone)


# ------------------------------------------------------------------------------------------------------------------
# the harness's files and the comparison
# ------------------------------------------------------------------------------------------------------------------
wave_lists = S.wave_lists
LIST_LENGTHS = S.LIST_LENGTHS


def case_words(c):
    w = np.zeros(CASE_WORDS, np.uint32)
    w[0] = KINDS.index(c["kind"])
    w[1] = bits(c["spread"])[0]
    w[2] = c["j"]
    w[3:9] = bits(c["item"])
    return w


def write_case_file(path, cases, order, tasks):
    words = np.stack([case_words(c) for c in cases])[order]
    with open(path, "wb") as f:
        f.write(struct.pack("<IIII", 0x31435244, len(words), len(tasks), seed_key()))
        f.write(words.tobytes())
        f.write(np.ascontiguousarray(tasks, np.uint32).tobytes())


def differing_words(got, want, nonfinite_item):
    """(words that differ, words compared by class): everything by its bits, but for the six ray words of a row whose ITEM is non-finite -
    there a word that is NaN on both sides passes (x86-64 and gfx950 propagate the payload and sign of an input NaN differently)."""
    float_words = np.zeros(got.shape, bool)
    float_words[:, 0:6] = np.asarray(nonfinite_item, bool)[:, None]
    return S.differing_words(got, want, float_words)


# ------------------------------------------------------------------------------------------------------------------
# the same edges through the public entry points (tests/test_gpu_draw_entry.py): batches of 65 items with K = 4 whose last item -
# the ragged lane after one full round of 64 - meets an edge with its sample ENTRY_SAMPLE; the other 64 are ordinary surfels
# ------------------------------------------------------------------------------------------------------------------
ENTRY_N, ENTRY_K, ENTRY_SAMPLE, ENTRY_BINS = 65, 4, 1, 3
ENTRY_SCENES = ("cornell", "grid3000")                                       # a lock-step list in LDS and 16-byte nodes from global memory
TOP_K = 8
TOP_FIRST_STREAM = (1 << 32) - ENTRY_N * TOP_K                               # 2^32 - 520: the last sample runs on stream 2^32 - 1
AT_HIT_SCENES = ("cornell", "prims33", "grid3000", "prims600")               # lock-step list, LDS tree, 16-byte nodes, register slots


def entry_items(orc, ow, desc):
    """float32 [65, 6]: every fourth of the first 260 items of gather_cases.items_of (surfels and free-space probes, all finite)."""
    items, _ = GC.items_of(orc, ow, desc)
    items = np.ascontiguousarray(items[np.arange(ENTRY_N) * 4])
    assert np.isfinite(items).all() and (items[:, 3:6] != 0).any(axis=1).all()
    return items


def entry_batches(orc):
    """name (the class of the case list it repeats) -> dict(kinds it applies to, stream j, axis of item 64 or None for the item's own,
    first_stream)."""
    es = edge_streams()
    out = {name: dict(kinds=KINDS, j=es[name][0], axis=None) for name in ("u1_zero", "u2_zero", "u3_zero")}
    u, v = unit_of(orc, 5000), in_sphere_of(orc, 6000)
    sv = _vec(orc.lib.orc_vec3_scale(0, _V(orc, v), GC.SPREAD))
    out["cos_near_zero_taken"] = dict(kinds=("cosine",), j=5000, axis=-u)
    out["cone_zero_sum"] = dict(kinds=("cone",), j=6000, axis=-sv)
    tiny = -sv
    tiny[0] = nudge(tiny[0], 1)
    out["cone_tiny_sum"] = dict(kinds=("cone",), j=6000, axis=tiny)
    u = unit_of(orc, 7000)
    out["hemi_dot_zero"] = dict(kinds=("hemisphere",), j=7000, axis=np.array([-u[1], u[0], 0.0], F))
    out["hemi_dot_subnormal"] = dict(kinds=("hemisphere",), j=7000, axis=u * F(2.0 ** -130))
    for b in out.values():
        b["first_stream"] = b["j"] - (ENTRY_N - 1) * ENTRY_K - ENTRY_SAMPLE
        assert b["first_stream"] >= 0
    return out


def entry_batch_items(items, batch):
    out = items.copy()
    if batch["axis"] is not None:
        out[ENTRY_N - 1, 3:6] = batch["axis"]
    return out


def entry_reference(orc, ow, desc, basis, items, kind, k, max_bounces, background, first_stream, spread=GC.SPREAD, bins=ENTRY_BINS):
    """The oracle's answers of every entry point that draws `kind` ("rays": none drawn, trt_radiance) for one batch: first rays [n, k, 6],
    per-sample colours, ends and depths through passes_cases.oracle_paths (cpu.rs:39-65 from the oracle's pieces on stream (seed, j, 0) for
    any j - tests/test_passes_cases.py pins it to orc.sample_batch), world.hit calls, and the folds of radiance_cases, passes_cases,
    ambient_cases (max_distance +inf) and probe_cases."""
    import ambient_cases as AC
    import passes_cases as PS
    import radiance_cases as R
    if kind == "rays":
        rays = np.ascontiguousarray(np.repeat(items[:, None, :], k, axis=1))
    elif kind in GC.LOBES:
        rays = GC.first_rays(orc, items, kind, k, spread, SEED, first_stream)
    else:
        rays = PC.first_rays(orc, items, kind, k, SEED, first_stream)[0]
    cols, ends, depths, hits = PS.oracle_paths(orc, ow, desc, rays, max_bounces, background, SEED, first_stream)
    ref = dict(rays=rays, cols=cols, ends=ends, depths=depths, n_rays=hits)
    if kind in PC.DOMAINS:
        ref["SH"] = PC.fold(basis, rays, cols, k)
    else:
        ref["S"], ref["M"] = R.fold(cols, k)
        ref["P"], ref["spent"] = PS.fold(cols, ends, depths, k, bins)
    if kind in GC.LOBES:
        ref["occ"] = AC.occlusion(ow, rays, float("inf"))
        ref["V"], ref["B"] = AC.fold(ref["occ"], rays, k)
    return ref


def at_hit_reference(orc, ow, items):
    """Ambient queries with the cone of spread 0 and K = 1, where the first ray is Ray::new(point, axis) whatever the stream: (rays
    [n, 1, 6], chosen item, its hit distance t*, and for max_distance = the float below t*, t* and the float above it: (max_distance,
    occluded bool [n, 1], V, B))."""
    import ambient_cases as AC
    rays = GC.first_rays(orc, items, "cone", 1, 0.0, SEED, 0)
    hit, t, _ = ow.hit_index_batch(rays.reshape(-1, 6), AC.T_MIN, float("inf"))
    ok = np.flatnonzero(hit & np.isfinite(t) & (t > 0.01))
    assert len(ok) >= 4
    chosen = int(ok[len(ok) // 2])
    t_star = F(t[chosen])
    calls = []
    for md in (np.nextafter(t_star, F(0.0)), t_star, np.nextafter(t_star, F(np.inf))):
        occ = AC.occlusion(ow, rays, float(md))
        calls.append((float(md), occ) + AC.fold(occ, rays, 1))
    return rays, chosen, t_star, calls
