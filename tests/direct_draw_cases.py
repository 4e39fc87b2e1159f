"""What tests/test_direct_draw_cases.py (CPU), tests/test_gpu_direct_draws.py and tests/test_gpu_direct_draw_entry.py (GPU) share, none of it
touching a GPU: the case list of the emitter draw of the direct-light and next-event queries (csrc/gather_draw.h direct_draw_from behind
direct_draw and direct_draw_at; the contract is tinyrt.h trt_direct, steps 2-7), the oracle's expectation of every case, a second float32
restatement with eighteen mutants, and the files of tests/native/direct_draw_cases.hip.

A case is (form, table t, stream j, sample word, shadow_end, surfel x, n): the draw for the surfel from RNG stream (SEED, j, word).
form: "item" (direct_draw: the surfel is loaded from an items array after the draws) or "vertex" (direct_draw_at: the surfel is held in
registers).  The expectation is 13 words - ray origin[3], ray direction[3], c[3] = colour * wgt (for dead samples too), t_max, live as
0 / 1, and the generator state s0, s1 after the three (quad) or four (sphere) draws - from the oracle's pieces exactly as
direct_cases.samples and nee_cases.draw put them together: orc_rng_seed, orc_rng_random, orc_random_unit_vector, orc_vec3_dot,
orc_ray_new, numpy float32 scalars otherwise.

A table is (E, P <= 64 records) with record e = records[e mod P]: E = 2^20 stays a few kilobytes in the case file, the harness expands it.
E in 1, 2, 3, 5, 64, 1000, 1 000 003, 2^20 - 1, 2^20; records of one table have distinct colours, positions and kinds; the table of E = 3
holds the kind words 2, 0x3F800000 and 0xFFFFFFFF (spheres, by the contract's "any kind other than 1"), the table of E = 5 a negative
area, the one of E = 64 an area of 0 (both used as given).  Three more tables serve the edges: `origin` (one quad with u = v = 0 at the
origin, so that y = +0 exactly and w = y - x = -x for ANY x, with a normal and an area of its own - a record is used as given),
`plane` (an axis-aligned quad in y = 0) and `degenerate`; the searched areas of wgt_edge are tables of one record each.

Classes (tests/README_direct_draws.md has the counts):
  generic        random surfels x consecutive streams per table and form; words 1, 2, 6; shadow_end 0.999, 0.5, 1; every 25th surfel one of
                 the four special items of gather_cases.items_of (NaN point, zero axis, inf component, axis of length 1e-9)
  pick_rounded   streams whose f32 pick uint32(u0 * float(E)) differs from floor(exact u0 * E), under E = 1 000 003, 2^20 - 1 and 1000
  pick_top       per E the stream with the largest u0 of 2^22 scanned (pick = E - 1) and a stream with u0 = 0 (pick = 0)
  u_zero         the streams of golden/draw_edge_streams.json and golden/direct_edge_streams.json (draw 1, 2, 3 or 4 exactly 0) against a
                 quad and against a sphere: u0 = 0, a = 0, b = 0; the sphere's u1, u2, u3 = 0 (the last: nl = 0/0, dead by NaN)
  cs_zero        n exactly perpendicular to w - (-w.y, w.x, 0), its rotations and power-of-two multiples - and n = +0 * sign(w): cs = +0
  cs_sign        n = +-2^e w with e = -132 .. -140 (cs subnormal of either sign) and n = -0 * sign(w) (cs = -0)
  on_the_light   x = y exactly (d2 = 0, the ray 0/0, t_max = 0); x = y nudged 1..3 floats in one or in all components; on `origin` offsets
                 of 2^-40, 2^-64, 2^-70, 2^-76 and the floats either side of 2^-39: d2 ordinary, d2 subnormal with d2 * d2 = 0 (inf or NaN
                 weight), d2 = 0 with w != 0; both sides of normalized()'s 2^-39 switch
  far            |w| about 2^40, 2^63 (d2 finite, d2 * d2 = inf: weight 0, live, finite t_max) and 2^65 (d2 = inf, t_max = inf: with a unit
                 n cs * cl is inf too and the weight inf / inf, dead by NaN; with |n| = 2^-10 the weight is 0 and the sample live)
  wgt_edge       for two fixed geometries the record's area searched float by float (bisection over its bits): the last area with a
                 finite weight and the first with inf; the first normal weight and the last subnormal one; the last area with weight 0
                 and the first with a non-zero one
  cl_zero        x in the plane of the quad: cl = 0, the weight +0, live, c = -0 where the colour is negative; nl.w subnormal of either sign
  degenerate     u = v = 0 quads, radius 0 and a negative radius, NaN / inf in a corner, a centre, a colour, an area
  tmax_edge      on `origin`, distances searched so that sqrt(d2) * shadow_end is the float below 0.001, 0.001 itself and the float above, for
                 each of the three shadow_end values
Every non-generic case is in the list in both forms with the same values.

Mutants of the restatement (restate(mut=k)); tests/test_direct_draw_cases.py prints which classes tell each from the oracle:
   1 pick by floor(exact product)      2 pick clamp omitted (EQUIVALENT)      3 live with cs >= 0          4 live with d2 >= 0 (EQUIVALENT)
   5 finiteness test omitted           6 finiteness test admits inf           7 area * (E * 1/pi)          8 ((cs * cl) / d2) / d2
   9 corner + (u * a + v * b)         10 y with one fused multiply-add       11 a quad takes four draws, a sphere three
  12 kind != 0 read as a quad         13 normal recomputed from cross(u, v)  14 |.| on cl omitted         15 a and b swapped
  16 subnormal cs flushed to zero     17 t_max as sqrt(d2 * shadow_end^2)    18 sample word off by one
Mutant 2: u0 <= 1 - 2^-23, and f32((1 - 2^-23) * E) < E for every E in 1 .. 2^20 (asserted for all of them on the CPU); rounding is
monotone, so u0 * float(E) < E for every draw and the clamp never acts.  Mutant 4: d2 is a sum of squares, so d2 >= 0 or NaN; with
d2 = 0, d2 * d2 = 0 and (cs * cl) / 0 is +-inf or NaN, whose product with the scale is +-inf or NaN: the weight is not finite and the
sample is dead by the third rule whatever the second says.
"""
import ctypes as C
import importlib.util
import json
import os
import struct

import numpy as np

import direct_cases as DC
import draw_cases as DR
import shade_cases as S

F = np.float32
SEED = DR.SEED
MASK = S.MASK
FORMS = ("item", "vertex")
WORDS = (1, 2, 6)
SHADOW_ENDS = (F(0.999), F(0.5), F(1.0))
T_MIN = F(0.001)
INV_PI = DC.INV_PI
MIN_NORMAL = DR.MIN_NORMAL
LO = S.LO
CASE_WORDS, OUT_WORDS, RECORD_WORDS = 11, 13, 20
MAX_PERIOD = 64
MAIN_E = (1, 2, 3, 5, 64, 1000, 1000003, (1 << 20) - 1, 1 << 20)
ROUNDED_E = (1000003, (1 << 20) - 1, 1000)
GENERIC_PER_CELL = 120
SCAN = 1 << 22
N_MUTANTS = 18
MUTANT_NAMES = {1: "pick by floor(exact product)", 2: "pick clamp omitted", 3: "live with cs >= 0", 4: "live with d2 >= 0", 5: "finiteness test omitted",
                6: "finiteness test admits inf", 7: "area * (E * 1/pi)", 8: "((cs * cl) / d2) / d2", 9: "corner + (u * a + v * b)",
                10: "y with one fused multiply-add", 11: "a quad takes four draws, a sphere three", 12: "kind != 0 read as a quad",
                13: "normal recomputed from cross(u, v)", 14: "|.| on cl omitted", 15: "a and b swapped", 16: "subnormal cs flushed to zero",
                17: "t_max as sqrt(d2 * shadow_end^2)", 18: "sample word off by one"}
EQUIVALENT_MUTANTS = (2, 4)
# classes whose rows may hold NaN words although surfel and record are finite: 0/0 of a zero draw, of w = 0, of a zero normal
NAN_CLASSES = {"u_zero", "on_the_light", "far", "degenerate", "wgt_edge"}
ORDINARY_SURFELS = np.array([[0.5, -1.25, 2.0, 0.36, 0.48, -0.8], [-3.0, 0.125, 0.75, -1.5, 2.0, 2.5]], F)
HERE = os.path.dirname(os.path.abspath(__file__))

bits, nextf = S.bits, S.nextf


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_GEN = _load("make_draw_edge_streams")


def edge_streams():
    """u1_zero .. u3_zero of golden/draw_edge_streams.json and u4_zero of golden/direct_edge_streams.json: streams (SEED, j, 1)."""
    out = DR.edge_streams()
    with open(os.path.join(HERE, "golden", "direct_edge_streams.json")) as f:
        doc = json.load(f)
    assert doc["seed"] == SEED and doc["sample"] == 1
    out["u4_zero"] = [int(j) for j in doc["u4_zero"]]
    return out


def first_draw_k(j, word):
    """uint64 array: k with u0 = k / 2^23, the first draw of streams (SEED, j, word) - the vectorised trt-rng v1 of the golden scan."""
    with np.errstate(over="ignore"):
        s0, s1 = _GEN.rng_seed(SEED, np.asarray(j, np.uint32), word)
        r, _, _ = _GEN.rng_next(s0, s1)
    return (r >> np.uint32(9)).astype(np.uint64)


def picks_of(k, E):
    """(the contract's pick uint32(u0 * float(E)) in float32, floor of the exact product) for draws u0 = k / 2^23."""
    u0 = k.astype(np.float64).astype(F) / F(1 << 23)
    return (u0 * F(E)).astype(np.int64), ((k * np.uint64(E)) >> np.uint64(23)).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------
# tables
# ------------------------------------------------------------------------------------------------------------------
def _mixed(orc, g, P, first_quad=True):
    recs = []
    for i in range(P):
        color = g.uniform(0.5, 10.0, 3)
        if (i % 2 == 0) == first_quad:
            recs.append(DC.quad_record(orc, g.uniform(-4, 4, 3), g.uniform(-2, 2, 3), g.uniform(-2, 2, 3), color))
        else:
            recs.append(DC.sphere_record(g.uniform(-4, 4, 3), g.uniform(0.2, 1.5), color))
    return np.concatenate(recs)


def _given_quad(corner, u, v, normal, color, area):
    """A quad record whose normal and area are the caller's own: a record is used as given."""
    e = np.zeros(1, DC.EMITTER_DTYPE)
    e["kind"], e["geometry"], e["a"], e["b"], e["c"], e["normal"], e["color"], e["area"] = 1, DC.NO_GEOMETRY, corner, u, v, normal, color, area
    return e


def wgt_table(area):
    return dict(name="wgt", E=1, records=_given_quad((1.0, 2.0, 3.0), (0, 0, 0), (0, 0, 0), (0.0, 0.6, 0.8), (1.5, 0.25, 3.0), area))


def tables(orc):
    """The fixed tables, in order: one per E of MAIN_E (named "E<E>"), "E2s" (E2 with its records swapped), "origin", "plane", "degenerate"."""
    g = np.random.default_rng([SEED, 11])
    out = []
    for E in MAIN_E:
        P = {1: 1, 2: 2, 3: 3, 5: 5, 64: 64, 1000: 37, 1000003: 61}.get(E, 64)
        recs = _mixed(orc, g, P)
        if E == 3:                                                          # kind words the contract reads as spheres; every field of a quad filled in
            recs = np.concatenate([DC.sphere_record(g.uniform(-4, 4, 3), g.uniform(0.2, 1.5), g.uniform(0.5, 10.0, 3)) for _ in range(3)])
            recs["kind"] = (2, 0x3F800000, 0xFFFFFFFF)
            recs["b"][:, 1:3] = g.uniform(-2, 2, (3, 2)).astype(F)
            recs["c"], recs["normal"] = g.uniform(-2, 2, (3, 3)).astype(F), g.uniform(-1, 1, (3, 3)).astype(F)
        if E == 5:
            recs["area"][1] = -recs["area"][1]
        if E == 64:
            recs["area"][2] = 0.0
        out.append(dict(name="E%d" % E, E=E, records=recs))
    e2 = out[1]["records"]
    out.append(dict(name="E2s", E=2, records=np.ascontiguousarray(e2[::-1])))
    out.append(dict(name="origin", E=1, records=_given_quad((0, 0, 0), (0, 0, 0), (0, 0, 0), (0.6, 0.0, 0.8), (2.0, -3.0, 0.5), 1.0)))
    out.append(dict(name="plane", E=1, records=_given_quad((-1.0, 0.0, -1.0), (2.0, 0, 0), (0, 0, 2.0), (0.0, 1.0, 0.0), (-1.0, 2.0, -0.5), 4.0)))
    deg = [DC.quad_record(orc, (1.0, 2.0, -1.0), (0, 0, 0), (0, 0, 0), (3.0, 1.0, 2.0)),              # normal 0/0, area 0
           _given_quad((-2.0, 1.0, 0.5), (0, 0, 0), (0, 0, 0), (0.0, 1.0, 0.0), (1.0, 5.0, 2.5), 1.0),
           DC.sphere_record((0.5, -1.0, 2.0), 0.0, (6.0, 1.0, 1.0)),
           DC.sphere_record((2.0, 2.0, -2.0), -1.5, (1.0, 7.0, 1.0)),
           DC.quad_record(orc, (np.nan, 0.0, 1.0), (1.0, 0, 0), (0, 0, 1.0), (2.0, 2.0, 8.0)),
           DC.sphere_record((1.0, np.inf, 0.0), 0.5, (3.0, 3.0, 1.0)),
           DC.quad_record(orc, (0.0, 3.0, 0.0), (1.0, 0, 0), (0, 0, 1.0), (np.inf, 1.0, 2.0)),
           DC.sphere_record((-1.0, -1.0, -1.0), 0.5, (1.0, np.nan, 4.0)),
           DC.quad_record(orc, (3.0, 0.0, -3.0), (1.0, 0, 0.5), (0, 1.0, 1.0), (5.0, 4.0, 3.0)),
           DC.sphere_record((-3.0, 1.0, 3.0), 0.75, (4.0, 5.0, 6.0))]
    deg[8]["area"], deg[9]["area"] = np.nan, np.inf
    out.append(dict(name="degenerate", E=len(deg), records=np.concatenate(deg)))
    for t in out:
        assert 1 <= len(t["records"]) <= MAX_PERIOD and 1 <= t["E"] <= (1 << 20) and (len(t["records"]) <= t["E"])
    return out


def table_index(tabs, name):
    return [t["name"] for t in tabs].index(name)


def record_of(table, e):
    return table["records"][e % len(table["records"])]


def expand(table):
    """The table as the entry points take it: E records."""
    return np.ascontiguousarray(table["records"][np.arange(table["E"]) % len(table["records"])])


# ------------------------------------------------------------------------------------------------------------------
# the oracle's pieces
# ------------------------------------------------------------------------------------------------------------------
def _V(orc, a):
    return orc.Vec3(float(a[0]), float(a[1]), float(a[2]))


def _arr(v):
    return np.array([v.x, v.y, v.z], F)


def stream_state(orc, j, word):
    rng = (C.c_uint32 * 2)()
    orc.lib.orc_rng_seed(SEED, j & MASK, word, C.byref(rng))
    return rng


def stream_draws(orc, j, word=1, n=4):
    rng = stream_state(orc, j, word)
    return [F(orc.lib.orc_rng_random(C.byref(rng))) for _ in range(n)]


def states_after(orc, j, word, n):
    """The generator state after each of the first n outputs."""
    rng = stream_state(orc, j, word)
    out = []
    for _ in range(n):
        orc.lib.orc_rng_next_u32(C.byref(rng))
        out.append((int(rng[0]), int(rng[1])))
    return out


def expect(orc, table, j, word, shadow_end, x, n, tr=None):
    """uint32 [13]: steps 2-7 of tinyrt.h trt_direct for the surfel (x, n) on stream (SEED, j, word), in the arithmetic of
    direct_cases.samples / nee_cases.draw, operator by operator.  tr: dict that receives intermediate values."""
    tr = {} if tr is None else tr
    lib = orc.lib
    E = table["E"]
    fE = F(E)
    x, n = np.asarray(x, F), np.asarray(n, F)
    rng = stream_state(orc, j, word)
    with np.errstate(all="ignore"):
        u0 = F(lib.orc_rng_random(C.byref(rng)))
        e = min(int(u0 * fE), E - 1)
        rec = record_of(table, e)
        quad = rec["kind"] == 1
        if quad:
            a = F(lib.orc_rng_random(C.byref(rng)))
            b = F(lib.orc_rng_random(C.byref(rng)))
            y = (rec["a"] + rec["b"] * a) + rec["c"] * b
            nl = rec["normal"]
        else:
            nl = _arr(lib.orc_random_unit_vector(C.byref(rng)))
            y = rec["a"] + nl * rec["b"][0]
        assert y.dtype == F
        w = y - x
        wv = _V(orc, w)
        d2 = F(lib.orc_vec3_dot(wv, wv))
        cs = F(lib.orc_vec3_dot(_V(orc, n), wv))
        cl = np.abs(F(lib.orc_vec3_dot(_V(orc, nl), wv)))
        scale = (rec["area"] * fE) * INV_PI
        wgt = ((cs * cl) / (d2 * d2)) * scale
        assert wgt.dtype == F
        live = bool(cs > 0 and d2 > 0 and np.isfinite(wgt))
        ray = lib.orc_ray_new(_V(orc, x), wv)
        t_max = np.sqrt(d2) * F(shadow_end)
        c = (rec["color"] * wgt).astype(F)
    rec_finite = all(np.isfinite(rec[f]).all() for f in ("a", "b", "c", "normal", "color", "area"))
    tr.update(u0=u0, pick=e, quad=bool(quad), y=y, nl=np.array(nl, F), w=w, d2=d2, cs=cs, cl=cl, wgt=wgt, live=live, t_max=t_max, rec_finite=rec_finite)
    return np.concatenate([np.frombuffer(bytes(ray), np.uint32), bits(c), bits(t_max).reshape(1), np.array([int(live), rng[0], rng[1]], np.uint32)])


def expect_case(orc, tabs, c, tr=None):
    return expect(orc, tabs[c["t"]], c["j"], c["word"], c["shadow_end"], c["x"], c["n"], tr)


def expectations(orc, tabs, cases):
    """(uint32 [n, 13], bool [n]: the row's surfel or picked record is non-finite)."""
    out = np.zeros((len(cases), OUT_WORDS), np.uint32)
    nonfinite = np.zeros(len(cases), bool)
    for i, c in enumerate(cases):
        tr = {}
        out[i] = expect_case(orc, tabs, c, tr)
        nonfinite[i] = not (tr["rec_finite"] and np.isfinite(c["x"]).all() and np.isfinite(c["n"]).all())
    return out, nonfinite


# ------------------------------------------------------------------------------------------------------------------
# the second restatement: numpy float32 scalars with shade_cases' own dot and a plain a / sqrt(a.a), over orc_random_in_unit_sphere
# ------------------------------------------------------------------------------------------------------------------
def normalized(a):
    return a / np.sqrt(S.dot(a, a))


def restate(orc, table, j, word, shadow_end, x, n, mut=0, tr=None):
    """uint32 [13] as `expect`."""
    tr = {} if tr is None else tr
    lib = orc.lib
    E = table["E"]
    fE = F(E)
    x, n, se = np.asarray(x, F), np.asarray(n, F), F(shadow_end)
    word = word + 1 if mut == 18 else word
    rng = stream_state(orc, j, word)
    with np.errstate(all="ignore"):
        u0 = F(lib.orc_rng_random(C.byref(rng)))
        if mut == 1:
            pick = (int(round(float(u0) * (1 << 23))) * E) >> 23
        else:
            pick = int(u0 * fE)
        if mut != 2:
            pick = min(pick, E - 1)
        assert 0 <= pick < E                                                 # (mutant 2 never leaves the table: see the module's text)
        rec = record_of(table, pick)
        corner, eu, ev = rec["a"], rec["b"], rec["c"]
        quad = bool(rec["kind"] != 0) if mut == 12 else bool(rec["kind"] == 1)
        if quad:
            a = F(lib.orc_rng_random(C.byref(rng)))
            b = F(lib.orc_rng_random(C.byref(rng)))
            if mut == 15:
                a, b = b, a
            if mut == 9:
                y = corner + (eu * a + ev * b)
            elif mut == 10:
                first = corner + eu * a
                y = np.array([S._fma(ev[k], b, first[k]) for k in range(3)], F)
            else:
                y = (corner + eu * a) + ev * b
            nl = normalized(S.cross(eu, ev)) if mut == 13 else rec["normal"]
            if mut == 11:
                lib.orc_rng_next_u32(C.byref(rng))
        else:
            nl = normalized(_arr(lib.orc_random_in_unit_sphere(C.byref(rng))))
            y = corner + nl * eu[0]
            if mut == 11:
                rng[0], rng[1] = states_after(orc, j, word, 3)[2]
        w = y - x
        d2 = S.dot(w, w)
        cs = S.dot(n, w)
        if mut == 16 and np.abs(cs) < MIN_NORMAL:
            cs = F(0.0)
        cl = S.dot(nl, w)
        if mut != 14:
            cl = np.abs(cl)
        scale = rec["area"] * (fE * INV_PI) if mut == 7 else (rec["area"] * fE) * INV_PI
        wgt = (((cs * cl) / d2) / d2 if mut == 8 else (cs * cl) / (d2 * d2)) * scale
        facing = bool(cs >= 0) if mut == 3 else bool(cs > 0)
        apart = bool(d2 >= 0) if mut == 4 else bool(d2 > 0)
        finite = True if mut == 5 else (not np.isnan(wgt)) if mut == 6 else bool(np.isfinite(wgt))
        live = facing and apart and finite
        d = normalized(w)
        t_max = np.sqrt(d2 * (se * se)) if mut == 17 else np.sqrt(d2) * se
        c = (rec["color"] * wgt).astype(F)
    tr.update(u0=u0, pick=pick, quad=quad, y=y, nl=np.array(nl, F), w=w, d2=d2, cs=cs, cl=cl, wgt=wgt, live=live, t_max=t_max)
    return np.concatenate([bits(x), bits(d), bits(c), bits(t_max).reshape(1), np.array([int(live), rng[0], rng[1]], np.uint32)])


def restate_case(orc, tabs, c, mut=0, tr=None):
    return restate(orc, tabs[c["t"]], c["j"], c["word"], c["shadow_end"], c["x"], c["n"], mut, tr)


# ------------------------------------------------------------------------------------------------------------------
# the case list
# ------------------------------------------------------------------------------------------------------------------
def _special_surfels():
    return np.array([[np.nan, 1.0, 2.0, 0.0, 0.0, 1.0], [1.0, 2.0, 3.0, 0.0, 0.0, 0.0], [1.0, 2.0, 3.0, np.inf, 0.0, 1.0], [1.0, 2.0, 3.0, 0.0, 1e-9, 0.0]], F)


def bisect_bits(pred, lo=1, hi=0x7F7FFFFF):
    """pred over positive floats by their bits, monotone (False .. False True .. True): (last False, first True) as floats, or None
    where pred does not change in [lo, hi]."""
    as_f = lambda b: np.array([b], np.uint32).view(F)[0]
    if pred(as_f(lo)) or not pred(as_f(hi)):
        return None
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if pred(as_f(mid)) else (mid, hi)
    return as_f(lo), as_f(hi)


def tmax_edge_distances(se):
    """{-1, 0, 1} -> (w float32 [3]) with sqrt(w.w) * se the float below 0.001, 0.001 itself, the float above: a search over the floats t
    about 0.001 / se in w = (t, 0, 0) and, where that reaches no such value, (t, t / 2, 0) and (t, t, t / 4)."""
    se = F(se)
    want = {-1: nextf(T_MIN, -1), 0: T_MIN, 1: nextf(T_MIN, 1)}
    found = {}
    for shape in ((1.0, 0.0, 0.0), (1.0, 0.5, 0.0), (1.0, 1.0, 0.25)):
        length = float(np.sqrt(sum(s * s for s in shape)))
        t0 = int(bits(F(float(T_MIN) / float(se) / length))[0])
        t = (t0 + np.arange(-4000, 4001)).astype(np.uint32).view(F)
        w = np.stack([t * F(s) for s in shape], axis=1)
        with np.errstate(all="ignore"):
            d2 = (w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2]
            tm = np.sqrt(d2) * se
        for k, v in want.items():
            hit = np.flatnonzero(tm == v)
            if k not in found and len(hit):
                found[k] = w[hit[len(hit) // 2]].copy()
        if len(found) == 3:
            break
    assert len(found) == 3, (se, found)
    return found


class Maker:
    def __init__(self, orc):
        self.orc = orc
        self.tabs = tables(orc)
        self.cases = []
        self.g = np.random.default_rng([SEED, 12])

    def table(self, name):
        return table_index(self.tabs, name)

    def add(self, cls, t, j, x, n, word=1, se=SHADOW_ENDS[0], forms=FORMS, **kw):
        assert 0 <= j < (1 << 32) and 0 <= t < len(self.tabs)
        for form in forms:
            self.cases.append(dict(cls=cls, form=form, t=int(t), j=int(j), word=int(word), shadow_end=F(se), x=np.array(x, F), n=np.array(n, F), **kw))

    def trace(self, t, j, word=1, x=(0, 0, 0), n=(0, 0, 0), se=SHADOW_ENDS[0]):
        tr = {}
        expect(self.orc, self.tabs[t], j, word, se, x, n, tr)
        return tr

    def aim(self, y):
        """A surfel one to five units from y that faces it."""
        g = self.g
        d = g.normal(size=3)
        d /= np.linalg.norm(d)
        x = (np.asarray(y, np.float64) - d * g.uniform(1.0, 5.0)).astype(F)
        n = d + 0.3 * g.normal(size=3)
        return x, (n / np.linalg.norm(n)).astype(F)

    def aimed(self, cls, t, j, word=1, se=SHADOW_ENDS[0], **kw):
        x, n = self.aim(self.trace(t, j, word)["y"])
        self.add(cls, t, j, x, n, word, se, **kw)

    def stream_with_pick(self, t, pick, start, word=1):
        j = np.arange(start, start + 4096, dtype=np.uint64)
        got, _ = picks_of(first_draw_k(j, word), self.tabs[t]["E"])
        return int(j[np.flatnonzero(got == pick)[0]])

    # ---- classes ----
    def generic(self):
        g = self.g
        special = _special_surfels()
        names = ["E%d" % E for E in MAIN_E] + ["E2s", "degenerate"]
        for ti, name in enumerate(names):
            t = self.table(name)
            for fi, form in enumerate(FORMS):
                j0 = 100000 + 10000 * ti + 5000 * fi
                for i in range(GENERIC_PER_CELL):
                    x = g.uniform(-6.0, 6.0, 3).astype(F)
                    n = g.normal(size=3)
                    n = (n / np.linalg.norm(n)).astype(F) * F(DR.GC.AXIS_SCALES[i % 3])
                    if i % 25 == 12:
                        x, n = special[(i // 25) % 4, 0:3], special[(i // 25) % 4, 3:6]
                    self.add("generic", t, j0 + i, x, n, WORDS[i % 3], SHADOW_ENDS[(i // 3) % 3], forms=(form,))

    def picks(self):
        j = np.arange(SCAN, dtype=np.uint64)
        k = first_draw_k(j, 1)
        for E in ROUNDED_E:
            t = self.table("E%d" % E)
            got, exact = picks_of(k, E)
            rows = np.flatnonzero(got != exact)[:24]
            for r in rows:
                self.aimed("pick_rounded", t, int(j[r]), exact=int(exact[r]))
        zero = edge_streams()["u1_zero"][0]
        top = int(np.argmax(k))
        for E in MAIN_E:
            t = self.table("E%d" % E)
            self.aimed("pick_top", t, top, want=E - 1)
            self.aimed("pick_top", t, zero, want=0)

    def u_zero(self):
        for name, streams in edge_streams().items():
            for j in streams[:4]:
                for tn in ("E2", "E2s"):
                    for s in ORDINARY_SURFELS:
                        self.add("u_zero", self.table(tn), j, s[0:3], s[3:6], zero=name)

    def cosines(self):
        t = self.table("E1000")
        z = F(0.0)
        for j in range(9000, 9012):
            tr = self.trace(t, j)
            x, _ = self.aim(tr["y"])
            with np.errstate(all="ignore"):
                w = tr["y"] - x
            assert (w != 0).all()
            for perp in ([-w[1], w[0], z], [z, -w[2], w[1]], [w[2], z, -w[0]]):
                for scale in (1.0, -1.0, 0.25, -4.0):
                    self.add("cs_zero", t, j, x, np.array(perp, F) * F(scale))
            self.add("cs_zero", t, j, x, np.copysign(F(0.0), w))
            self.add("cs_sign", t, j, x, np.copysign(F(0.0), -w), negative_zero=True)
            for e in (-132, -136, -140):
                for sign in (1.0, -1.0):
                    self.add("cs_sign", t, j, x, w * F(sign * 2.0 ** e))

    def on_the_light(self):
        t = self.table("E1000")
        for j in range(9100, 9108):
            y = self.trace(t, j)["y"]
            n = self.aim(y)[1]
            self.add("on_the_light", t, j, y, n, exact=True)
            for k in (1, -1, 2, 3):
                for comps in ((0,), (1,), (2,), (0, 1, 2)):
                    x = y.copy()
                    for cc in comps:
                        x[cc] = DR.nudge(x[cc], k)
                    self.add("on_the_light", t, j, x, n)
        t = self.table("origin")
        offsets = [F(2.0 ** -40), F(2.0 ** -64), F(2.0 ** -70), F(2.0 ** -76), LO, nextf(LO, -1), nextf(LO, 1)]
        for k, off in enumerate(offsets):
            for shape in ((1.0, 0.0, 0.0), (1.0, 1.0, 1.0), (1.0, 0.0, 2.0)):
                for n in ((1.0, 0.0, 0.0), (0.6, 0.0, 0.8)):
                    self.add("on_the_light", t, 9200 + k, -(np.array(shape, F) * off), n, offset=float(off))
        self.add("on_the_light", t, 9210, (0.0, 0.0, 0.0), (0.6, 0.0, 0.8), exact=True)

    def far(self):
        t = self.table("origin")
        for k, e in enumerate((40, 63, 65)):
            for shape in ((1.0, 0.0, 0.0), (0.6, 0.0, 0.8), (1.0, 1.0, 1.0), (-1.0, 0.5, 1.0)):
                for se in SHADOW_ENDS:
                    for short in (1.0, 2.0 ** -10):                          # |n| = 2^-10 keeps cs * cl finite at |w| = 2^65
                        self.add("far", t, 9300 + k, -(np.array(shape, F) * F(2.0 ** e)), np.array([0.6, 0.0, 0.8], F) * F(short), se=se, log2=e)

    def wgt_edge(self):
        geometries = (((1.0, 2.0, 3.0) - 1e-3 * np.array([0.3, 0.5, 0.8]), (0.0, 0.0, 1.0)), ((-29.0, -38.0, -47.0), (0.0, 0.0, 1.0)))
        preds = (("inf", lambda w: bool(np.isinf(w))), ("normal", lambda w: bool(w >= MIN_NORMAL)), ("nonzero", lambda w: bool(w > 0)))
        for gi, (x, n) in enumerate(geometries):
            x = np.asarray(x, np.float64).astype(F)
            j = 9400 + gi

            def wgt_of(area):
                tr = {}
                expect(self.orc, wgt_table(area), j, 1, SHADOW_ENDS[0], x, n, tr)
                return tr["wgt"]
            for name, pred in preds:
                edge = bisect_bits(lambda area: pred(wgt_of(area)))
                if edge is None:
                    continue
                for side, area in zip(("below", "above"), edge):
                    self.tabs.append(wgt_table(area))
                    self.add("wgt_edge", len(self.tabs) - 1, j, x, n, edge=name, side=side)

    def cl_zero(self):
        t = self.table("plane")
        subs = [F(0.0), F(2.0 ** -135), F(-2.0 ** -135), F(2.0 ** -140), F(-2.0 ** -140), F(2.0 ** -149), F(-2.0 ** -149)]
        for j in range(9500, 9506):
            y = self.trace(t, j)["y"]
            assert y[1] == 0
            for s in subs:
                x = np.array([y[0] - F(0.3), s, y[2] - F(0.4)], F)
                self.add("cl_zero", t, j, x, (0.6, 0.0, 0.8), height=float(s))

    def degenerate(self):
        t = self.table("degenerate")
        for r in range(self.tabs[t]["E"]):
            for k in range(2):
                j = self.stream_with_pick(t, r, 20000 + 5000 * k)
                s = ORDINARY_SURFELS[k]
                self.add("degenerate", t, j, s[0:3], s[3:6], record=r)

    def tmax_edge(self):
        t = self.table("origin")
        for si, se in enumerate(SHADOW_ENDS):
            for side, w in tmax_edge_distances(se).items():
                self.add("tmax_edge", t, 9600 + si, -w, (0.6, 0.0, 0.8), se=se, side=side)

    def all(self):
        self.generic()
        self.picks()
        self.u_zero()
        self.cosines()
        self.on_the_light()
        self.far()
        self.wgt_edge()
        self.cl_zero()
        self.degenerate()
        self.tmax_edge()
        return self.cases, self.tabs


def case_list(orc):
    """(cases, tables): the fixed tables of tables() followed by the one-record tables of wgt_edge."""
    return Maker(orc).all()


def nan_words_allowed(c, nonfinite):
    return bool(nonfinite) or c["cls"] in NAN_CLASSES


# ------------------------------------------------------------------------------------------------------------------
# the harness's files and the comparison
# ------------------------------------------------------------------------------------------------------------------
wave_lists = S.wave_lists
LIST_LENGTHS = S.LIST_LENGTHS
seed_key = DR.seed_key


def case_words(c):
    w = np.zeros(CASE_WORDS, np.uint32)
    w[0], w[1], w[2], w[3] = FORMS.index(c["form"]), c["t"], c["j"], c["word"]
    w[4] = bits(c["shadow_end"])[0]
    w[5:8], w[8:11] = bits(c["x"]), bits(c["n"])
    return w


def write_case_file(path, cases, tabs, order, tasks):
    words = np.stack([case_words(c) for c in cases])[order]
    with open(path, "wb") as f:
        f.write(struct.pack("<IIIII", 0x31434444, len(words), len(tasks), len(tabs), seed_key()))
        f.write(words.tobytes())
        f.write(np.ascontiguousarray(tasks, np.uint32).tobytes())
        for t in tabs:
            recs = np.ascontiguousarray(t["records"])
            f.write(struct.pack("<II", t["E"], len(recs)))
            f.write(recs.tobytes())


def differing_words(got, want, nonfinite):
    """(words that differ, words compared by class).  Live rows: all 13 words by their bits.  Dead rows, and rows whose surfel or record
    is non-finite: the live flag and the state by their bits, the ten float words by their bits except that a word that is NaN on both
    sides passes (x86-64 and gfx950 propagate the payload and sign of a NaN differently) - shade_cases.differing_words' rule."""
    want = np.asarray(want, np.uint32)
    float_words = np.zeros(want.shape, bool)
    float_words[:, 0:10] = ((want[:, 10] == 0) | np.asarray(nonfinite, bool))[:, None]
    return S.differing_words(got, want, float_words)


# ------------------------------------------------------------------------------------------------------------------
# the same edges through the public entry points (tests/test_gpu_direct_draw_entry.py): batches of 65 items with K = 4 whose last item -
# the ragged lane after one full round of 64 - meets the edge with its sample ENTRY_SAMPLE; the other 64 are ordinary surfels
# ------------------------------------------------------------------------------------------------------------------
ENTRY_N, ENTRY_K, ENTRY_SAMPLE = DR.ENTRY_N, DR.ENTRY_K, DR.ENTRY_SAMPLE
ENTRY_SCENES = DR.ENTRY_SCENES                                               # a lock-step list in LDS and 16-byte nodes from global memory
NEE_BOUNCES = 3
TMAX_SIDES = ("tmax_below", "tmax_at", "tmax_above")


class Periodic:
    """A table of E records as direct_cases.samples and nee_cases.draw read one: len() and [e]."""

    def __init__(self, table):
        self.table = table

    def __len__(self):
        return self.table["E"]

    def __getitem__(self, e):
        return record_of(self.table, e)


def entry_first_stream(j):
    fs = j - (ENTRY_N - 1) * ENTRY_K - ENTRY_SAMPLE
    assert fs >= 0
    return fs


def direct_entry_batches(orc):
    """name -> dict(table, j: the stream of item 64's sample 1, first_stream, shadow_end, surfel float32 [6] of item 64, device_only).
    Every batch but the three tmax ones IS a case of the list (sample word 1, the word of trt_direct).  tmax_*: the table is `origin`'s
    record followed by direct_cases' virtual quad, the stream one whose draw picks the first while the three other samples of item 64
    pick the second - so exactly one sample of the batch has its t_max on the edge."""
    cases, tabs = case_list(orc)

    def first(pred):
        for c in cases:
            if c["form"] == "item" and c["word"] == 1 and c["j"] >= ENTRY_N * ENTRY_K and pred(c):
                return c
        raise AssertionError("no such case")

    def sphere_picked(c):
        tr = {}
        expect_case(orc, tabs, c, tr)
        return not tr["quad"]

    chosen = dict(cs_zero=first(lambda c: c["cls"] == "cs_zero"),
                  on_the_light=first(lambda c: c["cls"] == "on_the_light" and c.get("exact") and tabs[c["t"]]["E"] > 1),
                  wgt_max=first(lambda c: c["cls"] == "wgt_edge" and c["edge"] == "inf" and c["side"] == "below"),
                  wgt_inf=first(lambda c: c["cls"] == "wgt_edge" and c["edge"] == "inf" and c["side"] == "above"),
                  cl_zero=first(lambda c: c["cls"] == "cl_zero" and c["height"] == 0),
                  u4_zero=first(lambda c: c["cls"] == "u_zero" and c["zero"] == "u4_zero" and sphere_picked(c)),
                  pick_rounded=first(lambda c: c["cls"] == "pick_rounded" and tabs[c["t"]]["E"] == 1000003))
    out = {}
    for name, c in chosen.items():
        out[name] = dict(table=tabs[c["t"]], j=c["j"], shadow_end=c["shadow_end"], surfel=np.concatenate([c["x"], c["n"]]), device_only=name == "pick_rounded")
    two = dict(name="origin2", E=2, records=np.concatenate([tabs[table_index(tabs, "origin")]["records"], DC.quad_record(orc, **DC.VIRTUAL_QUAD)]))
    j = np.arange(30000, 40000, dtype=np.uint64)
    p, _ = picks_of(first_draw_k(j, 1), 2)
    at = np.flatnonzero((p[1:-2] == 0) & (p[:-3] == 1) & (p[2:-1] == 1) & (p[3:] == 1))[0] + 1
    se = SHADOW_ENDS[0]
    for side, w in tmax_edge_distances(se).items():
        # x = +w, so y - x = -w: the same d2; the surfel lies in the positive octant and faces the origin
        out[TMAX_SIDES[side + 1]] = dict(table=two, j=int(j[at]), shadow_end=se, surfel=np.concatenate([w, -np.array([0.6, 0.0, 0.8], F)]).astype(F), device_only=False)
    for b in out.values():
        b["first_stream"] = entry_first_stream(b["j"])
    return out


def direct_entry_items(items, batch):
    out = np.array(items, F)
    out[ENTRY_N - 1] = batch["surfel"]
    return out


def direct_entry_reference(orc, ow, items, batch):
    """direct_cases.reference of the batch (items: direct_entry_items' answer)."""
    return DC.reference(orc, ow, items, Periodic(batch["table"]), k=ENTRY_K, seed=SEED, first_stream=batch["first_stream"], shadow_end=batch["shadow_end"])


def first_lambertian_vertex(orc, ow, desc, ray6, max_bounces, stream):
    """The first vertex of the path of (SEED, stream, 0) at which tinyrt.h trt_nee step 5 draws: (x = the new ray's origin, n = the
    hit record's normal, d = scatters made before), or None.  passes_cases.oracle_path's loop, stopped there."""
    import passes_cases as P
    mats = P.material_table(orc, ow, desc)
    rng = stream_state(orc, stream, 0)
    ray = orc.Ray(_V(orc, ray6[0:3]), _V(orc, ray6[3:6]))
    new_ray, attenuation = orc.Ray(), orc.Vec3()
    remain = max_bounces
    while remain > 0:
        rec, _ = ow.hit(ray, 0.001, float("inf"))
        if rec is None:
            return None
        kind, albedo, param = mats[rec.material]
        if not orc.lib.orc_material_scatter(kind, albedo, param, C.byref(ray), C.byref(rec), C.byref(rng), C.byref(new_ray), C.byref(attenuation)):
            return None
        d = max_bounces - remain
        ray = orc.Ray(new_ray.origin, new_ray.direction)
        remain -= 1
        if kind == 0 and remain > 0:
            return _arr(ray.origin), _arr(rec.normal), d
    return None


def nee_entry_setup(orc, ow, desc, items):
    """The batch of the next-event tests on a scene: the first first_stream from 50000 on for which sample 1 of item 64 (the cosine
    source's first ray, gather_cases.first_rays) meets a Lambertian surface first, that vertex, and E = 1 tables built around it:
      light_on_vertex   a u = v = 0 quad whose corner is x: w = 0, dead, no walk
      sphere_on_vertex  a sphere of radius 0 at x
      tmax_below, tmax_at (where a float gives it), tmax_above
                        a u = v = 0 quad whose corner is x moved along the normal's largest component, searched float by float about
                        0.001 / shadow_end so that t_max is the nearest value below 0.001, 0.001 itself, and the nearest above."""
    import gather_cases as GC
    se = SHADOW_ENDS[0]
    for fs in range(50000, 50200):
        j = fs + (ENTRY_N - 1) * ENTRY_K + ENTRY_SAMPLE
        ray = GC.first_rays(orc, items, "cosine", ENTRY_K, GC.SPREAD, SEED, fs, only=[ENTRY_N - 1])[ENTRY_N - 1, ENTRY_SAMPLE]
        v = first_lambertian_vertex(orc, ow, desc, ray, NEE_BOUNCES, j)
        if v is not None and v[2] == 0:
            break
    else:
        raise AssertionError("no Lambertian first hit")
    x, n, d = v
    color = (3.0, 2.0, 4.0)
    zero = (0.0, 0.0, 0.0)
    tables = dict(light_on_vertex=_given_quad(x, zero, zero, n, color, 1.0), sphere_on_vertex=DC.sphere_record(x, 0.0, color))
    axis = int(np.argmax(np.abs(n)))
    sign = 1.0 if n[axis] > 0 else -1.0
    c0 = int(bits(F(float(x[axis]) + sign * float(T_MIN) / float(se)))[0])
    cand = (c0 + np.arange(-4000, 4001)).astype(np.uint32).view(F)
    with np.errstate(all="ignore"):
        w = cand - x[axis]
        tm = np.sqrt(w * w) * se
    ok = np.isfinite(tm) & (np.sign(w) == sign)
    below, above, at = np.flatnonzero(ok & (tm < T_MIN)), np.flatnonzero(ok & (tm > T_MIN)), np.flatnonzero(ok & (tm == T_MIN))
    assert len(below) and len(above)
    picks = {"tmax_below": below[np.argmax(tm[below])], "tmax_above": above[np.argmin(tm[above])]}
    if len(at):
        picks["tmax_at"] = at[0]
    t_max = {}
    for name, k in picks.items():
        corner = x.copy()
        corner[axis] = cand[k]
        tables[name] = _given_quad(corner, zero, zero, n, color, 1.0)
        t_max[name] = tm[k]
    return dict(first_stream=fs, j=j, x=x, n=n, d=d, shadow_end=se, tables=tables, t_max=t_max)


def nee_entry_reference(orc, ow, desc, items, setup, table, background, source_is_diffuse):
    import gather_cases as GC
    import nee_cases as NC
    rays = GC.first_rays(orc, items, "cosine", ENTRY_K, GC.SPREAD, SEED, setup["first_stream"])
    ref = NC.nee_paths(orc, ow, desc, rays, table, max_bounces=NEE_BOUNCES, background=background, seed=SEED, first_stream=setup["first_stream"],
                       shadow_end=setup["shadow_end"], source_is_diffuse=source_is_diffuse)
    return NC.finish(ref, ENTRY_K)
