"""What tests/test_direct_pick_cases.py, tests/test_emitter_pick_build.py, tests/test_gpu_direct_pick.py and
tests/test_gpu_direct_pick_draws.py share, none of it touching a GPU: the restatement of the direct-light queries that choose their emitter
through an alias table (tinyrt.h trt_emitter_pick_build, trt_direct_pick, trt_direct_mis_pick) with the CPU oracle's pieces.

Built on direct_cases and direct_mis_cases by import, as direct_mis_cases is built on direct_cases:
  - build() restates trt_emitter_pick_build in numpy: f32 powers, a double total rounded once, one f32 division per prob, Vose's
    construction in double with the header's list order.
  - samples() is direct_cases.samples with the new steps 2 and 5: the draws are the oracle's (orc_rng_seed on stream (seed, j, 1),
    orc_rng_random, orc_random_unit_vector), the arithmetic numpy float32 scalars, occlusion the oracle's World.hit.
  - mis_samples() hands that to direct_mis_cases.samples as its `base` - wl, the lobe ray and its hit are that module's - and restates
    the hit side of a light hit anew: ph = power / total_power in the place of 1 / E.
Fixtures are direct_cases' own (324 items, seed 5, first_stream 1000, the table of direct_cases.table_of)."""
import ctypes as C

import numpy as np

import direct_cases as D
import direct_mis_cases as M
import nee_cases as N
import nee_mis_cases as NM

f32 = np.float32
K, SEED, FIRST_STREAM = D.K, D.SEED, D.FIRST_STREAM
SHADOW_END = D.SHADOW_END
BALANCE, POWER = M.BALANCE, M.POWER
HEURISTICS = M.HEURISTICS
# tinyrt.h trt_emitter_pick (16 bytes)
PICK_DTYPE = np.dtype([("q", np.float32), ("alias", np.uint32), ("prob", np.float32), ("reserved", np.uint32)])
assert PICK_DTYPE.itemsize == 16
LUM = (f32(0.2126), f32(0.7152), f32(0.0722))
# deliberately wrong restatements of the draw: u1 <= q; the alias not clamped (a record past the table reads as a dead sample); area *
# (1 / p); prob of the slot in place of the chosen emitter's; u1 drawn before u0 - and of the hit side: float(E) in place of 1 / ph; the
# luminance summed in another parenthesisation
DRAW_MUTANTS = ("u1_le_q", "alias_unclamped", "area_times_inv_p", "prob_of_slot", "u1_first")
HIT_MUTANTS = ("hit_uses_E", "luminance_parens")
MUTANTS = DRAW_MUTANTS + HIT_MUTANTS

_vec, _arr = D._vec, D._arr


def luminance(color, mutant=None):
    """((0.2126 r + 0.7152 g) + 0.0722 b) in float32 scalars."""
    r, g, b = f32(color[0]), f32(color[1]), f32(color[2])
    with np.errstate(all="ignore"):
        if mutant == "luminance_parens":
            return LUM[0] * r + (LUM[1] * g + LUM[2] * b)
        return (LUM[0] * r + LUM[1] * g) + LUM[2] * b


def powers(table):
    """power_e = luminance(color) * area per record, float32."""
    with np.errstate(all="ignore"):
        out = np.array([luminance(rec["color"]) * f32(rec["area"]) for rec in table], np.float32)
    return out


def build(table, weights=None):
    """trt_emitter_pick_build restated: (records, total).  Written apart from the library's code: plain Python lists used as stacks."""
    E = len(table)
    w = powers(table) if weights is None else np.asarray(weights, np.float32)
    assert w.shape == (E,) and np.isfinite(w).all() and (w >= 0).all()
    total = f32(sum(float(x) for x in w))                                   # double, in table order, rounded once
    assert total > 0 and np.isfinite(total)
    out = np.zeros(E, PICK_DTYPE)
    with np.errstate(all="ignore"):
        out["prob"] = w / total
    c = [float(w[e]) if out["prob"][e] > 0 else 0.0 for e in range(E)]
    S, lost = 0.0, 0.0                                                      # the header's compensated sum
    for x in c:
        t = S + x
        lost += (S - t) + x if S >= x else (x - t) + S
        S = t
    S += lost
    scaled = [(x * float(E)) / S for x in c]
    small = [e for e in range(E) if scaled[e] < 1.0]
    large = [e for e in range(E) if not scaled[e] < 1.0]
    q = [1.0] * E
    alias = list(range(E))
    while small and large:
        s, l = small.pop(), large.pop()
        q[s], alias[s] = scaled[s], l
        scaled[l] = (scaled[l] + scaled[s]) - 1.0
        (small if scaled[l] < 1.0 else large).append(l)
    heaviest = int(np.argmax(np.array(c)))                                  # the first of the largest
    for s in small:
        if scaled[s] == 0.0:
            q[s], alias[s] = 0.0, heaviest
    out["q"] = np.clip(np.array(q, np.float64).astype(np.float32), f32(0.0), f32(1.0))
    out["alias"] = alias
    return out, total


def implied(pick):
    """The probability the alias structure gives each emitter, in double: (q_k + sum over the other slots j with alias_j = k of (1 - q_j)) / E."""
    E = len(pick)
    qd = pick["q"].astype(np.float64)
    out = qd.copy()
    others = pick["alias"] != np.arange(E)
    np.add.at(out, pick["alias"][others], 1.0 - qd[others])
    return out / E


def draws(orc, seed, stream, n=2):
    """The first n draws of stream (seed, stream, 1) as float32."""
    rng = (C.c_uint32 * 2)()
    orc.lib.orc_rng_seed(seed, stream & 0xFFFFFFFF, 1, C.byref(rng))
    return [f32(orc.lib.orc_rng_random(C.byref(rng))) for _ in range(n)]


def samples(orc, ow, items, table, pick, k=K, seed=SEED, first_stream=FIRST_STREAM, shadow_end=SHADOW_END, mutant=None, only=None, occlusion=True,
            item_index=None):
    """The contract of tinyrt.h trt_direct_pick, sample by sample: direct_cases.samples' dict (e, live, walked, occ, rays, t_max, wgt, c)
    and slot (k of step 2), took_alias and state (the generator's two words after the sample's draws) besides.  `pick`: PICK_DTYPE records, used as given (a wrong table has defined results)."""
    assert mutant is None or mutant in DRAW_MUTANTS
    n, E = len(items), len(table)
    assert len(pick) == E
    shadow_end = f32(shadow_end)
    out = dict(e=np.zeros((n, k), np.int64), live=np.zeros((n, k), bool), walked=np.zeros((n, k), bool), occ=np.zeros((n, k), bool),
               rays=np.zeros((n, k, 6), np.float32), t_max=np.zeros((n, k), np.float32), c=np.zeros((n, k, 3), np.float32),
               wgt=np.zeros((n, k), np.float32), slot=np.zeros((n, k), np.int64), took_alias=np.zeros((n, k), bool),
               state=np.zeros((n, k, 2), np.uint32))
    rng = (C.c_uint32 * 2)()
    lib = orc.lib
    fE = f32(E)
    with np.errstate(all="ignore"):
        for i in (range(n) if only is None else only):
            x, nrm = _vec(orc, items[i, 0:3]), _vec(orc, items[i, 3:6])
            item = i if item_index is None else int(item_index[i])
            for s in range(k):
                lib.orc_rng_seed(seed, (first_stream + item * k + s) & 0xFFFFFFFF, 1, C.byref(rng))
                # ---- step 2 ----
                u0 = f32(lib.orc_rng_random(C.byref(rng)))
                u1 = f32(lib.orc_rng_random(C.byref(rng)))
                if mutant == "u1_first":
                    u0, u1 = u1, u0
                slot = min(int(u0 * fE), E - 1)
                q = f32(pick["q"][slot])
                keep = bool(u1 <= q) if mutant == "u1_le_q" else bool(u1 < q)          # a NaN q: False
                alias = int(pick["alias"][slot])
                e = slot if keep else (alias if mutant == "alias_unclamped" else min(alias, E - 1))
                out["slot"][i, s], out["took_alias"][i, s] = slot, not keep
                if e >= E:                                                   # (the mutant) a read past the table: no sample
                    out["e"][i, s] = -1
                    continue
                rec = table[e]
                if rec["kind"] == 1:
                    a = f32(lib.orc_rng_random(C.byref(rng)))
                    b = f32(lib.orc_rng_random(C.byref(rng)))
                    y = (rec["a"] + rec["b"] * a) + rec["c"] * b
                    nl = rec["normal"]
                else:
                    nl = _arr(lib.orc_random_unit_vector(C.byref(rng)))
                    y = rec["a"] + nl * rec["b"][0]
                assert y.dtype == np.float32
                out["state"][i, s] = (rng[0], rng[1])                        # the generator after the sample's last draw
                w = y - items[i, 0:3]
                wv = _vec(orc, w)
                d2 = f32(lib.orc_vec3_dot(wv, wv))
                cs = f32(lib.orc_vec3_dot(nrm, wv))
                cl = np.abs(f32(lib.orc_vec3_dot(_vec(orc, nl), wv)))
                # ---- step 5 ----
                p = f32(pick["prob"][slot if mutant == "prob_of_slot" else e])
                scale = (rec["area"] * (f32(1.0) / p) if mutant == "area_times_inv_p" else rec["area"] / p) * D.INV_PI
                geom = (cs * cl) / (d2 * d2)
                wgt = geom * scale
                assert wgt.dtype == np.float32
                live = bool(cs > 0 and d2 > 0 and np.isfinite(wgt))
                ray = lib.orc_ray_new(x, wv)
                t_max = np.sqrt(d2) * shadow_end
                walked = live and bool(t_max > f32(D.T_MIN))
                occ = False
                if walked and occlusion:
                    occ = ow.hit(ray, D.T_MIN, float(t_max))[0] is not None
                out["e"][i, s], out["live"][i, s], out["walked"][i, s], out["occ"][i, s] = e, live, walked, occ
                out["rays"][i, s] = np.frombuffer(bytes(ray), np.float32)
                out["t_max"][i, s] = t_max
                out["wgt"][i, s] = wgt
                if live and not occ:
                    out["c"][i, s] = rec["color"] * wgt
    return out


def mis_samples(orc, ow, desc, items, table, pick, total_power, heuristic=BALANCE, k=K, seed=SEED, first_stream=FIRST_STREAM, shadow_end=SHADOW_END,
                mutant=None, only=None, item_index=None, base=None):
    """The contract of tinyrt.h trt_direct_mis_pick, sample by sample: direct_mis_cases.samples over samples() above as its base (the
    shadow term, wl, the lobe ray, what it hit), with wb, tb and c of every light hit restated: ph = power / total_power from the hit
    material's colour and the hit primitive's area, g = ((csh * clh) / (t * t)) * ((area / ph) * (1 / pi)).  ph_bits [n, k]: ph as uint32
    (0 where no light was hit)."""
    assert mutant is None or mutant in MUTANTS
    if base is None:
        base = samples(orc, ow, items, table, pick, k=k, seed=seed, first_stream=first_stream, shadow_end=shadow_end, only=only,
                       item_index=item_index, mutant=mutant if mutant in DRAW_MUTANTS else None)
    out = M.samples(orc, ow, desc, items, table, heuristic=heuristic, k=k, seed=seed, first_stream=first_stream, shadow_end=shadow_end, only=only,
                    item_index=item_index, base=base)
    lib = orc.lib
    mats = M.P.material_table(orc, ow, desc)
    total_power = f32(total_power)
    out["ph_bits"] = np.zeros(out["has_b"].shape, np.uint32)
    with np.errstate(all="ignore"):
        for i, s in zip(*np.nonzero(out["has_b"])):
            axis = _vec(orc, items[i, 3:6])
            r6 = out["lobe_rays"][i, s]
            ray = orc.Ray(_vec(orc, r6[0:3]), _vec(orc, r6[3:6]))
            hit, geometry = ow.hit_index(ray, D.T_MIN, float("inf"))
            assert hit is not None and geometry == out["geo"][i, s]
            _, emission, _ = mats[hit.material]
            t = f32(hit.t)
            csh = f32(lib.orc_vec3_dot(axis, ray.direction))
            clh = np.abs(f32(lib.orc_vec3_dot(hit.normal, ray.direction)))
            area = NM.area_of(table, geometry)
            em = _arr(emission)
            ph = (luminance(em, mutant) * area) / total_power
            g = ((csh * clh) / (t * t)) * ((area * f32(len(table)) if mutant == "hit_uses_E" else area / ph) * D.INV_PI)
            assert g.dtype == np.float32
            qg = M.q(g, heuristic)
            weighted = bool(csh > 0 and np.isfinite(qg))
            wb = qg / (f32(1.0) + qg) if weighted else f32(1.0)
            out["full"][i, s], out["wb"][i, s], out["tb"][i, s] = not weighted, wb, em * wb
            out["ph_bits"][i, s] = np.array([ph], np.float32).view(np.uint32)[0]
            out["c"][i, s] = out["tl"][i, s] + out["tb"][i, s] if out["has_l"][i, s] else out["tb"][i, s]
    return out


def finish(smp, k, mis):
    """S, M and the counters' expectations (n_samples, n_walks, n_rays); frozen."""
    if mis:
        return M.finish(smp, k)
    smp["S"], smp["M"] = D.fold(smp, k)
    smp["n_samples"] = smp["c"].shape[0] * smp["c"].shape[1]
    smp["n_walks"] = smp["n_rays"] = int(smp["walked"].sum())
    return D.freeze(smp)


# ---- the draw one case per lane (tests/native/direct_pick_cases.hip, tests/test_gpu_direct_pick_draws.py) ----
OUT_WORDS = 15                                                              # ray[6], c[3], t_max, live, wgt, geometry, s0, s1


def f32_slot_streams(orc, E, want, limit=20000):
    """The first `want` streams (SEED, FIRST_STREAM + s, 1) whose slot uint32(u0 * float(E)) in f32 is not the exact floor."""
    found = []
    for stream in range(limit):
        u0 = draws(orc, SEED, FIRST_STREAM + stream, 1)[0]
        if int(u0 * f32(E)) != int(float(u0) * E):
            found.append(FIRST_STREAM + stream)
            if len(found) == want:
                break
    assert len(found) == want
    return found


def draw_cases(orc, items, table):
    """(cases, tables) for the per-lane harness.  A case is dict(cls, t, j, x6): the surfel x6 draws from tables[t] = (emitter records,
    pick records) on stream (SEED, j, 1).  `table`: three records, a quad first (direct_cases.table_of of the Cornell box); `items`:
    surfels, unit floor ones and odd ones mixed.  Classes: generic (the power table, every item, live and dead), edge_of_q (q[k] set to
    the case's own u1 and to the next float up), q_0 / q_1 / q_nan, alias_clamped, prob_0 / prob_overflow / prob_subnormal, table_of_one,
    f32_slot (E = 65521, the table's three records in turn)."""
    assert len(table) == 3 and table["kind"][0] == 1
    power, _ = build(table)
    tables, cases = [(table, power)], []
    rng = np.random.default_rng([SEED, 17])
    n = len(items)

    def add(cls, t, j, i):
        cases.append(dict(cls=cls, t=t, j=int(j) & 0xFFFFFFFF, x6=items[i]))

    for i in range(n):
        add("generic", 0, FIRST_STREAM + 8 * i, i)
    for c in range(24):                                                     # each with tables of its own
        i, j = int(rng.integers(n)), FIRST_STREAM + 5000 + c
        u0, u1 = draws(orc, SEED, j)
        k = min(int(u0 * f32(3.0)), 2)
        for q in (u1, np.nextafter(u1, f32(2.0))):
            pk = power.copy()
            pk["q"][k], pk["alias"][k] = q, (k + 1) % 3
            tables.append((table, pk))
            add("edge_of_q", len(tables) - 1, j, i)
    for cls, q in (("q_0", 0.0), ("q_1", 1.0), ("q_nan", np.nan)):
        pk = power.copy()
        pk["q"], pk["alias"] = q, [1, 2, 0]
        tables.append((table, pk))
        for c in range(32):
            add(cls, len(tables) - 1, FIRST_STREAM + 6000 + c, int(rng.integers(n)))
    for alias in (3, 2 ** 31, 0xFFFFFFFF):
        pk = power.copy()
        pk["q"], pk["alias"] = 0.0, alias
        tables.append((table, pk))
        for c in range(16):
            add("alias_clamped", len(tables) - 1, FIRST_STREAM + 7000 + c, int(rng.integers(n)))
    for cls, p in (("prob_0", 0.0), ("prob_overflow", 1e-37)):
        pk = power.copy()
        pk["prob"][0], pk["q"], pk["alias"] = p, 0.0, 0                     # every sample goes to the lamp
        tables.append((table, pk))
        for c in range(16):
            add(cls, len(tables) - 1, FIRST_STREAM + 8000 + c, int(rng.integers(n)))
    small = table.copy()
    small[2:] = D.sphere_record((50.0, 50.0, 50.0), 0.1, (1e-30, 1e-30, 1e-30))
    pk = power.copy()
    pk["prob"][2], pk["q"], pk["alias"] = 1e-39, 0.0, 2
    tables.append((small, pk))
    for c in range(32):
        add("prob_subnormal", len(tables) - 1, FIRST_STREAM + 9000 + c, int(rng.integers(n)))
    tables.append((table[:1], build(table[:1])[0]))
    for c in range(16):
        add("table_of_one", len(tables) - 1, FIRST_STREAM + 10000 + c, int(rng.integers(n)))
    E = 65521
    big = np.ascontiguousarray(table[np.arange(E) % 3])
    tables.append((big, build(big)[0]))
    for j in f32_slot_streams(orc, E, 4):
        add("f32_slot", len(tables) - 1, j, int(rng.integers(n)))
    return cases, tables


def draw_expectations(orc, cases, tables):
    """uint32 [n, OUT_WORDS] and the restatement's own flags per case (slot, took_alias, e, live): samples() without occlusion, one case at
    a time on its own stream.  Words 6..8 are colour * wgt for every row here (samples() keeps c of a dead sample 0)."""
    exp = np.zeros((len(cases), OUT_WORDS), np.uint32)
    flags = dict(slot=np.zeros(len(cases), np.int64), took_alias=np.zeros(len(cases), bool), e=np.zeros(len(cases), np.int64),
                 live=np.zeros(len(cases), bool))
    for r, c in enumerate(cases):
        tab, pk = tables[c["t"]]
        smp = samples(orc, None, c["x6"][None, :], tab, pk, k=1, first_stream=0, item_index=[c["j"]], occlusion=False)
        e = int(smp["e"][0, 0])
        with np.errstate(all="ignore"):
            col = (tab["color"][e] * smp["wgt"][0, 0]).astype(np.float32)
        exp[r, 0:6] = smp["rays"][0, 0].view(np.uint32)
        exp[r, 6:9] = col.view(np.uint32)
        exp[r, 9] = smp["t_max"][0].view(np.uint32)[0]
        exp[r, 10] = int(smp["live"][0, 0])
        exp[r, 11] = smp["wgt"][0].view(np.uint32)[0]
        exp[r, 12] = tab["geometry"][e]
        exp[r, 13:15] = smp["state"][0, 0]
        for name in flags:
            flags[name][r] = smp[name][0, 0]
    return exp, flags


def write_draw_cases(path, cases, tables, order):
    import struct
    with open(path, "wb") as f:
        f.write(struct.pack("<IIII", 0x31435044, len(order), len(tables), SEED))
        for r in order:
            c = cases[r]
            f.write(struct.pack("<II", c["t"], c["j"]))
            f.write(np.array([SHADOW_END], np.float32).tobytes())
            f.write(np.ascontiguousarray(c["x6"], np.float32).tobytes())
        for tab, pk in tables:
            f.write(struct.pack("<I", len(tab)))
            f.write(np.ascontiguousarray(tab).tobytes())
            f.write(np.ascontiguousarray(pk).tobytes())


def dim_lights():
    """The 60 small sphere lights of the many-light room: radius 1, two units off the left, right and back walls of the Cornell box, four
    rows of five on each."""
    spots = []
    for y in (20.0, 40.0, 60.0, 80.0):
        for a in (10.0, 30.0, 50.0, 70.0, 90.0):
            spots += [(2.0, y, a), (98.0, y, a), (a, y, 98.0)]
    assert len(spots) == 60
    return spots


def many_light_room(trt, orc):
    """(description, oracle world, nee_cases' 40 floor surfels, the scene's own table of 61) of the Cornell box with the lamp at y = 99
    and 60 sphere lights of 0.05 x the lamp's colour along the walls: the lamp carries 94 % of the power and 1 / 61 of a uniform choice."""
    desc, _, items, _ = N.lowered_cornell(trt, orc)
    lamp = [m for m in desc["materials"] if m[0] == "light"][0]
    dim = ("dim_light", D.LIGHT, tuple(0.05 * ch for ch in lamp[2]), 0.0)
    geos = list(desc["geometries"]) + [("sphere", spot, 1.0, dim[0]) for spot in dim_lights()]
    room = dict(desc, materials=list(desc["materials"]) + [dim], geometries=geos)
    ow, _ = orc.world_from_description(room)
    table = D.emitters_of(orc, room)
    assert len(table) == 61 and table["kind"][0] == 1
    return room, ow, items, table


differing = D.differing
assert_same_bits = D.assert_same_bits
