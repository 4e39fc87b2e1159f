"""Scenes, cases and expectations of the shade-level test (tests/test_shade_cases.py on the CPU, tests/test_gpu_shade.py on the GPU):
one pass of the loop body of CpuSampler::single_point_sampling after the hit query (cpu.rs:48-62) - rt_path.h shade_hit - case by
case, and the vector helpers of rt_device.h on chosen vectors.  Everything is seeded numpy; a ray is used as given.

Scenes (32 primitives: the LDS accessor; the GPU harness also reads the SAME packed scene through SceneAcc<MODE_GLOBAL>, whose
element offsets are the LDS accessor's - no padding with far-away spheres is needed for "the zoo from global memory"):
  zoo        every scattering albedo <= 1 (SceneLayout::lazy_color set).  One sphere and one quad per material - a Lambertian, metals
             of fuzz 0, 1, -0.5, 1.5 (both clamped at creation, metal.rs:12-14; the scene file carries the clamped value, as the C API
             hands it to the scene compiler), 0.3, dielectrics of index 1.5, 1/1.5, 1.0, 2.4, 0.9, a light of colour above 1; the
             dielectric quads and the fuzz-1 metal quad are axis-aligned (their unit normal is exact, so a case can choose
             -dot(normal, d) to the bit), the others rotated and sheared; a rotated quad of index 1.5, a tiny (|n| ~ 1e-12) and a
             huge (|n| ~ 1e12) quad, a unit sphere of radius -1 at the origin, a large sphere hit from inside, a quad in the plane
             y = 1 and two quads whose normal is (2^-39, b, 1) with b one float either side of 2^-39.
  hot        the zoo with the Lambertian's albedo above 1 and a metal's at 3e30: lazy_color off, only the carried colour is legal.

A case is (origin, direction, geometry index or -1 = miss, t, colour, attenuation, remain, RNG state, background).  t is the
oracle's own orc_sphere_hit / orc_quad_hit answer for that primitive alone in 0.001..inf.  A direction is unit length to within
rounding, or - class dielectric_scaled_dir - the output of Ray::new for a vector so small that its squared length is a subnormal
of one or two bits: |d| is then 0.9 .. 1.2, which is what a fuzz-1 metal bounce can hand to the next hit.

The generator is xoroshiro64* with output s0 * 0x9E3779BB: the first two draws of a state are chosen by solving s0 from the first
output with the multiplier's inverse and s1 from the second through the inverse of t ^ (t << 9); a chosen THIRD draw is reached
by stepping the generator backwards twice from a state whose output it is (xoroshiro's step is a bijection - no search needed).

Classes (the defining property of each is asserted on the CPU by tests/test_shade_cases.py):
  generic                  GENERIC_PER_CELL seeded cases per (material kind x sphere / quad x front / back face), cycling through the
                           materials of the kind; remain 1 or 2; attenuation 1, small, random, on `hot` also inf; every fourth
                           with a colour carried in
  lam_zero_sum             near_zero taken, the sum exactly zero (u2 = 0: the unit vector is (-+0, 0, 1); normal (0, 0, -1))
  lam_tiny_sum             near_zero taken, the sum non-zero and below 1e-7 in every component ((u1, u2) = (0.25, 0.5), normal (0, -1, 0))
  lam_not_near_zero        near_zero not taken by the nearest sums the 23-bit draws can reach: (u1, u2) one step of 2^-23 from
                           (0.25, 0.5) - the largest component is then 1e-7 .. 2e-6 (a step in u1 turns theta by 7.5e-7)
  lam_u3_zero              third draw 0: in_sphere is the zero vector, normalized gives 0/0, the new ray is NaN
  lam_domain_edge          dir = (2^-39, b, 2) with b one float below / above 2^-39: plain and short path of normalized()
  metal_incidence          every fuzz at normal and at grazing incidence, sphere and quad
  metal_tiny_dir           fuzz 1, in_sphere within an ulp or two of -reflected per component: |dir| ~ 1e-7 and its z component
                           2^-40 .. 3 * 2^-40, both sides of normalized()'s 2^-39 switch
  metal_below_surface      the scattered direction points into the surface (the reference still scatters)
  dielectric_tir_straddle  ri * sinv the nearest product above 1.0 that any float cosv gives, 1.0 itself, and the nearest below, for
                           every (index, face) that can reflect totally; each with a draw of 0 and of 1 - 2^-23.  sinv is a function
                           of the float cosv alone and cosv^2 skips floats, so the products are a fixed set per index: the nearest
                           above 1.0 is one float up for ri = 1/0.9, two for 1.5, three for 2.4; the nearest below is one float down
                           (six for 2.4)
  dielectric_cos_above_one the unclamped -dot(normal, d) is above 1.0 (spheres hit through their centre, the rotated quad along its normal)
  dielectric_scaled_dir    |d| off 1 by up to 20 % (see above) at normal incidence and at 45 degrees: the clamps and the fabs of refract() matter
  dielectric_draw_edge     first draw = the largest 23-bit value below the reflectance, the reflectance itself where representable
                           (index 1.0, 1 - cos = 0.5: 1/32), the next value above
  dielectric_grazing       reflectance -> 1
  front_face_sphere        tangent rays: dot(d, p - c) exactly 0 (back face; integer constructions on the unit sphere) and within
                           4e-7 r of 0 - a few ulp of the operands - on both sides (a seeded search over tangent rays keeps those)
  front_face_quad          grazing rays: dot(d, n) within a few ulp of 0 on both sides (an exact 0 cannot hit: t = x / 0)
  extreme_quad             the tiny and the huge quad, front and back face, ordinary incidence, finite scattered ray
  extreme_quad_grazing     the huge quad with dot(d, n) / |n| within 2e-6 of 0 on both sides
  front_face_far           hits at t ~ 1e6, where point - center cancels
  generic_big_inside       the sphere of radius 1000.5 hit from inside
  light                    ends the path, leaves ray, attenuation, remain and rng alone
  miss                     several backgrounds and attenuations

Mutants of the restatement the case list does NOT distinguish from the oracle (tests/test_shade_cases.py reports the others' killers):
  10  x^5 as (x2 * x2) * x: IEEE multiplication is commutative, so this IS x * (x2 * x2) - 0 of 4 194 304 random x in (-0.25, 2) differ.
"""
import ctypes as C
import struct

import numpy as np

SEED = 1
GENERIC_PER_CELL = 64
F = np.float32
MASK = 0xFFFFFFFF
MULT = 0x9E3779BB
MULT_INV = pow(MULT, -1, 1 << 32)
LAMBERTIAN, METAL, DIELECTRIC, LIGHT = 0, 1, 2, 3
KIND_NAMES = ("lambertian", "metal", "dielectric", "light")
LO, HI = F(2.0 ** -39), F(2.0 ** 39)
CASE_WORDS, OUT_WORDS, VEC_WORDS, VEC_OUT_WORDS = 22, 21, 7, 20
LIST_LENGTHS = (1, 63, 64, 65)
N_MUTANTS = 12
MUTANT_NAMES = {1: "near_zero eps 1e-8", 2: "near_zero branch removed", 3: "no clamp in the scatter's cosine", 4: "no clamp in refract",
                5: ">= in the total-reflection test", 6: ">= in reflectance-versus-draw", 7: "a draw consumed on total reflection",
                8: "front_face with <=", 9: "index not inverted on the front face", 10: "x^5 as (x2 * x2) * x", 11: "no fabs in refract",
                12: "dot with fused multiply-adds"}


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def nextf(x, k=1):
    """x moved k floats up (k < 0: down) - finite non-zero x of either sign."""
    x = F(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, F(np.inf) if k > 0 else F(-np.inf))
    return x


# ------------------------------------------------------------------------------------------------------------------
# trt-rng v1, forwards and backwards
# ------------------------------------------------------------------------------------------------------------------
def _rotl(x, k):
    return ((x << k) | (x >> (32 - k))) & MASK


def rng_step(s0, s1):
    """(output, (s0', s1'))"""
    r = (s0 * MULT) & MASK
    s1 ^= s0
    return r, (_rotl(s0, 26) ^ s1 ^ ((s1 << 9) & MASK), _rotl(s1, 13))


def rng_unstep(a, b):
    t = _rotl(b, 32 - 13)
    s0 = _rotl(a ^ t ^ ((t << 9) & MASK), 32 - 26)
    return s0, t ^ s0


def draw_word(u, low=0):
    """A generator output whose random::<f32>() is u (a multiple of 2^-23 in [0, 1)); `low`: the nine bits the float does not see."""
    k = int(round(float(u) * (1 << 23)))
    assert 0 <= k < (1 << 23) and k / (1 << 23) == float(u), u
    return (k << 9) | (low & 0x1FF)


def state_for_draws(u1, u2, low=0):
    r1, r2 = draw_word(u1, low), draw_word(u2, low >> 9)
    s0 = (r1 * MULT_INV) & MASK
    x = ((r2 * MULT_INV) & MASK) ^ _rotl(s0, 26)                       # = t ^ (t << 9), t = s1 ^ s0
    t = (x ^ (x << 9) ^ (x << 18) ^ (x << 27)) & MASK
    s = (s0, t ^ s0)
    assert s != (0, 0)
    return s


def state_for_third_draw(r3, s1_after):
    a = (r3 * MULT_INV) & MASK
    return rng_unstep(*rng_unstep(a, s1_after))


def u_of(r):
    return F((r >> 9) / float(1 << 23))


# ------------------------------------------------------------------------------------------------------------------
# scenes
# ------------------------------------------------------------------------------------------------------------------
MATERIALS = [("lam", LAMBERTIAN, (0.8, 0.5, 0.3), 0.0),
             ("met0", METAL, (0.9, 0.8, 0.7), 0.0), ("met1", METAL, (0.7, 0.7, 0.9), 1.0), ("metneg", METAL, (0.5, 0.9, 0.6), -0.5),
             ("met15", METAL, (1.0, 0.6, 0.4), 1.5), ("met03", METAL, (0.6, 0.6, 0.6), 0.3),
             ("die15", DIELECTRIC, (1.0, 1.0, 1.0), 1.5), ("die067", DIELECTRIC, (0.9, 1.0, 0.9), 1.0 / 1.5), ("die10", DIELECTRIC, (1.0, 0.9, 0.8), 1.0),
             ("die24", DIELECTRIC, (0.7, 0.8, 1.0), 2.4), ("die09", DIELECTRIC, (1.0, 1.0, 0.5), 0.9),
             ("light", LIGHT, (4.0, 2.5, 1.5), 0.0)]
TIR_FACES = (("die15", False), ("die067", True), ("die24", False), ("die09", True))      # (material, front face) with ri > 1


def scene_names():
    return ["zoo", "hot"]


def _f(v):
    return tuple(float(F(x)) for x in v)


def description(name):
    """tiny-raytracer_amd.scenes format; geometry indices: 0-11 the materials' spheres, 12-23 their quads, then GEO below."""
    g = np.random.default_rng([SEED, 1000])
    mats = [list(m) for m in MATERIALS]
    if name == "hot":
        mats[0][2] = (1.5, 0.9, 0.5)
        mats[5][2] = (3e30, 0.5, 3e30)
    else:
        assert name == "zoo", name
    mats = [(m[0], m[1], _f(m[2]), float(F(m[3]))) for m in mats]
    geos = []
    for m in MATERIALS:
        geos.append(("sphere", _f(g.uniform(-3, 3, 3)), float(F(g.uniform(0.3, 1.2))), m[0]))
    axis_aligned = {"die15": 2, "die067": 2, "die10": 2, "die24": 0, "die09": 1, "met1": 2}      # axis of the normal
    for m in MATERIALS:
        c = np.round(g.uniform(-3, 3, 3) * 4) / 4
        if m[0] == "lam":                                                  # the quad in the plane z = 1: n = (0, 0, 4)
            geos.append(("quad", (-1.0, -1.0, 1.0), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0), m[0]))
        elif m[0] in axis_aligned:
            a = axis_aligned[m[0]]
            u, v = np.zeros(3), np.zeros(3)
            u[(a + 1) % 3], v[(a + 2) % 3] = 2.0, 2.0                       # u x v = 4 e_a
            geos.append(("quad", _f(c), _f(u), _f(v), m[0]))
        else:                                                              # rotated and sheared
            geos.append(("quad", _f(g.uniform(-3, 3, 3)), _f(g.uniform(-2, 2, 3)), _f(g.uniform(-2, 2, 3)), m[0]))
    lo = float(LO)
    geos += [("sphere", (0.0, 0.0, 0.0), -1.0, "lam"),                                                     # 24 unit
             ("sphere", (0.0, -1000.0, 0.0), 1000.5, "die15"),                                             # 25 big
             ("quad", (0.5, 0.25, -0.5), (1e-6, 2e-7, 0.0), (0.0, 3e-7, 1e-6), "met03"),                   # 26 tiny
             ("quad", (-5e5, 10.0, -5e5), (1e6, 2e5, 0.0), (0.0, 3e5, 1e6), "lam"),                        # 27 huge
             ("quad", (-1.0, 1.0, -1.0), (0.0, 0.0, 2.0), (2.0, 0.0, 0.0), "lam"),                         # 28 plane y = 1: n = (0, 4, 0)
             ("quad", (-0.5, -0.5, 3.0), (1.0, 0.0, -lo), (0.0, 1.0, -float(nextf(LO, -1))), "lam"),       # 29 tilt_below: n = (2^-39, below, 1)
             ("quad", (-0.5, -0.5, 5.0), (1.0, 0.0, -lo), (0.0, 1.0, -float(nextf(LO, 1))), "lam"),        # 30 tilt_above
             ("quad", _f(g.uniform(-3, 3, 3)), _f(g.uniform(-2, 2, 3)), _f(g.uniform(-2, 2, 3)), "die15")]  # 31 rotated dielectric
    geos = [(q[0], _f(q[1]), q[2], q[3]) if q[0] == "sphere" else (q[0], _f(q[1]), _f(q[2]), _f(q[3]), q[4]) for q in geos]
    cam = dict(focus_distance=9.0, defocus_angle=0.0, position=(0.0, 1.0, 9.0), look_at=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), vertical_fov=50.0,
               width=8, height=8)
    return dict(name="shade_" + name, materials=mats, geometries=geos, camera=cam, background=(0.0, 0.0, 0.0))


GEO = dict(unit=24, big=25, tiny=26, huge=27, plane_y=28, tilt_below=29, tilt_above=30, rot_die=31)


def clamp_fuzz(kind, param):
    """Metal::new (metal.rs:12-14)."""
    p = F(param)
    return float(min(max(p, F(0.0)), F(1.0))) if kind == METAL else float(p)


def file_description(desc):
    """The description as the scene compiler gets it from the C API: the fuzz of a metal clamped."""
    return dict(desc, materials=[(n, k, a, clamp_fuzz(k, p)) for n, k, a, p in desc["materials"]])


class Scene:
    def __init__(self, name, desc=None):
        import walk_ray_cases as W
        self.name = name
        self.desc = description(name) if desc is None else desc
        names = [m[0] for m in self.desc["materials"]]
        self.mat_index = {n: i for i, n in enumerate(names)}
        self.mats = [(k, np.array(a, F), F(clamp_fuzz(k, p))) for _, k, a, p in self.desc["materials"]]
        self.geo_mat = [names.index(q[-1]) for q in self.desc["geometries"]]
        self.kind, self.a, self.b, self.c = W.geometry_arrays(self.desc)
        self.lazy = all(k == LIGHT or bool((np.abs(a) <= F(1.0)).all()) for k, a, _ in self.mats)
        self.n = len(self.kind)
        of_sphere, of_quad = np.flatnonzero(self.kind == 0), np.flatnonzero(self.kind == 1)
        self.prim = np.zeros(self.n, np.uint32)                           # rt_path.h reference: kind bit | index within kind
        self.prim[of_sphere] = np.arange(len(of_sphere))
        self.prim[of_quad] = 0x40000000 | np.arange(len(of_quad))
        with np.errstate(all="ignore"):
            self.quad_n = np.stack([cross(self.b[i], self.c[i]) for i in range(self.n)])

    def material(self, gi):
        return self.mats[self.geo_mat[gi]]

    def geos_of(self, mat_kind, shape, only_material_prims=True):
        return [i for i in range(24 if only_material_prims else self.n) if self.kind[i] == shape and self.material(i)[0] == mat_kind]

    def geo_of(self, mat_name, shape):
        return self.mat_index[mat_name] + (12 if shape == 1 else 0)

    def hit(self, orc, gi, o, d):
        """The oracle's record for primitive gi alone in 0.001..inf, or None."""
        ray = orc.Ray(orc.Vec3(*[float(x) for x in o]), orc.Vec3(*[float(x) for x in d]))
        rec = orc.HitRecord()
        if self.kind[gi] == 0:
            ok = orc.lib.orc_sphere_hit(orc.Vec3(*self.a[gi].tolist()), float(self.b[gi, 0]), C.byref(ray), 0.001, float("inf"), C.byref(rec))
        else:
            ok = orc.lib.orc_quad_hit(orc.Vec3(*self.a[gi].tolist()), orc.Vec3(*self.b[gi].tolist()), orc.Vec3(*self.c[gi].tolist()), C.byref(ray),
                                      0.001, float("inf"), C.byref(rec))
        return rec if ok else None


# ------------------------------------------------------------------------------------------------------------------
# float32 restatement of HitRecord::new + Material::scatter (numpy scalars: every operation rounds once, nothing contracts),
# with the twelve mutants
# ------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    # a * b is exact in float64; the sum is rounded to 53 bits and then to 24 (a double rounding in ~2^-29 of the cases: this is a mutant's arithmetic)
    return F(np.float64(a) * np.float64(b) + np.float64(c))


def dot(a, b, fma=False):
    if fma:
        return _fma(a[2], b[2], _fma(a[1], b[1], a[0] * b[0]))
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F)


def normalized(a, fma=False):
    return a / np.sqrt(dot(a, a, fma))


def reflect(v, n, fma=False):
    return v - (F(2.0) * dot(v, n, fma)) * n


def fmin1(c):
    return c if c < F(1.0) else F(1.0)                                     # fminf(c, 1): a NaN gives 1


def refract(v, n, eta, mut=0):
    fma = mut == 12
    c = -dot(n, v, fma)
    if mut != 4:
        c = fmin1(c)
    perp = eta * (v + n * c)
    k = F(1.0) - dot(perp, perp, fma)
    parallel = (-np.sqrt(k if mut == 11 else np.abs(k))) * n
    return parallel + perp


def _vec(v):
    return np.array([v.x, v.y, v.z], F)


def _state(s):
    return (C.c_uint32 * 2)(int(s[0]), int(s[1]))


def restate(orc, sc, case, mut=0, tr=None):
    """(point[3], direction[3], s0, s1) of the scattered ray as uint32 words, or None for a light.  tr: dict that receives intermediate values."""
    tr = {} if tr is None else tr
    fma = mut == 12
    with np.errstate(all="ignore"):
        o, d, gi = case["o"], case["d"], case["geo"]
        point = o + case["t"] * d
        outward = point - sc.a[gi] if sc.kind[gi] == 0 else sc.quad_n[gi]
        ff = dot(d, outward, fma)
        front = bool(ff <= F(0.0)) if mut == 8 else bool(ff < F(0.0))
        nu = normalized(outward, fma)
        normal = nu if front else -nu
        kind, _, param = sc.material(gi)
        state = _state(case["rng"])
        tr.update(front_dot=ff, front=front, normal=normal, point=point)
        if kind == LAMBERTIAN:
            in_sphere = _vec(orc.lib.orc_random_in_unit_sphere(_state(case["rng"])))
            dirv = normal + _vec(orc.lib.orc_random_unit_vector(state))
            eps = F(1e-8) if mut == 1 else F(1e-7)
            nz = bool((np.abs(dirv) < eps).all())
            tr.update(in_sphere=in_sphere, sum=dirv, near_zero=nz)
            if nz and mut != 2:
                dirv = normal
        elif kind == METAL:
            reflected = reflect(d, normal, fma)
            in_sphere = _vec(orc.lib.orc_random_in_unit_sphere(state))
            dirv = reflected + param * in_sphere
            tr.update(reflected=reflected, in_sphere=in_sphere)
        elif kind == DIELECTRIC:
            ri = F(1.0) / param if (front and mut != 9) else param
            raw = -dot(normal, d, fma)
            cosv = raw if mut == 3 else fmin1(raw)
            sinv = np.sqrt(F(1.0) - cosv * cosv)
            prod = ri * sinv
            tir = bool(prod >= F(1.0)) if mut == 5 else bool(prod > F(1.0))
            sqrt_r0 = (F(1.0) - ri) / (F(1.0) + ri)
            r0 = sqrt_r0 * sqrt_r0
            x = F(1.0) - cosv
            x2 = x * x
            p5 = (x2 * x2) * x if mut == 10 else x * (x2 * x2)
            reflectance = r0 + (F(1.0) - r0) * p5
            tr.update(ri=ri, cos_raw=raw, prod=prod, tir=tir, reflectance=reflectance)
            if tir:
                if mut == 7:
                    orc.lib.orc_rng_random(state)
                do_reflect = True
            else:
                u = F(orc.lib.orc_rng_random(state))
                do_reflect = bool(reflectance >= u) if mut == 6 else bool(reflectance > u)
                tr.update(u=u)
            tr.update(do_reflect=do_reflect)
            dirv = reflect(d, normal, fma) if do_reflect else refract(d, normal, ri, mut)
            if not do_reflect:
                perp = ri * (d + normal * fmin1(-dot(normal, d)))
                tr.update(refract_k=F(1.0) - dot(perp, perp))
        else:
            return None
        tr.update(dir=dirv)
        new_d = normalized(dirv, fma)
        return np.concatenate([bits(point), bits(new_d), np.array([state[0], state[1]], np.uint32)])


def oracle_scatter(orc, sc, case):
    """The same words from orc_sphere_hit / orc_quad_hit + orc_material_scatter."""
    gi = case["geo"]
    rec = sc.hit(orc, gi, case["o"], case["d"])
    assert rec is not None
    kind, albedo, param = sc.material(gi)
    ray = orc.Ray(orc.Vec3(*case["o"].tolist()), orc.Vec3(*case["d"].tolist()))
    state, new, att = _state(case["rng"]), orc.Ray(), orc.Vec3()
    ok = orc.lib.orc_material_scatter(int(kind), orc.Vec3(*albedo.tolist()), float(param), C.byref(ray), C.byref(rec), C.byref(state), C.byref(new),
                                      C.byref(att))
    if not ok:
        return None
    return np.concatenate([np.frombuffer(bytes(new), np.uint32), np.array([state[0], state[1]], np.uint32)])


def expectation(orc, sc, case):
    """The loop body of single_point_sampling after the hit query (rt_oracle.c / cpu.rs:48-62): 16 words - ray.o, ray.d, colour,
    attenuation, remain, rng, ended.  Colour and attenuation in numpy float32."""
    o, d, color, atten, remain, rng = bits(case["o"]), bits(case["d"]), case["color"], case["atten"], case["remain"], case["rng"]
    with np.errstate(all="ignore"):
        if case["geo"] < 0:
            color = color + atten * case["bg"]
            ended = 1
        else:
            kind, albedo, _ = sc.material(case["geo"])
            emission = albedo if kind == LIGHT else np.zeros(3, F)
            color = color + atten * emission
            sw = oracle_scatter(orc, sc, case)
            if sw is None:
                ended = 1
            else:
                atten = atten * albedo
                o, d, rng = sw[0:3], sw[3:6], (int(sw[6]), int(sw[7]))
                remain -= 1
                ended = 1 if remain == 0 else 0
    return np.concatenate([o, d, bits(color), bits(atten), np.array([remain, rng[0], rng[1], ended], np.uint32)])


# ------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------
def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _perp(d, g):
    p = np.cross(d, g.normal(size=3))
    return p / np.linalg.norm(p)


class CaseMaker:
    def __init__(self, orc, sc, seed=SEED):
        self.orc, self.sc, self.seed = orc, sc, seed
        self.cases = []

    def rng(self, salt):
        return np.random.default_rng([self.seed, salt])

    def add(self, cls, o, d, gi, rng, color=(0, 0, 0), atten=(1, 1, 1), remain=2, bg=(0, 0, 0), exact_d=False, need_hit=True):
        d = np.asarray(d, np.float64)
        with np.errstate(all="ignore"):
            c = dict(cls=cls, o=np.asarray(o, np.float64).astype(F), d=(d if exact_d else _unit(d)).astype(F), geo=int(gi), color=np.array(color, F),
                     atten=np.array(atten, F), remain=int(remain), rng=(int(rng[0]), int(rng[1])), bg=np.array(bg, F))
        if gi < 0:
            c["t"], c["front"] = F(np.inf), None
        else:
            rec = self.sc.hit(self.orc, gi, c["o"], c["d"])
            if rec is None:
                assert not need_hit, (cls, gi, o, d)
                return None
            c["t"], c["front"] = F(rec.t), bool(rec.front_face)
        c["lazy_ok"] = bool(self.sc.lazy and (bits(c["color"]) == 0).all())
        self.cases.append(c)
        return c

    def drop(self, c):
        assert self.cases[-1] is c
        self.cases.pop()

    def trace(self, c):
        tr = {}
        restate(self.orc, self.sc, c, 0, tr)
        return tr

    # -- rays at a primitive
    def aim(self, g, gi, want_front, grazing=None):
        """(origin, direction) float64 of a ray that meets primitive gi (a material sphere / quad) on the wanted side."""
        sc = self.sc
        a, b, c = sc.a[gi].astype(np.float64), sc.b[gi].astype(np.float64), sc.c[gi].astype(np.float64)
        if sc.kind[gi] == 0:
            r = abs(b[0])
            target = a + r * _unit(g.normal(size=3)) * g.uniform(0.0, 0.9)
            o = a + r * _unit(g.normal(size=3)) * (g.uniform(1.5, 4.0) if want_front else g.uniform(0.0, 0.8))
            return o, target - o
        n = _unit(np.cross(b, c))
        target = a + g.uniform(0.05, 0.95) * b + g.uniform(0.05, 0.95) * c
        side = 1.0 if want_front else -1.0                               # front face: travelling against n
        if grazing is not None:
            dirv = _unit(_perp(n, g) - side * grazing * n)
        else:
            dirv = _unit(-side * n * g.uniform(0.2, 1.0) + _perp(n, g) * g.uniform(0.0, 1.0))
        return target - dirv * g.uniform(0.5, 3.0), dirv

    def random_state(self, g):
        return int(g.integers(0, 1 << 32)), int(g.integers(1, 1 << 32))

    def generic(self, per_cell=GENERIC_PER_CELL):
        sc = self.sc
        g = self.rng(1)
        for kind in (LAMBERTIAN, METAL, DIELECTRIC, LIGHT):
            for shape in (0, 1):
                geos = sc.geos_of(kind, shape)
                for want_front in (True, False):
                    got = tries = 0
                    while got < per_cell:
                        tries += 1
                        assert tries < 50 * per_cell
                        gi = geos[tries % len(geos)]
                        o, d = self.aim(g, gi, want_front)
                        pick = got % 4
                        atten = [(1, 1, 1), tuple(g.uniform(1e-6, 1e-3, 3)), tuple(g.uniform(0, 1, 3)),
                                 (np.inf, 1.0, np.inf) if sc.name == "hot" else (0.25, 0.5, 1.0)][pick]
                        color = tuple(g.uniform(0, 2, 3)) if (got // 4) % 4 == 3 else (0, 0, 0)
                        c = self.add("generic", o, d, gi, self.random_state(g), color=color, atten=atten, remain=1 + (got // 2) % 2, need_hit=False)
                        if c is None:
                            continue
                        if c["front"] != want_front:
                            self.drop(c)
                            continue
                        got += 1

    def lambertian(self):
        sc, g = self.sc, self.rng(2)
        quad_z1 = sc.geo_of("lam", 1)
        for u1 in (0.0, 0.25, 0.7109375):
            self.add("lam_zero_sum", (0.2, 0.3, -1.0), (0, 0, 1), quad_z1, state_for_draws(u1, 0.0, low=int(g.integers(0, 1 << 18))), exact_d=True)
        for low in (0, 77, 1 << 17):
            self.add("lam_tiny_sum", (0.1, -1.0, 0.4), (0, 1, 0), GEO["plane_y"], state_for_draws(0.25, 0.5, low=low), exact_d=True)
        step = 2.0 ** -23
        for du1, du2 in ((step, 0), (-step, 0), (0, step), (0, -step), (step, -step)):
            self.add("lam_not_near_zero", (0.1, -1.0, 0.4), (0, 1, 0), GEO["plane_y"], state_for_draws(0.25 + du1, 0.5 + du2), exact_d=True)
        for r3, shape in ((0, 0), (5, 1), (511, 0), (256, 1)):
            gi = sc.geo_of("lam", shape) if shape == 0 else GEO["huge"]
            o, d = self.aim(g, gi, True)
            self.add("lam_u3_zero", o, d, gi, state_for_third_draw(r3, int(g.integers(0, 1 << 32))), remain=1 + r3 % 2)
        for gi, z in ((GEO["tilt_below"], 3.0), (GEO["tilt_above"], 5.0)):
            for u1 in (0.0, 0.5):
                self.add("lam_domain_edge", (0.1, -0.2, z + 1.5), (0, 0, -1), gi, state_for_draws(u1, 0.0, low=int(g.integers(0, 1 << 18))), exact_d=True)

    def metal(self):
        sc, g = self.sc, self.rng(3)
        for name in ("met0", "met1", "metneg", "met15", "met03"):
            for shape in (0, 1):
                gi = sc.geo_of(name, shape)
                if shape == 0:
                    a, r = sc.a[gi].astype(np.float64), abs(float(sc.b[gi, 0]))
                    u = _unit(g.normal(size=3))
                    self.add("metal_incidence", a + 3.0 * r * u, -u, gi, self.random_state(g))                       # through the centre
                    p = _perp(u, g)
                    self.add("metal_incidence", a + r * (1.0 - 1e-5) * p - 4.0 * u, u, gi, self.random_state(g))      # nearly tangent
                else:
                    n = _unit(np.cross(sc.b[gi].astype(np.float64), sc.c[gi].astype(np.float64)))
                    mid = sc.a[gi] + 0.5 * sc.b[gi].astype(np.float64) + 0.5 * sc.c[gi].astype(np.float64)
                    self.add("metal_incidence", mid + 2.0 * n, -n, gi, self.random_state(g))
                    o, d = self.aim(g, gi, True, grazing=1e-4)
                    self.add("metal_incidence", o, d, gi, self.random_state(g))
        # below the surface: grazing incidence on the fuzz-1 metals, states whose in_sphere points down
        found = 0
        for name in ("met1", "met15", "met03"):
            for shape in (0, 1):
                gi = sc.geo_of(name, shape)
                got = 0
                for _ in range(200):
                    if shape == 0:
                        a, r = sc.a[gi].astype(np.float64), abs(float(sc.b[gi, 0]))
                        u = _unit(g.normal(size=3))
                        o, d = a + r * 0.98 * _perp(u, g) - 4.0 * u, u
                    else:
                        o, d = self.aim(g, gi, True, grazing=0.05)
                    c = self.add("metal_below_surface", o, d, gi, self.random_state(g), need_hit=False)
                    if c is None:
                        continue
                    tr = self.trace(c)
                    with np.errstate(all="ignore"):
                        below = bool(dot(tr["dir"], tr["normal"]) < F(0.0))
                    if not below:
                        self.drop(c)
                        continue
                    got += 1
                    found += 1
                    if got == 3:
                        break
        assert found >= 6
        self.metal_tiny_dir()

    def metal_tiny_dir(self):
        """u3 = 1 - 2^-23 (|in_sphere| = 1 to the ulp) and u2 so close to 1/2 that in_sphere.z is 2^-17 .. 2^-16: a scan of the state
        behind the third draw; the ray is -in_sphere mirrored in the fuzz-1 metal's plane z = const, moved by an ulp or two."""
        sc, g = self.sc, self.rng(4)
        gi = sc.geo_of("met1", 1)
        s1b = g.integers(0, 1 << 32, 1 << 22, dtype=np.uint64)
        a = np.uint64((0xFFFFFFFF * MULT_INV) & MASK)
        m = np.uint64(MASK)

        def rotl(x, k):
            return ((x << np.uint64(k)) | (x >> np.uint64(32 - k))) & m

        def unstep(a_, b_):
            t = rotl(b_, 19)
            s0 = rotl(a_ ^ t ^ ((t << np.uint64(9)) & m), 6)
            return s0, t ^ s0

        p0, p1 = unstep(np.full(len(s1b), a, np.uint64), s1b)               # the state before the third draw: its output is the second
        u2 = ((p0 * np.uint64(MULT)) & m) >> np.uint64(9)
        z = np.abs(1.0 - 2.0 * u2.astype(np.float64) / (1 << 23))
        idx = np.flatnonzero((z >= 2.0 ** -17 * 1.05) & (z < 2.0 ** -16 * 0.95))
        assert len(idx) >= 4
        made = 0
        mid = sc.a[gi].astype(np.float64) + 0.5 * sc.b[gi].astype(np.float64) + 0.5 * sc.c[gi].astype(np.float64)
        for i in idx[:8]:
            state = rng_unstep(int(p0[i]), int(p1[i]))
            v = _vec(self.orc.lib.orc_random_in_unit_sphere(_state(state)))
            if not (2.0 ** -17 <= abs(float(v[2])) < 2.0 ** -16):
                continue
            for k in (1, 2, 3):
                d = np.array([nextf(-v[0], 1), nextf(-v[1], -1), nextf(v[2], k if v[2] > 0 else -k)], F)      # reflected = (d.x, d.y, -d.z)
                o = mid - 2.0 * d.astype(np.float64)
                self.add("metal_tiny_dir", o, d.astype(np.float64), gi, state, exact_d=True)
            made += 1
            if made == 3:
                break
        assert made >= 2

    def draw_edges(self, cls, o, d, gi, exact_d, low=0, **kw):
        """The case three times: first draw = the largest 23-bit value below the reflectance, the reflectance if representable, the next above."""
        probe = self.add(cls, o, d, gi, (1, 1), exact_d=exact_d, **kw)
        tr = self.trace(probe)
        refl = float(tr["reflectance"])
        self.drop(probe)
        if tr["tir"]:                                                       # no draw there
            return
        k = refl * (1 << 23)
        ks = {int(np.ceil(k)) - 1, int(np.floor(k)) + 1}
        if k == int(k):
            ks.add(int(k))
        for kk in sorted(ks):
            if 0 <= kk < (1 << 23):
                self.add(cls, o, d, gi, state_for_draws(kk / float(1 << 23), 0.5, low=low), exact_d=exact_d, **kw)

    def dielectric(self):
        sc, g = self.sc, self.rng(5)
        one = F(1.0)
        # total reflection: the floats cosv around sqrt(1 - 1/ri^2), on the axis-aligned quads (-dot(normal, d) = |d.axis| exactly)
        for name, front in TIR_FACES:
            gi = sc.geo_of(name, 1)
            param = sc.material(gi)[2]
            with np.errstate(all="ignore"):
                ri = one / param if front else param
                c0 = F(np.sqrt(1.0 - 1.0 / float(ri) ** 2))
                cand = (int(bits(c0)[0]) + np.arange(-4000, 4001)).astype(np.uint32).view(F)
                prod = ri * np.sqrt(one - cand * cand)
            axis = int(np.argmax(np.abs(sc.quad_n[gi])))
            nsign = np.sign(sc.quad_n[gi][axis])
            mid = sc.a[gi].astype(np.float64) + 0.5 * sc.b[gi].astype(np.float64) + 0.5 * sc.c[gi].astype(np.float64)
            for want in (prod[prod > one].min(), one, prod[prod < one].max()):        # the nearest products the floats cosv can give
                sel = np.flatnonzero(prod == want)
                for j in ([sel[0], sel[-1]] if len(sel) > 1 else list(sel)):
                    cosv = float(cand[j])
                    d = np.zeros(3)
                    d[axis] = (-1.0 if front else 1.0) * nsign * cosv                  # front face: against n
                    d[(axis + 1) % 3] = float(F(np.sqrt(1.0 - cosv * cosv)))
                    for u in (0.0, 1.0 - 2.0 ** -23):
                        self.add("dielectric_tir_straddle", mid - 2.0 * d, d, gi, state_for_draws(u, 0.25, low=int(g.integers(0, 1 << 18))), exact_d=True,
                                 remain=1 + j % 2)
        # -dot(normal, d) above 1 before the clamp
        found = 0
        for name in ("die15", "die067", "die10", "die24", "die09"):
            gi = sc.geo_of(name, 0)
            a, r = sc.a[gi].astype(np.float64), abs(float(sc.b[gi, 0]))
            got = 0
            for _ in range(300):
                u = _unit(g.normal(size=3))
                c = self.add("dielectric_cos_above_one", a + g.uniform(1.5, 3.0) * r * u, -u, gi, self.random_state(g))
                if float(self.trace(c)["cos_raw"]) > 1.0:
                    got += 1
                    found += 1
                    if got == 3:
                        break
                else:
                    self.drop(c)
        gi = GEO["rot_die"]
        n = _unit(np.cross(sc.b[gi].astype(np.float64), sc.c[gi].astype(np.float64)))
        for _ in range(200):
            target = sc.a[gi] + g.uniform(0.05, 0.95) * sc.b[gi].astype(np.float64) + g.uniform(0.05, 0.95) * sc.c[gi].astype(np.float64)
            side = g.choice([-1.0, 1.0])
            dirv = _unit(-side * n + 1e-4 * g.normal(size=3))                        # within 1e-4 of the normal: 1 - cos ~ 1e-8, below the rounding
            c = self.add("dielectric_cos_above_one", target - g.uniform(0.5, 2.0) * dirv, dirv, gi, self.random_state(g), need_hit=False)
            if c is not None and float(self.trace(c)["cos_raw"]) > 1.0:
                found += 1
                break
            if c is not None:
                self.drop(c)
        assert found >= 8
        # |d| off 1: Ray::new of a vector whose squared length is a subnormal of one or two bits
        for name in ("die15", "die10", "die067"):
            gi = sc.geo_of(name, 1)
            mid = sc.a[gi].astype(np.float64) + 0.5 * sc.b[gi].astype(np.float64) + 0.5 * sc.c[gi].astype(np.float64)
            for side in (-1.0, 1.0):
                for slant in (0.0, 1.0):
                    for scale in (1.1, 1.3, 1.55, 1.2):
                        tiny = np.array([slant, 0.0, side]) * scale * 2.0 ** (-74.0 - 0.5 * slant)
                        r = self.orc.lib.orc_ray_new(self.orc.Vec3(0, 0, 0), self.orc.Vec3(*[float(F(x)) for x in tiny]))
                        d = _vec(r.direction).astype(np.float64)
                        if not np.isfinite(d).all() or abs(np.linalg.norm(d) - 1.0) < 1e-3:
                            continue
                        self.draw_edges("dielectric_scaled_dir", mid - 2.0 * d, d, gi, True)
                        self.add("dielectric_scaled_dir", mid - 2.0 * d, d, gi, state_for_draws(1.0 - 2.0 ** -23, 0.5), exact_d=True, remain=1)
        # the draw against the reflectance
        gi = sc.geo_of("die10", 1)
        mid = sc.a[gi].astype(np.float64) + 0.5 * sc.b[gi].astype(np.float64) + 0.5 * sc.c[gi].astype(np.float64)
        for side in (-1.0, 1.0):
            d = np.array([float(F(np.sqrt(0.75))), 0.0, side * 0.5])
            self.draw_edges("dielectric_draw_edge", mid - 2.0 * d, d, gi, True, low=int(g.integers(0, 1 << 18)))
        for k in range(16):
            kind_geos = sc.geos_of(DIELECTRIC, k % 2)
            gi = kind_geos[(k // 2) % len(kind_geos)]
            o, d = self.aim(g, gi, k % 4 < 2)
            if self.add("dielectric_draw_edge", o, d, gi, (1, 1), need_hit=False) is None:
                continue
            self.drop(self.cases[-1])
            self.draw_edges("dielectric_draw_edge", o, d, gi, False)
        # grazing
        for name in ("die15", "die067", "die10", "die24", "die09"):
            gi = sc.geo_of(name, 1)
            for want_front in (True, False):
                o, d = self.aim(g, gi, want_front, grazing=10.0 ** -g.integers(2, 6))
                self.add("dielectric_grazing", o, d, gi, self.random_state(g))
        # the large sphere from inside, the negative radius
        for _ in range(4):
            u = _unit(g.normal(size=3))
            self.add("generic_big_inside", (0.0, 0.2, 0.0) + g.uniform(-1, 1, 3) * 0.1, u, GEO["big"], self.random_state(g))

    def front_face(self):
        sc, g = self.sc, self.rng(6)
        self.add("front_face_sphere", (-5.0, 1.0, 0.0), (1, 0, 0), GEO["unit"], self.random_state(g), exact_d=True)      # dot = 0 exactly: back face
        self.add("front_face_sphere", (3.0, 0.0, -1.0), (-1, 0, 0), GEO["unit"], self.random_state(g), exact_d=True)
        count = {-1: 0, 0: 0, 1: 0}
        spheres = [i for i in range(12)] + [GEO["unit"]]
        for k in range(3000):
            gi = spheres[k % len(spheres)]
            a, r = sc.a[gi].astype(np.float64), abs(float(sc.b[gi, 0]))
            d = _unit(g.normal(size=3))
            o = a + r * (1.0 - g.choice([0.0, 1e-7, 3e-7, 1e-6])) * _perp(d, g) - d * g.uniform(2.0, 6.0)
            c = self.add("front_face_sphere", o, d, gi, self.random_state(g), need_hit=False)
            if c is None:
                continue
            ff = float(self.trace(c)["front_dot"])
            sgn = int(np.sign(ff))
            if abs(ff) > 4e-7 * r or count[sgn] >= 8:
                self.drop(c)
                continue
            count[sgn] += 1
            if min(count.values()) >= 8:
                break
        assert count[-1] >= 4 and count[1] >= 4, count
        count = {-1: 0, 1: 0}
        quads = [i for i in range(12, 24)] + [GEO["rot_die"]]
        for k in range(3000):
            gi = quads[k % len(quads)]
            n = sc.quad_n[gi].astype(np.float64)
            nl = np.linalg.norm(n)
            dirv = _unit(_perp(n / nl, g) + (n / nl) * g.choice([-1.0, 1.0]) * g.choice([3e-7, 6e-7, 1.2e-6]))
            target = sc.a[gi] + g.uniform(0.2, 0.8) * sc.b[gi].astype(np.float64) + g.uniform(0.2, 0.8) * sc.c[gi].astype(np.float64)
            c = self.add("front_face_quad", target - dirv * g.uniform(0.5, 2.0), dirv, gi, self.random_state(g), need_hit=False)
            if c is None:
                continue
            ff = float(self.trace(c)["front_dot"])
            sgn = int(np.sign(ff))
            if sgn == 0 or abs(ff) > 2e-6 * nl or count[sgn] >= 8:
                self.drop(c)
                continue
            count[sgn] += 1
            if min(count.values()) >= 8:
                break
        assert count[-1] >= 4 and count[1] >= 4, count
        got = 0
        for k in range(200):
            gi = k % 12
            a, r = sc.a[gi].astype(np.float64), abs(float(sc.b[gi, 0]))
            d = _unit(g.normal(size=3))
            o = a + r * g.uniform(0.0, 0.9) * _perp(d, g) - d * 1.0e6
            if self.add("front_face_far", o, d, gi, self.random_state(g), need_hit=False) is not None:
                got += 1
                if got == 8:
                    break
        assert got >= 4

    def extreme_quads(self):
        """The tiny (|n| ~ 1e-12, metal) and the huge (|n| ~ 1e12, Lambertian) quad: the host's precomputed n.normalized() and the
        un-normalised dot(d, n) < 0 at those magnitudes - both faces at ordinary incidence (a grazing ray cannot be aimed at a quad
        of 1e-6: t = x / dot(d, n) loses it), and the huge quad also with dot(d, n) / |n| within 2e-6 of 0 on both sides."""
        sc, g = self.sc, self.rng(8)
        for gi in (GEO["tiny"], GEO["huge"]):
            for want_front in (True, False):
                got = 0
                for _ in range(200):
                    o, d = self.aim(g, gi, want_front)
                    c = self.add("extreme_quad", o, d, gi, self.random_state(g), remain=1 + got % 2, need_hit=False)
                    if c is None:
                        continue
                    if c["front"] != want_front or not np.isfinite(self.trace(c)["dir"]).all():
                        self.drop(c)
                        continue
                    got += 1
                    if got == 6:
                        break
                assert got >= 4, (gi, want_front, got)
        gi = GEO["huge"]
        n = sc.quad_n[gi].astype(np.float64)
        nl = np.linalg.norm(n)
        count = {-1: 0, 1: 0}
        for _ in range(2000):
            dirv = _unit(_perp(n / nl, g) + (n / nl) * g.choice([-1.0, 1.0]) * g.choice([3e-7, 6e-7, 1.2e-6]))
            target = sc.a[gi] + g.uniform(0.4, 0.6) * sc.b[gi].astype(np.float64) + g.uniform(0.4, 0.6) * sc.c[gi].astype(np.float64)
            c = self.add("extreme_quad_grazing", target - dirv * g.uniform(0.5, 2.0), dirv, gi, self.random_state(g), need_hit=False)
            if c is None:
                continue
            ff = float(self.trace(c)["front_dot"])
            sgn = int(np.sign(ff))
            if sgn == 0 or abs(ff) > 2e-6 * nl or count[sgn] >= 6:
                self.drop(c)
                continue
            count[sgn] += 1
            if min(count.values()) >= 6:
                break
        assert count[-1] >= 3 and count[1] >= 3, count

    def light_and_miss(self):
        sc, g = self.sc, self.rng(7)
        for k in range(8):
            gi = sc.geo_of("light", k % 2)
            o, d = self.aim(g, gi, k % 4 < 2)
            color = (0, 0, 0) if k < 4 else tuple(g.uniform(0, 3, 3))
            atten = [(1, 1, 1), (0.5, 0.25, 1e-20), tuple(g.uniform(0, 1, 3)), (np.inf, 0.0, 2.0) if sc.name == "hot" else (1e-30, 1.0, 0.0)][k % 4]
            self.add("light", o, d, gi, self.random_state(g), color=color, atten=atten, remain=1 + k % 2, need_hit=False)
        backgrounds = [(0, 0, 0), (0.5, 0.7, 1.0), (1e30, 1e-30, 2.0), (-0.0, 1.0, 3.0)]
        for k in range(16):
            atten = [(1, 1, 1), (1e-3, 0.5, 1e-38), tuple(g.uniform(0, 1, 3)), (np.inf, 0.0, 1e30) if sc.name == "hot" else (0.0, -0.0, 1.0)][k % 4]
            color = (0, 0, 0) if k < 12 else tuple(g.uniform(0, 3, 3))
            self.add("miss", g.uniform(-3, 3, 3), g.normal(size=3), -1, self.random_state(g), color=color, atten=atten, remain=1 + k % 3, bg=backgrounds[k // 4 if k < 12 else k % 4])

    def all(self):
        self.generic()
        self.lambertian()
        self.metal()
        self.dielectric()
        self.front_face()
        self.extreme_quads()
        self.light_and_miss()
        return self.cases


def case_list(orc, sc):
    return CaseMaker(orc, sc).all()


def expectations(orc, sc, cases):
    return np.stack([expectation(orc, sc, c) for c in cases])


SHADE_KIND_MISS = 0xFFFFFFFF
INFO_UNSET = 0x5EEDC0DE                  # what the harness puts into ShadeInfo::kind and ::normal before the call


def info_expectation(orc, sc, case, hide_light):
    """shade_hit_info (rt_path.h, the next-event queries' forwarder): the 16 words of expectation(), then info.kind and info.normal -
    the material kind and the oracle's hit-record normal, or SHADE_KIND_MISS and the untouched normal on a miss.  With hide_light a
    light's emission is Vec3::zero(): colour = colour + attenuation * 0 in the body's operation order; nothing else moves."""
    w = expectation(orc, sc, case)
    if case["geo"] < 0:
        return np.concatenate([w, np.array([SHADE_KIND_MISS] + [INFO_UNSET] * 3, np.uint32)])
    kind = sc.material(case["geo"])[0]
    if hide_light and kind == LIGHT:
        with np.errstate(all="ignore"):
            w[6:9] = bits(case["color"] + case["atten"] * np.zeros(3, F))
    rec = sc.hit(orc, case["geo"], case["o"], case["d"])
    return np.concatenate([w, np.array([kind], np.uint32), bits(_vec(rec.normal))])


def info_expectations(orc, sc, cases, hide_light):
    return np.stack([info_expectation(orc, sc, c, hide_light) for c in cases])


def kind_of_case(sc, c):
    """Material kind of the case's primitive (-1: miss)."""
    return -1 if c["geo"] < 0 else int(sc.material(c["geo"])[0])


# ------------------------------------------------------------------------------------------------------------------
# the harness's files
# ------------------------------------------------------------------------------------------------------------------
def wave_lists(n, seed=SEED):
    """(case index per file position, tasks (begin, count)): the whole list in one shuffle - the lanes of a wave hold whatever kinds the
    shuffle deals them - then lists of 1, 63, 64 and 65 cases from a second shuffle; every case appears at least twice."""
    g = np.random.default_rng([seed, 88])
    order = [g.permutation(n)]
    tasks = [(0, n)]
    second = g.permutation(n)
    pos, k = 0, 0
    while pos < n:
        m = min(LIST_LENGTHS[k % len(LIST_LENGTHS)], n - pos)
        tasks.append((n + pos, m))
        pos += m
        k += 1
    order.append(second)
    return np.concatenate(order), np.array(tasks, np.uint32)


def case_words(sc, c):
    w = np.zeros(CASE_WORDS, np.uint32)
    w[0:3], w[3:6], w[6:9], w[9:12] = bits(c["o"]), bits(c["d"]), bits(c["color"]), bits(c["atten"])
    w[12], w[13], w[14] = c["remain"], c["rng"][0], c["rng"][1]
    w[15] = 0xFFFFFFFF if c["geo"] < 0 else sc.prim[c["geo"]]
    w[16] = bits(c["t"])[0]
    w[17:20] = bits(c["bg"])
    w[21] = 1 if c["lazy_ok"] else 0
    return w


def write_case_file(path, sc, cases, order, tasks):
    words = np.stack([case_words(sc, c) for c in cases])[order]
    with open(path, "wb") as f:
        f.write(struct.pack("<III", 0x31434853, len(words), len(tasks)))
        f.write(words.tobytes())
        f.write(np.ascontiguousarray(tasks, np.uint32).tobytes())


def write_scene_file(path, desc):
    import walk_ray_cases as W
    W.write_scene_file(path, file_description(desc))


def moved_indices(desc, k=1):
    """The description with every dielectric index moved k floats up (the GPU test's negative control)."""
    return dict(desc, materials=[(n, kd, a, float(nextf(p, k)) if kd == DIELECTRIC else p) for n, kd, a, p in desc["materials"]])


# ------------------------------------------------------------------------------------------------------------------
# vector operations
# ------------------------------------------------------------------------------------------------------------------
def vector_cases(seed=SEED):
    """float32 [n, 7]: a, b, s - for normalized(a), ray_new(b, a), reflect(a, b), refract(a, b, s), near_zero(a), ray_at(Ray{a, b}, s)."""
    g = np.random.default_rng([seed, 99])
    sub = np.array([1e-40], np.float64).astype(F)[0]
    edge = [LO, nextf(LO, -1), nextf(LO, 1), HI, nextf(HI, -1), nextf(HI, 1), F(0.0), F(-0.0), sub, F(np.inf), F(np.nan), -LO, -nextf(HI, 1)]
    a = [[x, y, z] for x in edge for y in edge for z in edge]
    a += [[HI, LO, LO], [HI, HI, HI], [LO, LO, LO], [nextf(LO, -1), HI, F(1.0)], [F(1e-7), F(9.9999994e-8), F(-1e-7)], [F(9.9999994e-8)] * 3,
          [F(1e-8), F(-9e-8), F(0.0)], [F(1.0000001e-7), F(0.0), F(0.0)]]
    a = np.array(a, F)
    n_rand = 4096
    mant = g.uniform(1.0, 2.0, (n_rand, 3)) * g.choice([-1.0, 1.0], (n_rand, 3))
    rand = (mant * 2.0 ** g.integers(-45, 46, (n_rand, 3))).astype(F)
    rand[::7] = (mant[::7] * 2.0 ** g.integers(-41, -37, (len(mant[::7]), 3))).astype(F)          # around the lower switch
    rand[3::7] = (mant[3::7] * 2.0 ** g.integers(37, 41, (len(mant[3::7]), 3))).astype(F)         # around the upper switch
    unit = g.normal(size=(n_rand // 2, 3))
    unit = (unit / np.linalg.norm(unit, axis=1, keepdims=True)).astype(F)                         # what reflect / refract see
    a = np.concatenate([a, rand, unit])
    n = len(a)
    bn = g.normal(size=(n, 3))
    b = (bn / np.linalg.norm(bn, axis=1, keepdims=True)).astype(F)
    b[::5] = a[g.permutation(n)][::5]                                                              # edge values as the second operand too
    s = g.choice(np.array([1.5, 1.0 / 1.5, 1.0, 2.4, 0.9, 0.0, 1e6, 1e-3, -2.0], np.float64), n).astype(F)
    s[::11] = np.resize(np.array(edge, F), len(s[::11]))
    return np.concatenate([a, b, s[:, None]], axis=1).astype(F)


def vector_expectation(orc, vc):
    """uint32 [n, 20] from orc_ray_new, orc_vec3_reflect / refract, orc_vec3_eq against 0 (the tolerant PartialEq IS near_zero of the
    difference, a - 0 = a for every float, and its special case - both components +inf - cannot apply against 0), orc_ray_at."""
    L = orc.lib
    out = np.zeros((len(vc), VEC_OUT_WORDS), np.uint32)
    V = lambda v: orc.Vec3(*[float(x) for x in v])
    zero = orc.Vec3(0.0, 0.0, 0.0)
    for i, row in enumerate(vc):
        a, b, s = row[0:3], row[3:6], float(row[6])
        va, vb = V(a), V(b)
        # (a NaN passes through ctypes' float -> double -> float with its payload kept on x86-64; the comparison treats NaN words by class)
        out[i, 0:3] = np.frombuffer(bytes(L.orc_ray_new(zero, va)), np.uint32)[3:6]
        out[i, 3:9] = np.frombuffer(bytes(L.orc_ray_new(vb, va)), np.uint32)
        out[i, 9:12] = np.frombuffer(bytes(L.orc_vec3_reflect(va, vb)), np.uint32)
        out[i, 12:15] = np.frombuffer(bytes(L.orc_vec3_refract(va, vb, s)), np.uint32)
        out[i, 15] = 1 if L.orc_vec3_eq(va, zero) else 0
        ray = orc.Ray(va, vb)
        out[i, 16:19] = np.frombuffer(bytes(L.orc_ray_at(C.byref(ray), s)), np.uint32)
    return out


def write_vector_file(path, vc):
    with open(path, "wb") as f:
        f.write(struct.pack("<II", 0x31564853, len(vc)))
        f.write(np.ascontiguousarray(vc, F).tobytes())


VEC_FLOAT_WORDS = (np.arange(VEC_OUT_WORDS) < 19) & (np.arange(VEC_OUT_WORDS) != 15)


def differing_words(got, want, float_words):
    """(words that differ - float words that are NaN on both sides excepted -, float words that are NaN on both sides with different
    bits): boolean arrays of got's shape.  float_words: which words of a record are floats."""
    got, want = np.asarray(got, np.uint32), np.asarray(want, np.uint32)
    nan = lambda w: (w & 0x7FFFFFFF) > 0x7F800000
    both_nan = nan(got) & nan(want) & float_words
    return (got != want) & ~both_nan, (got != want) & both_nan
