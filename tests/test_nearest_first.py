"""The nearest-first leaf phase (tiny-raytracer_amd/csrc/nearest_first.h) without a GPU.

tests/native/nearest_first_check.c replays the phase against the walk-order phase it replaces on the CPU oracle - the header's own margin,
host derivation and decision procedure - on 2 M rays per scene: same (t bits, primitive) in every phase, the margin's headroom, and how
rare the two cold paths are on Cornell's path distribution.  The host derivation (P per axis, the switch) is compiled with g++ and
checked against numpy.  The scenes of this file are the GPU test's too (tests/test_gpu_nearest_first.py)."""
import os
import re
import subprocess

import numpy as np
import pytest
from test_gpu_flat_reuse import SCENES as REUSE_SCENES, _scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tiny-raytracer_amd", "csrc")
ODIR = os.path.join(ROOT, "oracle")
COLD_RAYS = os.path.join(ROOT, "tests", "golden", "nearest_first_cold_rays.txt")
RAYS = 2_000_000


def _room(trt, lo, hi, light_inset=3.0):
    """A closed room of six quads with a light COPLANAR with its ceiling."""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    dx, dy, dz = (x1 - x0, 0.0, 0.0), (0.0, y1 - y0, 0.0), (0.0, 0.0, z1 - z0)
    geos = [("quad", (x0, y0, z0), dx, dz, "white"), ("quad", (x0, y1, z0), dx, dz, "white"), ("quad", (x0, y0, z0), dy, dz, "red"),
            ("quad", (x1, y0, z0), dy, dz, "white"), ("quad", (x0, y0, z1), dx, dy, "white"), ("quad", (x0, y0, z0), dx, dy, "white")]
    i = light_inset
    geos.append(("quad", (x0 + i, y1, z0 + i), (x1 - x0 - 2 * i, 0.0, 0.0), (0.0, 0.0, z1 - z0 - 2 * i), "light"))
    return geos


def _camera(position, look_at, w, h, fov=70.0):
    return dict(focus_distance=10.0, defocus_angle=0.0, position=position, look_at=look_at, up=(0.0, 1.0, 0.0), vertical_fov=fov, width=w, height=h)


def coincident_quads(trt, w=88, h=80):
    """Duplicated coincident quads of different materials inside a room: exact ties in t, decided by walk order."""
    geos = _room(trt, (-10.0, -10.0, -10.0), (10.0, 10.0, 10.0))
    for mat in ("red", "metal", "white"):
        geos.append(("quad", (-4.0, -4.0, 3.0), (8.0, 0.0, 0.0), (0.0, 8.0, 0.0), mat))                  # three copies of a panel
    for mat in ("glass", "red"):
        geos.append(("quad", (-6.0, -3.0, -2.0), (0.0, 6.0, 0.0), (0.0, 0.0, 6.0), mat))                # two of another, other axis
    geos.append(("quad", (-10.0, -10.0, -10.0), (20.0, 0.0, 0.0), (0.0, 0.0, 20.0), "metal"))           # and a second floor
    return _scene(trt, "coincident_quads", geos, _camera((7.0, 2.0, -8.5), (-2.0, -1.0, 3.0), w, h))


def box_on_floor(trt, w=96, h=88):
    """A box standing on the floor of a room: its bottom face is coplanar with the floor, its side faces end on it."""
    geos = _room(trt, (-10.0, 0.0, -10.0), (10.0, 20.0, 10.0)) + trt.scenes._box((-3.0, 0.0, -2.0), (4.0, 7.0, 5.0), "white")
    return _scene(trt, "box_on_floor", geos, _camera((7.5, 12.0, -8.5), (0.0, 3.0, 1.0), w, h))


def coplanar_light(trt, w=88, h=88):
    """A light coplanar with the ceiling and nearly as large, and a second one coplanar with a wall."""
    geos = _room(trt, (-8.0, -8.0, -8.0), (8.0, 8.0, 8.0), light_inset=1.0)
    geos.append(("quad", (8.0, -4.0, -4.0), (0.0, 8.0, 0.0), (0.0, 0.0, 8.0), "light"))
    geos.append(("quad", (-3.0, -8.0, -3.0), (6.0, 0.0, 0.0), (0.0, 0.0, 6.0), "metal"))                 # a plate coplanar with the floor
    return _scene(trt, "coplanar_light", geos, _camera((-6.0, 1.0, -6.5), (2.0, 0.0, 2.0), w, h))


def _moved(trt, name, by, w, h):
    desc = box_on_floor(trt, w, h)
    move = lambda p: tuple(float(np.float32(a) + np.float32(b)) for a, b in zip(p, by))
    desc["geometries"] = [("quad", move(g[1]), g[2], g[3], g[4]) for g in desc["geometries"]]
    desc["camera"] = dict(desc["camera"], position=move(desc["camera"]["position"]), look_at=move(desc["camera"]["look_at"]))
    desc["name"] = name
    return desc


def far_room(trt, w=96, h=96):
    """box_on_floor translated so that every plane sits at |coordinate| >= 1024: the reference's 5e-5 box padding rounds away there, a
    quad's box has no thickness, and the reference's slab test (end <= start fails the box) never reaches the quad: an empty frame."""
    return _moved(trt, "far_room", (3072.0, -2048.0, 5120.0), w, h)


def wide_room(trt, w=96, h=96):
    """box_on_floor a hundred times as large, planes up to |coordinate| = 1000: the padding is one ulp of the plane there (6.1e-5) and
    distances reach 2000, whose own rounding is larger - the box entry and the quad's t are a rounding apart either way, so winners with
    start > t, which take the walk-order re-run, do occur."""
    geos = _room(trt, (-1000.0, 0.0, -1000.0), (1000.0, 1000.0, 1000.0), light_inset=300.0) + trt.scenes._box((-300.0, 0.0, -200.0), (400.0, 700.0, 500.0), "white")
    return _scene(trt, "wide_room", geos, _camera((750.0, 600.0, -850.0), (0.0, 300.0, 100.0), w, h))


EXTRA_SCENES = {"coincident_quads": coincident_quads, "box_on_floor": box_on_floor, "coplanar_light": coplanar_light, "far_room": far_room,
                "wide_room": wide_room}
CPU_SCENES = dict(REUSE_SCENES, **EXTRA_SCENES)               # cornell, box_stacks, thin_sheets, signed_zero_planes + the five above


def write_scene_file(trt, desc, path):
    kinds = {m[0]: m[1] for m in desc["materials"]}
    with open(path, "w") as f:
        f.write("%.9g %.9g %.9g\n" % tuple(desc["camera"]["position"]))
        for g in desc["geometries"]:
            assert g[0] == "quad"
            f.write(" ".join("%.9g" % x for v in g[1:4] for x in v) + " %d\n" % (kinds[g[4]] == trt.scenes.LIGHT))


def recorded_cold_rays():
    """tests/golden/nearest_first_cold_rays.txt: scene name -> lines "ox oy oz dx dy dz path" (f32 bit patterns in hex; path 1: the ray
    took the residual loop, 2: the walk-order re-run)."""
    out = {}
    if os.path.exists(COLD_RAYS):
        for line in open(COLD_RAYS).read().splitlines():
            name, rest = line.split(" ", 1)
            out.setdefault(name, []).append(rest)
    return out


LINE = re.compile(r"(\d+) quads (\d+) rays (\d+) phases: mismatches (\d+) oracle_mismatches (\d+) worst_ratio (\S+) second (\S+) rerun (\S+) "
                  r"residual_count (\d+) rerun_count (\d+) out_of_domain (\d+) tests_ref (\S+) tests_nf (\S+) kept (\d+) (\d+)")
KEYS = ("quads", "rays", "phases", "mismatches", "oracle_mismatches", "worst_ratio", "second", "rerun", "residual_count", "rerun_count",
        "out_of_domain", "tests_ref", "tests_nf", "kept_residual", "kept_rerun")


@pytest.fixture(scope="module")
def runs(trt, orc, tmp_path_factory):
    """name -> figures of one run of the check program; all scenes side by side, each run once.  'cornell_paths' is Cornell with the
    path distribution alone; it also replays the recorded cold-path rays of tests/golden."""
    d = tmp_path_factory.mktemp("nearest_first")
    exe = str(d / "nearest_first_check")
    subprocess.run(["g++", "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I" + ODIR, "-I" + CSRC,
                    os.path.join(ROOT, "tests", "native", "nearest_first_check.c"), "-L" + ODIR, "-loracle", "-lm", "-Wl,-rpath," + ODIR, "-o", exe], check=True)
    procs, recorded = {}, recorded_cold_rays()
    for name, make in CPU_SCENES.items():
        write_scene_file(trt, make(trt), d / (name + ".txt"))
        replay = []
        if name in recorded:                                       # the recorded rays of this scene take their recorded path again
            (d / (name + "_recorded.txt")).write_text("\n".join(recorded[name]) + "\n")
            replay = [str(d / (name + "_recorded.txt"))]
        procs[name] = subprocess.Popen([exe, str(d / (name + ".txt")), str(RAYS), "mix", str(d / (name + "_cold.txt"))] + replay, stdout=subprocess.PIPE,
                                       stderr=subprocess.PIPE, text=True)
    procs["cornell_paths"] = subprocess.Popen([exe, str(d / "cornell.txt"), str(RAYS), "paths"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    out = {}
    for name, p in procs.items():
        so, se = p.communicate(timeout=900)
        print(name, so.strip())
        m = LINE.search(so)
        assert m, (name, so, se)
        fig = {k: (float(v) if "." in v or "e" in v or "n" in v else int(v)) for k, v in zip(KEYS, m.groups())}
        fig.update(returncode=p.returncode, stdout=so, stderr=se, cold=str(d / (name + "_cold.txt")))
        out[name] = fig
    return out


@pytest.mark.parametrize("scene", sorted(CPU_SCENES) + ["cornell_paths"])
def test_every_phase_gives_the_reference_phases_hit(runs, scene):
    """Assertion 1: (t bits, primitive) of the nearest-first phase are the walk-order phase's, from (+inf, none) and from every carried
    (T0, P0), on at least 2 M rays per scene; and the chained phases give the oracle's closest hit."""
    f = runs[scene]
    assert f["returncode"] == 0, f["stdout"] + f["stderr"]
    assert f["mismatches"] == 0 and f["oracle_mismatches"] == 0
    assert f["rays"] + f["out_of_domain"] >= RAYS and f["out_of_domain"] <= 100
    assert f["phases"] > f["rays"] or scene == "far_room"             # (far_room: no box is ever entered)


@pytest.mark.parametrize("scene", sorted(CPU_SCENES) + ["cornell_paths"])
def test_margin_headroom(runs, scene):
    """Assertion 2: (start - t) / E over all hits of pending leaves stays below 0.25 (the derivation in the header allows 0.54)."""
    assert runs[scene]["worst_ratio"] <= 0.25, runs[scene]["stdout"]


def test_cold_paths_are_rare_on_cornells_paths(runs):
    """Assertion 3: on Cornell's path distribution at most 1 % of the rays test a second leaf and at most 0.1 % re-run the phase."""
    f = runs["cornell_paths"]
    print("second test %.3e of rays, re-run %.3e" % (f["second"], f["rerun"]))
    assert f["second"] <= 0.01
    assert f["rerun"] <= 0.001
    assert f["tests_nf"] < f["tests_ref"]


def test_both_cold_paths_occur(runs):
    """Assertion 4: the residual loop and the walk-order re-run each ran at least 100 times, so assertion 1 covers them."""
    assert sum(f["residual_count"] for f in runs.values()) >= 100
    assert sum(f["rerun_count"] for f in runs.values()) >= 100
    assert runs["cornell"]["stdout"].startswith("replayed 64 recorded rays") and runs["wide_room"]["stdout"].startswith("replayed 64 recorded rays")


def test_recorded_cold_rays_are_what_the_program_records(runs):
    """tests/golden/nearest_first_cold_rays.txt (the GPU test's rays): 64 rays that took the residual loop on Cornell and 64 that
    took the re-run on wide_room, as the program writes them."""
    want = ["cornell " + l for l in open(runs["cornell"]["cold"]).read().splitlines() if l.endswith(" 1")]
    want += ["wide_room " + l for l in open(runs["wide_room"]["cold"]).read().splitlines() if l.endswith(" 2")]
    assert len(want) == 128
    assert open(COLD_RAYS).read().splitlines() == want


# ---------------------------------------------------------------------------------------------------------------------------------
# the host derivation: P per axis and the switch
DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "nearest_first.h"
static std::vector<unsigned char> slurp(const char* path) {
    std::vector<unsigned char> b;
    if (FILE* f = fopen(path, "rb")) { int c; while ((c = fgetc(f)) != EOF) b.push_back((unsigned char)c); fclose(f); }
    return b;
}
int main(int, char** argv) {   // leaf list, quad records, n_spheres, enabled
    const std::vector<unsigned char> leaves = slurp(argv[1]), quads = slurp(argv[2]);
    const uint32_t nl = (uint32_t)(leaves.size() / 32u), nq = (uint32_t)(quads.size() / 80u);
    const uint32_t aq = trt::axis_quads_flag(nq ? quads.data() : nullptr, nq, nl, true, true, true);
    float P[3];
    const uint32_t nf = trt::nearest_first_flag(leaves.data(), nl, nq ? quads.data() : nullptr, nq, (uint32_t)atoi(argv[3]), aq, atoi(argv[4]) != 0, P);
    printf("%u %u %a %a %a\n", aq, nf, P[0], P[1], P[2]);
    return 0;
}
"""


@pytest.fixture(scope="module")
def flag_of(trt, tmp_path_factory):
    d = tmp_path_factory.mktemp("nearest_first_flag")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, str(src), "-o", str(exe)], check=True)
    count = [0]

    def run(desc, enabled=True, shift=None):
        """(axis_quads, nearest_first, P, numpy's P) for a scene description; quads only are packed (spheres become non-quad leaves)."""
        s = trt.Scene(trt.world_from_description(desc)[0])
        box, prim, _ = s.nodes()
        leaves, order = np.array(box[prim >= 0], np.float32), prim[prim >= 0]
        if shift is not None:
            leaves = leaves + np.float32(shift)
        geos = desc["geometries"]
        quad_index, recs = {}, []
        f32 = lambda v: np.asarray(v, np.float32)
        for i, g in enumerate(geos):
            if g[0] != "quad":
                continue
            quad_index[i] = len(recs)
            c, u, v = f32(g[1]), f32(g[2]), f32(g[3])
            if shift is not None:
                c = c + np.float32(shift)
            n = np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]], np.float32)
            nn = np.float32(np.float32(n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
            dd = np.float32(np.float32(n[0] * c[0] + n[1] * c[1]) + n[2] * c[2])
            recs.append(np.concatenate([n, [dd], c, [0.0], v, n / nn, u, n / np.sqrt(nn)]).astype(np.float32))
        words = np.zeros((len(leaves), 8), np.uint32)
        words[:, :6] = leaves.view(np.uint32)
        words[:, 6] = np.arange(1, len(leaves) + 1)
        words[:, 7] = [quad_index[int(i)] | 0x40000000 if int(i) in quad_index else 0 for i in order]
        count[0] += 1
        fl, fq = d / ("leaves%d.bin" % count[0]), d / ("quads%d.bin" % count[0])
        fl.write_bytes(words.tobytes())
        fq.write_bytes(np.asarray(recs, np.float32).tobytes() if recs else b"")
        out = subprocess.run([str(exe), str(fl), str(fq), str(len(geos) - len(recs)), "1" if enabled else "0"], capture_output=True, text=True, check=True).stdout.split()
        p_numpy = np.maximum(np.abs(leaves).reshape(-1, 2, 3).max(axis=(0, 1)), np.float32(2.0 ** -32))
        return int(out[0]), int(out[1]), np.array([float.fromhex(x) for x in out[2:5]], np.float32), p_numpy
    return run


@pytest.mark.parametrize("scene", sorted(CPU_SCENES))
def test_plane_maximum_is_numpys_and_the_switch_is_on(trt, flag_of, scene):
    aq, nf, p, p_numpy = flag_of(CPU_SCENES[scene](trt))
    assert (aq, nf) == (1, 1)
    assert np.array_equal(p, p_numpy)


def test_switch_is_off_with_a_sphere_a_rotated_quad_far_planes_or_the_environment(trt, flag_of):
    from test_gpu_axis_quads import box_stacks_rotated
    desc = REUSE_SCENES["box_stacks"](trt)
    assert flag_of(desc)[:2] == (1, 1)
    with_sphere = dict(desc, geometries=desc["geometries"] + [("sphere", (5.0, 35.0, 5.0), 2.0, "metal")])
    assert flag_of(with_sphere)[:2] == (1, 0)                          # every QUAD is axis-exact, but the scene has a sphere
    assert flag_of(box_stacks_rotated(trt))[:2] == (0, 0)
    aq, nf, p, p_numpy = flag_of(desc, shift=2.0 ** 20)                # P > 2^20
    assert (aq, nf) == (1, 0) and np.array_equal(p, p_numpy) and p.max() > 2.0 ** 20
    assert flag_of(desc, shift=2.0 ** 19)[:2] == (1, 1)
    assert flag_of(desc, enabled=False)[:2] == (1, 0)                  # TRT_NEAREST_FIRST=0


def test_environment_switch_is_read_with_the_other_defaults():
    src = open(os.path.join(CSRC, "capi.hip")).read()
    assert 'env("TRT_NEAREST_FIRST")' in src and "defaults().nearest_first" in src
