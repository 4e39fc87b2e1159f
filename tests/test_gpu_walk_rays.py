"""Every production walk, ray by ray, against the oracle's closest hit: (hit?, t bits, primitive) for chosen rays - no tolerance.

tests/native/walk_rays.hip (built here for gfx950 with the library's own CXXFLAGS, once with the hand-written box loops and once with
-DTRT_ASM_BOX_LOOP=0) runs the rays of tests/walk_ray_cases.py through one small kernel per walk variant: walk_flat (reuse masks on /
all zero; 2, 7, 16 slots), the resumable walk_fast_lds (2, 5, 16 slots x 0, 1, 8, 63 stragglers), the resumable walk_compact and the
two-rays-per-lane walk_compact2 (2, 4 slots x 0, 8 stragglers), walk_fast with register slots (WALK_REGS; WALK_RUNTIME with 1 / 2 / 4),
the run-time choice of each LDS-stack walk, and closest_hit_ref on the reference tree - whichever of them the scene has.  The wave lists
mix the ray classes (fast, exact-path and NaN rays in one wave), refill a wave three times so that parked stragglers resume beside fresh
rays, come in lengths that are no multiple of 64, and fill whole waves with one ray; every copy of a ray must get the oracle's answer.
The fast / ref flags the harness reports must equal the host's prediction, so the production loops - not the reference-tree fallback -
produced the answers they are credited with.

Measured on an MI355X (seed 1):
  * rays / wave lists per scene: 3846-5318 rays in 30-39 lists (192 per class; each ray also in a shuffle of all classes and every second one
    in a second shuffle cut into ragged lists, both with a NaN ray, another special ray and an axis-parallel ray dealt in after every 30
    rays; one ray per class 64 times).  Walk variants per build: 25 on scenes of at most 32 primitives (6 lock-step, 12 LDS tree, 4 register,
    2 run-time, reference tree), 18 on larger LDS-resident scenes, 14 on scenes with 16-byte nodes (4 + 4 one / two rays per lane, 4
    register, 1 run-time, reference tree): 15 scenes x 2 builds, 2.80 million answers.
  * before the special rays were dealt into the mixed lists (3633-5021 rays per scene, 2.64 million answers, one harness process per scene
    and build): 0 mismatches; control (i), every reuse bit set on Cornell: 1237 of 3903 rays differ from the oracle; control (ii), the root
    box as every leaf box on sphere_grid(3000): 143 of the 192 far_sliver rays differ (436 of 4721 rays in all); this file 17.5 s, the whole
    `-m gpu` suite with it 128.5 s (282 tests), so 111 s without it: 16 %, above the tenth the issue allows.  Ray counts are not what it
    costs: building the harness twice took 5.5-12 s and starting 30 processes most of the rest, the kernels themselves well under a
    second.  The file therefore now builds the two harnesses side by side and runs all scenes in one process per build.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import walk_ray_cases as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tiny-raytracer_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def library_cxxflags():
    """CXXFLAGS of the library's Makefile: the harness is built with the flags the walks are built with."""
    with open(os.path.join(CSRC, "Makefile")) as f:
        m = re.search(r"^CXXFLAGS\s*\?=\s*(.+)$", f.read(), re.M)
    assert m, "CXXFLAGS not found in the library's Makefile"
    flags = m.group(1).split()
    assert "-ffp-contract=off" in flags and "-O3" in flags, flags
    return flags


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """{'asm': exe, 'cxx': exe}: the two builds, compiled side by side."""
    out = tmp_path_factory.mktemp("walk_rays")
    exes, procs = {}, []
    for tag, extra in (("asm", []), ("cxx", ["-DTRT_ASM_BOX_LOOP=0"])):
        exes[tag] = str(out / ("walk_rays_" + tag))
        procs.append(subprocess.Popen([HIPCC, "--offload-arch=gfx950", *library_cxxflags(), *extra, "-I", CSRC, "-o", exes[tag],
                                       os.path.join(ROOT, "tests", "native", "walk_rays.hip"), os.path.join(CSRC, "scene_host.cpp")]))
    codes = [p.wait(timeout=900) for p in procs]                          # both, before anything is asserted
    assert codes == [0, 0], "the harness does not compile"
    return exes


def expected_variants(flat, lds, compact, controls):
    v = []
    if flat:
        v += [f"flat_s{s}_reuse{r}" for r in (1, 0) for s in (2, 7, 16)]
    if lds:
        v += [f"lds_s{s}_strag{k}" for s in (2, 5, 16) for k in (0, 1, 8, 63)]
    if compact:
        v += [f"{w}_s{s}_strag{k}" for s in (2, 4) for k in (0, 8) for w in ("compact", "compact2")]
    v += ["regs", "runtime_regs_s1", "runtime_regs_s2", "runtime_regs_s4"]
    v += ["runtime_flat_s7"] if flat else []
    v += ["runtime_lds_s5"] if lds else []
    v += ["runtime_compact_s4"] if compact else []
    v += ["ref_tree"]
    if controls:
        v += ["control_flat_s7_reuse_all_ones"] if flat else []
        v += ["control_compact_s4_root_leaf_boxes"] if compact else []
    return v


@pytest.fixture(scope="module")
def results(trt, orc, harness, tmp_path_factory):
    """Every scene's rays through both builds of the harness - one child process per build, each under its own time limit, a non-zero
    exit fails everything and nothing is run again - compared with the oracle's answers.
    name -> dict(rays, labels, variants: {(build, variant): indices of the rays that differ}, counts, fast_share)."""
    d = tmp_path_factory.mktemp("rays")
    prepared = {}
    for name in W.scene_names():
        desc = W.scene(trt, name)
        ow, _ = orc.world_from_description(desc)
        bbox, prim, _ = ow.bvh_dump()
        sc = trt.world_from_description(desc)[0].get_bvh()
        lds = sc.info()["lds_bytes"] > 0
        compact = sc.compact_nodes() is not None and not lds
        flat = lds and len(desc["geometries"]) <= 32
        limit = W.origin_limit(sc.cull_nodes()[0][0]) if compact else None
        rays, tasks, labels = W.wave_lists(W.RayMaker(desc, bbox, prim, limit=limit).classes())
        hit, t, geo = W.oracle_answers(ow, rays)
        assert not hit[np.isnan(rays).any(axis=1)].any()                      # NaN rays are misses with t = inf
        assert (t.view(np.uint32)[~hit] == 0x7F800000).all() and (geo[~hit] == -1).all()
        W.write_scene_file(str(d / f"{name}.scene"), desc)
        W.write_ray_file(str(d / f"{name}.rays"), rays, tasks)
        prepared[name] = dict(desc=desc, lds=lds, compact=compact, flat=flat, limit=limit, rays=rays, tasks=tasks, labels=np.array(labels),
                              hit=hit, t=t.view(np.uint32), geo=geo)
    out = {name: dict(rays=p["rays"], labels=p["labels"], variants={}, counts={}) for name, p in prepared.items()}
    for build in ("asm", "cxx"):
        controls = build == "asm"
        cmd = [harness[build], "controls" if controls else "plain"]
        for name in prepared:
            cmd += [str(d / f"{name}.scene"), str(d / f"{name}.rays"), str(d / f"{name}.{build}.bin"), str(d / f"{name}.{build}.txt")]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and " 0 unanswered" in r.stdout, (build, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        for name, p in prepared.items():
            rays, desc = p["rays"], p["desc"]
            with open(d / f"{name}.{build}.txt") as f:
                lines = f.read().split("\n")
            layout = dict(kv.split("=") for kv in lines[0].split()[1:])
            variants = [l.split()[1] for l in lines[1:] if l.startswith("variant ")]
            assert variants == expected_variants(p["flat"], p["lds"], p["compact"], controls), (name, build, variants)
            assert int(layout["asm"]) == (1 if build == "asm" else 0)
            all_finite = int(layout["all_finite"]) != 0
            host_limit = np.array([int(x, 16) for x in layout["limit"].split(",")], np.uint32).view(np.float32)
            if p["compact"]:
                assert np.array_equal(host_limit.view(np.uint32), p["limit"].view(np.uint32)), (host_limit, p["limit"])
            words = np.fromfile(d / f"{name}.{build}.bin", np.uint32).reshape(len(variants), len(rays), 3)
            for k, v in enumerate(variants):
                got_geo = W.prim_to_geometry(desc, words[k, :, 0])
                bad = (got_geo != p["geo"]) | (words[k, :, 1] != p["t"]) | ((words[k, :, 0] != 0xFFFFFFFF) != p["hit"])
                out[name]["variants"][(build, v)] = np.flatnonzero(bad)
                # the flags trav_begin gave each ray against the host's prediction (the resumable 16-byte-node walks always check the
                # fused loop's domain, the run-time choice only where the hand-written loop exists)
                domain = v.startswith("compact") or v.startswith("control_compact") or (v == "runtime_compact_s4" and build == "asm")
                fast = W.predict_flags(rays, all_finite, host_limit if domain else None)
                ref = ~fast | (v == "ref_tree")
                flags = fast.astype(np.uint32) | (ref.astype(np.uint32) << 1)
                out[name]["variants"][(build, v, "flags")] = np.flatnonzero(words[k, :, 2] != flags)
            out[name]["counts"][build] = (len(rays), len(p["tasks"]), len(variants))
            out[name]["fast_share"] = float(W.predict_flags(rays, all_finite, host_limit if p["compact"] else None).mean())
    return out


@pytest.mark.parametrize("name", W.scene_names())
def test_every_walk_gives_the_oracles_hit_for_every_ray(results, name):
    res = results[name]
    n_bad = {k: len(v) for k, v in res["variants"].items() if not k[1].startswith("control_")}
    print(f"\n{name}: {res['counts']} (rays, wave lists, variants) per build, share of rays on the production loops {res['fast_share']:.2f}, "
          f"mismatches {sum(n_bad.values())}")
    for key, bad in res["variants"].items():
        build, v = key[0], key[1]
        if len(key) == 3:
            assert len(bad) == 0, (name, build, v, "fast / ref flags differ from the host's prediction", bad[:5], res["rays"][bad[:5]])
            continue
        if v.startswith("control_"):
            continue
        assert len(bad) == 0, (name, build, v, f"{len(bad)} of {len(res['rays'])} rays differ from the oracle", bad[:5], res["labels"][bad[:5]],
                               res["rays"][bad[:5]])
    assert 0.0 < res["fast_share"] < 1.0 or name == "nonfinite"               # the lists mix fast and exact-path rays (a non-finite scene has no fast ray)


def test_control_all_reuse_bits_set_is_seen(results):
    """Negative control (i): the lock-step walk on Cornell with every reuse bit set keeps intervals it must compute - wrong answers."""
    res = results["cornell"]
    bad = res["variants"][("asm", "control_flat_s7_reuse_all_ones")]
    print("\ncontrol (i): all reuse bits set on Cornell:", len(bad), "of", len(res["rays"]), "rays differ from the oracle")
    assert len(bad) >= 1


def test_control_root_box_as_leaf_boxes_is_seen_by_the_far_slivers(results):
    """Negative control (ii): walk_compact on sphere_grid(3000) with the leaf-list boxes replaced by the root box - the exact leaf-box re-test
    then lets everything through - takes the sphere test's false hits: mismatches on far_sliver."""
    res = results["grid3000"]
    bad = res["variants"][("asm", "control_compact_s4_root_leaf_boxes")]
    labels = res["labels"]
    sliver = np.flatnonzero(labels == "a:far_sliver")
    n = int(np.isin(sliver, bad).sum())
    print("\ncontrol (ii): root box as every leaf box on sphere_grid(3000):", n, "of", len(sliver), "far_sliver rays differ,", len(bad), "of",
          len(labels), "rays in all")
    assert n >= 1
