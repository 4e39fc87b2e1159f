"""The inputs of the ray-level walk test (tests/walk_ray_cases.py, run on the GPU by tests/test_gpu_walk_rays.py) checked on the CPU: the
generator is deterministic, the oracle's orc_world_hit_index is pinned to orc_world_hit and to the primitive tests, and the rays are
not vacuous - conditions on the reference and on the host-side scene alone.

Measured (seed 1; the lists of the GPU test, 192 rays per class and scene; the far_sliver conditions on 2000 rays of L = 1000):
  * oracle hit share per (scene, class) except `special`: smallest 0.27 (nonfinite, far_sliver), then 0.34 (thin_sheets, near_axis_parallel),
    0.35 (degenerate, far_sliver; nonfinite, at_corners), 0.36 (thin_sheets, on_plane_axis_parallel); the bound is 0.25.
  * far_sliver: the aimed-at sphere's own test hits while its box misses for 0.91 (random_spheres) and 0.93 (sphere_grid(3000)) of the
    rays; BVH and brute force disagree on 0.97 and 0.99.  On Cornell they never disagree (0 of 1356 rays of all classes).
  * sphere_grid(3000), far_sliver: 1.00 of the rays pass the grown f16 leaf node of the aimed-at sphere (fused slab arithmetic, replayed)
    while failing its exact f32 box - the rays for which walk_compact's exact leaf-box re-test alone keeps the false hit out - and all of
    them are inside the fused loop's domain.
  * COMPACT_DOMAIN check on sphere_grid(3000): origin_limit 0.41 inside / 0.59 outside, near_axis_parallel 0.19 inside / 0.81 outside.
  * ties: the `degenerate` scene's twin spheres (geometries 16, 17) and the `signed_zero_planes` scene's twin quads (0, 1: the same quad
    written with +0 and -0) get 6 and 2 of the 8 rays aimed at each pair (something nearer takes the others), always through the first of the pair in leaf order.
"""
import ctypes as C

import numpy as np
import pytest

import walk_ray_cases as W

MIN_HIT_SHARE = 0.25


@pytest.fixture(scope="module")
def cases(trt, orc):
    """name -> (desc, oracle world, RayMaker, classes), built once."""
    out = {}
    for name in W.scene_names():
        desc = W.scene(trt, name)
        ow, _ = orc.world_from_description(desc)
        bbox, prim, _ = ow.bvh_dump()
        sc = trt.world_from_description(desc)[0].get_bvh()
        limit = W.origin_limit(sc.cull_nodes()[0][0]) if sc.compact_nodes() is not None else None
        mk = W.RayMaker(desc, bbox, prim, limit=limit)
        out[name] = (desc, ow, mk, mk.classes(), sc)
    return out


def _ray(orc, r):
    return orc.Ray(orc.Vec3(*r[:3]), orc.Vec3(*r[3:]))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_generator_is_deterministic_and_the_lists_cover_every_ray(cases, orc):
    for name, (desc, ow, mk, classes, _) in cases.items():
        bbox, prim, _ = ow.bvh_dump()
        again = W.RayMaker(desc, bbox, prim, limit=mk.limit).classes()
        assert list(again) == list(classes)
        for k in classes:
            assert classes[k].dtype == np.float32 and classes[k].shape[1] == 6 and len(classes[k]) > 0, (name, k)
            assert np.array_equal(_bits(classes[k]), _bits(again[k])), (name, k)
        rays, tasks, labels = W.wave_lists(classes)
        rays2, tasks2, _ = W.wave_lists(again)
        assert np.array_equal(_bits(rays), _bits(rays2)) and np.array_equal(tasks, tasks2)
        # the wave lists partition the ray array
        assert tasks[0, 0] == 0 and np.array_equal(tasks[1:, 0], np.cumsum(tasks[:-1, 1])) and int(tasks[:, 1].sum()) == len(rays) == len(labels)
        total = sum(len(v) for v in classes.values())
        assert labels.count("b") >= total and sum(l.startswith("a:") for l in labels) == total
        assert any(c % 64 for c in tasks[:, 1]) and any(c > 64 for c in tasks[:, 1]) and labels.count("d:special") == 64
        # every mixed list holds NaN rays, exact-path rays and (unless the scene is not finite) fast rays, in every stretch of 64
        all_finite = bool(np.isfinite(W.geometry_arrays(desc)[1]).all())
        fast = W.predict_flags(rays, all_finite)
        nan = np.isnan(rays).any(axis=1)
        mixed = [(b, c) for b, c in tasks if labels[b] in ("b", "c")]
        assert len(mixed) >= 10 and any(c % 64 for _, c in mixed)
        for b, c in mixed:
            for w0 in range(b, b + c, 64):
                w1 = min(w0 + 64, b + c)
                if w1 - w0 < 33:
                    continue                                                  # (a ragged tail shorter than one deal)
                assert nan[w0:w1].any() and (~fast & ~nan)[w0:w1].any() and (fast[w0:w1].any() or not all_finite), (name, b, w0)
    assert {"far_sliver", "origin_limit"} <= set(cases["grid3000"][3]) and "far_sliver" not in cases["cornell"][3]
    special = cases["cornell"][3]["special"]
    assert np.isnan(special).any(axis=1).sum() >= 15 and np.isinf(special).any() and (special[:, 3:] == 0).all(axis=1).any()


def test_hit_index_is_orc_world_hit_and_names_the_primitive_that_gives_t(cases, orc):
    """orc_world_hit_index: same hit, same t bits as orc_world_hit on every ray class of every scene, and the primitive it names
    reproduces that t through orc_sphere_hit / orc_quad_hit with the same range."""
    checked = hits = 0
    inf = float("inf")
    for name, (desc, ow, mk, classes, _) in cases.items():
        kind, a, b, c = W.geometry_arrays(desc)
        for cls, rays in classes.items():
            rays = rays[:64]
            hit, t, idx = W.oracle_answers(ow, rays)
            for i, r in enumerate(rays):
                ray = _ray(orc, r)
                rec, _ = ow.hit(ray)
                rec2, one = ow.hit_index(ray)
                assert (rec is not None) == bool(hit[i]) == (rec2 is not None), (name, cls, i)
                assert one == idx[i] and (idx[i] >= 0) == bool(hit[i]), (name, cls, i)
                checked += 1
                if rec is None:
                    assert np.isinf(t[i]) and idx[i] == -1
                    continue
                hits += 1
                assert _bits([rec.t])[0] == _bits([t[i]])[0] == _bits([rec2.t])[0], (name, cls, i)
                g = int(idx[i])
                own = orc.HitRecord()
                if kind[g] == 0:
                    ok = orc.lib.orc_sphere_hit(orc.Vec3(*a[g]), float(b[g, 0]), C.byref(ray), 0.001, inf, C.byref(own))
                else:
                    ok = orc.lib.orc_quad_hit(orc.Vec3(*a[g]), orc.Vec3(*b[g]), orc.Vec3(*c[g]), C.byref(ray), 0.001, inf, C.byref(own))
                assert ok and _bits([own.t])[0] == _bits([t[i]])[0], (name, cls, i, g)
    assert checked > 5000 and hits > 2500


def test_every_class_hits_something_in_every_scene(cases):
    shares = {}
    for name, (desc, ow, mk, classes, _) in cases.items():
        for cls, rays in classes.items():
            shares[(name, cls)] = float(W.oracle_answers(ow, rays)[0].mean())
    low = sorted((v, k) for k, v in shares.items() if k[1] != "special")
    print("smallest hit shares:", low[:6])
    for share, key in low:
        assert share >= MIN_HIT_SHARE, (key, share)
    # NaN rays hit nothing
    for name, (desc, ow, mk, classes, _) in cases.items():
        sp = classes["special"]
        hit = W.oracle_answers(ow, sp)[0]
        assert not hit[np.isnan(sp).any(axis=1)].any(), name


@pytest.mark.parametrize("name", ["random_spheres", "grid3000"])
def test_far_slivers_are_decided_by_the_leaf_box_alone(cases, orc, name):
    """L = 1000: the aimed-at sphere's own f32 test reports a hit although the ray passes above its box, and the leaf box keeps that
    hit out of the BVH's answer; brute force takes it."""
    desc, ow, mk, _, _ = cases[name]
    rays, sphere, L = mk.far_sliver(2000, Ls=(1000.0,))
    rays = W.f32(rays)
    _, a, b, _ = W.geometry_arrays(desc)
    inf = float("inf")
    false_hit = 0
    rec = orc.HitRecord()
    for i, r in enumerate(rays):
        ray = _ray(orc, r)
        s = int(sphere[i])
        centre, radius = orc.Vec3(*a[s]), float(b[s, 0])
        box = orc.lib.orc_sphere_bbox(centre, radius)
        if orc.lib.orc_sphere_hit(centre, radius, C.byref(ray), 0.001, inf, C.byref(rec)) and not orc.lib.orc_aabb_intersect(C.byref(box), C.byref(ray), 0.001, inf):
            false_hit += 1
    tree_hit, tree_t, _ = W.oracle_answers(ow, rays)
    brute_hit, brute_t = ow.hit_bruteforce_batch(rays)
    differ = int(((tree_hit != brute_hit) | (_bits(tree_t) != _bits(brute_t))).sum())
    print(name, "sphere hits but its box misses:", false_hit / len(rays), "BVH != brute force:", differ / len(rays))
    assert false_hit >= len(rays) / 2 and differ >= len(rays) / 2


def test_cornell_bvh_and_brute_force_agree(cases, orc):
    desc, ow, mk, classes, _ = cases["cornell"]
    n = 0
    for cls, rays in classes.items():
        tree_hit, tree_t, _ = W.oracle_answers(ow, rays)
        brute_hit, brute_t = ow.hit_bruteforce_batch(rays)
        assert np.array_equal(tree_hit, brute_hit) and np.array_equal(_bits(tree_t), _bits(brute_t)), cls
        n += len(rays)
    assert n > 1000


@pytest.mark.parametrize("name, pair", [("degenerate", (16, 17)), ("signed_zero_planes", (0, 1))])
def test_ties_go_to_the_first_in_left_first_order(cases, name, pair):
    """Coincident twin spheres (`degenerate`) and twin quads (`signed_zero_planes`: one quad written with +0 and with -0 - coplanar and
    overlapping): both give the same t, and the one that comes first in the BVH's leaf order wins (bvh.rs:96-101).  The rays are part
    of the scene's `surface` class, whatever its size."""
    desc, ow, mk, classes, _ = cases[name]
    rays, groups = mk.tie_rays()
    assert len(rays) >= 8 and pair in groups
    rays = W.f32(rays)
    surface = {r.tobytes() for r in classes["surface"]}
    assert all(r.tobytes() in surface for r in rays)
    _, prim, _ = ow.bvh_dump()
    order = [int(p) for p in prim if p in pair]
    mine = np.array([g == pair for g in groups])
    hit, _, geo = W.oracle_answers(ow, rays[mine])
    print(name, "rays at the twins", pair, ":", int(mine.sum()), "hit the first in leaf order:", int((geo == order[0]).sum()), "the second:", int((geo == order[1]).sum()))
    assert (geo == order[0]).sum() >= 1 and (geo == order[1]).sum() == 0


def test_far_slivers_pass_the_grown_f16_leaf_node_and_fail_the_exact_box(cases):
    """The node-test replay of test_fused_slab_arithmetic_on_the_grown_f16_boxes_is_conservative on the leaf node of the aimed-at sphere:
    these are the rays for which walk_compact's coarse test lets the leaf through and only the exact re-test keeps the false hit out."""
    desc, ow, mk, _, sc = cases["grid3000"]
    lo16, hi16, link = sc.compact_nodes()
    box, prim, _ = sc.cull_nodes()
    node_of = np.full(len(desc["geometries"]), -1)
    node_of[prim[prim >= 0]] = np.flatnonzero(prim >= 0)
    rays, sphere, _ = mk.far_sliver(2000, Ls=(1000.0,))
    rays = W.f32(rays)
    f32_, ld = np.float32, np.longdouble
    node = node_of[sphere]
    assert (node >= 0).all() and ((link[node] & 0x80000000) != 0).all()
    o, d = rays[:, :3], rays[:, 3:]
    inv = (f32_(1.0) / d).astype(f32_)
    lo32, hi32 = box[node, :3].astype(f32_), box[node, 3:].astype(f32_)
    a, b = ((lo32 - o).astype(f32_) * inv).astype(f32_), ((hi32 - o).astype(f32_) * inv).astype(f32_)
    exact = ~(np.minimum(np.maximum(a, b).min(axis=1), f32_(np.inf)) <= np.maximum(np.minimum(a, b).max(axis=1), f32_(0.001)))
    m = (o * inv).astype(f32_)
    ga = (lo16[node].astype(ld) * inv.astype(ld) - m.astype(ld)).astype(f32_)
    gb = (hi16[node].astype(ld) * inv.astype(ld) - m.astype(ld)).astype(f32_)
    coarse = ~(np.maximum(ga, gb).min(axis=1) <= np.maximum(np.minimum(ga, gb).max(axis=1), f32_(0.001)))
    share = float((coarse & ~exact).mean())
    print("pass the grown f16 leaf node, fail the exact box:", share, "inside the fused loop's domain:", float(W.predict_flags(rays, True, mk.limit).mean()))
    assert share >= 0.25
    assert W.predict_flags(rays, True, mk.limit).all()                        # ... and they walk the fused loop, not the reference tree


def test_both_sides_of_the_fused_loops_domain(cases):
    desc, ow, mk, classes, _ = cases["grid3000"]
    for cls in ("origin_limit", "near_axis_parallel"):
        inside = W.predict_flags(classes[cls], True, mk.limit)
        print(cls, "inside the domain:", float(inside.mean()))
        assert 0.10 <= inside.mean() <= 0.90, cls
    # the limit itself is inside, one ulp above it is outside
    ol = classes["origin_limit"]
    assert W.predict_flags(ol[0::5], True, mk.limit).all() and W.predict_flags(ol[1::5], True, mk.limit).all()
    assert not W.predict_flags(ol[2::5], True, mk.limit).any()
