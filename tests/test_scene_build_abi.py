"""trt_scene_create_on_device / trt_scene_get_packed at the C boundary, without a GPU: declarations, the refusals made before
any device work, and the packed scene of host-built scenes decoded region by region against the node dumps and the world."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from scene_build_worlds import fuzz_world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("trt_scene_create_on_device", "trt_scene_get_packed")


def test_new_symbols_exported_and_declared(trt):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tinyrt.h")).read(), flags=re.S)
    raw = C.CDLL(trt._lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(raw, name)
        assert name in trt._lib.SIGNATURES
    assert trt.lib.trt_abi_version() == 4


def _create_on_device(trt, world, **options):
    h = C.c_void_p()
    opt = trt.api.scene_options(**options)
    rc = trt.lib.trt_scene_create_on_device(world._h, C.byref(opt), C.byref(h))
    if rc == 0:
        trt.lib.trt_scene_destroy(h)
    return rc, trt.lib.trt_last_error().decode()


def test_no_device_is_refused(trt):
    if trt.lib.trt_device_count() > 0:
        pytest.skip("a device is visible here (tests/test_gpu_scene_build.py covers it)")
    rc, msg = _create_on_device(trt, fuzz_world(trt, 10, 1))
    assert rc == trt._lib.ERR_NO_DEVICE and msg


@pytest.mark.parametrize("prune", [0.0, -0.5, 1.5, float("nan")])
def test_bad_options_refused_before_device_work(trt, prune):
    rc, msg = _create_on_device(trt, fuzz_world(trt, 10, 1), cull_prune=prune)
    assert rc == trt._lib.ERR_INVALID_ARG and "cull_prune" in msg


def test_empty_world_refused_like_the_host_compiler(trt):
    w = trt.World()
    w.add_material("m", trt.Lambertian((0.5, 0.5, 0.5)))
    rc, msg = _create_on_device(trt, w)
    h = C.c_void_p()
    assert trt.lib.trt_scene_create_ex(w._h, None, C.byref(h)) == rc == trt._lib.ERR_INVALID_ARG
    assert trt.lib.trt_last_error().decode() == msg == "world has no geometry"


def test_get_packed_refuses_small_cap(trt):
    s = trt.Scene(fuzz_world(trt, 50, 3))
    n = s.info()["device_bytes"]
    buf = np.zeros(n, np.uint8)
    assert trt.lib.trt_scene_get_packed(s._h, buf.ctypes.data, n - 1) == trt._lib.ERR_INVALID_ARG
    assert trt.lib.trt_scene_get_packed(s._h, buf.ctypes.data, n) == 0


def layout(info):
    """Offsets (in 16-byte elements) of the packed scene's regions, from the counts (scene.h SceneLayout)."""
    nc, nn, ns, nm = info["num_cull_nodes"], info["num_nodes"], info["num_spheres"], info["num_materials"]
    nq, nl = info["num_quads"], info["num_spheres"] + info["num_quads"]
    off_sphere = 2 * nc
    n_u32 = 4 * (off_sphere + ns + 5 * nq + nm) + ns + nm
    hot = (4 * n_u32 + 15) & ~15
    off_ref = hot // 16
    off_leaf = off_ref + 2 * nn
    end = off_leaf + 2 * (nl + 4)
    off_compact = end if info["device_bytes"] > 16 * end else 0
    return dict(off_sphere=off_sphere, off_ref=off_ref, off_leaf=off_leaf, off_compact=off_compact, end=end)


def _nodes(f4, first, n):
    e = f4[first:first + 8 * n].reshape(n, 8)
    box = np.concatenate([e[:, 0:4], e[:, 4:6]], axis=1)
    return box, e[:, 6].view(np.uint32), e[:, 7].view(np.uint32)


def _check_packed(trt, world, spheres, **options):
    s = trt.Scene(world, **options)
    info = s.info()
    blob = s.packed()
    assert blob.dtype == np.uint8 and blob.size == info["device_bytes"]
    L = layout(info)
    f4 = blob.view(np.float32)
    quad = 0x40000000
    for (box, prim, skip), first in ((s.cull_nodes(), 0), (s.nodes(), L["off_ref"])):
        n = len(skip)
        pbox, pskip, plink = _nodes(f4, 4 * first, n)
        assert np.array_equal(pbox.view(np.uint32), box.view(np.uint32))
        assert np.array_equal(pskip, np.minimum(skip, n).astype(np.uint32))
        inner = prim < 0
        assert np.array_equal(plink[inner], (0x80000000 | (np.arange(n)[inner] + 1)).astype(np.uint32))
        assert not np.any(plink[~inner] & 0x80000000)
    # leaf list: the reference tree's leaves in walk order, skip = successor, then 4 copies of the last
    box, prim, _ = s.nodes()
    leaves = prim >= 0
    nl = int(leaves.sum())
    lbox, lskip, llink = _nodes(f4, 4 * L["off_leaf"], nl + 4)
    assert np.array_equal(lbox[:nl].view(np.uint32), box[leaves].view(np.uint32))
    assert np.array_equal(lskip[:nl], np.arange(1, nl + 1, dtype=np.uint32))
    assert np.array_equal(llink[:nl], _nodes(f4, 4 * L["off_ref"], len(prim))[2][leaves])
    for k in range(4):
        assert np.array_equal(lbox[nl + k].view(np.uint32), lbox[nl - 1].view(np.uint32)) and llink[nl + k] == llink[nl - 1]
    # spheres: (center, radius) in insertion order of the spheres
    if len(spheres):
        sp = f4[4 * L["off_sphere"]:4 * (L["off_sphere"] + info["num_spheres"])].reshape(-1, 4)
        assert np.array_equal(sp.view(np.uint32), np.asarray(spheres, np.float32).reshape(-1, 4).view(np.uint32))
    # compact nodes
    cn = s.compact_nodes()
    assert (cn is None) == (L["off_compact"] == 0)
    if cn is not None:
        nc = info["num_cull_nodes"]
        words = blob[16 * L["off_compact"]:16 * (L["off_compact"] + nc)].view(np.uint32).reshape(nc, 4)
        lo, hi, link = cn
        assert np.array_equal(words[:, :3].copy().view(np.float16).reshape(nc, 6), np.concatenate([lo, hi], axis=1))
        inner = (words[:, 3] & 0x80000000) == 0
        assert np.array_equal(np.where(inner, words[:, 3] >> 4, words[:, 3]), link)
        assert 16 * (L["off_compact"] + nc) == info["device_bytes"]
    else:
        assert 16 * L["end"] == info["device_bytes"]


def test_packed_regions_cornell(trt):
    desc = trt.scenes.cornell(64, 64)
    world, _ = trt.world_from_description(desc)
    _check_packed(trt, world, [])
    _check_packed(trt, world, [], compact_nodes=1)


def test_packed_regions_random_spheres(trt):
    world, _ = trt.world_from_description(trt.scenes.random_spheres(64, 36))
    _check_packed(trt, world, [])
    _check_packed(trt, world, [], compact_nodes=1, cull_prune=0.9)


def test_packed_regions_sphere_grid(trt):
    world, _ = trt.world_from_description(trt.scenes.sphere_grid(3000, 64, 36))
    _check_packed(trt, world, [])


def test_packed_regions_mixed_fuzz_world(trt):
    rng = np.random.default_rng(7)
    w = trt.World()
    w.add_material("m", trt.Lambertian((0.5, 0.5, 0.5)))
    spheres = []
    for i in range(300):
        if i % 3 == 0:
            w.add_geometry(trt.Quad(tuple(rng.uniform(-5, 5, 3)), tuple(rng.uniform(-1, 1, 3)), tuple(rng.uniform(-1, 1, 3)), 0))
        else:
            c, r = rng.uniform(-5, 5, 3).astype(np.float32), np.float32(rng.uniform(0.1, 1))
            spheres.append([*c, r])
            w.add_geometry(trt.Sphere(tuple(float(x) for x in c), float(r), 0))
    _check_packed(trt, w, spheres)
    _check_packed(trt, w, spheres, compact_nodes=1, cull_prune=0.2)
    _check_packed(trt, fuzz_world(trt, 500, 11, special=0.05), [], compact_nodes=1)
