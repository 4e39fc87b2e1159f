"""First-hit feature buffers (trt_render_aov and its device form) and the primary-ray export (trt_primary_rays and its device form)
against the CPU oracle, bit for bit.

Scenes (tests/walk_ray_cases.py, each with its own camera): cornell (lock-step list), prims33 (LDS tree, 256 lanes), random_spheres and
mixed400 (LDS trees, 768 lanes), prims600 (register slots through the launch plan's fallback), grid3000 (16-byte nodes from global
memory); every test that compiles a scene asserts the kernel shape Scene.aov_plan reports for it.  Images: 67 x 35 (ragged: 2345 pixels,
no multiple of a wave, of a run or of a workgroup) and 131 x 70, 3 samples per pixel, seed 5.  Both sizes launch at least two workgroups
wherever the plan allows it - a 768-lane workgroup holds twelve runs of 256 pixels, so the small image of such a scene is one workgroup
and the large one three.  The oracle's coverage share per scene must lie in [0.05, 0.95], so that no test passes on an all-hit or
all-miss image; no pixel is ever left out of a comparison.

What is compared with what:
 1. the exported rays with a Python restatement of pointgen.rs:41-43 + camera.rs:58-66 in np.float32 over the oracle's RNG, unit-disk
    and Ray::new functions;
 2. albedo and coverage with whole frames of the oracle's RENDERER: the same geometry with every material a Light of that material's
    albedo, max_bounces = 1, the scene's background, is the albedo buffer; lights of colour 1 over background 0 the coverage buffer;
 3. normal, depth and the two index buffers with the numpy fold, in sample order, of orc_world_hit_index on the rays of 1 (mixed400
    interleaves spheres and quads: a kind-local primitive index instead of the insertion index fails here);
 4. every buffer with the numpy fold of trt_intersect on the exported rays, and the device forms with the host forms;
 5. split sample ranges, two shards, every subset of buffers with guard bytes behind each, and the device scene compiler with one pass.

 6. the scenes compiled with another placement option or by the device compiler (test_gpu_queries.OTHER_WALKS: the LDS tree on Cornell, the
    lock-step list with more than 32 leaves, register slots from global memory and as the streamed plan's own walk, each route to the
    fallback) at 67 x 35: normal, depth and the indices with the oracle fold of 3, albedo and coverage with the default compilation's
    bytes, which 2 pins to the oracle's renderer.

Bits are compared, except that a component the reference fold makes NaN is compared by NaN-ness (tests/test_gpu_queries.py
assert_records_equal).  Every GPU step is one in-process call; nothing is built here and no child process is started."""
import ctypes as C
import itertools

import numpy as np
import pytest

import test_gpu_queries as G
import walk_ray_cases as W

pytestmark = pytest.mark.gpu

SCENES = ["cornell", "prims33", "random_spheres", "mixed400", "prims600", "grid3000"]
SIZES = [(67, 35), (131, 70)]
SPP, SEED = 3, 5
MISS = 0xFFFFFFFF
# (scene, scene options, kernel shape): the compilations whose walks the default ones above do not launch - aov_kernel<MODE_GLOBAL,
# WALK_REGS, 256> among them - at SIZES[0]; tests/test_aov_abi.py checks without a GPU that SCENES and these reach all of kAovKernels
WALK_CASES = G.OTHER_WALKS
INV = np.float32(1.0) / np.float32(SPP)                                     # imager.rs:35


def restated_rays(orc, ocam, seed, s, rows=None):
    """float32 [rows, W, 6]: restated_rays_of_pixels for every pixel of the image rows `rows` (all by default), row by row."""
    width, height = ocam.width, ocam.height
    rows = list(range(height)) if rows is None else list(rows)
    return restated_rays_of_pixels(orc, ocam, seed, s, [y * width + x for y in rows for x in range(width)]).reshape(len(rows), width, 6)


def restated_rays_of_pixels(orc, ocam, seed, s, pixels):
    """float32 [len(pixels), 6]: SamplePointGenerator::generate's body (pointgen.rs:41-43) and Camera::get_ray (camera.rs:58-66) for
    sample s of the pixels `pixels` (y * W + x), in the order given.  The random numbers are drawn pixel by pixel from the oracle's
    functions in the reference's order (u, v, the unit disk); the vector arithmetic is numpy's float32 (one IEEE operation per operator,
    no fusing) in the reference's order; Ray::new is the oracle's."""
    width, height = ocam.width, ocam.height
    n = len(pixels)
    ru, rv, px, py = (np.zeros(n, np.float32) for _ in range(4))
    xs, ys = np.zeros(n, np.float32), np.zeros(n, np.float32)
    rng = (C.c_uint32 * 2)()
    for i, pixel in enumerate(pixels):
        y, x = divmod(int(pixel), width)
        orc.lib.orc_rng_seed(seed, y * width + x, s, rng)
        ru[i] = orc.lib.orc_rng_random(rng)
        rv[i] = orc.lib.orc_rng_random(rng)
        p = orc.lib.orc_random_in_unit_disk(rng)
        px[i], py[i] = p.x, p.y
        xs[i], ys[i] = x, y
    u = ((xs + ru) / np.float32(width - 1))[:, None]
    v = ((ys + rv) / np.float32(height - 1))[:, None]
    vec = lambda name: np.array(getattr(ocam, name).tolist(), np.float32)[None, :]          # noqa: E731
    origin = (vec("position") + px[:, None] * vec("defocus_disk_u")) + py[:, None] * vec("defocus_disk_v")
    target = (vec("viewport_upper_left") + u * vec("horizontal")) - v * vec("vertical")
    direction = target - origin
    assert origin.dtype == direction.dtype == np.float32
    out = np.zeros((n, 6), np.float32)
    for i in range(n):
        r = orc.lib.orc_ray_new(orc.Vec3(*origin[i]), orc.Vec3(*direction[i]))
        out[i, :3] = r.origin.tolist()
        out[i, 3:] = r.direction.tolist()
    return out


def fold(per_sample, hit=None, start=None):
    """The imager's rule in float32, in sample order: acc = acc + value * (1/spp); with `hit`, only where the sample hit."""
    acc = np.zeros(per_sample[0].shape, np.float32) if start is None else start.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for k, v in enumerate(per_sample):
            nxt = acc + v.astype(np.float32) * INV
            acc = nxt if hit is None else np.where(hit[k], nxt, acc)
    assert acc.dtype == np.float32
    return acc


def assert_same(got, want, what):
    """Bits; a component that is NaN in `want` by NaN-ness.  Every element is compared."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    if got.dtype == np.float32:
        same = np.where(np.isnan(want), np.isnan(got), got.view(np.uint32) == want.view(np.uint32))
    else:
        same = got == want
    bad = np.argwhere(~same)
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def expected_workgroups(plan, n):
    waves = -(-n // 256)
    return -(-waves // (plan["threads_per_workgroup"] // 64))


@pytest.fixture(scope="module")
def case(trt, orc):
    """(scene name, (width, height)) -> everything about one scene at one image size, computed once on first use and shared, never
    changed: description, cameras, oracle world, product scene, the restated rays of the three samples, the oracle's first-hit records
    for them and the one-pass feature buffers of the product."""
    cache = {}

    def get(name, size):
        if (name, size) in cache:
            return cache[(name, size)]
        width, height = size
        n = width * height
        desc = W.scene(trt, name)
        desc = dict(desc, camera=dict(desc["camera"], width=width, height=height))
        ow, ocam = orc.world_from_description(desc)
        world, cam = trt.world_from_description(desc)
        sc = world.get_bvh()
        plan = sc.aov_plan(n)
        assert G.plan_shape(plan) == G.DEFAULT_SHAPES[name], (name, plan)
        assert plan["rays_per_wave"] == 256 and plan["workgroups"] == expected_workgroups(plan, n), plan
        # more than one workgroup wherever the plan allows it: always at the large size, at the small one unless a workgroup holds 12 runs
        assert plan["workgroups"] >= 2 or (size == SIZES[0] and plan["threads_per_workgroup"] == 768), (name, size, plan)
        rays = [restated_rays(orc, ocam, SEED, s).reshape(n, 6) for s in range(SPP)]
        rec = []
        for s in range(SPP):
            hit, t, geo = ow.hit_index_batch(rays[s])
            normal = np.zeros((n, 3), np.float32)
            mat = np.full(n, MISS, np.uint32)
            for i in np.flatnonzero(hit):
                r, idx = ow.hit_index(orc.Ray(orc.Vec3(*rays[s][i, :3]), orc.Vec3(*rays[s][i, 3:])))
                assert r is not None and idx == geo[i] and np.float32(r.t).view(np.uint32) == t[i].view(np.uint32)
                normal[i] = r.normal.tolist()
                mat[i] = r.material
            rec.append(dict(hit=hit, t=t, geo=np.where(hit, geo.astype(np.int64), MISS).astype(np.uint32), normal=normal, mat=mat))
        share = float(np.mean([r["hit"].mean() for r in rec]))
        print(f"\n{name} {width}x{height}: {len(desc['geometries'])} primitives, oracle coverage share {share:.3f}, "
              f"{plan['workgroups']} workgroups of {plan['threads_per_workgroup']} lanes, walk {plan['walk']}")
        assert 0.05 <= share <= 0.95, (name, size, share)
        renderer = trt.Renderer(SPP, 1, 50, False, desc["background"], seed=SEED)
        aov = renderer.render_aov(cam, sc)
        cache[(name, size)] = dict(desc=desc, ow=ow, ocam=ocam, world=world, cam=cam, scene=sc, rays=rays, rec=rec, n=n, size=size,
                                   renderer=renderer, aov=aov)
        return cache[(name, size)]

    return get


CASES = [(name, size) for name in SCENES for size in SIZES]
CASE_IDS = [f"{name}-{w}x{h}" for name, (w, h) in CASES]


@pytest.mark.parametrize("name,size", CASES, ids=CASE_IDS)
def test_exported_rays_are_the_restated_reference_rays(trt, case, name, size):
    c = case(name, size)
    for s in range(SPP):
        got = c["cam"].primary_rays(s, SPP, seed=SEED)
        assert got.shape == (size[1], size[0], 6)
        assert_same(got.reshape(-1, 6), c["rays"][s], (name, size, "sample", s))
    # the seed and the sample key the stream
    assert not np.array_equal(c["cam"].primary_rays(0, SPP, seed=SEED + 1).reshape(-1, 6), c["rays"][0])
    with pytest.raises(trt.TinyRTError) as e:
        c["cam"].primary_rays(SPP, SPP, seed=SEED)
    assert e.value.code == trt._lib.ERR_INVALID_ARG


def light_world(orc, desc, colour=None):
    """The oracle world of `desc` with every material a Light: of the material's own albedo, or of `colour`."""
    lights = [(m[0], 3, tuple(m[2]) if colour is None else colour, 0.0) for m in desc["materials"]]        # 3 = TRT_LIGHT
    return orc.world_from_description(dict(desc, materials=lights))[0]


@pytest.mark.parametrize("name,size", CASES, ids=CASE_IDS)
def test_albedo_and_coverage_are_whole_frames_of_the_oracles_renderer(trt, orc, case, name, size):
    c = case(name, size)
    desc = c["desc"]
    want_albedo, _ = orc.render(light_world(orc, desc), c["ocam"], SPP, 1, desc["background"], seed=SEED, nthreads=4)
    want_cov, _ = orc.render(light_world(orc, desc, (1.0, 1.0, 1.0)), c["ocam"], SPP, 1, (0.0, 0.0, 0.0), seed=SEED, nthreads=4)
    assert_same(c["aov"]["albedo"], want_albedo, (name, size, "albedo"))
    for ch in range(3):
        assert_same(c["aov"]["coverage"], np.ascontiguousarray(want_cov[:, :, ch]), (name, size, "coverage", ch))
    cov = c["aov"]["coverage"]
    assert 0.05 <= float(cov.mean()) <= 0.95 and (cov == 0).any() and (cov > 0.9).any()


@pytest.mark.parametrize("name,size", CASES, ids=CASE_IDS)
def test_normal_depth_and_indices_are_the_fold_of_the_oracles_first_hits(trt, case, name, size):
    c = case(name, size)
    width, height = size
    rec, aov = c["rec"], c["aov"]
    hits = [r["hit"] for r in rec]
    assert_same(aov["normal"].reshape(-1, 3), fold([r["normal"] for r in rec]), (name, size, "normal"))
    assert_same(aov["depth"].reshape(-1), fold([r["t"] for r in rec], hits), (name, size, "depth"))
    assert_same(aov["coverage"].reshape(-1), fold([h.astype(np.float32) for h in hits]), (name, size, "coverage"))
    assert_same(aov["geometry"].reshape(-1), rec[0]["geo"], (name, size, "geometry"))
    assert_same(aov["material"].reshape(-1), rec[0]["mat"], (name, size, "material"))
    miss0 = ~rec[0]["hit"]
    assert miss0.any() and (~miss0).any()
    assert (aov["geometry"].reshape(-1)[miss0] == MISS).all() and (aov["material"].reshape(-1)[miss0] == MISS).all()
    assert aov["geometry"].shape == (height, width) and aov["normal"].shape == (height, width, 3)


def intersect_fold(c, background, first=0, last=SPP, start=None, rays=None):
    """The six buffers from trt_intersect on the exported rays of samples [first, last), folded in numpy."""
    sc, cam = c["scene"], c["cam"]
    mats = np.array([m[2] for m in c["desc"]["materials"]], np.float32)
    recs = []
    for s in range(first, last):
        r = cam.primary_rays(s, SPP, seed=SEED).reshape(-1, 6) if rays is None else rays[s]
        recs.append(sc.intersect(r))
    hits = [r["geometry"] != MISS for r in recs]
    albedo = [np.where(h[:, None], mats[np.where(h, r["material"], 0)], np.array(background, np.float32)[None, :]) for r, h in zip(recs, hits)]
    st = start or {}
    out = dict(albedo=fold(albedo, start=st.get("albedo")), normal=fold([r["normal"] for r in recs], start=st.get("normal")),
               depth=fold([r["t"] for r in recs], hits, start=st.get("depth")),
               coverage=fold([h.astype(np.float32) for h in hits], start=st.get("coverage")))
    if first == 0:
        out["geometry"], out["material"] = recs[0]["geometry"].copy(), recs[0]["material"].copy()
    return out


@pytest.mark.parametrize("name,size", CASES, ids=CASE_IDS)
def test_buffers_are_the_fold_of_trt_intersect_on_the_exported_rays(trt, case, name, size):
    c = case(name, size)
    want = intersect_fold(c, c["desc"]["background"])
    for ch in trt.AOV_CHANNELS:
        assert_same(c["aov"][ch].reshape(want[ch].shape), want[ch], (name, size, ch))


def device_buffers(trt, torch, n, channels, pad=64, fill=0xCD):
    """channel -> uint8 tensor of the channel's n pixels plus `pad` guard pixels, filled with `fill`."""
    dev = torch.device("cuda:0")
    return {ch: torch.full(((n + pad) * trt.AOV_CHANNELS[ch][1] * 4,), fill, dtype=torch.uint8, device=dev) for ch in channels}


def channel_bytes(trt, aov, ch):
    return np.ascontiguousarray(aov[ch]).view(np.uint8).reshape(-1)


@pytest.mark.parametrize("name,size", CASES, ids=CASE_IDS)
def test_device_forms_equal_the_host_forms(trt, case, name, size):
    import torch
    c = case(name, size)
    n = c["n"]
    side = torch.cuda.Stream()
    for stream in (None, side):
        bufs = device_buffers(trt, torch, n, trt.AOV_CHANNELS)
        rays = torch.full(((n + 64) * 24,), 0xCD, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        ptr = 0 if stream is None else stream.cuda_stream
        c["renderer"].render_aov_device(c["cam"], c["scene"], {ch: t.data_ptr() for ch, t in bufs.items()}, stream_ptr=ptr)
        c["cam"].primary_rays_device(1, SPP, rays.data_ptr(), seed=SEED, stream_ptr=ptr)
        (torch.cuda.current_stream() if stream is None else stream).synchronize()
        torch.cuda.synchronize()
        for ch, t in bufs.items():
            h = t.cpu().numpy()
            k = n * trt.AOV_CHANNELS[ch][1] * 4
            assert h[:k].tobytes() == channel_bytes(trt, c["aov"], ch).tobytes(), (name, size, ch, stream is not None)
            assert (h[k:] == 0xCD).all(), (name, size, ch, "bytes behind the buffer were written")
        h = rays.cpu().numpy()
        assert h[:n * 24].tobytes() == c["cam"].primary_rays(1, SPP, seed=SEED).tobytes() and (h[n * 24:] == 0xCD).all()


@pytest.mark.parametrize("name,size", CASES, ids=CASE_IDS)
def test_split_sample_ranges_equal_one_pass(trt, case, name, size):
    c = case(name, size)
    r = c["renderer"]
    first = r.render_aov(c["cam"], c["scene"], sample_begin=0, sample_end=2)
    ids = {ch: first[ch].copy() for ch in ("geometry", "material")}
    assert not np.array_equal(first["coverage"], c["aov"]["coverage"])                             # (two of three samples: not the frame yet)
    both = r.render_aov(c["cam"], c["scene"], buffers=first, sample_begin=2, sample_end=3, accumulate=1)
    for ch in trt.AOV_CHANNELS:
        assert_same(both[ch], c["aov"][ch], (name, size, ch))
    # the pass without sample 0 left the indices as the first pass wrote them, and writes none of its own
    assert np.array_equal(both["geometry"], ids["geometry"]) and np.array_equal(both["material"], ids["material"])
    marked = {ch: np.full(c["aov"][ch].shape, 0xABABABAB, np.uint32) for ch in ("geometry", "material")}
    r.render_aov(c["cam"], c["scene"], channels=("geometry", "material"), buffers=marked, sample_begin=1, sample_end=3, accumulate=1)
    assert (marked["geometry"] == 0xABABABAB).all() and (marked["material"] == 0xABABABAB).all()


@pytest.mark.parametrize("name,size", CASES, ids=CASE_IDS)
def test_two_shards_assemble_to_the_full_frame(trt, case, name, size):
    c = case(name, size)
    width, height = size
    tiles = __import__("importlib").import_module("tiny-raytracer_amd.tiles")
    seen = np.zeros(height, np.int32)
    for rank in range(2):
        lay = tiles.band_layout(height, 2, rank)
        rows = np.array(lay["rows"])
        bands = dict(band_rows=16, band_stride=2, band_offset=rank, rows_local=lay["rows_local"])
        part = c["renderer"].render_aov(c["cam"], c["scene"], **bands)
        for ch in trt.AOV_CHANNELS:
            assert part[ch].shape[0] == len(rows)
            assert_same(part[ch], np.ascontiguousarray(c["aov"][ch][rows]), (name, size, ch, "shard", rank))
        got = c["cam"].primary_rays(2, SPP, seed=SEED, **bands)
        assert_same(got, np.ascontiguousarray(c["rays"][2].reshape(height, width, 6)[rows]), (name, size, "rays of shard", rank))
        seen[rows] += 1
    assert (seen == 1).all()


@pytest.mark.parametrize("name", SCENES)
def test_any_subset_of_buffers_gives_the_same_bytes_and_leaves_the_guards(trt, case, name):
    import torch
    c = case(name, SIZES[0])
    n = c["n"]
    names = list(trt.AOV_CHANNELS)
    want = {ch: torch.from_numpy(channel_bytes(trt, c["aov"], ch).copy()).to("cuda:0") for ch in names}
    subsets = [s for k in range(1, 7) for s in itertools.combinations(names, k)]
    assert len(subsets) == 63
    for subset in subsets:
        bufs = device_buffers(trt, torch, n, subset)
        c["renderer"].render_aov_device(c["cam"], c["scene"], {ch: t.data_ptr() for ch, t in bufs.items()})
        torch.cuda.synchronize()
        for ch, t in bufs.items():
            k = len(want[ch])
            assert torch.equal(t[:k], want[ch]), (name, subset, ch)
            assert bool((t[k:] == 0xCD).all()), (name, subset, ch, "bytes behind the buffer were written")
    with pytest.raises(trt.TinyRTError) as e:
        c["renderer"].render_aov_device(c["cam"], c["scene"], {})
    assert e.value.code == trt._lib.ERR_INVALID_ARG


@pytest.mark.parametrize("name", SCENES)
def test_the_device_compiled_scene_gives_the_same_bytes(trt, case, name):
    c = case(name, SIZES[0])
    other = trt.Scene(c["world"], on_device=True)
    assert G.plan_shape(other.aov_plan(c["n"])) == G.DEFAULT_SHAPES[name]
    got = c["renderer"].render_aov(c["cam"], other)
    for ch in trt.AOV_CHANNELS:
        assert got[ch].tobytes() == c["aov"][ch].tobytes(), (name, ch)


@pytest.mark.parametrize("name,options,shape", WALK_CASES,
                         ids=["%s-%s" % (name, ",".join("%s=%s" % kv for kv in sorted(options.items()))) for name, options, _ in WALK_CASES])
def test_every_other_walk_gives_the_oracles_first_hits_and_the_default_compilations_bytes(trt, case, name, options, shape):
    c = case(name, SIZES[0])
    other = c["world"].get_bvh(**options)
    assert other is not c["scene"]
    plan = other.aov_plan(c["n"])
    assert G.plan_shape(plan) == shape, (name, options, plan)
    assert plan["rays_per_wave"] == 256 and plan["workgroups"] == expected_workgroups(plan, c["n"]), plan
    aov = c["renderer"].render_aov(c["cam"], other)
    rec = c["rec"]
    hits = [r["hit"] for r in rec]
    assert_same(aov["normal"].reshape(-1, 3), fold([r["normal"] for r in rec]), (name, options, "normal"))
    assert_same(aov["depth"].reshape(-1), fold([r["t"] for r in rec], hits), (name, options, "depth"))
    assert_same(aov["coverage"].reshape(-1), fold([h.astype(np.float32) for h in hits]), (name, options, "coverage"))
    assert_same(aov["geometry"].reshape(-1), rec[0]["geo"], (name, options, "geometry"))
    assert_same(aov["material"].reshape(-1), rec[0]["mat"], (name, options, "material"))
    for ch in ("albedo", "coverage"):
        assert aov[ch].tobytes() == c["aov"][ch].tobytes(), (name, options, ch)
