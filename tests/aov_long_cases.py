"""The image sizes, the pixels around the run boundaries and the oracle's fold of the feature-buffer test at frame size
(tests/test_gpu_aov_long.py on the GPU; tests/test_aov_long_cases.py runs the same arithmetic and the same oracle without one).

The feature buffers are launched by the rule of the queries (stream_plan.h plan_batch): a wave owns a run of 256 local pixels until the
image has more than n0 = 256 x wave_slots pixels, then of roundup64(ceil(n / wave_slots)).  Everything here is derived from
Scene.aov_plan for a given compute-unit count (0: the device at hand), never assumed:

  long image    width = int(sqrt(n0 x 131 / 70)) | 1 - odd, so runs begin at every column; the aspect of tests/test_gpu_aov.py, at which
                the scene cameras see geometry and background - and height = n0 // width + 1, so n = width x height is just past n0: runs
                of 320 pixels, a ragged last wave (the width steps by 2 until n is no multiple of the run)
  n0 image      2048 x n0 / 2048: runs of 256, every wave slot used
  doubled image the long image's width, twice its height: about 2 n pixels, runs half as long again as twice 256 (576 at 256 compute
                units); the first of two shards of 16-row bands owns at least `height` of its rows, more than n0 pixels

The picked pixels: the 32 on either side of rays_per_wave x w for 96 waves w spread evenly over 1 .. waves - 1, and the image's last 64."""
import math

import numpy as np

import test_gpu_aov as A
import test_gpu_queries as G
import walk_ray_cases as W

SCENES = ["cornell", "random_spheres", "prims600", "grid3000"]
BAND_SCENES = ["cornell", "random_spheres"]
SPP, SEED = 2, 5
BAND_ROWS = 16
BOUNDARY_WAVES, EITHER_SIDE, LAST = 96, 32, 64
MISS = 0xFFFFFFFF
INV = np.float32(1.0) / np.float32(SPP)                                     # imager.rs:35


def expected_run(n, slots):
    """plan_batch's run for n items over `slots` resident wave slots."""
    return 256 if -(-n // 256) <= slots else (-(-n // slots) + 63) & ~63


def sizes(sc, name, compute_units=0):
    """The three images of scene `sc` on `compute_units`, each with its asserted plan: dict(slots, n0, long=dict(width, height, n,
    per_wave, waves, last), at_n0=dict(...), doubled=dict(...), shard=dict(rows_local, n, per_wave, ...))."""
    tiles = __import__("importlib").import_module("tiny-raytracer_amd.tiles")
    plan = lambda n: sc.aov_plan(n, compute_units)                          # noqa: E731
    one = plan(1)
    assert G.plan_shape(one) == G.DEFAULT_SHAPES[name], (name, one)
    slots = one["wave_slots"]
    n0 = 256 * slots
    at = plan(n0)
    assert at["rays_per_wave"] == 256 and at["waves"] == slots and G.plan_shape(at) == G.DEFAULT_SHAPES[name], at

    def image(width, height):
        n = width * height
        q = plan(n)
        per_wave, waves = q["rays_per_wave"], q["waves"]
        assert G.plan_shape(q) == G.DEFAULT_SHAPES[name] and q["wave_slots"] == slots, (name, q)
        assert per_wave == expected_run(n, slots), (name, n, q)
        assert (waves - 1) * per_wave < n <= waves * per_wave and waves <= slots, (name, n, q)
        return dict(width=width, height=height, n=n, per_wave=per_wave, waves=waves, last=n - (waves - 1) * per_wave,
                    workgroups=q["workgroups"], threads=q["threads_per_workgroup"], compute_units=q["compute_units"])

    width = int(math.sqrt(n0 * 131 / 70)) | 1
    while True:
        long = image(width, n0 // width + 1)
        if long["n"] % long["per_wave"] != 0:
            break
        width += 2                                                          # (a device on which the last wave's run would be whole)
    assert long["width"] % 2 == 1 and long["n"] > n0 and long["per_wave"] > 256 and 0 < long["last"] < long["per_wave"], (name, long)
    assert n0 % 2048 == 0
    at_n0 = image(2048, n0 // 2048)
    assert at_n0["n"] == n0 and at_n0["per_wave"] == 256 and at_n0["waves"] == slots and at_n0["last"] == 256, (name, at_n0)
    doubled = image(long["width"], 2 * long["height"])
    assert doubled["per_wave"] > long["per_wave"], (name, doubled, long)
    lay = tiles.band_layout(doubled["height"], 2, 0, BAND_ROWS)
    shard = dict(image(long["width"], lay["rows_local"]), rows=lay["rows"],
                 bands=dict(band_rows=BAND_ROWS, band_stride=2, band_offset=0, rows_local=lay["rows_local"]))
    assert shard["n"] > n0 and shard["per_wave"] > 256 and lay["rows_local"] >= long["height"], (name, shard["n"], n0)
    return dict(slots=slots, n0=n0, long=long, at_n0=at_n0, doubled=doubled, shard=shard)


def describe(name, tag, im):
    return (f"{name} {tag}: {im['compute_units']} CUs, {im['threads']} lanes, {im['width']} x {im['height']} = {im['n']} pixels: "
            f"{im['per_wave']} per wave, {im['waves']} waves in {im['workgroups']} workgroups, the last wave owns {im['last']}")


def picked_pixels(im):
    """int64, sorted, no duplicates: the pixels around 96 run boundaries and the last 64 of the image."""
    per_wave, waves, n = im["per_wave"], im["waves"], im["n"]
    ws = np.unique(np.round(np.linspace(1, waves - 1, BOUNDARY_WAVES)).astype(np.int64))
    assert len(ws) == BOUNDARY_WAVES and ws[0] == 1 and ws[-1] == waves - 1, (waves, ws)
    around = (ws[:, None] * per_wave + np.arange(-EITHER_SIDE, EITHER_SIDE)[None, :]).reshape(-1)
    picked = np.unique(np.concatenate([around[around < n], np.arange(n - LAST, n)]))         # (a last wave of fewer than 32 pixels)
    assert picked[0] >= 0 and picked[-1] == n - 1 and (BOUNDARY_WAVES - 1) * 2 * EITHER_SIDE + LAST <= len(picked) <= BOUNDARY_WAVES * 2 * EITHER_SIDE + LAST
    # the boundaries fall on many columns of the odd width, on both sides of a row's end among them
    assert len(np.unique((ws * per_wave) % im["width"])) >= BOUNDARY_WAVES // 2
    return picked


def with_camera(desc, width, height):
    return dict(desc, camera=dict(desc["camera"], width=width, height=height))


def fold(per_sample, hit=None):
    """The imager's rule in float32, in sample order: acc = acc + value * (1/spp); with `hit`, only where the sample hit."""
    acc = np.zeros(per_sample[0].shape, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k, v in enumerate(per_sample):
            nxt = acc + v.astype(np.float32) * INV
            acc = nxt if hit is None else np.where(hit[k], nxt, acc)
    assert acc.dtype == np.float32
    return acc


def oracle_at(orc, desc, pixels):
    """The oracle's rays (restated as tests/test_gpu_aov.py restates them), first hits and the six folded buffers at `pixels` of the image
    of `desc`: dict(rays=[float32 [k, 6] per sample], buffers=dict(channel -> array), share, geometries, hit0)."""
    ow, ocam = orc.world_from_description(desc)
    mats = np.array([m[2] for m in desc["materials"]], np.float32)
    background = np.array(desc["background"], np.float32)[None, :]
    k = len(pixels)
    rays, rec = [], []
    for s in range(SPP):
        r = A.restated_rays_of_pixels(orc, ocam, SEED, s, pixels)
        hit, t, geo = ow.hit_index_batch(r)
        normal = np.zeros((k, 3), np.float32)
        mat = np.full(k, MISS, np.uint32)
        for i in np.flatnonzero(hit):
            h, idx = ow.hit_index(orc.Ray(orc.Vec3(*r[i, :3]), orc.Vec3(*r[i, 3:])))
            assert h is not None and idx == geo[i] and np.float32(h.t).view(np.uint32) == t[i].view(np.uint32)
            normal[i] = h.normal.tolist()
            mat[i] = h.material
        albedo = np.where(hit[:, None], mats[np.where(hit, mat, 0)], background).astype(np.float32)
        rays.append(r)
        rec.append(dict(hit=hit, t=t, geo=np.where(hit, geo.astype(np.int64), MISS).astype(np.uint32), normal=normal, mat=mat, albedo=albedo))
    hits = [r["hit"] for r in rec]
    buffers = dict(albedo=fold([r["albedo"] for r in rec]), normal=fold([r["normal"] for r in rec]), depth=fold([r["t"] for r in rec], hits),
                   coverage=fold([np.ones(k, np.float32) for _ in rec], hits), geometry=rec[0]["geo"], material=rec[0]["mat"])
    seen = np.unique(np.concatenate([r["geo"][r["hit"]] for r in rec]))
    return dict(rays=rays, buffers=buffers, share=float(np.mean([h.mean() for h in hits])), geometries=len(seen), hit0=rec[0]["hit"])


def assert_not_vacuous(name, o):
    """The picked pixels see geometry and background: a hit share in [0.05, 0.95], at least 7 geometries, sample 0 with both."""
    assert 0.05 <= o["share"] <= 0.95, (name, "hit share", o["share"])
    assert o["geometries"] >= 7, (name, "distinct geometries", o["geometries"])
    assert o["hit0"].any() and (~o["hit0"]).any(), (name, "sample 0 has only hits or only misses")


def scene_and_description(trt, name):
    desc = W.scene(trt, name)
    return desc, trt.world_from_description(desc)[0].get_bvh()
