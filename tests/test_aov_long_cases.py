"""The inputs of tests/test_gpu_aov_long.py (tests/aov_long_cases.py) without a GPU: the launch arithmetic of its three images at 64, 256
and 304 compute units for its four scenes, and at 256 the picked pixels under the oracle - so that the GPU test never meets a run of 256
where it wants a longer one, or a set of boundary pixels that is all hits or all misses, for the first time on a GPU."""
import numpy as np
import pytest

import aov_long_cases as L
import test_gpu_aov as A
import test_gpu_queries as G


@pytest.fixture(scope="module")
def scenes(trt):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = L.scene_and_description(trt, name)
        return cache[name]

    return get


@pytest.mark.parametrize("cus", (64, 256, 304))
@pytest.mark.parametrize("name", L.SCENES)
def test_the_three_images_launch_as_the_gpu_test_wants_them(trt, scenes, name, cus):
    _, sc = scenes(name)
    z = L.sizes(sc, name, cus)                                              # (asserts the shapes and every plan it reads)
    slots, n0, long, doubled, shard = z["slots"], z["n0"], z["long"], z["doubled"], z["shard"]
    print("\n" + "\n".join(L.describe(name, tag, z[tag]) for tag in ("long", "at_n0", "doubled", "shard")))
    assert long["compute_units"] == cus and G.plan_shape(sc.aov_plan(long["n"], cus)) == G.DEFAULT_SHAPES[name]
    # both sides of the threshold, stated without the helper
    assert sc.aov_plan(n0, cus)["rays_per_wave"] == 256 and sc.aov_plan(n0 + 1, cus)["rays_per_wave"] == 320
    assert n0 < long["n"] <= n0 + long["width"] and long["per_wave"] == 320 == ((-(-long["n"] // slots) + 63) & ~63)
    assert long["n"] % 320 != 0 and long["last"] == long["n"] % 320 and long["waves"] <= slots
    assert long["width"] % 2 == 1 and abs(long["width"] / long["height"] - 131 / 70) < 0.01
    # twice the pixels: a run of 513 to 575 pixels rounded up
    assert doubled["n"] == 2 * long["n"] and doubled["per_wave"] == 576 > long["per_wave"]
    # the first of two shards of the doubled image owns at least the long image's rows: more than n0 pixels, lengthened runs of its own
    assert shard["n"] > n0 and shard["height"] >= long["height"] and shard["per_wave"] in (320, 384)
    rows = np.array(shard["rows"])
    assert len(rows) == shard["height"] and rows[0] == 0 and rows[L.BAND_ROWS] == 2 * L.BAND_ROWS and rows[-1] < doubled["height"]
    # the picked pixels: both sides of 96 boundaries, no multiple of 256 among the boundaries but the few that are one by chance
    picked = L.picked_pixels(long)
    bounds = picked[(picked % long["per_wave"]) == 0]
    assert len(bounds) >= L.BOUNDARY_WAVES and (bounds % 256 != 0).sum() >= L.BOUNDARY_WAVES // 2
    assert len(np.unique(picked // long["width"])) >= L.BOUNDARY_WAVES


@pytest.mark.parametrize("name", L.SCENES)
def test_the_picked_pixels_see_hits_and_misses_under_the_oracle(trt, orc, scenes, name):
    desc, sc = scenes(name)
    long = L.sizes(sc, name, 256)["long"]
    picked = L.picked_pixels(long)
    o = L.oracle_at(orc, L.with_camera(desc, long["width"], long["height"]), picked)
    print(f"\n{name}: {len(picked)} picked pixels of {long['width']} x {long['height']}: hit share {o['share']:.2f}, {o['geometries']} geometries")
    L.assert_not_vacuous(name, o)
    for ch, (dtype, k) in trt.AOV_CHANNELS.items():
        assert o["buffers"][ch].dtype == dtype and o["buffers"][ch].shape == ((len(picked), 3) if k == 3 else (len(picked),))


def test_the_pixel_form_of_the_restated_rays_is_the_row_form(trt, orc):
    """restated_rays (rows) and restated_rays_of_pixels (a list) are one body: the same arrays for the same pixels, in any order."""
    desc = L.with_camera(L.W.scene(trt, "cornell"), 67, 35)
    _, ocam = orc.world_from_description(desc)
    rows = A.restated_rays(orc, ocam, L.SEED, 1, rows=[3, 34, 0])
    assert rows.shape == (3, 67, 6) and rows.dtype == np.float32
    pixels = [3 * 67 + 66, 34 * 67, 0, 66, 34 * 67 + 66]
    got = A.restated_rays_of_pixels(orc, ocam, L.SEED, 1, pixels)
    want = np.stack([rows[0, 66], rows[1, 0], rows[2, 0], rows[2, 66], rows[1, 66]])
    assert got.tobytes() == want.tobytes()
    assert A.restated_rays(orc, ocam, L.SEED, 1).reshape(-1, 6)[pixels].tobytes() == got.tobytes()
