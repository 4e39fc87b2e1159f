"""Scenes and the child script of the scene-facts tests (tests/test_scene_facts.py, tests/test_gpu_scene_facts.py; README_scene_facts.md):
the scenes of tests/test_gpu_flat_literal.py plus the ones below, each with the depth it renders at and the facts (tinyrt.h
trt_scene_facts) its handle must claim with the library's defaults."""
import test_gpu_flat_literal as T
from test_gpu_flat_reuse import _scene

SPP, SEED, W, H = T.SPP, T.SEED, T.W, T.H
NO_SPHERE, AXIS_EXACT, NEAREST_FIRST, LAZY, STRAIGHT = 1, 2, 4, 8, 16
LAMBERTIAN, METAL, DIELECTRIC, LIGHT = (1 << (8 + k) for k in range(4))
ALL_SWITCHES = NO_SPHERE | AXIS_EXACT | NEAREST_FIRST | LAZY


def _room(trt, extra, name, **kw):
    return _scene(trt, name, trt.scenes._box((-5.0, 0.0, 0.0), (5.0, 10.0, 10.0), "white") + extra, T._cam((0.0, 5.0, 0.5), (0.0, 4.0, 6.0), fov=75.0, focus=5.0), **kw)


def closed_room(trt):
    """Six Lambertian quads around the camera and no light: every path ends on the budget (depth 3), every colour is +0."""
    return _room(trt, [], "closed_room")


def floor_under_sky(trt):
    """One floor quad under a bright background: nearly every ray leaves through the miss exit, pool refills follow one another."""
    return _scene(trt, "floor_under_sky", [("quad", (-3.0, 0.0, 2.0), (6.0, 0.0, 0.0), (0.0, 0.0, 6.0), "red")], T._cam((0.0, 2.0, -3.0), (0.0, 0.5, 5.0)),
                  background=(0.9, 1.0, 1.2))


def lights_only(trt):
    """Two light quads: every hit ends its path."""
    geos = [("quad", (-3.0, -2.0, 5.0), (2.5, 0.0, 0.0), (0.0, 4.0, 0.0), "light"), ("quad", (0.5, -2.0, 6.0), (2.5, 0.0, 0.0), (0.0, 4.0, 0.0), "light")]
    return _scene(trt, "lights_only", geos, T._cam((0.0, 0.0, -4.0), (0.0, 0.0, 5.0)), background=(0.1, 0.2, 0.3))


LAMP = ("quad", (-2.0, 9.9, 3.0), (4.0, 0.0, 0.0), (0.0, 0.0, 4.0), "light")


def metal_room(trt):
    return _room(trt, [("quad", (-3.0, 1.0, 8.0), (6.0, 0.0, 0.0), (0.0, 6.0, 0.0), "metal"), LAMP], "metal_room")


def glass_room(trt):
    return _room(trt, [("quad", (-3.0, 1.0, 6.0), (6.0, 0.0, 0.0), (0.0, 6.0, 0.0), "glass"), LAMP], "glass_room")


def tilted_quad(trt):
    """A room with one quad that is not axis-exact: the handle's axis-exact switch is off, and with it the nearest-first one."""
    return _room(trt, [("quad", (-3.0, 1.0, 6.0), (6.0, 0.0, 1.0), (0.0, 6.0, 2.0), "red"), LAMP], "tilted_quad")


def thirty_three_quads(trt):
    """One leaf more than a scene's own kernel takes: nothing is claimed (facts test only; never rendered here)."""
    geos = [("quad", (-5.0 + 0.3 * i, 0.0, 2.0), (0.25, 0.0, 0.0), (0.0, 0.0, 2.0), "white") for i in range(32)] + [LAMP]
    return _scene(trt, "thirty_three_quads", geos, T._cam((0.0, 4.0, -7.0), (0.0, 1.0, 5.0)))


NEW = {"closed_room": closed_room, "floor_under_sky": floor_under_sky, "lights_only": lights_only, "metal_room": metal_room, "glass_room": glass_room,
       "tilted_quad": tilted_quad}
SCENES = dict(T.SCENES, **NEW)
DEPTH = {name: T.DEPTH for name in SCENES}
DEPTH["closed_room"] = 3
TUNING = T.TUNING
BIG = dict(name="cornell_128", width=128, height=128, spp=8)          # several batches per wave, refills between rounds, idle lanes at the tail

# what trt_scene_facts gives with the library's defaults
FACTS = {
    "cornell": ALL_SWITCHES | STRAIGHT | LAMBERTIAN | LIGHT,
    "one_quad": ALL_SWITCHES | STRAIGHT | LIGHT,
    "three_quads": ALL_SWITCHES | LAMBERTIAN | METAL | LIGHT,
    "thirty_two_quads": ALL_SWITCHES | LAMBERTIAN | METAL | DIELECTRIC | LIGHT,
    "coplanar_and_signed_zero": ALL_SWITCHES | LAMBERTIAN | METAL | DIELECTRIC | LIGHT,
    "wide_room": ALL_SWITCHES | LAMBERTIAN | METAL | DIELECTRIC | LIGHT,
    "quads_and_a_sphere": LAZY | LAMBERTIAN | DIELECTRIC | LIGHT,                       # a sphere: nothing that depends on "no sphere"
    "closed_room": ALL_SWITCHES | STRAIGHT | LAMBERTIAN,                                # kinds exclude light
    "floor_under_sky": ALL_SWITCHES | STRAIGHT | LAMBERTIAN,
    "lights_only": ALL_SWITCHES | STRAIGHT | LIGHT,
    "metal_room": ALL_SWITCHES | LAMBERTIAN | METAL | LIGHT,
    "glass_room": ALL_SWITCHES | LAMBERTIAN | DIELECTRIC | LIGHT,
    "tilted_quad": NO_SPHERE | LAZY | STRAIGHT | LAMBERTIAN | LIGHT,                    # not axis-exact, hence not nearest-first
}

# argv: repository root, output .npz, scene names ... ("cornell_128": BIG).  Every scene is rendered twice on one handle.
CHILD = r"""
import os
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
trt = __import__("tiny-raytracer_amd")
import scene_facts_scenes as S
out = {}
for name in sys.argv[3:]:
    before = trt.lib.trt_flat_literal_compilations()
    big = name == S.BIG["name"]
    desc = trt.scenes.cornell(S.BIG["width"], S.BIG["height"]) if big else S.SCENES[name](trt)
    pw, pcam = trt.world_from_description(desc)
    scene = pw.get_bvh()
    r = trt.Renderer(S.BIG["spp"] if big else S.SPP, 1, S.T.DEPTH if big else S.DEPTH[name], False, desc["background"], seed=S.SEED, backend=S.T.STREAMED)
    r.tuning = dict(S.TUNING.get(name, {}))
    plan = r.launch_plan(pcam, scene)
    assert plan["walk"] == S.T.WALK_FLAT and plan["kernel_walk"] == S.T.WALK_FLAT, plan
    out[name + "_frame"] = r.render(pcam, scene).data
    out[name + "_unit_facts"] = np.array([trt.lib.trt_flat_literal_facts()], np.uint64)      # of the unit that render compiled and launched
    out[name + "_counters"] = np.array([r.last_stats["samples"], r.last_stats["rays"]], np.uint64)
    out[name + "_again"] = r.render(pcam, scene).data
    out[name + "_compilations"] = np.array([trt.lib.trt_flat_literal_compilations() - before], np.uint64)
    out[name + "_facts"] = np.array([trt.lib.trt_scene_facts(scene._h)], np.uint64)
out["diagnostic"] = np.array([trt.lib.trt_flat_literal_diagnostic().decode()])
np.savez(sys.argv[2], **out)
"""
