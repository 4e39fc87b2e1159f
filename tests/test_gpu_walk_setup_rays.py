"""The short walk setup (rt_path.h trav_begin) ray by ray: caller-supplied rays through trt_intersect_device whose direction components
sit at the edges of the setup's range guard, against the oracle's closest hit - the bits of t and the primitive, no tolerance.

Queries take directions as given (never normalised), so a component can be any float.  Per scene, for each of four targets (primitive
centres), each axis, each edge value and each sign, two rays: the target direction with that one component replaced, once from a
fixed origin inside the scene and once from the origin that puts the target at t = 1 (huge, infinite or NaN where the component is).
Edge values: 2^-40 and 2^40 (the guard's ends), their neighbours outside and inside, 2^-41 and 2^41, 2^-60 and 2^60 (the ends of the
nearest-first and compact domains of 1/d), 0, a subnormal, inf and NaN.  They are shuffled among ordinary rays (seeded) and sent in
batches of 64 and of 65 + 64, so that a wave holds lanes that take the short setup beside lanes that take the plain one.

Scenes: Cornell (lock-step walk, axis-exact quads, nearest-first leaf phase), the reference's five-sphere world as the lock-step list
(its sphere tests are the ones whose d.d stays in the leaf phase) and as an LDS tree (flat_walk=0), and sphere_grid(669), the smallest
grid that no longer fits LDS: 16-byte nodes from global memory, where the compact domain's origin limit applies too."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MISS = 0xFFFFFFFF
LDS, GLOBAL = 1, 0
LDS_TREE, LOCK_STEP, NODES16 = 1, 2, 3                                      # trt_launch_plan.walk
F = np.float32
EDGES = [F(2.0 ** -40), np.nextafter(F(2.0 ** -40), F(0)), np.nextafter(F(2.0 ** -40), F(1)), F(2.0 ** 40), np.nextafter(F(2.0 ** 40), F(np.inf)),
         np.nextafter(F(2.0 ** 40), F(0)), F(2.0 ** -41), F(2.0 ** 41), F(2.0 ** -60), F(2.0 ** 60), F(0.0), F(1e-40), F(np.inf), F(np.nan)]
# name -> (description, scene options, (scene mode, walk) the query plan must show, origin inside the scene)
CASES = {
    "cornell": (lambda trt: trt.scenes.cornell(8, 8), {}, (LDS, LOCK_STEP), (52.0, 71.0, 5.0)),
    "dummy_spheres_lock_step": (lambda trt: trt.scenes.dummy_spheres("renderer", 8, 8), {}, (LDS, LOCK_STEP), (0.1, 0.6, 1.5)),
    "dummy_spheres_lds_tree": (lambda trt: trt.scenes.dummy_spheres("renderer", 8, 8), dict(flat_walk=0), (LDS, LDS_TREE), (0.1, 0.6, 1.5)),
    "grid669_global": (lambda trt: trt.scenes.sphere_grid(669, 8, 8), {}, (GLOBAL, NODES16), None),
}


def centre(g):
    """A point of geometry g of a scene description: a sphere's centre, a quad's middle."""
    if g[0] == "sphere":
        return np.asarray(g[1], np.float64)
    return np.asarray(g[1], np.float64) + 0.5 * np.asarray(g[2], np.float64) + 0.5 * np.asarray(g[3], np.float64)


def edge_rays(desc, inside):
    geos = desc["geometries"]
    targets = [centre(geos[k]) for k in np.linspace(0, len(geos) - 1, 4).astype(int)]
    rng = np.random.default_rng(20)
    rays, is_edge = [], []
    with np.errstate(over="ignore", invalid="ignore"):
        for p in targets:
            base = p - inside
            base = base / np.linalg.norm(base) if np.linalg.norm(base) > 0 else np.array([0.3, 0.5, 0.8])
            for axis in range(3):
                for v in EDGES:
                    for sign in (1.0, -1.0):
                        d = base.astype(np.float32)
                        d[axis] = F(sign) * v
                        rays.append(np.concatenate([np.asarray(inside, np.float32), d]))
                        rays.append(np.concatenate([(p.astype(np.float32) - d).astype(np.float32), d]))
                        is_edge += [True, True]
            for _ in range(84):                                              # ordinary rays towards and around the target, as many as edge ones
                d = (base + 0.3 * rng.standard_normal(3)) * rng.uniform(0.25, 4.0)
                rays.append(np.concatenate([np.asarray(inside, np.float32), d.astype(np.float32)]))
                is_edge.append(False)
    rays, is_edge = np.asarray(rays, np.float32), np.asarray(is_edge)
    order = np.random.default_rng(21).permutation(len(rays))
    return np.ascontiguousarray(rays[order]), is_edge[order]


@pytest.mark.parametrize("name", list(CASES))
def test_rays_at_the_guards_edges_get_the_oracles_hit(trt, orc, name):
    import torch
    make, options, shape, inside = CASES[name]
    desc = make(trt)
    world = trt.world_from_description(desc)[0]
    sc = trt.Scene(world, **options) if options else world.get_bvh()
    plan = sc.query_plan(129)
    assert (plan["scene_mode"], plan["walk"]) == shape and plan["fallback"] == 0, (name, plan)
    if inside is None:                                                       # the grid: a point above its middle
        pts = np.array([centre(g) for g in desc["geometries"]])
        inside = tuple(pts.mean(axis=0) + np.array([0.0, 3.0 * pts[:, 1].std() + 1.0, 0.0]))
    rays, is_edge = edge_rays(desc, np.asarray(inside, np.float64))
    ow, _ = orc.world_from_description(desc)
    hit, t, geo = ow.hit_index_batch(rays)
    in_range = np.all((np.abs(rays[:, 3:]) >= F(2.0 ** -40)) & (np.abs(rays[:, 3:]) <= F(2.0 ** 40)), axis=1)
    print(f"\n{name}: {len(rays)} rays, {int(is_edge.sum())} with an edge component, {int(in_range.sum())} inside the guard's range, "
          f"oracle hit share {hit.mean():.2f} ({hit[in_range].mean():.2f} inside, {hit[~in_range].mean():.2f} outside)")
    assert hit[in_range].any() and hit[~in_range].any() and (~hit).any()    # both kinds of lane hit something, and some ray misses
    rays_d = torch.from_numpy(rays).cuda()
    for batch in (64, 65 + 64):
        out = torch.full((len(rays) * 28,), 0xCD, dtype=torch.uint8, device=rays_d.device)
        for b in range(0, len(rays), batch):
            n = min(batch, len(rays) - b)
            sc.intersect_device(rays_d.data_ptr() + 24 * b, n, out.data_ptr() + 28 * b)
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(trt.HIT_DTYPE)
        bad = np.flatnonzero((got["geometry"] != MISS) != hit)
        assert len(bad) == 0, (name, batch, "hit?", len(bad), bad[:5], rays[bad[:5]])
        bad = np.flatnonzero(got["t"].view(np.uint32) != t.view(np.uint32))
        assert len(bad) == 0, (name, batch, "t", len(bad), bad[:5], rays[bad[:5]], got["t"][bad[:5]], t[bad[:5]])
        bad = np.flatnonzero(got["geometry"][hit].astype(np.int64) != geo[hit].astype(np.int64))
        assert len(bad) == 0, (name, batch, "primitive", len(bad), bad[:5])
