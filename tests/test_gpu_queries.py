"""Ray queries (trt_intersect / trt_occluded and their device forms) against the oracle's BVH closest hit, ray by ray, no tolerance:
hit?, the bits of t, the geometry INSERTION index, material, front_face and the bits of the normal equal orc_world_hit_index(ray, 0.001,
t_max) - BVH::hit with the leaf boxes' part in the answer, not a brute-force loop.

Scenes (tests/walk_ray_cases.py): cornell (lock-step list, quads), prims33 (the first LDS tree), random_spheres and mixed400 (LDS trees,
768 lanes), prims600 (an LDS copy of 59 680 B: register slots at 512 lanes, reached through the fallback of the launch plan), grid3000 and
grid3000_far_sphere (16-byte nodes from global memory, both sides of the fused loop's domain), degenerate, nonfinite.  Rays:
every class of RayMaker(...).classes(48), concatenated and shuffled with a fixed seed - 352 to 424 per scene, the smallest sets that
still hold every ray class the walks can get wrong.  Per scene the oracle's hit share must lie in [0.1, 0.9], so neither hits nor misses
go untested; no ray is ever dropped from a comparison.

mixed400 interleaves spheres and quads in insertion order: an implementation that reported the kernels' own primitive reference (index
within its kind) instead of the insertion index fails the closest-hit check there.

PLAN_CASES lists every (scene, scene options) this module asks, with the kernel shape (Scene.query_plan) it was chosen for; each test
that compiles a scene asserts that shape, and tests/test_query_abi.py checks without a GPU that the list reaches every instantiation of
query.hip kQueryKernels and every route to the register-slot fallback.

Batches: the oracle comparisons ask a few hundred rays (two waves of workgroup 0).  test_batches_past_one_workgroup tiles those rays on
the device to the first ray of workgroup 1, to 100 003 rays and to the smallest batch that lengthens a wave's run beyond 256 rays on
the device at hand (some millions), and compares every record with the oracle-checked answer of its ray on the device.

Every GPU step is one in-process call; nothing is built here and no child process is started."""
import numpy as np
import pytest

import walk_ray_cases as W

pytestmark = pytest.mark.gpu

LDS, GLOBAL = 1, 0
LDS_TREE, LOCK_STEP, NODES16, REGISTER_SLOTS = 1, 2, 3, 5                   # trt_launch_plan.walk
# scene -> (scene mode, walk, threads per workgroup, register-slot fallback taken) of the query kernel its default compilation is here to run
DEFAULT_SHAPES = {
    "cornell": (LDS, LOCK_STEP, 256, 0), "prims33": (LDS, LDS_TREE, 256, 0), "random_spheres": (LDS, LDS_TREE, 768, 0),
    "mixed400": (LDS, LDS_TREE, 768, 0), "prims600": (LDS, REGISTER_SLOTS, 512, 1),                 # planned as LDS tree / 512 lanes: no instantiation
    "grid3000": (GLOBAL, NODES16, 256, 0), "grid3000_far_sphere": (GLOBAL, NODES16, 256, 0),
    "degenerate": (LDS, LOCK_STEP, 256, 0), "nonfinite": (LDS, LOCK_STEP, 256, 0),
}
SCENES = list(DEFAULT_SHAPES)
# scenes compiled with another placement option (another walk), or by the device compiler, and the shape each is here to run
OTHER_WALKS = [
    ("cornell", dict(flat_walk=0), (LDS, LDS_TREE, 256, 0)),
    ("prims33", dict(flat_walk=1), (LDS, LOCK_STEP, 256, 0)),                                       # the lock-step list with more than 32 leaves
    ("grid3000", dict(compact_nodes=0), (GLOBAL, REGISTER_SLOTS, 256, 1)),                          # planned as a tree walk on 32-byte nodes
    ("grid3000", dict(compact_nodes=-1), (GLOBAL, NODES16, 256, 0)),
    ("random_spheres", dict(on_device=True), (LDS, LDS_TREE, 768, 0)),
    ("grid3000", dict(on_device=True), (GLOBAL, NODES16, 256, 0)),
    ("mixed400", dict(flat_walk=1), (LDS, REGISTER_SLOTS, 512, 1)),                                 # planned as lock-step list / 768 lanes
    ("grid3000", dict(flat_walk=1, compact_nodes=0), (GLOBAL, REGISTER_SLOTS, 256, 1)),             # planned as lock-step list from global memory
    ("prims600", dict(flat_walk=1), (LDS, REGISTER_SLOTS, 512, 0)),                                 # the streamed plan's own walk: no fallback
    ("prims600", dict(on_device=True), (LDS, REGISTER_SLOTS, 512, 1)),
]
PLAN_CASES = [(name, {}, shape) for name, shape in DEFAULT_SHAPES.items()] + OTHER_WALKS


def plan_shape(q):
    return (q["scene_mode"], q["walk"], q["threads_per_workgroup"], q["fallback"])
MISS = 0xFFFFFFFF
INF_BITS = 0x7F800000


def miss_records(n, trt):
    r = np.zeros(n, trt.HIT_DTYPE)
    r["t"] = np.inf
    r["geometry"] = MISS
    r["material"] = MISS
    return r


def oracle_records(trt, orc, ow, rays, t_max=None):
    """trt_hit records from orc_world_hit_index, one call per ray (t_max[i] NaN: not asked, a miss by the documented rule)."""
    out = miss_records(len(rays), trt)
    nan_normal = np.zeros((len(rays), 3), bool)
    for i, r in enumerate(rays):
        t1 = float("inf") if t_max is None else float(t_max[i])
        if t1 != t1:
            continue
        rec, idx = ow.hit_index(orc.Ray(orc.Vec3(*r[:3]), orc.Vec3(*r[3:])), 0.001, t1)
        if rec is None:
            assert idx == -1
            continue
        out[i] = (rec.t, idx, rec.material, rec.front_face, tuple(rec.normal.tolist()))
        nan_normal[i] = np.isnan(out[i]["normal"])
    return out, nan_normal


def assert_records_equal(got, want, nan_normal, what):
    for f in ("geometry", "material", "front_face"):
        bad = np.flatnonzero(got[f] != want[f])
        assert len(bad) == 0, (what, f, len(bad), bad[:5], got[f][bad[:5]], want[f][bad[:5]])
    bad = np.flatnonzero(got["t"].view(np.uint32) != want["t"].view(np.uint32))
    assert len(bad) == 0, (what, "t", len(bad), bad[:5], got["t"][bad[:5]], want["t"][bad[:5]])
    gn, wn = got["normal"], want["normal"]
    same = np.where(nan_normal, np.isnan(gn) == np.isnan(wn), gn.view(np.uint32) == wn.view(np.uint32))      # a NaN component: NaN-ness, else bits
    bad = np.flatnonzero(~same.all(axis=1))
    assert len(bad) == 0, (what, "normal", len(bad), bad[:5], gn[bad[:5]], wn[bad[:5]])
    miss = want["geometry"] == MISS
    assert got[miss].tobytes() == want[miss].tobytes(), (what, "miss records differ from the documented miss record")


def t_max_cases(t_inf, hit):
    """One of the nine interval ends per ray, in turn by index, from the oracle's hit distance t for t_max = inf; rays that miss (t = inf)
    also get 1.0 and 1e30."""
    n = len(t_inf)
    t = t_inf.astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        table = [np.full(n, np.inf, np.float32), t, np.nextafter(t, np.float32(np.inf)), (np.float32(0.5) * t).astype(np.float32),
                 (np.float32(2.0) * t).astype(np.float32), np.full(n, 0.001, np.float32), np.full(n, 0.0005, np.float32),
                 np.full(n, -1.0, np.float32), np.full(n, np.nan, np.float32), np.full(n, 1.0, np.float32), np.full(n, 1e30, np.float32)]
    which = np.where(hit, np.arange(n) % 9, np.arange(n) % 11)
    return np.choose(which, table).astype(np.float32), which


@pytest.fixture(scope="module")
def case(trt, orc):
    """name -> everything about one scene, computed once on first use and shared: description, oracle world, default product scene, rays,
    the oracle's answers for t_max = inf and for the per-ray t_max table."""
    cache = {}

    def get(name):
        if name in cache:
            return cache[name]
        desc = W.scene(trt, name)
        ow, _ = orc.world_from_description(desc)
        bbox, prim, _ = ow.bvh_dump()
        world = trt.world_from_description(desc)[0]
        sc = world.get_bvh()
        lds = sc.info()["lds_bytes"] > 0
        assert plan_shape(sc.query_plan(1)) == DEFAULT_SHAPES[name], (name, sc.query_plan(1))
        compact = sc.compact_nodes() is not None and not lds
        limit = W.origin_limit(sc.cull_nodes()[0][0]) if compact else None
        classes = W.RayMaker(desc, bbox, prim, limit=limit).classes(48)
        rays = np.concatenate(list(classes.values())).astype(np.float32)
        rays = np.ascontiguousarray(rays[np.random.default_rng([W.SEED, 4242]).permutation(len(rays))])
        hit, t, geo = ow.hit_index_batch(rays)
        share = float(hit.mean())
        print(f"\n{name}: {len(desc['geometries'])} primitives, {len(rays)} rays, oracle hit share {share:.2f}, "
              f"{'LDS' if lds else 'global memory'}{', 16-byte nodes' if compact else ''}")
        assert 0.1 <= share <= 0.9, (name, share)
        want, nan_normal = oracle_records(trt, orc, ow, rays)
        assert np.array_equal(want["geometry"] != MISS, hit) and np.array_equal(want["t"].view(np.uint32), t.view(np.uint32))
        assert np.array_equal(want["geometry"].astype(np.int64)[hit], geo[hit].astype(np.int64))
        tm, which = t_max_cases(t, hit)
        want_tm, nan_normal_tm = oracle_records(trt, orc, ow, rays, tm)
        cache[name] = dict(desc=desc, ow=ow, world=world, scene=sc, lds=lds, compact=compact, rays=rays, hit=hit, t=t, geo=geo, want=want,
                           nan_normal=nan_normal, t_max=tm, which=which, want_tm=want_tm, nan_normal_tm=nan_normal_tm)
        return cache[name]

    return get


@pytest.mark.parametrize("name", SCENES)
def test_closest_hit_is_the_oracles(trt, case, name):
    c = case(name)
    got = c["scene"].intersect(c["rays"])
    # the batch answers first: hit?, the bits of t, the geometry insertion index
    assert np.array_equal(got["geometry"] != MISS, c["hit"])
    assert np.array_equal(got["t"].view(np.uint32), c["t"].view(np.uint32))
    assert np.array_equal(got["geometry"][c["hit"]].astype(np.int64), c["geo"][c["hit"]].astype(np.int64))
    assert_records_equal(got, c["want"], c["nan_normal"], name)
    nan_ray = np.isnan(c["rays"]).any(axis=1)
    assert nan_ray.any() and (got["geometry"][nan_ray] == MISS).all()                            # a ray with a NaN component hits nothing
    assert got[~c["hit"]].tobytes() == miss_records(int((~c["hit"]).sum()), trt).tobytes()


@pytest.mark.parametrize("name", SCENES)
def test_per_ray_t_max(trt, case, name):
    c = case(name)
    tm, which, want = c["t_max"], c["which"], c["want_tm"]
    got = c["scene"].intersect(c["rays"], tm)
    assert_records_equal(got, want, c["nan_normal_tm"], name)
    hit_inf = c["hit"]
    miss = got["geometry"] == MISS
    assert miss[np.isnan(tm)].all() and np.isnan(tm).sum() > 0                                   # NaN: a miss, asserted directly
    assert miss[hit_inf & (which == 1)].all() and (hit_inf & (which == 1)).sum() > 0              # t_max = t: the end is exclusive
    assert miss[np.isin(which, (5, 6, 7))].all()                                                # 0.001, 0.0005, -1: an empty range
    kept = hit_inf & (which == 2)
    same = got["geometry"][kept].astype(np.int64) == c["geo"][kept]
    print(f"\n{name}: t_max = nextafter(t): {int(same.sum())} of {int(kept.sum())} rays keep their primitive; "
          f"t_max = 0.5 t: {int((~miss[hit_inf & (which == 3)]).sum())} of {int((hit_inf & (which == 3)).sum())} hit something nearer")
    assert (got["geometry"][hit_inf & (which == 0)].astype(np.int64) == c["geo"][hit_inf & (which == 0)]).all()


@pytest.mark.parametrize("name", SCENES)
def test_occlusion_is_intersects_hit_flag(trt, case, name):
    c = case(name)
    sc = c["scene"]
    for tm, want in ((None, c["want"]), (c["t_max"], c["want_tm"])):
        occ = sc.occluded(c["rays"], tm)
        raw = occ.view(np.uint8)
        assert ((raw == 0) | (raw == 1)).all()
        bad = np.flatnonzero(occ != (want["geometry"] != MISS))
        assert len(bad) == 0, (name, tm is None, len(bad), bad[:5], c["rays"][bad[:5]])
        assert 0 < int(occ.sum()) < len(occ)


def _device_query(trt, sc, rays_d, n, t_max_d, any_hit, stream_ptr=0, pad=64):
    """One device-form call on torch tensors; the output is `pad` records longer and pre-filled with 0xCD.  Returns the whole buffer (uint8 tensor)."""
    import torch
    item = 1 if any_hit else 28
    out = torch.full(((n + pad) * item,), 0xCD, dtype=torch.uint8, device=rays_d.device)
    fn = sc.occluded_device if any_hit else sc.intersect_device
    fn(rays_d.data_ptr(), n, out.data_ptr(), t_max_d.data_ptr() if t_max_d is not None else 0, stream_ptr)
    return out


@pytest.mark.parametrize("name", ["cornell", "random_spheres", "grid3000"])
def test_batch_shapes_write_every_record_and_nothing_behind(trt, case, name):
    """Prefixes of 1, 63, 64, 65 and 257 rays and the full set, both query kinds, through the device forms: records [0, n) equal the
    host form's, the 64 records behind n keep their 0xCD fill."""
    import torch
    c = case(name)
    sc, rays = c["scene"], c["rays"]
    dev = torch.device("cuda:0")
    rays_d = torch.from_numpy(rays).to(dev)
    tm_d = torch.from_numpy(c["t_max"]).to(dev)
    full_hits = sc.intersect(rays, c["t_max"])
    full_occ = sc.occluded(rays, c["t_max"]).view(np.uint8)
    for n in (1, 63, 64, 65, 257, len(rays)):
        for any_hit in (False, True):
            item = 1 if any_hit else 28
            out = _device_query(trt, sc, rays_d, n, tm_d, any_hit)
            torch.cuda.synchronize()
            h = out.cpu().numpy()
            assert (h[n * item:] == 0xCD).all(), (name, n, any_hit, "bytes behind the batch were written")
            want = (full_occ[:n] if any_hit else full_hits[:n]).tobytes()
            assert h[:n * item].tobytes() == want, (name, n, any_hit)
    # n == 0 succeeds and touches nothing
    out = _device_query(trt, sc, rays_d, 0, None, False)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xCD).all()
    assert len(sc.intersect(np.zeros((0, 6), np.float32))) == 0 and len(sc.occluded(np.zeros((0, 6), np.float32))) == 0


@pytest.mark.parametrize("name", ["mixed400", "grid3000_far_sphere"])
def test_device_forms_equal_the_host_form_on_any_stream(trt, case, name):
    import torch
    c = case(name)
    sc, rays, n = c["scene"], c["rays"], len(c["rays"])
    dev = torch.device("cuda:0")
    rays_d = torch.from_numpy(rays).to(dev)
    tm_d = torch.from_numpy(c["t_max"]).to(dev)
    host = {(False, False): sc.intersect(rays).tobytes(), (False, True): sc.intersect(rays, c["t_max"]).tobytes(),
            (True, False): sc.occluded(rays).view(np.uint8).tobytes(), (True, True): sc.occluded(rays, c["t_max"]).view(np.uint8).tobytes()}
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for any_hit in (False, True):
        for with_tm in (False, True):
            item = 1 if any_hit else 28
            a = _device_query(trt, sc, rays_d, n, tm_d if with_tm else None, any_hit)                    # default stream
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                b = _device_query(trt, sc, rays_d, n, tm_d if with_tm else None, any_hit, side.cuda_stream)
            side.synchronize()
            torch.cuda.synchronize()
            assert a.cpu().numpy()[:n * item].tobytes() == host[(any_hit, with_tm)], (name, any_hit, with_tm, "default stream")
            assert b.cpu().numpy()[:n * item].tobytes() == host[(any_hit, with_tm)], (name, any_hit, with_tm, "side stream")


def test_queries_and_a_render_enqueued_back_to_back(trt, case):
    """Two queries and a small render of one scene on one stream without a synchronisation in between: each gives its stand-alone answer."""
    import torch
    c = case("cornell")
    sc, rays, n = c["scene"], c["rays"], len(c["rays"])
    desc = dict(c["desc"])
    cam = trt.Camera(**dict(desc["camera"], width=32, height=32))
    r = trt.Renderer(2, 1, 4, False, desc["background"], seed=3)
    alone = r.render(cam, sc).data
    want_hits, want_occ = sc.intersect(rays).tobytes(), sc.occluded(rays).view(np.uint8).tobytes()
    dev = torch.device("cuda:0")
    rays_d = torch.from_numpy(rays).to(dev)
    acc = torch.zeros((32, 32, 3), dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        hits = _device_query(trt, sc, rays_d, n, None, False, stream.cuda_stream)
        r.render_device(cam, sc, acc.data_ptr(), stream.cuda_stream)
        occ = _device_query(trt, sc, rays_d, n, None, True, stream.cuda_stream)
    stream.synchronize()
    assert hits.cpu().numpy()[:n * 28].tobytes() == want_hits
    assert occ.cpu().numpy()[:n].tobytes() == want_occ
    assert np.array_equal(acc.cpu().numpy().view(np.uint32), alone.view(np.uint32))


@pytest.mark.parametrize("name,options", [(name, options) for name, options, _ in OTHER_WALKS])
def test_every_walk_and_both_compilers_answer_alike(trt, case, name, options):
    """The scene compiled with another placement option (another walk: LDS tree instead of the lock-step list and the reverse, register
    slots instead of 16-byte nodes, the register-slot fallback on a scene compiled for the lock-step list) or by the device compiler:
    it launches the kernel shape it is listed for, and all answers are the default scene's, byte for byte."""
    shape = next(s for n, o, s in OTHER_WALKS if (n, o) == (name, options))
    c = case(name)
    other = c["world"].get_bvh(**options)
    assert other is not c["scene"]
    assert plan_shape(other.query_plan(len(c["rays"]))) == shape, (name, options, other.query_plan(len(c["rays"])))
    for tm in (None, c["t_max"]):
        assert other.intersect(c["rays"], tm).tobytes() == c["scene"].intersect(c["rays"], tm).tobytes(), (name, options)
        assert other.occluded(c["rays"], tm).tobytes() == c["scene"].occluded(c["rays"], tm).tobytes(), (name, options)
    assert_records_equal(other.intersect(c["rays"]), c["want"], c["nan_normal"], (name, options))


def _first_mismatches(out, n, item, want_d, idx):
    """Record i of the device buffer `out` against record idx[i] of want_d ([P, item] uint8), compared on the device; the bytes behind
    record n against the 0xCD fill.  Returns (indices of the first differing records, copied back only on a mismatch; tail intact?)."""
    import torch
    got = out[:n * item].view(n, item)
    want = want_d[idx]
    bad = []
    if not torch.equal(got, want):
        bad = (got != want).any(dim=1).nonzero().flatten()[:5].cpu().tolist()
    return bad, bool((out[n * item:] == 0xCD).all())


@pytest.mark.parametrize("name", ["cornell", "random_spheres", "prims600", "grid3000"])
def test_batches_past_one_workgroup(trt, case, name):
    """The scene's P rays and its t_max table tiled on the device to n rays (ray i = ray i mod P; P is no power of two, so every wave sees
    another phase of lane mixes, refills and parked stragglers), through both device forms with and without t_max: record i is the byte
    image of record i mod P of the host form's answer for the P rays - which the tests above compare with the oracle - and the 64 records
    behind the batch keep their fill.  n: the first ray of workgroup 1, 100 003, and the smallest batch that makes launch_query lengthen a
    wave's run beyond 256 rays on this device (256 x wave slots + 1: the non-resumable loop over more than four rounds, the resumable
    refill over more than four refills, per-wave runs rounded to 64)."""
    import torch
    c = case(name)
    sc, rays, P = c["scene"], c["rays"], len(c["rays"])
    assert P & (P - 1) != 0 and 352 <= P <= 424
    dev = torch.device("cuda:0")
    base = sc.query_plan(1)
    assert plan_shape(base) == DEFAULT_SHAPES[name]
    waves_per_wg = base["threads_per_workgroup"] // 64
    sizes = [256 * waves_per_wg + 1, 100003, 256 * base["wave_slots"] + 1]
    assert sizes[0] == {256: 1025, 512: 2049, 768: 3073}[base["threads_per_workgroup"]] and sizes[2] > sizes[1]
    rays_d = torch.from_numpy(rays).to(dev)
    tm_d = torch.from_numpy(c["t_max"]).to(dev)
    want = {(False, False): sc.intersect(rays), (False, True): sc.intersect(rays, c["t_max"]),
            (True, False): sc.occluded(rays).view(np.uint8), (True, True): sc.occluded(rays, c["t_max"]).view(np.uint8)}
    assert_records_equal(want[(False, False)], c["want"], c["nan_normal"], name)
    assert_records_equal(want[(False, True)], c["want_tm"], c["nan_normal_tm"], name)
    want_d = {k: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(P, -1)).to(dev) for k, v in want.items()}
    for n in sizes:
        q = sc.query_plan(n)
        assert q["workgroups"] > 1 and q["waves"] * q["rays_per_wave"] >= n > (q["waves"] - 1) * q["rays_per_wave"]
        if n == sizes[2]:
            assert q["rays_per_wave"] == 320 and sc.query_plan(n - 1)["rays_per_wave"] == 256 and q["waves"] <= q["wave_slots"], q
            print(f"\n{name}: n = {n} rays on {q['compute_units']} CUs, walk {q['walk']} at {q['threads_per_workgroup']} threads: "
                  f"{q['rays_per_wave']} rays per wave, {q['waves']} waves, {q['workgroups']} workgroups")
        else:
            assert q["rays_per_wave"] == 256, q
        idx = torch.arange(n, device=dev) % P
        big_rays = rays_d[idx].contiguous()
        big_tm = tm_d[idx].contiguous()
        for any_hit in (False, True):
            for with_tm in (False, True):
                item = 1 if any_hit else 28
                out = _device_query(trt, sc, big_rays, n, big_tm if with_tm else None, any_hit)
                torch.cuda.synchronize()
                bad, tail_intact = _first_mismatches(out, n, item, want_d[(any_hit, with_tm)], idx)
                assert not bad, (name, n, any_hit, with_tm, "first differing rays", bad, [i % P for i in bad], q)
                assert tail_intact, (name, n, any_hit, with_tm, "bytes behind the batch were written")
                if n == sizes[1] and with_tm:
                    # negative control: against the answers shifted by one ray the same comparison reports a mismatch
                    shifted, _ = _first_mismatches(out, n, item, torch.roll(want_d[(any_hit, with_tm)], 1, 0), idx)
                    assert shifted, (name, any_hit, "the comparison cannot see a batch that is off by one ray")
                del out
        del idx, big_rays, big_tm


@pytest.mark.parametrize("name", ["cornell", "random_spheres", "grid3000"])
def test_host_forms_with_batch_sizes_that_are_no_multiple_of_16_bytes(trt, case, name):
    """query_host places t_max behind the rays and the answers behind t_max, each rounded up to 16 bytes: prefixes of 1, 3, 63 and 65 rays
    (24 n and 4 n no multiples of 16) through the host forms, with and without t_max, equal the prefix of the full answer."""
    c = case(name)
    sc, rays, tm = c["scene"], c["rays"], c["t_max"]
    for t in (None, tm):
        full_hits = sc.intersect(rays, t)
        full_occ = sc.occluded(rays, t).view(np.uint8)
        assert_records_equal(full_hits, c["want"] if t is None else c["want_tm"], c["nan_normal"] if t is None else c["nan_normal_tm"], name)
        for n in (1, 3, 63, 65):
            assert (24 * n) % 16 != 0 and (4 * n) % 16 != 0
            tn = None if t is None else np.ascontiguousarray(t[:n])
            assert sc.intersect(np.ascontiguousarray(rays[:n]), tn).tobytes() == full_hits[:n].tobytes(), (name, n, t is None)
            assert sc.occluded(np.ascontiguousarray(rays[:n]), tn).view(np.uint8).tobytes() == full_occ[:n].tobytes(), (name, n, t is None)


def _run_behind_a_barrier(jobs):
    """Every job on a host thread of its own, released together; returns their results in order (an exception in a thread is raised here)."""
    import threading
    barrier = threading.Barrier(len(jobs))
    results, errors = [None] * len(jobs), []

    def run(i):
        try:
            barrier.wait()
            results[i] = jobs[i]()
        except BaseException as e:                                         # noqa: B036 - reported by the test, below
            errors.append((i, e))
            barrier.abort()

    threads = [threading.Thread(target=run, args=(i,)) for i in range(len(jobs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    return results


def test_first_use_of_a_fresh_scene_from_several_threads(trt, case):
    """Eight host threads make the first query on a scene no call has touched yet (capi.hip query_scene_on_device: one thread uploads the
    scene and the index table, the others wait for it): every answer is the oracle-checked one.  Then once more on a second fresh scene
    whose first calls are renders and queries mixed."""
    c = case("mixed400")
    rays, desc = c["rays"], c["desc"]
    want_hits, want_occ = c["scene"].intersect(rays), c["scene"].occluded(rays)
    assert_records_equal(want_hits, c["want"], c["nan_normal"], "mixed400")
    assert np.array_equal(want_occ, c["want"]["geometry"] != MISS)

    fresh = c["world"].get_bvh(flat_walk=-1)                                # (an option given: compiled anew, never cached; -1 is the default)
    assert fresh is not c["scene"] and plan_shape(fresh.query_plan(len(rays), 256)) == DEFAULT_SHAPES["mixed400"]
    answers = _run_behind_a_barrier([lambda: (fresh.intersect(rays), fresh.occluded(rays))] * 8)
    for k, (hits, occ) in enumerate(answers):
        assert hits.tobytes() == want_hits.tobytes(), ("thread", k)
        assert np.array_equal(occ, want_occ), ("thread", k)

    cam = trt.Camera(**dict(desc["camera"], width=32, height=32))
    alone = trt.Renderer(2, 1, 4, False, desc["background"], seed=3).render(cam, c["scene"]).data
    fresh2 = c["world"].get_bvh(flat_walk=-1)
    assert fresh2 is not fresh and fresh2 is not c["scene"]

    def render():
        return trt.Renderer(2, 1, 4, False, desc["background"], seed=3).render(cam, fresh2).data

    answers = _run_behind_a_barrier([render, lambda: fresh2.intersect(rays), lambda: fresh2.occluded(rays), render] * 2)
    for k, got in enumerate(answers):
        if k % 4 in (0, 3):
            assert np.array_equal(got.view(np.uint32), alone.view(np.uint32)), ("thread", k, "render")
        elif k % 4 == 1:
            assert got.tobytes() == want_hits.tobytes(), ("thread", k, "intersect")
        else:
            assert np.array_equal(got, want_occ), ("thread", k, "occluded")
