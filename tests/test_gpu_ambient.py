"""Ambient queries (tinyrt.h trt_ambient, trt_ambient_device) on the GPU against the CPU oracle, bit for bit and item by item.

Sample s of item i has stream index j = first_stream + i * K + s.  Its first ray is trt_gather's, drawn from RNG stream (seed, j, 1) and
restated with the oracle's own scatter functions (tests/gather_cases.py first_rays); its answer is the oracle's World.hit over
[0.001, max_distance) (ow.hit_index_batch), and the fold is the contract's in numpy float32 (tests/ambient_cases.py): an unoccluded
sample adds inv_K and d * inv_K, an occluded one nothing.

Items, per scene: the 324 surfels of gather_cases.items_of - a full run of 256 for one wave, a ragged one of 68 for the next, with the
NaN, zero, inf and 1e-9 items.  K = 8, seed 5, first_stream = 1000, both lobes, the cone with spread 0.5, and two distances: +inf and
D = the median finite hit distance of the scene's and lobe's drawn rays, which removes about half the hits.  The scenes are
test_gpu_queries.DEFAULT_SHAPES plus test_gpu_queries.OTHER_WALKS; each case asserts the kernel shape Scene.ambient_plan reports, so all
six instantiations of ambient.hip kAmbientKernels run.  tests/test_ambient_cases.py asserts without a GPU that this reference is not
vacuous: an ignored distance, draw or lobe cannot pass."""
import numpy as np
import pytest

import ambient_cases as A
import gather_cases as GC
import test_gpu_queries as G
import walk_ray_cases as W

pytestmark = pytest.mark.gpu

K, SEED, FIRST, SPREAD = A.K, A.SEED, A.FIRST_STREAM, A.SPREAD
N = A.N_ITEMS
GUARD = 64                                                                  # entries on either side of a device buffer
FILL = 0xCD
CASES = [(name, {}, shape) for name, shape in G.DEFAULT_SHAPES.items()] + list(G.OTHER_WALKS)
IDS = ["%s-%s" % (name, "-".join("%s=%s" % kv for kv in sorted(options.items())) or "default") for name, options, _ in CASES]
LOBES, DISTANCES = A.LOBES, A.DISTANCES


@pytest.fixture(scope="module")
def reference(trt, orc):
    """name -> description, worlds, items, and per lobe the oracle's ambient query (ambient_cases.reference); computed once per scene,
    shared by every test and never changed."""
    cache = {}

    def get(name):
        if name not in cache:
            desc = W.scene(trt, name)
            ow, _ = orc.world_from_description(desc)
            items, _ = GC.items_of(orc, ow, desc)
            items.setflags(write=False)
            ref = dict(desc=desc, ow=ow, world=trt.world_from_description(desc)[0], items=items)
            for lobe in LOBES:
                ref[lobe] = A.freeze(A.reference(orc, ow, items, lobe))
            cache[name] = ref
        return cache[name]

    return get


@pytest.fixture(scope="module")
def case(reference):
    """(name, options) -> the reference of the scene plus the product scene compiled with the options, its shape asserted."""
    cache = {}

    def get(name, options, shape):
        key = (name, tuple(sorted(options.items())))
        if key not in cache:
            ref = reference(name)
            sc = ref["world"].get_bvh(**options)
            q = sc.ambient_plan(N)
            assert G.plan_shape(q) == shape, (name, options, q)
            kw = dict(samples_per_item=K, seed=SEED, first_stream=FIRST)
            cache[key] = dict(ref, scene=sc, kw={"cosine": dict(kw, lobe="cosine"), "cone": dict(kw, lobe="cone", spread=SPREAD)})
        return cache[key]

    return get


def params(c, lobe, dist, **over):
    return dict(c["kw"][lobe], max_distance=c[lobe][dist]["max_distance"], **over)


def sentinels(n=N):
    return np.full(n, 7.5, np.float32), np.full((n, 3), 7.5, np.float32)


@pytest.mark.parametrize("dist", DISTANCES)
@pytest.mark.parametrize("lobe", LOBES)
@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_host_form_is_the_oracles_fold(trt, case, name, options, shape, lobe, dist):
    c = case(name, options, shape)
    want = c[lobe][dist]
    V, B = sentinels()
    V, B, st = c["scene"].ambient(c["items"], visibility=V, bent=B, **params(c, lobe, dist))
    A.assert_same_bits(V, want["V"], (name, options, lobe, dist, "visibility"))
    A.assert_same_bits(B, want["B"], (name, options, lobe, dist, "bent"))
    assert st["samples"] == N * K and st["rays"] == N * K, (name, options, lobe, dist, st)
    # bent = NULL: visibility is unchanged
    V1, none, st1 = c["scene"].ambient(c["items"], **params(c, lobe, dist))
    assert none is None and V1.tobytes() == V.tobytes()
    assert st1["samples"] == N * K and st1["rays"] == N * K


def device_buffer(torch, n, width):
    return torch.full(((GUARD + n + GUARD) * 4 * width,), FILL, dtype=torch.uint8, device="cuda:0")


def payload(t, n, width):
    """(payload as float32 [n] or [n, 3], guards intact?)"""
    h = t.cpu().numpy()
    g, b = GUARD * 4 * width, n * 4 * width
    got = h[g:g + b].copy().view(np.float32)
    return (got if width == 1 else got.reshape(n, 3)), bool((h[:g] == FILL).all() and (h[g + b:] == FILL).all())


@pytest.mark.parametrize("dist", DISTANCES)
@pytest.mark.parametrize("lobe", LOBES)
@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_device_form_on_a_side_stream_equals_the_oracle_and_leaves_the_guards(trt, case, name, options, shape, lobe, dist):
    import torch
    c = case(name, options, shape)
    want = c[lobe][dist]
    d_items = torch.from_numpy(c["items"].copy()).to("cuda:0")
    side = torch.cuda.Stream()
    d_v, d_b = device_buffer(torch, N, 1), device_buffer(torch, N, 3)
    ctr = torch.full((16,), 3, dtype=torch.int64, device="cuda:0")          # the counters are added to
    torch.cuda.synchronize()
    c["scene"].ambient_device(d_items.data_ptr(), N, d_v.data_ptr() + GUARD * 4, d_b.data_ptr() + GUARD * 12, d_counters_ptr=ctr.data_ptr(),
                              stream_ptr=side.cuda_stream, **params(c, lobe, dist))
    side.synchronize()
    torch.cuda.synchronize()
    got_v, ok_v = payload(d_v, N, 1)
    got_b, ok_b = payload(d_b, N, 3)
    assert ok_v and ok_b, (name, options, lobe, dist, "guard bytes were written")
    A.assert_same_bits(got_v, want["V"], (name, options, lobe, dist, "visibility"))
    A.assert_same_bits(got_b, want["B"], (name, options, lobe, dist, "bent"))
    assert int(ctr[0]) == 3 + N * K and int(ctr[1]) == 3 + N * K and bool((ctr[2:] == 3).all())
    # without bent and without counters: the same visibility, the guards intact
    d_v1 = device_buffer(torch, N, 1)
    c["scene"].ambient_device(d_items.data_ptr(), N, d_v1.data_ptr() + GUARD * 4, **params(c, lobe, dist))
    torch.cuda.synchronize()
    got_v1, ok_v1 = payload(d_v1, N, 1)
    assert ok_v1 and got_v1.tobytes() == got_v.tobytes()


@pytest.mark.parametrize("lobe", LOBES)
@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_split_by_samples_leaves_the_bytes_of_one_pass(trt, case, name, options, shape, lobe):
    c = case(name, options, shape)
    for dist in DISTANCES:
        want = c[lobe][dist]
        V, B = sentinels()
        c["scene"].ambient(c["items"], sample_begin=0, sample_end=3, visibility=V, bent=B, **params(c, lobe, dist))
        V3, B3 = A.fold(want["occ"], c[lobe]["rays"], K, 0, 3)
        A.assert_same_bits(V, V3, (name, options, lobe, dist, "visibility [0, 3)"))
        A.assert_same_bits(B, B3, (name, options, lobe, dist, "bent [0, 3)"))
        _, _, st = c["scene"].ambient(c["items"], sample_begin=3, sample_end=8, accumulate=True, visibility=V, bent=B, **params(c, lobe, dist))
        A.assert_same_bits(V, want["V"], (name, options, lobe, dist, "visibility [0, 3) + [3, 8)"))
        A.assert_same_bits(B, want["B"], (name, options, lobe, dist, "bent [0, 3) + [3, 8)"))
        assert st["samples"] == N * 5 and st["rays"] == N * 5


@pytest.mark.parametrize("lobe", LOBES)
@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_split_by_items_leaves_the_bytes_of_one_call(trt, case, name, options, shape, lobe):
    c = case(name, options, shape)
    for dist in DISTANCES:
        kw = params(c, lobe, dist)
        one_v, one_b, _ = c["scene"].ambient(c["items"], bent=True, **kw)
        V, B = sentinels()
        a = 100
        c["scene"].ambient(c["items"][:a], visibility=V[:a], bent=B[:a], **kw)
        assert (V[a:] == 7.5).all() and (B[a:] == 7.5).all()                # entries outside the call's range are untouched
        kw["first_stream"] = FIRST + a * K
        assert kw["first_stream"] == 1800
        head_v, head_b = V[:a].copy(), B[:a].copy()
        c["scene"].ambient(c["items"][a:], visibility=V[a:], bent=B[a:], **kw)
        assert V[:a].tobytes() == head_v.tobytes() and B[:a].tobytes() == head_b.tobytes()
        assert V.tobytes() == one_v.tobytes() and B.tobytes() == one_b.tobytes(), (name, options, lobe, dist)       # byte for byte
        A.assert_same_bits(V, c[lobe][dist]["V"], (name, options, lobe, dist, "visibility"))
        A.assert_same_bits(B, c[lobe][dist]["B"], (name, options, lobe, dist, "bent"))


@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_nothing_to_trace(trt, case, name, options, shape):
    """An empty sample range zeroes the n entries without accumulate and leaves them with it; through the device form no byte outside
    [0, 4 n) or [0, 12 n) is written.  A max_distance of 0.001 and of -1 is an empty range of t: every sample is drawn and folds as
    unoccluded, nothing is walked, rays == 0."""
    import torch
    c = case(name, options, shape)
    for lobe in LOBES:
        kw = dict(c["kw"][lobe], sample_begin=3, sample_end=3)
        for accumulate in (False, True):
            V, B = sentinels()
            _, _, st = c["scene"].ambient(c["items"], accumulate=accumulate, visibility=V, bent=B, **kw)
            want = 7.5 if accumulate else 0.0
            assert (V == want).all() and (B == want).all(), (name, options, lobe, accumulate)
            assert st["rays"] == 0 and st["samples"] == 0
            V, _ = sentinels()
            c["scene"].ambient(c["items"], accumulate=accumulate, visibility=V, **kw)
            assert (V == want).all()
        open_v, open_b = A.fold(np.zeros((N, K), bool), c[lobe]["rays"], K)
        assert (open_v == open_v[0]).all() and open_v[0] == np.float32(1.0)                        # K x inv_K with K = 8: exactly 1
        for dist in (0.001, -1.0):
            V, B = sentinels()
            _, _, st = c["scene"].ambient(c["items"], max_distance=dist, visibility=V, bent=B, **c["kw"][lobe])
            A.assert_same_bits(V, open_v, (name, options, lobe, dist, "visibility"))
            A.assert_same_bits(B, open_b, (name, options, lobe, dist, "bent"))
            assert st["samples"] == N * K and st["rays"] == 0, (name, options, lobe, dist, st)
    d_items = torch.from_numpy(c["items"].copy()).to("cuda:0")
    for accumulate in (False, True):
        for with_bent in (True, False):
            d_v, d_b = device_buffer(torch, N, 1), device_buffer(torch, N, 3)
            c["scene"].ambient_device(d_items.data_ptr(), N, d_v.data_ptr() + GUARD * 4, d_b.data_ptr() + GUARD * 12 if with_bent else 0,
                                      accumulate=accumulate, sample_begin=2, sample_end=2, **c["kw"]["cone"])
            torch.cuda.synchronize()
            for t, width, written in ((d_v, 1, True), (d_b, 3, with_bent)):
                got, ok = payload(t, N, width)
                assert ok, (name, options, "guard bytes were written")
                assert (got.view(np.uint32) == (0 if written and not accumulate else 0xCDCDCDCD)).all()


@pytest.mark.parametrize("lobe", LOBES)
@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_the_drawn_rays_through_occluded_are_the_oracles_samples(trt, case, name, options, shape, lobe):
    """Three-way agreement without the fold: the n * K oracle-drawn first rays through Scene.occluded with t_max = D equal the oracle's
    per-sample answers, which folded equal Scene.ambient (above)."""
    c = case(name, options, shape)
    rays = c[lobe]["rays"].reshape(-1, 6)
    for dist in DISTANCES:
        want = c[lobe][dist]
        t_max = None if dist == "inf" else np.full(len(rays), want["max_distance"], np.float32)
        got = c["scene"].occluded(rays, t_max).reshape(N, K)
        assert (got == want["occ"]).all(), (name, options, lobe, dist, int((got != want["occ"]).sum()))


@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_a_cone_of_no_spread_is_one_occlusion_query(trt, orc, case, name, options, shape):
    """The cone lobe with spread 0 and K = 1 draws Ray::new(point, axis + 0 * v): visibility[i] == 1 - occluded(Ray::new(point, axis)),
    against an entry point that already passes its tests.  (axis + 0 * v is the axis but for a -0 component, which becomes +0: the
    bent sum is compared with the direction as drawn.)"""
    c = case(name, options, shape)
    items = c["items"]
    rays = np.zeros((N, 6), np.float32)
    for i in range(N):
        point, axis = orc.Vec3(*items[i, 0:3].tolist()), orc.Vec3(*items[i, 3:6].tolist())
        rays[i] = np.frombuffer(bytes(orc.lib.orc_ray_new(point, axis)), np.float32)
    drawn = GC.first_rays(orc, items, "cone", 1, 0.0, SEED, FIRST)[:, 0, :]
    with np.errstate(all="ignore"):
        assert (np.isnan(drawn) == np.isnan(rays)).all() and (drawn[~np.isnan(rays)] == rays[~np.isnan(rays)]).all()         # (-0 == +0)
    for dist in (float("inf"), c["cone"]["D"]["max_distance"]):
        occ = c["scene"].occluded(rays, None if dist == float("inf") else np.full(N, dist, np.float32))
        V, B, st = c["scene"].ambient(items, 1, lobe="cone", spread=0.0, max_distance=dist, seed=SEED, first_stream=FIRST, bent=True)
        want = np.where(occ, np.float32(0.0), np.float32(1.0)).astype(np.float32)
        A.assert_same_bits(V, want, (name, options, dist, "visibility"))
        assert 1 <= int(occ.sum()) <= N - 1, (name, options, dist, int(occ.sum()))                 # both answers occur
        want_v, want_b = A.fold(occ[:, None], drawn[:, None, :], 1)
        assert want_v.tobytes() == want.tobytes()
        A.assert_same_bits(B, want_b, (name, options, dist, "bent"))
        assert st["samples"] == N and st["rays"] == N
