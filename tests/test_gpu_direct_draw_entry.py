"""The edges of the emitter draw (tests/direct_draw_cases.py) through the public entry points that make it - trt_direct for an item's own
surfel, trt_nee at a path's Lambertian vertices - against the oracle, bit for bit.

Batches of 65 items with K = 4: items 0..63 are ordinary surfels of the scene (one full round of a wave), item 64 - the ragged lane -
meets an edge with its sample 1: first_stream = j - 64 K - 1 puts that sample on the edge stream j.  Cornell (lock-step list in LDS) and
grid3000 (16-byte nodes from global memory) run the two kernel forms of each unit; every plan's shape is asserted.  The host form runs,
and the device form on a side stream with guards around every buffer; radiance, moment2, `samples` and `rays` are compared with
direct_cases.reference / nee_cases.nee_paths.

trt_direct (direct_draw_cases.direct_entry_batches): cs exactly 0; x on the light; the last area with a finite weight (FLT_MAX) and the
next float (inf); cl = 0; a sphere's fourth draw 0; t_max the float below 0.001, 0.001 itself and the float above - one sample of the
batch, so `rays` grows by exactly one from the second to the third while the term is added in all three; and a table of E = 1 000 003,
built on the device by repeating a period of 61 records, with first_stream such that item 64's sample 1 picks another record than
floor(exact u0 E) would (device form only: the host form would copy 80 MB).

trt_nee (direct_draw_cases.nee_entry_setup): the table is the caller's, so it is built around the first Lambertian vertex x of item 64's
sample 1 (source COSINE, B = 3, source_is_diffuse 0 and 1): a degenerate quad whose corner is x (the light on the vertex: dead, no
walk), a corner searched float by float so that t_max straddles 0.001 (the walk count grows by one, the unoccluded term is added on
both sides; 0.001 itself where a float of the corner gives it), and a sphere of radius 0 at x.
"""
import numpy as np
import pytest

import direct_draw_cases as D
import draw_cases as DR
import gather_cases as GC
import passes_cases as PS
import radiance_cases as R
import test_gpu_queries as G
import walk_ray_cases as W

pytestmark = pytest.mark.gpu
N, K = D.ENTRY_N, D.ENTRY_K
EDGE = (N - 1, D.ENTRY_SAMPLE)
GUARD = 64                                                                  # floats of 7.5 on either side of a device buffer
DIRECT_BATCHES = ("cs_zero", "on_the_light", "wgt_max", "wgt_inf", "cl_zero", "u4_zero", "pick_rounded") + D.TMAX_SIDES
NEE_TABLES = ("light_on_vertex", "sphere_on_vertex", "tmax_below", "tmax_at", "tmax_above")


def same_bits(got, want, what):
    R.assert_same_bits(np.asarray(got).reshape(len(want), -1), np.asarray(want).reshape(len(want), -1), what)


@pytest.fixture(scope="module")
def scene(trt, orc):
    """name -> dict(desc, oracle world, product scene, background, the 65 items); the plans of both units asserted."""
    cache = {}

    def get(name):
        if name not in cache:
            desc = W.scene(trt, name)
            ow, _ = orc.world_from_description(desc)
            sc = trt.world_from_description(desc)[0].get_bvh()
            for q in (sc.direct_plan(N), sc.nee_plan(N)):
                assert G.plan_shape(q) == G.DEFAULT_SHAPES[name], (name, q)
            items = DR.entry_items(orc, ow, desc)
            items.setflags(write=False)
            cache[name] = dict(desc=desc, ow=ow, scene=sc, bg=PS.background_of(desc), items=items)
        return cache[name]

    return get


@pytest.fixture(scope="module")
def batches(orc):
    return D.direct_entry_batches(orc)


class Device:
    """Items and a table in HBM, guarded sums, counters and one side stream for a device-form call."""

    def __init__(self, items, table):
        import torch
        self.torch = torch
        self.items = torch.from_numpy(np.array(items, np.float32)).to("cuda:0")
        period = torch.from_numpy(np.ascontiguousarray(table["records"]).view(np.uint8).reshape(len(table["records"]), 80).copy()).to("cuda:0")
        self.E = table["E"]
        # the table is built on the device by repeating its period
        self.table = period[torch.arange(self.E, device="cuda:0") % len(period)].contiguous()
        assert self.table.shape == (self.E, 80)
        self.side = torch.cuda.Stream()
        self.sums = [torch.full((GUARD + N * 3 + GUARD,), 7.5, dtype=torch.float32, device="cuda:0") for _ in range(2)]
        self.ctr = torch.full((16,), 3, dtype=torch.int64, device="cuda:0")                 # the counters are added to
        torch.cuda.synchronize()

    def args(self):
        return (self.items.data_ptr(), N, self.table.data_ptr(), self.E, self.sums[0].data_ptr() + GUARD * 4, self.sums[1].data_ptr() + GUARD * 4)

    def kw(self):
        return dict(d_counters_ptr=self.ctr.data_ptr(), stream_ptr=self.side.cuda_stream)

    def results(self, what):
        self.side.synchronize()
        self.torch.cuda.synchronize()
        out = []
        for t in self.sums:
            h = t.cpu().numpy()
            assert (h[:GUARD] == 7.5).all() and (h[GUARD + N * 3:] == 7.5).all(), (what, "guard floats were written")
            out.append(h[GUARD:GUARD + N * 3].reshape(N, 3).copy())
        ctr = self.ctr.cpu().numpy()
        assert (ctr[2:] == 3).all()
        return out[0], out[1], int(ctr[0]) - 3, int(ctr[1]) - 3


def run_direct(orc, c, b, what):
    """(reference, items): both forms of trt_direct on the batch == the reference; the edge sample is the draw-level expectation."""
    items = D.direct_entry_items(c["items"], b)
    ref = D.direct_entry_reference(orc, c["ow"], items, b)
    tr = {}
    exp = D.expect(orc, b["table"], b["j"], 1, b["shadow_end"], items[N - 1, 0:3], items[N - 1, 3:6], tr)
    ray_bits, nan = D.bits(ref["rays"][EDGE]), np.isnan(ref["rays"][EDGE])
    assert ((ray_bits == exp[0:6]) | nan).all() and bool(ref["live"][EDGE]) == tr["live"] and ref["e"][EDGE] == tr["pick"], what
    assert np.isfinite(ref["rays"][:N - 1]).all(), what
    kw = dict(samples_per_item=K, seed=D.SEED, first_stream=b["first_stream"], shadow_end=float(b["shadow_end"]))
    if not b["device_only"]:
        S, M, st = c["scene"].direct(items, D.expand(b["table"]), moment2=True, **kw)
        same_bits(S, ref["S"], what + ("host radiance",))
        same_bits(M, ref["M"], what + ("host moment2",))
        assert st["samples"] == N * K and st["rays"] == ref["n_walks"], (what, st, ref["n_walks"])
    dev = Device(items, b["table"])
    c["scene"].direct_device(*dev.args(), **dev.kw(), **kw)
    S, M, samples, rays = dev.results(what)
    same_bits(S, ref["S"], what + ("device radiance",))
    same_bits(M, ref["M"], what + ("device moment2",))
    assert samples == N * K and rays == ref["n_walks"], (what, samples, rays, ref["n_walks"])
    return ref, items


@pytest.mark.parametrize("batch", DIRECT_BATCHES)
@pytest.mark.parametrize("name", D.ENTRY_SCENES)
def test_direct_an_edge_lane_in_a_mixed_wave(trt, orc, scene, batches, name, batch):
    c, b = scene(name), batches[batch]
    what = (name, batch)
    ref, items = run_direct(orc, c, b, what)
    live, walked = bool(ref["live"][EDGE]), bool(ref["walked"][EDGE])
    assert (live, walked) == dict(cs_zero=(False, False), on_the_light=(False, False), wgt_max=(True, False), wgt_inf=(False, False), cl_zero=(True, True),
                                  u4_zero=(False, False), pick_rounded=(True, True), tmax_below=(True, False), tmax_at=(True, False),
                                  tmax_above=(True, True))[batch], what
    if batch == "pick_rounded":
        u0 = D.stream_draws(orc, b["j"], 1, 1)[0]
        assert b["table"]["E"] == 1000003 and int(ref["e"][EDGE]) != (int(round(float(u0) * (1 << 23))) * 1000003) >> 23
    if batch == "wgt_max":
        assert ref["wgt"][EDGE] == np.finfo(np.float32).max
    # control: one stream further nothing meets the edge; the host form follows the oracle there, and the answers are others
    if not b["device_only"]:
        moved = dict(b, first_stream=b["first_stream"] + 1)
        ref_moved = D.direct_entry_reference(orc, c["ow"], items, moved)
        S, _, _ = c["scene"].direct(items, D.expand(b["table"]), samples_per_item=K, seed=D.SEED, first_stream=moved["first_stream"],
                                    shadow_end=float(b["shadow_end"]))
        same_bits(S, ref_moved["S"], what + ("one stream further",))
        # (the one record of the wgt tables is a point: no draw reaches its samples, the rows are the same on any stream)
        assert (S.view(np.uint32) != ref["S"].view(np.uint32)).any(axis=1).sum() >= (0 if batch.startswith("wgt") else 8), what


@pytest.mark.parametrize("name", D.ENTRY_SCENES)
def test_direct_t_max_about_the_lower_end_of_the_walk(trt, orc, scene, batches, name):
    """t_max = the float below 0.001, 0.001, the float above: `t_max > 0.001` walks only the third, `rays` grows by exactly one there, and
    the unoccluded term is added in all three (the three surfels are one float of distance apart: their own terms differ in the last
    bits, every other item's row is the same)."""
    c = scene(name)
    got = {}
    for side in D.TMAX_SIDES:
        b = batches[side]
        items = D.direct_entry_items(c["items"], b)
        ref = D.direct_entry_reference(orc, c["ow"], items, b)
        S, M, st = c["scene"].direct(items, D.expand(b["table"]), samples_per_item=K, seed=D.SEED, first_stream=b["first_stream"],
                                     shadow_end=float(b["shadow_end"]), moment2=True)
        same_bits(S, ref["S"], (name, side))
        assert ref["live"][EDGE] and not ref["occ"][EDGE] and (ref["c"][EDGE] != 0).all()
        got[side] = (S, st["rays"], ref)
    t = [D.bits(got[s][2]["t_max"][EDGE])[0] for s in D.TMAX_SIDES]
    assert t[0] + 1 == t[1] == D.bits(D.T_MIN)[0] == t[2] - 1
    assert got["tmax_below"][1] == got["tmax_at"][1] == got["tmax_above"][1] - 1, (name, [got[s][1] for s in D.TMAX_SIDES])
    for s in D.TMAX_SIDES[1:]:
        assert got[s][0][:N - 1].tobytes() == got["tmax_below"][0][:N - 1].tobytes()
    assert (got["tmax_below"][0][N - 1] != 0).all() and (got["tmax_above"][0][N - 1] != 0).all()


@pytest.mark.parametrize("diffuse", (False, True))
@pytest.mark.parametrize("name", D.ENTRY_SCENES)
def test_nee_a_table_built_around_a_vertex(trt, orc, scene, name, diffuse):
    c = scene(name)
    st = D.nee_entry_setup(orc, c["ow"], c["desc"], c["items"])
    kw = dict(samples_per_item=K, source="cosine", spread=GC.SPREAD, shadow_end=float(st["shadow_end"]), source_is_diffuse=diffuse, max_bounces=D.NEE_BOUNCES,
              background=c["bg"], seed=D.SEED, first_stream=st["first_stream"])
    refs = {}
    for tn in NEE_TABLES:
        if tn not in st["tables"]:
            assert tn == "tmax_at"                                          # no float of the corner gives 0.001 itself on this vertex
            continue
        what = (name, diffuse, tn)
        table = st["tables"][tn]
        ref = D.nee_entry_reference(orc, c["ow"], c["desc"], c["items"], st, table, c["bg"], diffuse)
        S, M, stats = c["scene"].nee(c["items"], table, moment2=True, **kw)
        same_bits(S, ref["S"], what + ("host radiance",))
        same_bits(M, ref["M"], what + ("host moment2",))
        assert stats["samples"] == N * K and stats["rays"] == ref["n_rays"], (what, stats, ref["n_rays"])
        dev = Device(c["items"], dict(E=1, records=table))
        c["scene"].nee_device(*dev.args(), **dev.kw(), **kw)
        S, M, samples, rays = dev.results(what)
        same_bits(S, ref["S"], what + ("device radiance",))
        same_bits(M, ref["M"], what + ("device moment2",))
        assert samples == N * K and rays == ref["n_rays"], (what, samples, rays, ref["n_rays"])
        refs[tn] = ref
    # the light on the vertex and the sphere of radius 0 there: that vertex's sample is dead and walks nothing; below (and at) 0.001 it
    # is live, unoccluded and walks nothing; above it walks - one ray more in the whole batch - and the term is added on both sides
    below, above = refs["tmax_below"], refs["tmax_above"]
    assert above["n_rays"] == below["n_rays"] + 1 and above["walks"][EDGE] == below["walks"][EDGE] + 1 and above["lit"][EDGE] == below["lit"][EDGE]
    assert np.array_equal(np.delete(above["walks"].ravel(), EDGE[0] * K + EDGE[1]), np.delete(below["walks"].ravel(), EDGE[0] * K + EDGE[1]))
    for tn in ("light_on_vertex", "sphere_on_vertex"):
        assert refs[tn]["lit"][EDGE] == below["lit"][EDGE] - 1 and refs[tn]["walks"][EDGE] <= below["walks"][EDGE]
    if "tmax_at" in refs:
        assert refs["tmax_at"]["n_rays"] == below["n_rays"] and refs["tmax_at"]["lit"][EDGE] == below["lit"][EDGE]
