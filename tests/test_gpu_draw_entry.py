"""The edges of the device-drawn first ray (tests/draw_cases.py) through the public entry points that draw it - trt_gather, trt_ambient,
trt_probe, trt_passes - and the top of the RNG stream range through those and trt_radiance, against the oracle, bit for bit.

Batches of 65 items with K = 4: items 0..63 are ordinary surfels of the scene (one full round of a wave), item 64 - the ragged lane -
meets an edge with its sample 1: first_stream = j - 64 K - 1 puts that sample on the edge stream j (draw_cases.entry_batches: the three
zero draws of golden/draw_edge_streams.json, near_zero taken, a cone sum of exactly zero and of one float, a hemisphere dot of exactly
zero and of a subnormal).  So the edge lane sits in a wave whose other lanes do ordinary work.  Cornell (lock-step list in LDS) and
grid3000 (16-byte nodes from global memory) run the two kernel forms of each unit; every plan's shape is asserted.  The calls are the
device forms on a side stream with guards around every buffer; samples and rays are compared with the oracle's counts - a NaN first
ray is traced and counted.  A u3 = 0 draw is a NaN ray from a finite item: in a probe it adds nothing (with K = 1 the item's row is
exactly 0), in passes it is a miss at depth 0 (slot B holds the background / K).

Reference: first rays from gather_cases.first_rays / probe_cases.first_rays, paths from passes_cases.oracle_paths (the oracle's pieces
on stream (seed, j, 0) for ANY j - orc.sample_batch numbers its streams from 0, which these j and 2^32 - 1 put out of reach;
tests/test_passes_cases.py pins oracle_paths to it), folds from radiance_cases, ambient_cases, probe_cases and passes_cases.

Top of the range: n = 65, K = 8, first_stream = 2^32 - 520, so the last sample runs on stream 2^32 - 1; the five host forms == the
oracle on every item, and first_stream one higher is refused.

Ambient max_distance at a hit: cone of spread 0, K = 1 (the ray is Ray::new(point, axis)), max_distance = the float below the chosen
item's hit distance t*, t* itself and the float above - [0.001, max_distance) excludes t* itself - on one scene per walk kind.
"""
import numpy as np
import pytest

import draw_cases as D
import gather_cases as GC
import passes_cases as PS
import probe_cases as PC
import radiance_cases as R
import test_gpu_queries as G
import walk_ray_cases as W

pytestmark = pytest.mark.gpu
N, K, BINS, DEPTH = D.ENTRY_N, D.ENTRY_K, D.ENTRY_BINS, PS.MAX_BOUNCES
GUARD = 64                                                                  # floats of 7.5 on either side of a device buffer
BATCHES = ("u1_zero", "u2_zero", "u3_zero", "cos_near_zero_taken", "cone_zero_sum", "cone_tiny_sum", "hemi_dot_zero", "hemi_dot_subnormal")


def same_bits(got, want, what):
    R.assert_same_bits(np.asarray(got).reshape(len(want), -1), np.asarray(want).reshape(len(want), -1), what)


@pytest.fixture(scope="module")
def scene(trt, orc):
    """name -> dict(desc, oracle world, product scene, background, the 65 items); the plan of every unit asserted."""
    cache = {}

    def get(name):
        if name not in cache:
            desc = W.scene(trt, name)
            ow, _ = orc.world_from_description(desc)
            sc = trt.world_from_description(desc)[0].get_bvh()
            shape = G.DEFAULT_SHAPES[name]
            for q in (sc.radiance_plan(N), sc.gather_plan(N), sc.ambient_plan(N), sc.probe_plan(N, PC.BANDS), sc.passes_plan(N, BINS)):
                assert G.plan_shape(q) == shape, (name, q)
            items = D.entry_items(orc, ow, desc)
            items.setflags(write=False)
            cache[name] = dict(desc=desc, ow=ow, scene=sc, bg=PS.background_of(desc), items=items)
        return cache[name]

    return get


class Device:
    """Guarded device buffers and one side stream for a run of device-form calls."""

    def __init__(self, items):
        import torch
        self.torch = torch
        self.items = torch.from_numpy(np.ascontiguousarray(items)).to("cuda:0")
        self.side = torch.cuda.Stream()
        self.bufs = []

    def buffer(self, floats):
        t = self.torch.full((GUARD + floats + GUARD,), 7.5, dtype=self.torch.float32, device="cuda:0")
        self.bufs.append((t, floats))
        return t.data_ptr() + GUARD * 4

    def counters(self):
        self.ctr = self.torch.full((16,), 3, dtype=self.torch.int64, device="cuda:0")      # the counters are added to
        return self.ctr.data_ptr()

    def ready(self):
        self.torch.cuda.synchronize()

    def results(self, what):
        self.side.synchronize()
        self.torch.cuda.synchronize()
        out = []
        for t, floats in self.bufs:
            h = t.cpu().numpy()
            assert (h[:GUARD] == 7.5).all() and (h[GUARD + floats:] == 7.5).all(), (what, "guard floats were written")
            out.append(h[GUARD:GUARD + floats].copy())
        ctr = self.ctr.cpu().numpy()
        assert (ctr[2:] == 3).all()
        return out, int(ctr[0]) - 3, int(ctr[1]) - 3


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("name", D.ENTRY_SCENES)
def test_an_edge_lane_in_a_mixed_wave(trt, orc, scene, name, batch):
    c = scene(name)
    b = D.entry_batches(orc)[batch]
    items = D.entry_batch_items(c["items"], b)
    fs = b["first_stream"]
    path = dict(max_bounces=DEPTH, background=c["bg"], seed=D.SEED, first_stream=fs)
    for kind in b["kinds"]:
        what = (name, batch, kind)
        ref = D.entry_reference(orc, c["ow"], c["desc"], trt.sh.basis, items, kind, K, DEPTH, c["bg"], fs)
        # the edge is there: sample 1 of item 64 is the draw-level case of that class, the rest of the batch is ordinary
        edge = ref["rays"][N - 1, D.ENTRY_SAMPLE]
        case = dict(kind=kind, spread=np.float32(GC.SPREAD), item=items[N - 1], j=b["j"])
        assert np.array_equal(D.bits(edge), D.bits(D.oracle_ray(orc, case))), what
        assert np.isfinite(ref["rays"][:N - 1]).all(), what
        dev = Device(items)
        if kind in GC.LOBES:
            p_s, p_m = dev.buffer(N * 3), dev.buffer(N * 3)
            p_v, p_b = dev.buffer(N), dev.buffer(N * 3)
            p_p, p_sp = dev.buffer(N * 6 * BINS), dev.buffer(N)
            ctr = dev.counters()
            dev.ready()
            s = dev.side.cuda_stream
            c["scene"].gather_device(dev.items.data_ptr(), N, p_s, p_m, d_counters_ptr=ctr, stream_ptr=s, samples_per_item=K, lobe=kind, spread=GC.SPREAD, **path)
            c["scene"].ambient_device(dev.items.data_ptr(), N, p_v, p_b, d_counters_ptr=ctr, stream_ptr=s, samples_per_item=K, lobe=kind, spread=GC.SPREAD,
                                      seed=D.SEED, first_stream=fs)
            c["scene"].passes_device(dev.items.data_ptr(), N, p_p, p_sp, d_counters_ptr=ctr, stream_ptr=s, samples_per_item=K, depth_bins=BINS, source=kind,
                                     spread=GC.SPREAD, **path)
            (S, M, V, B, P, SP), samples, rays = dev.results(what)
            same_bits(S.reshape(N, 3), ref["S"], what + ("gather radiance",))
            same_bits(M.reshape(N, 3), ref["M"], what + ("gather moment2",))
            same_bits(V, ref["V"], what + ("ambient visibility",))
            same_bits(B.reshape(N, 3), ref["B"], what + ("ambient bent",))
            same_bits(P.reshape(N, 2 * BINS, 3), ref["P"], what + ("passes",))
            same_bits(SP, ref["spent"], what + ("spent",))
            # gather and passes trace the oracle's world.hit calls each, ambient one occlusion walk per sample - a NaN ray included
            assert samples == 3 * N * K and rays == 2 * ref["n_rays"] + N * K, (what, samples, rays, ref["n_rays"])
            # control: one stream further nothing meets the edge; the host form follows the oracle there, and the answers are others
            # (a reference that ignored first_stream would show no differing row)
            ref_moved = D.entry_reference(orc, c["ow"], c["desc"], trt.sh.basis, items, kind, K, DEPTH, c["bg"], fs + 1)
            moved, _, _ = c["scene"].gather(items, K, lobe=kind, spread=GC.SPREAD, **dict(path, first_stream=fs + 1))
            same_bits(moved, ref_moved["S"], what + ("gather, one stream further",))
            assert (moved.view(np.uint32) != ref["S"].view(np.uint32)).any(axis=1).sum() >= 1, what
            if np.isnan(edge).any():
                # the NaN draw is a miss at depth 0: unoccluded, and in passes the background / K in slot B of item 64
                assert ref["ends"][N - 1, D.ENTRY_SAMPLE] == PS.SKY and ref["depths"][N - 1, D.ENTRY_SAMPLE] == 0 and not ref["occ"][N - 1, D.ENTRY_SAMPLE]
                only = PS.fold(ref["cols"][N - 1:, D.ENTRY_SAMPLE:D.ENTRY_SAMPLE + 1], ref["ends"][N - 1:, D.ENTRY_SAMPLE:D.ENTRY_SAMPLE + 1],
                               ref["depths"][N - 1:, D.ENTRY_SAMPLE:D.ENTRY_SAMPLE + 1], K, BINS)[0][0]
                assert np.array_equal(only[BINS], np.array(c["bg"], np.float32) * (np.float32(1.0) / np.float32(K))) and (np.delete(only, BINS, axis=0) == 0).all()
                assert np.isnan(B.reshape(N, 3)[N - 1]).all() and np.isfinite(B.reshape(N, 3)[:N - 1]).all()
        else:
            coeffs = PC.COEFFS
            p_sh, p_one = dev.buffer(N * coeffs * 3), dev.buffer(N * coeffs * 3)
            ctr = dev.counters()
            dev.ready()
            s = dev.side.cuda_stream
            c["scene"].probe_device(dev.items.data_ptr(), N, p_sh, d_counters_ptr=ctr, stream_ptr=s, samples_per_item=K, bands=PC.BANDS, domain=kind, **path)
            # K = 1 with item 64 on the edge stream itself
            one = dict(path, first_stream=b["j"] - (N - 1))
            c["scene"].probe_device(dev.items.data_ptr(), N, p_one, d_counters_ptr=ctr, stream_ptr=s, samples_per_item=1, bands=PC.BANDS, domain=kind, **one)
            ref1 = D.entry_reference(orc, c["ow"], c["desc"], trt.sh.basis, items, kind, 1, DEPTH, c["bg"], one["first_stream"])
            assert np.array_equal(D.bits(ref1["rays"][N - 1, 0]), D.bits(edge)), what
            (SH, SH1), samples, rays = dev.results(what)
            same_bits(SH.reshape(N, coeffs, 3), ref["SH"], what + ("sh",))
            same_bits(SH1.reshape(N, coeffs, 3), ref1["SH"], what + ("sh, K = 1",))
            assert samples == N * K + N and rays == ref["n_rays"] + ref1["n_rays"], (what, samples, rays)
            if np.isnan(edge).any():
                # traced, counted, adds nothing: the row of the K = 1 call is exactly +0, and no NaN anywhere
                assert (SH1.reshape(N, coeffs, 3)[N - 1].view(np.uint32) == 0).all() and (ref1["SH"][N - 1].view(np.uint32) == 0).all()
                assert np.isfinite(SH).all() and np.isfinite(SH1).all()
                assert (SH1.reshape(N, coeffs, 3)[:N - 1] != 0).any(axis=(1, 2)).sum() >= 8         # (the other rows are not: paths that end)


@pytest.mark.parametrize("name", D.ENTRY_SCENES)
def test_the_top_of_the_stream_range(trt, orc, scene, name):
    """first_stream + n K == 2^32: the last sample of the last item runs on stream 2^32 - 1, and the 32-bit sum in the kernels does not wrap."""
    c = scene(name)
    items, fs, k = c["items"], D.TOP_FIRST_STREAM, D.TOP_K
    assert fs + N * k == 1 << 32
    sc = c["scene"]
    path = dict(max_bounces=DEPTH, background=c["bg"], seed=D.SEED, first_stream=fs)
    refused = dict(path, first_stream=fs + 1)

    def refuses(call):
        with pytest.raises(trt._lib.TinyRTError) as e:
            call()
        assert e.value.code == trt._lib.ERR_INVALID_ARG and "2^32" in str(e.value)

    rays = np.ascontiguousarray(R.rays_of(c["desc"])[np.arange(N) * 4])
    ref = D.entry_reference(orc, c["ow"], c["desc"], trt.sh.basis, rays, "rays", k, DEPTH, c["bg"], fs)
    S, M, st = sc.radiance(rays, k, moment2=True, **path)
    same_bits(S, ref["S"], (name, "radiance"))
    same_bits(M, ref["M"], (name, "radiance moment2"))
    assert st["samples"] == N * k and st["rays"] == ref["n_rays"]
    refuses(lambda: sc.radiance(rays, k, **refused))
    for lobe in GC.LOBES:
        ref = D.entry_reference(orc, c["ow"], c["desc"], trt.sh.basis, items, lobe, k, DEPTH, c["bg"], fs)
        assert len({row.tobytes() for row in ref["S"]}) >= 20                                     # not vacuous
        S, M, st = sc.gather(items, k, lobe=lobe, spread=GC.SPREAD, moment2=True, **path)
        same_bits(S, ref["S"], (name, lobe, "gather"))
        same_bits(M, ref["M"], (name, lobe, "gather moment2"))
        assert st["samples"] == N * k and st["rays"] == ref["n_rays"]
        V, B, st = sc.ambient(items, k, lobe=lobe, spread=GC.SPREAD, seed=D.SEED, first_stream=fs, bent=True)
        same_bits(V, ref["V"], (name, lobe, "ambient"))
        same_bits(B, ref["B"], (name, lobe, "ambient bent"))
        assert st["samples"] == N * k and st["rays"] == N * k
        P, SP, st = sc.passes(items, k, depth_bins=BINS, source=lobe, spread=GC.SPREAD, **path)
        same_bits(P, ref["P"], (name, lobe, "passes"))
        same_bits(SP, ref["spent"], (name, lobe, "spent"))
        assert st["samples"] == N * k and st["rays"] == ref["n_rays"]
        refuses(lambda: sc.gather(items, k, lobe=lobe, spread=GC.SPREAD, **refused))
        refuses(lambda: sc.ambient(items, k, lobe=lobe, spread=GC.SPREAD, seed=D.SEED, first_stream=fs + 1))
        refuses(lambda: sc.passes(items, k, depth_bins=BINS, source=lobe, spread=GC.SPREAD, **refused))
    for domain in PC.DOMAINS:
        ref = D.entry_reference(orc, c["ow"], c["desc"], trt.sh.basis, items, domain, k, DEPTH, c["bg"], fs)
        SH, st = sc.probe(items, k, bands=PC.BANDS, domain=domain, **path)
        same_bits(SH, ref["SH"], (name, domain, "probe"))
        assert st["samples"] == N * k and st["rays"] == ref["n_rays"]
        refuses(lambda: sc.probe(items, k, bands=PC.BANDS, domain=domain, **refused))


@pytest.mark.parametrize("name", D.AT_HIT_SCENES)
def test_ambient_max_distance_at_a_hit(trt, orc, name):
    desc = W.scene(trt, name)
    ow, _ = orc.world_from_description(desc)
    sc = trt.world_from_description(desc)[0].get_bvh()
    assert G.plan_shape(sc.ambient_plan(N)) == G.DEFAULT_SHAPES[name]
    items = D.entry_items(orc, ow, desc)
    rays, chosen, t_star, calls = D.at_hit_reference(orc, ow, items)
    # on the CPU first: the range is [0.001, max_distance), so the hit at t* occludes only from the float above t*
    occ = [bool(o[chosen, 0]) for _, o, _, _ in calls]
    assert occ == [False, False, True], (name, chosen, t_star, occ)
    assert calls[1][2][chosen] == 1.0 and calls[2][2][chosen] == 0.0
    assert any(o.any() for _, o, _, _ in calls) and not all(o.all() for _, o, _, _ in calls)
    got = []
    for md, o, V, B in calls:
        v, b, st = sc.ambient(items, 1, lobe="cone", spread=0.0, max_distance=md, seed=D.SEED, first_stream=0, bent=True)
        same_bits(v, V, (name, md, "visibility"))
        same_bits(b, B, (name, md, "bent"))
        assert st["samples"] == N and st["rays"] == N
        got.append(float(v[chosen]))
    assert got == [1.0, 1.0, 0.0], (name, got)
