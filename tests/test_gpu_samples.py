"""Sample queries (tinyrt.h trt_samples, trt_samples_device) on the GPU against the CPU oracle, bit for bit and sample by sample.

Sample s of item i has stream index j = first_stream + i * K + s.  Its first ray is the item itself (source "rays": the 324 rays of
radiance_cases.rays_of) or is drawn from RNG stream (seed, j, 1) about one of the 324 items of gather_cases.items_of - the gather queries'
lobes restated by gather_cases.first_rays, the probe queries' domains by probe_cases.first_rays - and its path runs on stream (seed, j, 0):
orc.sample_batch over the first rays (radiance_cases.oracle_samples).  Record i * K + s of `colors` is that path's colour, of `directions`
the first ray's stored direction; the counters are the oracle's.

K = 8, max_bounces = 8, seed 5, first_stream = 1000.  The scenes are test_gpu_queries.DEFAULT_SHAPES plus test_gpu_queries.OTHER_WALKS;
each case asserts the kernel shape Scene.samples_plan reports, so all six instantiations of samples.hip run: all five sources on the first
case of each shape, cosine and sphere on the rest.  The range [3, 8) has R = 5, which divides neither 64 nor 256: the waves' runs cut items
in the middle."""
import numpy as np
import pytest

import gather_cases as GC
import probe_cases as PC
import radiance_cases as R
import test_gpu_queries as G
import walk_ray_cases as W

pytestmark = pytest.mark.gpu

K, DEPTH, SEED, FIRST = R.K, R.MAX_BOUNCES, R.SEED, R.FIRST_STREAM
N = R.N_RAYS
GUARD = 64                                                                  # 12-byte entries on either side of a device buffer
FILL = 0xCD
SOURCES = ("rays", "cosine", "cone", "sphere", "hemisphere")
CASES = [(name, {}, shape) for name, shape in G.DEFAULT_SHAPES.items()] + list(G.OTHER_WALKS)


def _pairs():
    seen, out = set(), []
    for name, options, shape in CASES:
        first = shape[:3] not in seen
        seen.add(shape[:3])
        for source in (SOURCES if first else ("cosine", "sphere")):
            out.append((name, options, shape, source))
    assert len(seen) == 6
    return out


PAIRS = _pairs()
IDS = ["%s-%s-%s" % (name, "-".join("%s=%s" % kv for kv in sorted(options.items())) or "default", source) for name, options, _, source in PAIRS]
every_pair = pytest.mark.parametrize("name,options,shape,source", PAIRS, ids=IDS)


def same_bits(got, want, what):
    R.assert_same_bits(got.reshape(-1, 3), want.reshape(-1, 3), what)


@pytest.fixture(scope="module")
def reference(trt, orc):
    """(name, source) -> the items [n, 6], the oracle's per-sample colours [n, K, 3], first directions [n, K, 3] and ray count; computed
    once per scene and source, shared by every test and never changed."""
    scenes, cache = {}, {}

    def get(name, source):
        if name not in scenes:
            desc = W.scene(trt, name)
            ow, _ = orc.world_from_description(desc)
            scenes[name] = dict(desc=desc, ow=ow, world=trt.world_from_description(desc)[0], bg=tuple(desc["background"]), rays=R.rays_of(desc),
                                items=GC.items_of(orc, ow, desc)[0])
        s = scenes[name]
        if (name, source) not in cache:
            if source == "rays":
                items = s["rays"]
                cols, n_rays = R.oracle_samples(orc, s["ow"], items, K, DEPTH, s["bg"], SEED, FIRST)
                dirs = np.ascontiguousarray(np.broadcast_to(items[:, None, 3:6], (N, K, 3)))
            else:
                items = s["items"]
                if source in GC.LOBES:
                    first, cols, n_rays = GC.oracle_gather(orc, s["ow"], items, source, K, DEPTH, s["bg"], SEED, FIRST)
                else:
                    first, cols, n_rays, _, _ = PC.oracle_probe(orc, s["ow"], items, source, K, DEPTH, s["bg"], SEED, FIRST)
                dirs = np.ascontiguousarray(first[:, :, 3:6])
            for a in (items, cols, dirs):
                a.setflags(write=False)
            cache[(name, source)] = dict(s, items=items, cols=cols, dirs=dirs, n_rays=n_rays)
        return cache[(name, source)]

    return get


@pytest.fixture(scope="module")
def case(reference):
    """(name, options, source) -> the reference plus the product scene compiled with the options, its shape asserted."""
    compiled = {}

    def get(name, options, shape, source):
        ref = reference(name, source)
        key = (name, tuple(sorted(options.items())))
        if key not in compiled:
            sc = ref["world"].get_bvh(**options)
            for n, rl in ((N, K), (N, 5), (1, 700)):
                q = sc.samples_plan(n, rl)
                assert G.plan_shape(q) == shape, (name, options, q)
                assert q["rays_per_wave"] == 256 and q["waves"] == -(-n * rl // 256)
            compiled[key] = sc
        kw = dict(samples_per_item=K, source=source, spread=GC.SPREAD, max_bounces=DEPTH, background=ref["bg"], seed=SEED, first_stream=FIRST)
        return dict(ref, scene=compiled[key], kw=kw)

    return get


def sentinel(n=N, k=K):
    return np.full((n, k, 3), 7.5, np.float32)


@every_pair
def test_host_form_is_the_oracles_colour_and_first_direction_of_every_sample(trt, case, name, options, shape, source):
    c = case(name, options, shape, source)
    cols, dirs, st = c["scene"].samples(c["items"], colors=sentinel(), directions=sentinel(), **c["kw"])
    same_bits(cols, c["cols"], (name, options, source, "colours"))
    same_bits(dirs, c["dirs"], (name, options, source, "directions"))
    assert st["samples"] == N * K
    assert st["rays"] == c["n_rays"], (name, options, source)
    # without the directions the colours are the same
    alone, none, st1 = c["scene"].samples(c["items"], **c["kw"])
    assert none is None and alone.tobytes() == cols.tobytes() and st1["rays"] == st["rays"]


@every_pair
def test_disjoint_ranges_fill_one_buffer_and_leave_the_rest(trt, case, name, options, shape, source):
    """[3, 8) into pre-filled buffers leaves samples 0 - 2 of every item as they were; [0, 3) then completes them to the bytes of one call."""
    c = case(name, options, shape, source)
    cols, dirs = sentinel(), sentinel()
    _, _, st = c["scene"].samples(c["items"], sample_begin=3, sample_end=8, colors=cols, directions=dirs, **c["kw"])
    assert (cols[:, :3] == 7.5).all() and (dirs[:, :3] == 7.5).all()
    same_bits(cols[:, 3:], c["cols"][:, 3:], (name, options, source, "[3, 8) colours"))
    same_bits(dirs[:, 3:], c["dirs"][:, 3:], (name, options, source, "[3, 8) directions"))
    assert st["samples"] == N * 5
    tail = cols[:, 3:].copy()
    _, _, st0 = c["scene"].samples(c["items"], sample_begin=0, sample_end=3, colors=cols, directions=dirs, **c["kw"])
    assert cols[:, 3:].tobytes() == tail.tobytes()
    same_bits(cols, c["cols"], (name, options, source, "[3, 8) + [0, 3) colours"))
    same_bits(dirs, c["dirs"], (name, options, source, "[3, 8) + [0, 3) directions"))
    assert st0["samples"] == N * 3 and st0["rays"] + st["rays"] == c["n_rays"]


@every_pair
def test_split_by_items_leaves_the_bytes_of_one_call(trt, case, name, options, shape, source):
    c = case(name, options, shape, source)
    one, one_d, _ = c["scene"].samples(c["items"], directions=True, **c["kw"])
    cols, dirs = sentinel(), sentinel()
    kw = dict(c["kw"])
    a = 100
    c["scene"].samples(c["items"][:a], colors=cols[:a], directions=dirs[:a], **kw)
    assert (cols[a:] == 7.5).all() and (dirs[a:] == 7.5).all()             # entries outside the call's items are untouched
    kw["first_stream"] = FIRST + a * K
    head = cols[:a].copy()
    c["scene"].samples(c["items"][a:], colors=cols[a:], directions=dirs[a:], **kw)
    assert cols[:a].tobytes() == head.tobytes()
    assert cols.tobytes() == one.tobytes() and dirs.tobytes() == one_d.tobytes(), (name, options, source)
    same_bits(cols, c["cols"], (name, options, source))


def device_buffer(torch, entries):
    return torch.full(((GUARD + entries + GUARD) * 12,), FILL, dtype=torch.uint8, device="cuda:0")


def payload(t, n, k):
    """(payload as float32 [n, k, 3], guards intact?)"""
    h = t.cpu().numpy()
    g, b = GUARD * 12, n * k * 12
    return h[g:g + b].copy().view(np.float32).reshape(n, k, 3), bool((h[:g] == FILL).all() and (h[g + b:] == FILL).all())


@every_pair
def test_device_form_on_a_side_stream_equals_the_oracle_and_leaves_the_guards(trt, case, name, options, shape, source):
    import torch
    c = case(name, options, shape, source)
    d_items = torch.from_numpy(c["items"].copy()).to("cuda:0")
    side = torch.cuda.Stream()
    d_c, d_d, d_c2 = device_buffer(torch, N * K), device_buffer(torch, N * K), device_buffer(torch, N * K)
    ctr = torch.full((16,), 3, dtype=torch.int64, device="cuda:0")          # the counters are added to
    torch.cuda.synchronize()
    c["scene"].samples_device(d_items.data_ptr(), N, d_c.data_ptr() + GUARD * 12, d_d.data_ptr() + GUARD * 12, d_counters_ptr=ctr.data_ptr(),
                              stream_ptr=side.cuda_stream, **c["kw"])
    c["scene"].samples_device(d_items.data_ptr(), N, d_c2.data_ptr() + GUARD * 12, stream_ptr=side.cuda_stream, **c["kw"])      # directions = NULL
    side.synchronize()
    torch.cuda.synchronize()
    cols, ok_c = payload(d_c, N, K)
    dirs, ok_d = payload(d_d, N, K)
    cols2, ok_c2 = payload(d_c2, N, K)
    assert ok_c and ok_d and ok_c2, (name, options, source, "guard bytes were written")
    same_bits(cols, c["cols"], (name, options, source, "colours"))
    same_bits(dirs, c["dirs"], (name, options, source, "directions"))
    assert cols2.tobytes() == cols.tobytes()
    assert int(ctr[0]) == 3 + N * K and int(ctr[1]) == 3 + c["n_rays"] and bool((ctr[2:] == 3).all())
    # a range through the device form: the records outside it keep their fill
    d_c3, d_d3 = device_buffer(torch, N * K), device_buffer(torch, N * K)
    c["scene"].samples_device(d_items.data_ptr(), N, d_c3.data_ptr() + GUARD * 12, d_d3.data_ptr() + GUARD * 12, sample_begin=3, sample_end=8, **c["kw"])
    torch.cuda.synchronize()
    cols3, ok3 = payload(d_c3, N, K)
    dirs3, ok3d = payload(d_d3, N, K)
    assert ok3 and ok3d
    assert (cols3[:, :3].view(np.uint32) == 0xCDCDCDCD).all() and (dirs3[:, :3].view(np.uint32) == 0xCDCDCDCD).all()
    same_bits(cols3[:, 3:], c["cols"][:, 3:], (name, options, source, "device [3, 8)"))
    same_bits(dirs3[:, 3:], c["dirs"][:, 3:], (name, options, source, "device [3, 8) directions"))


@every_pair
def test_nothing_to_trace(trt, case, name, options, shape, source):
    """An empty range touches nothing.  max_bounces == 0: the colours of the range become +0, the directions are not written, nothing is
    counted; through the device form no byte outside the range's colours is written."""
    import torch
    c = case(name, options, shape, source)
    cols, dirs = sentinel(), sentinel()
    _, _, st = c["scene"].samples(c["items"], sample_begin=3, sample_end=3, colors=cols, directions=dirs, **c["kw"])
    assert (cols == 7.5).all() and (dirs == 7.5).all() and st["samples"] == 0 and st["rays"] == 0
    kw = dict(c["kw"], max_bounces=0)
    _, _, st = c["scene"].samples(c["items"], sample_begin=3, sample_end=8, colors=cols, directions=dirs, **kw)
    assert (cols[:, :3] == 7.5).all() and (cols[:, 3:].view(np.uint32) == 0).all() and (dirs == 7.5).all()
    assert st["samples"] == 0 and st["rays"] == 0
    d_items = torch.from_numpy(c["items"].copy()).to("cuda:0")
    d_c, d_d = device_buffer(torch, N * K), device_buffer(torch, N * K)
    ctr = torch.full((16,), 3, dtype=torch.int64, device="cuda:0")
    c["scene"].samples_device(d_items.data_ptr(), N, d_c.data_ptr() + GUARD * 12, d_d.data_ptr() + GUARD * 12, d_counters_ptr=ctr.data_ptr(), **kw)
    c["scene"].samples_device(d_items.data_ptr(), N, d_d.data_ptr() + GUARD * 12, d_d.data_ptr() + GUARD * 12, d_counters_ptr=ctr.data_ptr(),
                              sample_begin=8, sample_end=8, **c["kw"])
    torch.cuda.synchronize()
    got, ok = payload(d_c, N, K)
    untouched, ok_d = payload(d_d, N, K)
    assert ok and ok_d
    assert (got.view(np.uint32) == 0).all() and (untouched.view(np.uint32) == 0xCDCDCDCD).all() and bool((ctr == 3).all())


K_ONE = 700


@pytest.mark.parametrize("source", ("cosine", "hemisphere"))
@pytest.mark.parametrize("name", ("cornell", "random_spheres", "grid3000"))
def test_one_item_over_three_waves(trt, orc, reference, name, source):
    """One item with K = 700: its samples are the runs of three waves (256, 256, 188), where the folding queries give them one lane."""
    ref = reference(name, source)
    sc = ref["world"].get_bvh()
    q = sc.samples_plan(1, K_ONE)
    assert q["waves"] == 3 and q["rays_per_wave"] == 256
    item = np.ascontiguousarray(ref["items"][7:8])
    if source in GC.LOBES:
        first, want, n_rays = GC.oracle_gather(orc, ref["ow"], item, source, K_ONE, DEPTH, ref["bg"], SEED, FIRST)
    else:
        first, want, n_rays, _, _ = PC.oracle_probe(orc, ref["ow"], item, source, K_ONE, DEPTH, ref["bg"], SEED, FIRST)
    cols, dirs, st = sc.samples(item, K_ONE, source=source, max_bounces=DEPTH, background=ref["bg"], seed=SEED, first_stream=FIRST,
                                colors=sentinel(1, K_ONE), directions=sentinel(1, K_ONE))
    same_bits(cols, want, (name, source, "colours"))
    same_bits(dirs, np.ascontiguousarray(first[:, :, 3:6]), (name, source, "directions"))
    assert st["samples"] == K_ONE and st["rays"] == n_rays
