"""Probe queries (tinyrt.h trt_probe, trt_probe_device) on the GPU against the CPU oracle, bit for bit and item by item.

Sample s of item i has stream index j = first_stream + i * K + s.  Its first ray is drawn from RNG stream (seed, j, 1) uniformly over the
sphere or over the hemisphere about the item's axis - restated with the oracle's own random_unit_vector, dot product and Ray::new - and its
path runs on stream (seed, j, 0): orc.sample_batch over the n * K drawn rays with one sample each (tests/probe_cases.py,
tests/radiance_cases.py).  The colours are folded against the basis at the ray's stored direction in numpy float32 exactly as the
contract states; a sample whose ray has a NaN component adds nothing.

Items, per scene (gather_cases.items_of): 324, a full run of 256 for one wave and a ragged one of 68 for the next, four of them with a NaN
point and zero, inf and 1e-9 axes.  K = 8, max_bounces = 8, seed 5, first_stream = 1000, both domains.  The scenes are
test_gpu_queries.DEFAULT_SHAPES plus test_gpu_queries.OTHER_WALKS; each case asserts the kernel shape Scene.probe_plan reports for bands 3
and for bands 2, so all six instantiations of both tables of probe.hip run.  That the reference is not vacuous is asserted without a GPU
(tests/test_probe_cases.py)."""
import numpy as np
import pytest

import probe_cases as PC
import radiance_cases as R
import test_gpu_queries as G
import walk_ray_cases as W

pytestmark = pytest.mark.gpu

K, DEPTH, SEED, FIRST = PC.K, PC.MAX_BOUNCES, PC.SEED, PC.FIRST_STREAM
N = PC.N_ITEMS
GUARD = 64                                                                  # 12-byte entries on either side of a device buffer
FILL = 0xCD
CASES = [(name, {}, shape) for name, shape in G.DEFAULT_SHAPES.items()] + list(G.OTHER_WALKS)
IDS = ["%s-%s" % (name, "-".join("%s=%s" % kv for kv in sorted(options.items())) or "default") for name, options, _ in CASES]
DOMAINS = PC.DOMAINS


def same_bits(got, want, what):
    R.assert_same_bits(got.reshape(len(got), -1), want.reshape(len(want), -1), what)


@pytest.fixture(scope="module")
def reference(trt, orc):
    """name -> description, world, items, and per domain the oracle's first rays [n, K, 6], per-sample colours [n, K, 3], ray count and
    fold [n, 9, 3]; computed once per scene, shared by every test and never changed."""
    cache = {}

    def get(name):
        if name in cache:
            return cache[name]
        desc = W.scene(trt, name)
        ow, _ = orc.world_from_description(desc)
        items, _ = PC.items_of(orc, ow, desc)
        bg = tuple(desc["background"])
        ref = dict(desc=desc, world=trt.world_from_description(desc)[0], items=items, bg=bg)
        for domain in DOMAINS:
            rays, cols, n_rays, _, _ = PC.oracle_probe(orc, ow, items, domain, K, DEPTH, bg, SEED, FIRST)
            S = PC.fold(trt.sh.basis, rays, cols, K)
            ref[domain] = dict(rays=rays, cols=cols, n_rays=n_rays, S=S)
            for a in (rays, cols, S):
                a.setflags(write=False)
        items.setflags(write=False)
        cache[name] = ref
        return ref

    return get


@pytest.fixture(scope="module")
def case(reference):
    """(name, options) -> the reference of the scene plus the product scene compiled with the options, its shape asserted for both tables."""
    cache = {}

    def get(name, options, shape):
        key = (name, tuple(sorted(options.items())))
        if key not in cache:
            ref = reference(name)
            sc = ref["world"].get_bvh(**options)
            for bands in (1, 2, 3):
                q = sc.probe_plan(N, bands)
                assert G.plan_shape(q) == shape, (name, options, bands, q)
            kw = dict(samples_per_item=K, max_bounces=DEPTH, background=ref["bg"], seed=SEED, first_stream=FIRST)
            cache[key] = dict(ref, scene=sc, kw={d: dict(kw, domain=d) for d in DOMAINS})
        return cache[key]

    return get


def sentinel(n=N, coeffs=9):
    return np.full((n, coeffs, 3), 7.5, np.float32)


@pytest.mark.parametrize("domain", DOMAINS)
@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_host_form_is_the_oracles_fold_for_every_number_of_bands(trt, case, name, options, shape, domain):
    """bands 3 against the oracle; bands 1 and 2 are its leading coefficients, by bits (bands 2 runs the 4-coefficient kernels, bands 1
    the same kernels storing one)."""
    c = case(name, options, shape)
    S, st = c["scene"].probe(c["items"], sh=sentinel(), **c["kw"][domain])
    same_bits(S, c[domain]["S"], (name, options, domain, "bands 3"))
    assert st["samples"] == N * K
    assert st["rays"] == c[domain]["n_rays"], (name, options, domain)
    for bands in (1, 2):
        coeffs = bands * bands
        Sb, stb = c["scene"].probe(c["items"], bands=bands, sh=sentinel(N, coeffs), **c["kw"][domain])
        assert Sb.shape == (N, coeffs, 3)
        same_bits(Sb, np.ascontiguousarray(c[domain]["S"][:, :coeffs]), (name, options, domain, "bands", bands))
        assert stb["samples"] == N * K and stb["rays"] == st["rays"]


def device_buffer(torch, entries):
    return torch.full(((GUARD + entries + GUARD) * 12,), FILL, dtype=torch.uint8, device="cuda:0")


def payload(t, n, coeffs):
    """(payload as float32 [n, coeffs, 3], guards intact?)"""
    h = t.cpu().numpy()
    g, b = GUARD * 12, n * coeffs * 12
    return h[g:g + b].copy().view(np.float32).reshape(n, coeffs, 3), bool((h[:g] == FILL).all() and (h[g + b:] == FILL).all())


@pytest.mark.parametrize("bands", (3, 2, 1))
@pytest.mark.parametrize("domain", DOMAINS)
@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_device_form_on_a_side_stream_equals_the_oracle_and_leaves_the_guards(trt, case, name, options, shape, domain, bands):
    import torch
    c = case(name, options, shape)
    coeffs = bands * bands
    d_items = torch.from_numpy(c["items"].copy()).to("cuda:0")
    side = torch.cuda.Stream()
    d_s = device_buffer(torch, N * coeffs)
    ctr = torch.full((16,), 3, dtype=torch.int64, device="cuda:0")          # the counters are added to
    torch.cuda.synchronize()
    c["scene"].probe_device(d_items.data_ptr(), N, d_s.data_ptr() + GUARD * 12, d_counters_ptr=ctr.data_ptr(), stream_ptr=side.cuda_stream,
                            bands=bands, **c["kw"][domain])
    side.synchronize()
    torch.cuda.synchronize()
    got, ok = payload(d_s, N, coeffs)
    assert ok, (name, options, domain, bands, "guard bytes were written")
    same_bits(got, np.ascontiguousarray(c[domain]["S"][:, :coeffs]), (name, options, domain, bands))
    assert int(ctr[0]) == 3 + N * K and int(ctr[1]) == 3 + c[domain]["n_rays"] and bool((ctr[2:] == 3).all())


@pytest.mark.parametrize("bands", (3, 2))
@pytest.mark.parametrize("domain", DOMAINS)
@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_split_by_samples_leaves_the_bytes_of_one_pass(trt, case, name, options, shape, domain, bands):
    c = case(name, options, shape)
    coeffs = bands * bands
    S = sentinel(N, coeffs)
    c["scene"].probe(c["items"], sample_begin=0, sample_end=3, bands=bands, sh=S, **c["kw"][domain])
    S3 = PC.fold(trt.sh.basis, c[domain]["rays"], c[domain]["cols"], K, bands, 0, 3)
    same_bits(S, S3, (name, options, domain, bands, "[0, 3)"))
    _, st = c["scene"].probe(c["items"], sample_begin=3, sample_end=8, accumulate=True, bands=bands, sh=S, **c["kw"][domain])
    same_bits(S, np.ascontiguousarray(c[domain]["S"][:, :coeffs]), (name, options, domain, bands, "[0, 3) + [3, 8)"))
    assert st["samples"] == N * 5


@pytest.mark.parametrize("domain", DOMAINS)
@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_split_by_items_leaves_the_bytes_of_one_call(trt, case, name, options, shape, domain):
    c = case(name, options, shape)
    one, _ = c["scene"].probe(c["items"], **c["kw"][domain])
    S = sentinel()
    kw = dict(c["kw"][domain])
    a = 100
    c["scene"].probe(c["items"][:a], sh=S[:a], **kw)
    assert (S[a:] == 7.5).all()                                             # entries outside the call's range are untouched
    kw["first_stream"] = FIRST + a * K
    assert kw["first_stream"] == 1800
    head = S[:a].copy()
    c["scene"].probe(c["items"][a:], sh=S[a:], **kw)
    assert S[:a].tobytes() == head.tobytes()
    assert S.tobytes() == one.tobytes(), (name, options, domain)            # byte for byte
    same_bits(S, c[domain]["S"], (name, options, domain))


@pytest.mark.parametrize("domain", DOMAINS)
@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_the_drawn_rays_through_radiance_fold_to_the_probe(trt, case, name, options, shape, domain):
    """Without the oracle's paths: the n * K oracle-drawn first rays through Scene.radiance with one sample each and the same
    first_stream (ray i * K + s has stream first_stream + i * K + s), projected and folded in numpy, equal Scene.probe.  Product against
    product."""
    c = case(name, options, shape)
    kw = {k: v for k, v in c["kw"][domain].items() if k not in ("samples_per_item", "domain")}
    cols, _, st1 = c["scene"].radiance(c[domain]["rays"].reshape(-1, 6), 1, **kw)
    want = PC.fold(trt.sh.basis, c[domain]["rays"], cols.reshape(N, K, 3), K)
    S, st = c["scene"].probe(c["items"], **c["kw"][domain])
    same_bits(S, want, (name, options, domain))
    assert st["rays"] == st1["rays"] and st["samples"] == st1["samples"] == N * K


@pytest.mark.parametrize("name,options,shape", CASES, ids=IDS)
def test_nothing_to_trace_zeroes_or_leaves(trt, case, name, options, shape):
    """max_bounces == 0 and an empty sample range: the 12 C n bytes are zeroed without accumulate and untouched with it; through the
    device form no byte outside them is written."""
    import torch
    c = case(name, options, shape)
    for domain, bands in (("sphere", 3), ("hemisphere", 2), ("sphere", 1)):
        coeffs = bands * bands
        for over in (dict(max_bounces=0), dict(sample_begin=3, sample_end=3)):
            kw = dict(c["kw"][domain], bands=bands, **over)
            for accumulate in (False, True):
                S = sentinel(N, coeffs)
                _, st = c["scene"].probe(c["items"], accumulate=accumulate, sh=S, **kw)
                assert (S == (7.5 if accumulate else 0.0)).all(), (name, options, domain, bands, over, accumulate)
                assert st["rays"] == 0 and st["samples"] == 0
    d_items = torch.from_numpy(c["items"].copy()).to("cuda:0")
    for bands in (3, 1):
        coeffs = bands * bands
        for accumulate in (False, True):
            d_s = device_buffer(torch, N * coeffs)
            c["scene"].probe_device(d_items.data_ptr(), N, d_s.data_ptr() + GUARD * 12, accumulate=accumulate, bands=bands,
                                    **dict(c["kw"]["hemisphere"], max_bounces=0))
            torch.cuda.synchronize()
            got, ok = payload(d_s, N, coeffs)
            assert ok, (name, options, bands, "guard bytes were written")
            assert (got.view(np.uint32) == (0xCDCDCDCD if accumulate else 0)).all()


@pytest.mark.parametrize("domain", DOMAINS)
def test_the_furnace(trt, orc, domain):
    """tests/test_probe_cases.py test_the_furnace's case - four probes inside one light, K = 4096 - bit for bit against its CPU reference,
    whose closed form is asserted there."""
    ref = PC.furnace_reference(orc, trt.LIGHT, trt.sh.basis)
    sc = trt.world_from_description(ref["desc"])[0].get_bvh()
    S, st = sc.probe(PC.FURNACE_ITEMS, PC.FURNACE_K, domain=domain, max_bounces=PC.FURNACE_DEPTH, background=ref["desc"]["background"], seed=SEED,
                     first_stream=FIRST)
    same_bits(S, ref[domain]["S"], ("furnace", domain))
    assert st["samples"] == 4 * PC.FURNACE_K and st["rays"] == ref[domain]["n_rays"]
