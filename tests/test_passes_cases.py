"""The reference the passes tests compare against (tests/passes_cases.py), without a GPU.

oracle_paths restates cpu.rs:39-65 with the class of every sample; here it is pinned to the oracle's own loop: on every scene the GPU
tests use and for every source its colours equal radiance_cases.oracle_samples (orc.sample_batch) byte for byte and its world.hit calls
are as many.  The array fold equals the fold written out scalar by scalar, identity 1 of tinyrt.h holds between it and
radiance_cases.fold, identity 2 across the numbers of bins, and the inputs reach every slot: the coverage conditions below are asserted
on the oracle's side, so they hold before any GPU is involved.  Observed values, measured with the CPU oracle, stand in brackets."""
import numpy as np
import pytest

import passes_cases as P
import radiance_cases as R

K, N = P.K, P.N_ITEMS


def test_the_scenes_reach_every_kernel_shape():
    """One scene per (scene mode, walk, workgroup shape) of test_gpu_queries' tables: six different shapes."""
    import test_gpu_queries as G
    shapes = []
    for name, options in P.CASES:
        if options:
            shape = [s for n, o, s in G.OTHER_WALKS if n == name and o == options]
            assert len(shape) == 1
            shapes.append(shape[0][:3])
        else:
            shapes.append(G.DEFAULT_SHAPES[name][:3])
    assert len(set(shapes)) == 6, shapes
    assert set(n for n, _ in P.CASES) == set(P.SCENES)


@pytest.mark.parametrize("source", P.SOURCES)
@pytest.mark.parametrize("name", P.SCENES)
def test_the_classifier_is_the_oracles_own_loop(trt, orc, name, source):
    ref = P.reference(trt, orc, name)
    r = ref[source]
    assert r["items"].shape == (N, 6) and r["rays"].shape == (N, K, 6) and N == 324
    cols, n_rays = R.oracle_samples(orc, ref["ow"], r["rays"].reshape(-1, 6), 1, P.MAX_BOUNCES, ref["bg"], P.SEED, P.FIRST_STREAM)
    assert cols.reshape(N, K, 3).tobytes() == r["cols"].tobytes(), (name, source)
    assert n_rays == r["n_rays"], (name, source)
    kinds, depths = r["kinds"], r["depths"]
    # what the classes say about the loop: a spent path scattered max_bounces times and its colour is 0; the others called world.hit
    # once more than they scattered
    spent = kinds == P.SPENT
    assert (depths[spent] == P.MAX_BOUNCES).all() and (depths[~spent] < P.MAX_BOUNCES).all()
    assert not r["cols"][spent].view(np.uint32).any()                       # exactly +0
    assert r["n_rays"] == int(depths[spent].sum() + (depths[~spent] + 1).sum())
    # a first ray with a NaN component hits nothing: SKY at depth 0 with the background
    nan_ray = np.isnan(r["rays"]).any(axis=2)
    assert nan_ray.any()
    assert (kinds[nan_ray] == P.SKY).all() and (depths[nan_ray] == 0).all()
    assert (r["cols"][nan_ray] == np.array(ref["bg"], np.float32)).all()


@pytest.mark.parametrize("source", P.SOURCES)
def test_the_inputs_reach_every_slot(trt, orc, source):
    """B = 4, max_bounces = 5, over the scenes used: each of the 8 slots is non-zero for at least 8 items, `spent` for at least 8, and
    at least one item has two or more non-zero slots."""
    slot_items, spent_items, multi = np.zeros(8, int), 0, 0
    for name in P.SCENES:
        r = P.reference(trt, orc, name)[source]
        passes, spent = P.fold(r["cols"], r["kinds"], r["depths"], K, 4)
        assert passes.shape == (N, 8, 3) and spent.shape == (N,)
        nonzero = (passes != 0.0).any(axis=2)
        slot_items += nonzero.sum(axis=0)
        spent_items += int((spent != 0.0).sum())
        multi += int((nonzero.sum(axis=1) >= 2).sum())
    print(source, "items with a non-zero slot", slot_items.tolist(), "spent", spent_items, "with two slots or more", multi)
    assert (slot_items >= 8).all(), (source, slot_items)                    # [21 - 1518; the emitters' slots come from cornell, prims33, prims600]
    assert spent_items >= 8, (source, spent_items)                          # [484 - 595]
    assert multi >= 1, (source, multi)                                      # [837 - 1114]


@pytest.mark.parametrize("source", P.SOURCES)
@pytest.mark.parametrize("name", P.SCENES)
def test_the_array_fold_is_the_scalar_fold(trt, orc, name, source):
    r = P.reference(trt, orc, name)[source]
    for bins in P.BINS:
        passes, spent = P.fold(r["cols"], r["kinds"], r["depths"], K, bins)
        for i in (0, 7, 100, N - 4, N - 1):
            want_p, want_s = P.fold_one_item(r["cols"][i], r["kinds"][i], r["depths"][i], K, bins)
            assert want_p.tobytes() == passes[i].tobytes(), (name, source, bins, i)
            assert np.float32(want_s).tobytes() == spent[i].tobytes(), (name, source, bins, i)
        # a split by samples continues the sums
        part_p, part_s = P.fold(r["cols"], r["kinds"], r["depths"], K, bins, end=3)
        again_p, again_s = P.fold(r["cols"], r["kinds"], r["depths"], K, bins, begin=3, passes=part_p, spent=part_s)
        assert again_p.tobytes() == passes.tobytes() and again_s.tobytes() == spent.tobytes()
        # every sample is in exactly one class: the spent shares and the samples with a slot add up to the samples
        slots = P.slots_of(r["kinds"], r["depths"], bins)
        assert ((slots >= 0).sum(axis=1) + (r["kinds"] == P.SPENT).sum(axis=1) == K).all()
        assert slots.max() < 2 * bins


def test_the_fold_leaves_the_other_slots_alone():
    """Not adding is not adding 0: a slot that holds -0 keeps its sign bit unless a sample of its own class arrives."""
    cols = np.array([[[1.0, 2.0, 3.0], [0.0, 0.0, 0.0], [4.0, 4.0, 4.0]]], np.float32)
    kinds = np.array([[P.LIGHT, P.SPENT, P.SKY]], np.int8)
    depths = np.array([[0, 5, 3]], np.int32)
    start = np.full((1, 4, 3), -0.0, np.float32)
    passes, spent = P.fold(cols, kinds, depths, 4, 2, passes=start, spent=np.array([-0.0], np.float32))
    assert passes[0, 0].tolist() == [0.25, 0.5, 0.75] and passes[0, 3].tolist() == [1.0, 1.0, 1.0]           # LIGHT d = 0; SKY d = 3 -> bin 1
    assert (passes[0, 1:3].view(np.uint32) == 0x80000000).all()             # untouched: still -0
    assert spent[0] == np.float32(0.25)


@pytest.mark.parametrize("source", P.SOURCES)
@pytest.mark.parametrize("name", P.SCENES)
def test_the_two_identities(trt, orc, name, source):
    """tinyrt.h trt_passes.  (1) With background 0 and one bin, slot 0 is the fold of trt_radiance / trt_gather byte for byte (the
    scenes' light colours and albedos are not negative).  (2) The slots at depth d < B - 1 do not depend on B."""
    ref = P.reference(trt, orc, name)
    r = ref[source]
    for _, kind, albedo, _ in ref["desc"]["materials"]:
        assert min(albedo) >= 0.0
    black = (0.0, 0.0, 0.0)
    cols, kinds, depths, _ = P.oracle_paths(orc, ref["ow"], ref["desc"], r["rays"], P.MAX_BOUNCES, black, P.SEED, P.FIRST_STREAM)
    passes, _ = P.fold(cols, kinds, depths, K, 1)
    S, _ = R.fold(cols, K)
    assert passes[:, 0, :].tobytes() == S.tobytes(), (name, source)
    assert not passes[:, 1, :].view(np.uint32).any()                        # the sky is black: +0
    by_bins = {b: P.fold(r["cols"], r["kinds"], r["depths"], K, b)[0] for b in P.BINS}
    for b in P.BINS:
        for b2 in P.BINS:
            for d in range(min(b, b2) - 1):
                assert by_bins[b][:, d].tobytes() == by_bins[b2][:, d].tobytes(), (name, source, b, b2, d)
                assert by_bins[b][:, b + d].tobytes() == by_bins[b2][:, b2 + d].tobytes(), (name, source, b, b2, d)


def test_the_slot_names(trt):
    ps = trt.passes
    assert [ps.slot("light", d, 4) for d in range(6)] == [0, 1, 2, 3, 3, 3]
    assert [ps.slot("sky", d, 4) for d in range(6)] == [4, 5, 6, 7, 7, 7]
    assert ps.slot("light", 3, 1) == 0 and ps.slot("sky", 0, 1) == 1 and ps.slot("sky", 1, 2) == 3
    for bad in (dict(kind="spent", depth=0, bins=2), dict(kind="light", depth=0, bins=0), dict(kind="light", depth=0, bins=5),
                dict(kind="sky", depth=-1, bins=2)):
        with pytest.raises(ValueError):
            ps.slot(**bad)
    p = np.arange(2 * 6 * 3, dtype=np.float32).reshape(2, 6, 3)
    assert np.array_equal(ps.direct(p), p[:, 0] + p[:, 3])
    assert np.array_equal(ps.indirect(p), p[:, 1] + p[:, 2] + p[:, 4] + p[:, 5])
    assert np.array_equal(ps.emitters(p), p[:, 0] + p[:, 1] + p[:, 2]) and np.array_equal(ps.sky(p), p[:, 3] + p[:, 4] + p[:, 5])
    assert np.allclose(ps.direct(p) + ps.indirect(p), ps.emitters(p) + ps.sky(p))
    with pytest.raises(ValueError):
        ps.direct(p[:, :2])
    with pytest.raises(ValueError):
        ps.bins_of(np.zeros((3, 5, 3)))
