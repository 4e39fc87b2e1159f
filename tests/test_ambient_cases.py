"""The reference of the ambient query tests (tests/ambient_cases.py) is not vacuous: conditions on the oracle's answers alone, no GPU.

For the nine scenes of test_gpu_queries.DEFAULT_SHAPES and both lobes, 324 items x 8 samples.  Measured with the CPU oracle when this file
was written: the occluded share at +inf lies between 0.066 (nonfinite) and 0.503 (cornell) and is about halved at D; between 85 and 652
samples change their answer between +inf and D; 95 to 245 items are partly open at +inf and 43 to 189 at D.  The bounds asserted below lie
under those figures: with them an ignored distance, an ignored draw or an ignored lobe cannot pass tests/test_gpu_ambient.py."""
import numpy as np
import pytest

import ambient_cases as A
import gather_cases as GC
import test_gpu_queries as G
import walk_ray_cases as W

SCENES = list(G.DEFAULT_SHAPES)


@pytest.fixture(scope="module")
def reference(trt, orc):
    cache = {}

    def get(name):
        if name not in cache:
            desc = W.scene(trt, name)
            ow, _ = orc.world_from_description(desc)
            items, _ = GC.items_of(orc, ow, desc)
            cache[name] = dict(items=items, **{lobe: A.freeze(A.reference(orc, ow, items, lobe)) for lobe in A.LOBES})
        return cache[name]

    return get


def differing(a, b):
    a, b = a.reshape(len(a), -1), b.reshape(len(b), -1)
    return int((a.view(np.uint32) != b.view(np.uint32)).any(axis=1).sum())


@pytest.mark.parametrize("lobe", A.LOBES)
@pytest.mark.parametrize("name", SCENES)
def test_the_reference_is_not_vacuous(reference, name, lobe):
    ref = reference(name)
    items, r = ref["items"], ref[lobe]
    far, near = r["inf"], r["D"]
    tag = (name, lobe, float(r["distance"]))
    assert np.isfinite(r["distance"]) and r["distance"] > A.T_MIN, tag
    share = far["occ"].mean()
    print(name, lobe, "D", float(r["distance"]), "occluded share", share, near["occ"].mean(), "changed", int((far["occ"] != near["occ"]).sum()))
    assert 0.05 <= share <= 0.6, (tag, share)
    assert not (near["occ"] & ~far["occ"]).any(), tag                       # a shorter range never adds a hit
    assert int((far["occ"] != near["occ"]).sum()) >= 80, tag
    for d in (far, near):
        partly = int(((d["V"] > 0.0) & (d["V"] < 1.0)).sum())
        print("   ", d["max_distance"], "partly open", partly, "distinct", len(set(d["V"].tolist())))
        assert partly >= 40, (tag, d["max_distance"], partly)
        assert len(set(d["V"].tolist())) >= 6, (tag, d["max_distance"])
        with np.errstate(all="ignore"):
            flat = d["V"][:, None] * items[:, 3:6]
        assert differing(d["B"], flat) >= 40, (tag, d["max_distance"])
    assert differing(far["V"], near["V"]) >= 10, tag


@pytest.mark.parametrize("name", SCENES)
def test_the_lobes_differ(reference, name):
    ref = reference(name)
    for dist in A.DISTANCES:
        n = differing(ref["cosine"][dist]["V"], ref["cone"][dist]["V"])
        print(name, dist, "items whose visibility differs between the lobes", n)
        assert n >= 10, (name, dist, n)
    assert differing(ref["cosine"]["rays"], ref["cone"]["rays"]) >= A.N_ITEMS - 4


def test_the_fold_is_the_contracts():
    """By hand on four samples: an occluded sample leaves the sums as they are (-0 stays -0), an unoccluded one adds, ranges continue."""
    rays = np.zeros((2, 4, 6), np.float32)
    rays[0, :, 3:6] = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0.5, 0.5, 0)]
    rays[1, :, 3:6] = [(0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)]
    occ = np.array([[False, True, False, False], [True, True, True, True]])
    V, B = A.fold(occ, rays, 4)
    assert V.tolist() == [0.75, 0.0] and B.tolist() == [[0.375, 0.125, 0.25], [0.0, 0.0, 0.0]]
    V2, B2 = A.fold(occ, rays, 4, 0, 2)
    V2, B2 = A.fold(occ, rays, 4, 2, 4, V2, B2)
    assert V2.tobytes() == V.tobytes() and B2.tobytes() == B.tobytes()
    Vn, Bn = A.fold(occ, rays, 4, vis=np.array([-0.0, -0.0], np.float32), bent=np.full((2, 3), -0.0, np.float32))
    assert np.signbit(Vn[1]) and np.signbit(Bn[1]).all() and not np.signbit(Vn[0])
    assert A.occlusion(None, rays, 0.001).sum() == 0 and A.occlusion(None, rays, -1.0).sum() == 0
