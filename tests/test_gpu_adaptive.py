"""The adaptive sampling driver (api.py Renderer.render_adaptive: render_moments, then select_pixels / render_pixels in a loop) on the
GPU against a restatement that drives the same loop over the CPU oracle (tests/adaptive_cases.py): every range is a whole-frame oracle
render that starts from the current state - orc.render with its running sums, and the numpy fold of the oracle's exact per-sample
colours for the second moments - of which only the active pixels' results are kept; the selection is restated in numpy.  Sums, second
moments, counts and the frame are compared bit for bit over every pixel.

Cases: Cornell 16 x 16 and random_spheres 19 x 13, cap N = 32, min_spp 4, step_spp 4, max_bounces 8, seed 5.  The tolerances were chosen
on the CPU so that the restatement leaves some pixels at min_spp and takes some to N (asserted below: a run in which all or none refine
shows nothing): Cornell rel_tol 0.2 leaves 82 of 256 pixels at 4 samples and takes 55 to 32; random_spheres rel_tol 0.1, abs_tol 0.01
leaves 100 of 247 at 4 and takes 30 to 32.  A third case (random_spheres, rel_tol 0.2, abs_tol 0.02) runs out of active pixels after
24 samples: the loop ends before the cap."""
import numpy as np
import pytest

import adaptive_cases as A
import denoise_color_cases as D
import walk_ray_cases as W

pytestmark = pytest.mark.gpu

SEED, N_CAP, MIN_SPP, STEP_SPP, BOUNCES = 5, 32, 4, 4, 8
CASES = [("cornell", (16, 16), 0.2, 0.0, True), ("random_spheres", (19, 13), 0.1, 0.01, True), ("random_spheres", (19, 13), 0.2, 0.02, False)]
CASE_IDS = ["cornell-16x16", "random_spheres-19x13", "random_spheres-19x13-ends-early"]


@pytest.fixture(scope="module")
def world_of(trt, orc):
    cache = {}

    def get(name, size):
        if (name, size) not in cache:
            desc = W.scene(trt, name)
            desc = dict(desc, camera=dict(desc["camera"], width=size[0], height=size[1]))
            ow, ocam = orc.world_from_description(desc)
            world, cam = trt.world_from_description(desc)
            samples = D.oracle_samples(orc, ow, ocam, N_CAP, BOUNCES, desc["background"], SEED)
            samples.setflags(write=False)
            cache[(name, size)] = dict(desc=desc, ow=ow, ocam=ocam, world=world, cam=cam, samples=samples)
        return cache[(name, size)]

    return get


@pytest.mark.parametrize("name,size,rel_tol,abs_tol,reaches_cap", CASES, ids=CASE_IDS)
def test_render_adaptive_equals_the_loop_over_the_oracle(trt, orc, world_of, name, size, rel_tol, abs_tol, reaches_cap):
    c = world_of(name, size)
    desc = c["desc"]

    def oracle_range(begin, end, state):
        return orc.render(c["ow"], c["ocam"], N_CAP, BOUNCES, desc["background"], seed=SEED, nthreads=4, sample_begin=begin, sample_end=end,
                          accum=state)[0]

    frame, s, m, count, history = A.restated_adaptive(c["samples"], MIN_SPP, STEP_SPP, rel_tol, abs_tol, render_range=oracle_range)
    hist = dict(zip(*[a.tolist() for a in np.unique(count, return_counts=True)]))
    print(f"\n{name} {size[0]}x{size[1]}: rel_tol {rel_tol}, abs_tol {abs_tol}: samples -> pixels {hist}; active per round {[len(a) for a in history]}")
    # the case shows something: some pixels never refine, some refine, and (where the case says so) some go all the way
    assert hist.get(MIN_SPP, 0) >= 20 and (count > MIN_SPP).sum() >= 20
    assert (hist.get(N_CAP, 0) >= 10) if reaches_cap else (count.max() < N_CAP and len(history[-1]) == 0)

    renderer = trt.Renderer(N_CAP, 1, BOUNCES, False, desc["background"], seed=SEED)
    got_frame, got_s, got_m, got_count = renderer.render_adaptive(c["cam"], c["world"], MIN_SPP, STEP_SPP, rel_tol, abs_tol)
    assert got_count.dtype == np.uint32 and np.array_equal(got_count, count), "sample counts differ"
    D.assert_same(got_s, s, (name, "sums"))
    D.assert_same(got_m, m, (name, "second moments"))
    D.assert_same(got_frame, frame, (name, "frame"))
    # every count is min_spp plus a multiple of step_spp, capped at N
    assert ((got_count - MIN_SPP) % STEP_SPP == 0).all() and got_count.min() >= MIN_SPP and got_count.max() <= N_CAP
    # a pixel once dropped is never sampled again: the active sets are nested, and a pixel's count is the end of the last round it was in
    for before, after in zip(history, history[1:]):
        assert np.isin(after, before).all()
    rounds = np.zeros(count.size, np.int64)
    for k, a in enumerate(history):                                        # round k samples history[k] from min_spp + k * step_spp on
        if MIN_SPP + k * STEP_SPP < N_CAP:
            rounds[a] += 1
    assert np.array_equal(np.minimum(MIN_SPP + rounds * STEP_SPP, N_CAP), count.reshape(-1))
    # a pixel with count k holds the bytes of a full render of samples [0, k)
    for k in sorted(set(count.reshape(-1).tolist())):
        full_s, full_m = D.fold_moments(c["samples"], N_CAP, 0, k)
        at = count == k
        assert got_s[at].tobytes() == full_s[at].tobytes() and got_m[at].tobytes() == full_m[at].tobytes(), (name, k)


def test_a_tolerance_nothing_exceeds_renders_min_spp_only(trt, world_of):
    c = world_of("cornell", (16, 16))
    renderer = trt.Renderer(N_CAP, 1, BOUNCES, False, c["desc"]["background"], seed=SEED)
    frame, s, m, count = renderer.render_adaptive(c["cam"], c["world"], MIN_SPP, STEP_SPP, 1e6, 0.0)
    assert (count == MIN_SPP).all()
    want_s, want_m = D.fold_moments(c["samples"], N_CAP, 0, MIN_SPP)
    D.assert_same(s, want_s, "sums at min_spp")
    D.assert_same(m, want_m, "moments at min_spp")
    D.assert_same(frame, want_s * (np.float32(N_CAP) / np.float32(MIN_SPP)), "frame at min_spp")
