"""Sample queries past one workgroup: source "rays" over the 324 rays of tests/radiance_cases.py through the device form, every colour
compared by its bits with orc.sample_batch as tests/test_gpu_radiance_long.py compares them - sample s of ray i has stream i * K + s
(first_stream = 0: trt_sample_batch's own numbering), so the oracle's list is each ray K times.

n * R at: the first sample of workgroup 1 (K = 4: 257 rays, 1 028 samples); 100 003 samples - a prime, so K = 309 with the range cut to
fit: 323 rays over [0, 309) and the last ray over [0, 196) in a second call with first_stream = 323 * K; and, on cornell at depth 4 only,
the smallest count at which samples_plan lengthens a wave's run past 256, rounded up to whole rays (about 8 s of oracle, as
tests/test_gpu_radiance_long.py records).  No sample is left out of a comparison, and the records no call owns keep their fill."""
import numpy as np
import pytest

import radiance_cases as R
import test_gpu_queries as G
import walk_ray_cases as W

pytestmark = pytest.mark.gpu

SEED = R.SEED
GUARD = 64
FILL = 0xCD
DEPTH = {"cornell": 4, "grid3000": 2}
N = R.N_RAYS


@pytest.fixture(scope="module")
def scene(trt, orc):
    cache = {}

    def get(name):
        if name not in cache:
            desc = W.scene(trt, name)
            sc = trt.world_from_description(desc)[0].get_bvh()
            assert G.plan_shape(sc.samples_plan(1, 1)) == G.DEFAULT_SHAPES[name]
            cache[name] = dict(desc=desc, ow=orc.world_from_description(desc)[0], scene=sc, rays=R.rays_of(desc), bg=tuple(desc["background"]))
        return cache[name]

    return get


def calls_of(sc, which):
    """(K, [(first ray, rays, sample_begin, sample_end)]): the calls that trace the wanted number of samples of the 324 rays."""
    q = sc.samples_plan(1, 1)
    assert q["rays_per_wave"] == 256
    if which == "workgroup1":
        total = 256 * (q["threads_per_workgroup"] // 64) + 1
    elif which == "100003":
        total = 100003
    else:
        total = 256 * q["wave_slots"] + 1                                   # ceil(n * R / 256) exceeds the resident wave slots
        assert sc.samples_plan(total - 1, 1)["rays_per_wave"] == 256 and sc.samples_plan(1, total)["rays_per_wave"] > 256
    k = -(-total // N)                                                      # the smallest K at which the 324 rays hold that many samples
    if which == "100003":
        full = total // k                                                   # rays traced over the whole range; the next one over the rest
        calls = [(0, full, 0, k), (full, 1, 0, total - full * k)]
        assert full + 1 == N
    else:
        calls = [(0, -(-total // k), 0, k)]                                 # whole rays: a few samples more than asked
        total = calls[0][1] * k
    assert sum(n * (e - b) for _, n, b, e in calls) == total and calls[0][1] * k >= total - k
    return k, total, calls


@pytest.mark.parametrize("which,name", [("workgroup1", "cornell"), ("workgroup1", "grid3000"), ("100003", "cornell"), ("100003", "grid3000"),
                                        ("longer_runs", "cornell")])
def test_long_batches_equal_the_oracle(trt, orc, scene, name, which):
    import torch
    c = scene(name)
    sc, depth = c["scene"], DEPTH[name]
    k, total, calls = calls_of(sc, which)
    if which == "100003":
        assert k == 309 and calls == [(0, 323, 0, 309), (323, 1, 0, 196)]
    q = sc.samples_plan(calls[0][1], k)
    assert q["workgroups"] >= 2 and q["waves"] * q["rays_per_wave"] >= calls[0][1] * k
    if which == "longer_runs":
        assert q["rays_per_wave"] > 256 and sc.samples_plan(calls[0][1] - 1, k)["rays_per_wave"] == 256
    # the oracle: every traced (ray, sample) in record order; record i * K + s is point i * K + s.  The untraced records are the tail of
    # the last ray only, so the traced ones are a prefix
    traced = np.zeros((N, k), bool)
    for first, n, b, e in calls:
        traced[first:first + n, b:e] = True
    last = int(traced.sum())
    assert traced.reshape(-1)[:last].all() and last == total
    rep = np.repeat(c["rays"][:-(-last // k)], k, axis=0)[:last]
    out, st = orc.sample_batch(c["ow"], R.points_of(orc.SamplePoint, rep), depth, c["bg"], SEED)
    want = R.colors_of(out, last)
    n_rays = st["rays"]
    d_rays = torch.from_numpy(c["rays"]).to("cuda:0")
    d_c = torch.full(((GUARD + N * k + GUARD) * 12,), FILL, dtype=torch.uint8, device="cuda:0")
    ctr = torch.zeros(16, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    for first, n, b, e in calls:
        sc.samples_device(d_rays.data_ptr() + first * 24, n, d_c.data_ptr() + (GUARD + first * k) * 12, d_counters_ptr=ctr.data_ptr(), samples_per_item=k,
                          source="rays", max_bounces=depth, background=c["bg"], seed=SEED, first_stream=first * k, sample_begin=b, sample_end=e)
    torch.cuda.synchronize()
    h = d_c.cpu().numpy()
    g = GUARD * 12
    assert (h[:g] == FILL).all() and (h[g + N * k * 12:] == FILL).all(), (name, which, "guard bytes were written")
    got = h[g:g + N * k * 12].view(np.float32).reshape(N * k, 3)
    assert (got[last:].view(np.uint32) == 0xCDCDCDCD).all(), (name, which, "a record outside the calls' ranges was written")
    R.assert_same_bits(np.ascontiguousarray(got[:last]), want, (name, which, total))
    assert int(ctr[0]) == total and int(ctr[1]) == n_rays and not bool(ctr[2:].any())
