"""bench.py on one GPU at a small size: the plain run prints the headline line and nothing else, --dump-outputs writes what the
timed steps computed (the running sums of the frame and the device counters), that frame is the oracle's bit for bit, and a
--full run of the same arguments adds its blocks without changing a bit of what is dumped."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, STEPS, WARMUP = 96, 80, 16, 2, 1
ARGS = ["--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP), "--width", str(W), "--height", str(H), "--spp-per-step", str(SPP)]


def _run(extra, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "TRT_BENCH_REHEARSAL")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + extra, capture_output=True, text=True, timeout=300,
                       env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert lines[-1].startswith("{"), "the JSON line is the last line of stdout"
    return json.loads(lines[-1])


def test_plain_run_dumps_the_oracles_frame_and_full_run_dumps_the_same(trt, orc, tmp_path):
    plain_dir, full_dir = tmp_path / "plain", tmp_path / "full"
    d = _run(["--dump-outputs", str(plain_dir)], tmp_path)
    assert d["metric"] == "Mray/s (primary+secondary)" and d["unit"] == "Mray/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["steps"] == STEPS and d["warmup"] == WARMUP and d["ms_per_step"] > 0 and d["value"] > 0
    assert not {"roofline", "cpu_baseline", "parity", "other_scenes"} & set(d), "a plain run reports the headline only"
    assert sorted(os.listdir(plain_dir)) == ["counters.npy", "frame.npy"]
    frame, counters = np.load(plain_dir / "frame.npy"), np.load(plain_dir / "counters.npy")
    assert frame.dtype == np.float32 and frame.shape == (H, W, 3) and counters.dtype == np.float64 and counters.shape == (16,)
    assert counters[0] == d["config"]["samples"] == STEPS * SPP * W * H and counters[1] == d["config"]["rays"]
    # warm-up and timed steps are consecutive slices of one frame: the sums hold samples [0, (WARMUP + STEPS) * SPP)
    desc = trt.scenes.cornell(W, H)
    ow, ocam = orc.world_from_description(desc)
    cpu, _ = orc.render(ow, ocam, 4096, 50, desc["background"], seed=1, nthreads=8, sample_begin=0, sample_end=(WARMUP + STEPS) * SPP)
    assert np.array_equal(frame.view(np.uint32), np.ascontiguousarray(cpu, np.float32).view(np.uint32))

    f = _run(["--full", "--cpu-seconds", "0", "--dump-outputs", str(full_dir)], tmp_path)
    assert f["roofline"]["launches_timed"] >= STEPS and f["config"]["rays"] == d["config"]["rays"]
    for name in ("frame.npy", "counters.npy"):
        assert np.array_equal(np.load(full_dir / name), np.load(plain_dir / name)), name
