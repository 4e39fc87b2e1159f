"""The streamed launch rule (csrc/stream_plan.h: streamed_launch_plan in stages, LdsLayout, the kernel tables as lists, plan_batch) on
the CPU.  tests/native/stream_plan_check.cpp is a stand-alone program: built with g++ - the header holds host arithmetic only - it sweeps
7.26 million combinations of scene size, layout flags and knobs (hot_bytes on either side of every threshold, which compiled scenes
cannot place) and 172 800 batch plans, holds every plan against a digest recorded from the rule before it was split into stages, checks
the invariants of test_host_boundary.py's _check_plan on all of them, and that every row of both kernel tables is chosen.  Once plain
and once under AddressSanitizer + UBSan; nothing is loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "asan_ubsan"])
def test_every_plan_is_the_recorded_one_and_keeps_the_invariants(tmp_path, flags):
    n = os.path.join(ROOT, "tests", "native")
    exe = str(tmp_path / "stream_plan_check")
    subprocess.run(["g++", "-std=c++17", *flags, "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(n, "hipstub"),
                    os.path.join(n, "stream_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "streamed plans 7257600 " in r.stdout and "batch plans 172800 " in r.stdout and "stream_plan_check ok: 37 kernel rows all chosen" in r.stdout, r.stdout
