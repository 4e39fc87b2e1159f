"""The host side the eight direct / nee queries share (csrc/emitter_query.h: the step runner over a query's ordered list of table checks,
the weighted parameters' check, and the two forms around a family's launcher), compiled as plain C++ with
tests/native/emitter_query_check.cpp - a stand-alone program with its own main - against the simulated HIP runtime of
tests/native/hipstub.  No GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_step_runner_and_the_two_forms(tmp_path):
    exe = str(tmp_path / "emitter_query_check")
    n = os.path.join(ROOT, "tests", "native")
    c = os.path.join(ROOT, "tiny-raytracer_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-I" + os.path.join(n, "hipstub"), "-x", "c++", os.path.join(c, "capi.hip"),
                    os.path.join(c, "scene_host.cpp"), os.path.join(n, "launch_stub.cpp"), os.path.join(n, "hipstub", "hipstub.cpp"),
                    os.path.join(n, "emitter_query_check.cpp"), "-lpthread", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok all" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
