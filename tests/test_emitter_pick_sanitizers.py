"""The alias table's host code (csrc/emitter_pick.h: the body of trt_emitter_pick_build and the table checks of trt_direct_pick and
trt_direct_mis_pick), compiled as plain C++ with tests/native/emitter_pick_check.cpp - a stand-alone program with its own main - under
AddressSanitizer and UndefinedBehaviorSanitizer, against the simulated HIP runtime of tests/native/hipstub.  No GPU, nothing loaded
into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_builder_and_the_table_checks_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "emitter_pick_check")
    n = os.path.join(ROOT, "tests", "native")
    c = os.path.join(ROOT, "tiny-raytracer_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                    "-I" + os.path.join(n, "hipstub"), "-x", "c++", os.path.join(c, "capi.hip"), os.path.join(c, "scene_host.cpp"),
                    os.path.join(n, "launch_stub.cpp"), os.path.join(n, "hipstub", "hipstub.cpp"), os.path.join(n, "emitter_pick_check.cpp"),
                    "-lpthread", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=120)
    assert r.returncode == 0 and "ok all" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
