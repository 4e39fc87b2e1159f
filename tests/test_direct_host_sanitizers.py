"""trt_scene_emitters reads the scene's lights back from the packed scene (capi.hip), and the emitter init functions compute a record's
normal and area (scene_host.cpp): host code, compiled here as plain C++ with tests/native/emitters_check.cpp - a stand-alone program -
under AddressSanitizer and UndefinedBehaviorSanitizer, against the simulated HIP runtime of tests/native/hipstub.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scene_emitters_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "emitters_check")
    n = os.path.join(ROOT, "tests", "native")
    c = os.path.join(ROOT, "tiny-raytracer_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                    "-I" + os.path.join(n, "hipstub"), "-x", "c++", os.path.join(c, "capi.hip"), os.path.join(c, "scene_host.cpp"),
                    os.path.join(n, "launch_stub.cpp"), os.path.join(n, "hipstub", "hipstub.cpp"), os.path.join(n, "emitters_check.cpp"), "-lpthread",
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=120)
    assert r.returncode == 0 and "ok all" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
