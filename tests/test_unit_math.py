"""The unit-domain forms of the sampling math (rt_device.h dm_sincos_nonneg / dm_acos_unit / dm_cbrt_unit / random_in_unit_sphere_unit)
against the general functions they are cut from, exhaustively, on the CPU: tests/native/unit_math_check.cpp compiles rt_device.h as plain
C++ (IEEE f32, -ffp-contract=off, the same fma calls) and compares bit for bit.  The device's own arithmetic is compared in
tests/test_gpu_unit_math.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("unit_math") / "unit_math_check")
    n = os.path.join(ROOT, "tests", "native")
    subprocess.run(["g++", "-std=c++17", "-O2", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-I" + os.path.join(n, "hipstub"),
                    "-I" + os.path.join(ROOT, "tiny-raytracer_amd", "csrc"), os.path.join(n, "unit_math_check.cpp"), "-lpthread", "-o", out], check=True)
    return out


def run(exe, what):
    r = subprocess.run([exe, what], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and " 0 mismatches" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]


def test_unit_forms_equal_the_general_functions_on_all_2_23_inputs(exe):
    """sin / cos of theta = 2 pi u, acos(1 - 2u), sin / cos of that phi and cbrt(u) for every u = k 2^-23; also that every theta, phi,
    1 - 2u and u lies inside the domain its form is specified for."""
    run(exe, "math")


def test_composed_sampler_equals_random_in_unit_sphere(exe):
    """2^22 generator states, two consecutive draws each, the generator's state afterwards included."""
    run(exe, "sphere")


def test_primary_ray_quotients_equal_the_division(exe):
    """pixel_uv against `/` for every numerator a column and a draw can give at W = 2, 3, 300, 2048, 3840 (0 + 0 included), and the plain
    division - inf and NaN included - for a 1-wide and a 1-high image."""
    run(exe, "div")
