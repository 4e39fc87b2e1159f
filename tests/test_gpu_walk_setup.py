"""The short walk setup (rt_path.h trav_begin): the three 1/d through rt_device.h recip_in_range behind one range guard on the direction.

tests/native/recip_exhaustive.hip, built here for gfx950 with the library's own CXXFLAGS (the flags the walks are built with):
  * `recip`: every float d with 2^-40 <= |d| <= 2^40, both signs - 2 x (80 x 2^23 + 1) = 1 342 177 282 values - through recip_in_range and
    through `1.0f / d` in the same kernel; 0 mismatches expected, and every value must have been tested.
  * `flags`: trav_begin's fields and the flags closest_hit derives from them (fast, ref, the node count, nearest-first eligibility), new code
    against the formulas of before the short setup copied into the test kernel, bit for bit.  Direction components per axis: the two
    range ends, the floats just outside and just inside them, 2^-60 and 2^60 with their outer neighbours, +-0, subnormals, the least and
    the largest normal, +-inf, a quiet and a signalling NaN, 1 and 0.577 - each with both signs, every combination of the three axes;
    origins: finite, huge on one axis (beyond the compact origin limit), +-inf and NaN on one axis, all NaN; scene layouts with all_finite
    set and clear and with a compact origin limit of zero; every value of compact_domain, COMPACT_DOMAIN and ref_tree.
"""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tiny-raytracer_amd", "csrc")


def library_cxxflags():
    with open(os.path.join(CSRC, "Makefile")) as f:
        m = re.search(r"^CXXFLAGS\s*\?=\s*(.+)$", f.read(), re.M)
    assert m, "CXXFLAGS not found in the library's Makefile"
    flags = [x for x in m.group(1).split() if x != "-fPIC"]
    assert "-ffp-contract=off" in flags and "-O3" in flags, flags
    return flags


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("walk_setup") / "recip_exhaustive")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", *library_cxxflags(), "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "native", "recip_exhaustive.hip")], check=True)
    return exe


def test_recip_in_range_equals_division_on_every_float_of_its_range(program):
    r = subprocess.run([program, "recip"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "1342177282 of 1342177282 values tested, 0 mismatches" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]


def test_setup_fields_equal_the_plain_setup_at_the_guards_edges(program):
    r = subprocess.run([program, "flags"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and " 0 mismatches" in r.stdout and r.stdout.startswith("flags: "), r.stdout[-4000:] + r.stderr[-2000:]
