"""gather_ray and probe_ray (csrc/gather_draw.h), the two functions that draw a sample's first ray on the device, case by case against
the oracle - every word, no tolerance.

tests/native/draw_cases.hip (built here for gfx950 with the library's own CXXFLAGS) seeds the product's rng_seed(seed_key, j, 1) for
each case of tests/draw_cases.py, calls gather_ray (cosine, cone) or probe_ray (sphere, hemisphere) and writes back the six words of
the ray and the generator state, which must be the oracle's after exactly three draws.  The list goes in twice: one wave takes the
whole shuffled list 64 cases at a time (its lanes hold different lobes, domains and branches), then waves with lists of 1, 63, 64 and
65 cases from a second shuffle; every copy must equal the expectation.

NaN words compare by their bits - the 0/0 of a u3 = 0 draw and of a zero sum give the oracle's bit patterns on gfx950 - except in
rows whose ITEM is non-finite, where x86-64 and gfx950 propagate an input NaN's payload and sign differently: there a word that is
NaN on both sides passes, and the count of such words is printed.

Negative control: the same list with every stream moved by one against the unmoved expectation - every generic row must differ.

tests/README_draws.md holds the measured figures.
"""
import os
import re
import subprocess
import time

import numpy as np
import pytest

import draw_cases as D

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tiny-raytracer_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def library_cxxflags():
    """CXXFLAGS of the library's Makefile: the harness is built with the flags gather_ray and probe_ray are built with."""
    with open(os.path.join(CSRC, "Makefile")) as f:
        m = re.search(r"^CXXFLAGS\s*\?=\s*(.+)$", f.read(), re.M)
    assert m, "CXXFLAGS not found in the library's Makefile"
    flags = m.group(1).split()
    assert "-ffp-contract=off" in flags and "-O3" in flags, flags
    return flags


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("draw_cases") / "draw_cases")
    t0 = time.time()
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", *library_cxxflags(), "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "native", "draw_cases.hip")],
                       timeout=900)
    assert r.returncode == 0, "the harness does not compile"
    print(f"\nharness built in {time.time() - t0:.1f} s")
    return exe


@pytest.fixture(scope="module")
def results(orc, harness, tmp_path_factory):
    """One child process for both runs, under its own time limit; a non-zero exit fails everything and nothing is run again."""
    d = tmp_path_factory.mktemp("draws")
    cases = D.case_list(orc)
    order, tasks = D.wave_lists(len(cases))
    exp = D.expectations(orc, cases)[order]
    exp.setflags(write=False)
    D.write_case_file(str(d / "cases.bin"), cases, order, tasks)
    t0 = time.time()
    r = subprocess.run([harness, str(d / "cases.bin"), "0", str(d / "out.bin"), "1", str(d / "moved.bin")], capture_output=True, text=True, timeout=120)
    print(f"\nharness ran in {time.time() - t0:.2f} s: {r.stdout.strip()}")
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    out = {k: np.fromfile(d / f"{k}.bin", np.uint32).reshape(len(order), D.OUT_WORDS) for k in ("out", "moved")}
    rows = [cases[i] for i in order]
    return dict(cases=cases, rows=rows, order=order, tasks=tasks, exp=exp, nonfinite=np.array([not np.isfinite(c["item"]).all() for c in rows]), **out)


def test_every_word_equals_the_oracle(results):
    res = results
    got, exp = res["out"], res["exp"]
    assert not (got == 0xCDCDCDCD).all(axis=1).any()                                          # every record written
    bad, by_class = D.differing_words(got, exp, res["nonfinite"])
    per_class = {}
    for c in res["rows"]:
        per_class[c["cls"]] = per_class.get(c["cls"], 0) + 1
    nan_by_bits = int((np.isnan(exp[~res["nonfinite"]][:, 0:6].view(F))).sum())
    print(f"\n{len(got)} answers ({len(res['cases'])} cases, each twice), {int(bad.sum())} differing words, {int(by_class.sum())} NaN words compared by class, "
          f"{nan_by_bits} NaN words compared by bits; per class: {per_class}")
    where = np.flatnonzero(bad.any(axis=1))
    assert len(where) == 0, (f"{len(where)} answers differ", [(int(res["order"][p]), res["rows"][p]["cls"], res["rows"][p]["kind"]) for p in where[:8]],
                             got[where[:3]], exp[where[:3]])
    # every copy of a case gets the same bits, whichever wave and lane it had
    n = len(res["cases"])
    first, second = np.argsort(res["order"][:n]), n + np.argsort(res["order"][n:])
    assert np.array_equal(got[first], got[second])


def test_exactly_three_draws_are_taken(results, orc):
    """The state written back is the oracle's after three outputs - not two, not four."""
    res = results
    assert np.array_equal(res["out"][:, 6:8], res["exp"][:, 6:8])
    import ctypes as C
    for p in range(0, len(res["rows"]), 997):
        rng = D.stream_state(orc, res["rows"][p]["j"])
        states = []
        for _ in range(4):
            orc.lib.orc_rng_next_u32(C.byref(rng))
            states.append((int(rng[0]), int(rng[1])))
        got = (int(res["out"][p, 6]), int(res["out"][p, 7]))
        assert got == states[2] and got != states[1] and got != states[3]


def test_control_streams_moved_by_one_are_seen_in_every_generic_row(results, orc):
    res = results
    generic = np.array([c["cls"] == "generic" for c in res["rows"]])
    differs = (res["moved"] != res["exp"]).any(axis=1)
    ray_differs = (res["moved"][:, 0:6] != res["exp"][:, 0:6]).any(axis=1)
    print(f"\ncontrol: {int(differs.sum())} of {len(differs)} answers differ, {int((differs & generic).sum())} of {int(generic.sum())} generic ones; "
          f"the ray itself in {int((ray_differs & generic).sum())}")
    assert differs[generic].all()
    # the ray itself too, wherever the draw reaches it: a cone of spread 0 is Ray::new(point, axis) for every stream (its state still differs)
    drawn = np.array([not (c["kind"] == "cone" and c["spread"] == 0) for c in res["rows"]])
    assert ray_differs[generic & drawn & ~res["nonfinite"]].all() and not ray_differs[generic & ~drawn & ~res["nonfinite"]].any()
    # and the moved run is no garbage: it is the oracle's answer for the moved streams
    moved_cases = [dict(c, j=(c["j"] + 1) & 0xFFFFFFFF) for c in res["cases"]]
    exp_moved = D.expectations(orc, moved_cases)[res["order"]]
    bad, _ = D.differing_words(res["moved"], exp_moved, res["nonfinite"])
    assert not bad.any()
