"""The alias draw of trt_direct_pick / trt_direct_mis_pick (csrc/gather_draw.h: direct_draw_from with the AliasPick policy, through the
forwarder both PICK kernels call), one case per lane against tests/direct_pick_cases.py - every word, no tolerance.

tests/native/direct_pick_cases.hip (built here for gfx950 with the library's own CXXFLAGS) seeds the product's rng_seed(seed_key, j, 1)
for each case of direct_pick_cases.draw_cases, draws on the case's own emitter and pick tables and writes back the ray, c, t_max, the
live flag, wgt, the record's geometry word and the generator state, which must be the restatement's after exactly four (quad) or five
(sphere) draws.  The list goes in shuffled, twice, so the lanes of a wave mix tables, quads and spheres, kept slots and aliases, live
and dead samples, and every copy of a case must get the same bits whichever lane it had; 1200 cases are no multiple of 64 x 4.

The classes a whole query reaches only by luck are here by construction: q[k] set to the case's own u1 (takes the alias) and to the next
float up (keeps the slot); q = 0, 1 and NaN; aliases past the table; prob = 0, a prob that overflows area / p, a subnormal prob that does
not; E = 1; and E = 65521 on streams where uint32(u0 * float(E)) in f32 is not the exact floor.

Live rows compare by their bits in all 15 words.  In dead rows the flag, the geometry word and the state compare by their bits and the
float words too, except that a word that is NaN on both sides passes (which NaN a dead sample carries is not contract)."""
import os
import subprocess
import time

import numpy as np
import pytest

import direct_mis_cases as M
import direct_pick_cases as P
from test_gpu_direct_draws import CSRC, HIPCC, ROOT, library_cxxflags

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("direct_pick_cases") / "direct_pick_cases")
    t0 = time.time()
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", *library_cxxflags(), "-I", CSRC, "-o", exe,
                        os.path.join(ROOT, "tests", "native", "direct_pick_cases.hip")], timeout=900)
    assert r.returncode == 0, "the harness does not compile"
    print(f"\nharness built in {time.time() - t0:.1f} s")
    return exe


@pytest.fixture(scope="module")
def results(trt, orc, harness, tmp_path_factory):
    """One child process, under its own time limit; a non-zero exit fails everything and nothing is run again."""
    d = tmp_path_factory.mktemp("direct_pick_draws")
    sc = M.scene(trt, orc, "cornell")
    cases, tables = P.draw_cases(orc, sc["items"], sc["table"])
    exp, flags = P.draw_expectations(orc, cases, tables)
    g = np.random.default_rng([P.SEED, 18])
    order = np.concatenate([g.permutation(len(cases)), g.permutation(len(cases))])
    P.write_draw_cases(str(d / "cases.bin"), cases, tables, order)
    t0 = time.time()
    r = subprocess.run([harness, str(d / "cases.bin"), str(d / "out.bin")], capture_output=True, text=True, timeout=120)
    print(f"\nharness ran in {time.time() - t0:.2f} s: {r.stdout.strip()}")
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    out = np.fromfile(d / "out.bin", np.uint32).reshape(len(order), P.OUT_WORDS)
    return dict(cases=cases, order=order, exp=exp, flags=flags, out=out, cls=np.array([c["cls"] for c in cases]))


def differing_words(got, exp):
    """bool [n, 15]: words that differ, where a float word of a dead row that is NaN on both sides passes."""
    bad = got != exp
    dead = exp[:, 10] == 0
    both_nan = np.isnan(got[:, 0:12].view(np.float32)) & np.isnan(exp[:, 0:12].view(np.float32))
    both_nan[:, 10] = False
    bad[:, 0:12] &= ~(both_nan & dead[:, None])
    return bad


def test_every_word_equals_the_restatement(results):
    res = results
    got, exp = res["out"], res["exp"][res["order"]]
    assert not (got == 0xCDCDCDCD).all(axis=1).any()                                          # every record written
    bad = differing_words(got, exp)
    cls = res["cls"][res["order"]]
    where = np.flatnonzero(bad.any(axis=1))
    print(f"\n{len(got)} answers ({len(res['cases'])} cases, each twice; {int((exp[:, 10] == 1).sum())} live), {int(bad.sum())} differing words")
    assert len(where) == 0, (f"{len(where)} answers differ", sorted(set(cls[where])), got[where[:3]], exp[where[:3]])
    # every copy of a case gets the same bits, whichever wave and lane it had
    n = len(res["cases"])
    first, second = np.argsort(res["order"][:n]), n + np.argsort(res["order"][n:])
    assert np.array_equal(got[first], got[second])
    # exactly four or five draws: the state is the restatement's (which the words above include), and lanes of one wave hold it all
    for w in range(2):
        lanes = res["order"][64 * w:64 * w + 64]
        f = res["flags"]
        kinds = {(bool(f["took_alias"][i]), bool(f["live"][i])) for i in lanes}
        assert len(kinds) == 4 and len(set(res["cls"][lanes])) >= 4, (w, kinds)


def test_the_classes_hold_what_they_are_for(results, orc):
    """On the device's own words: which record a lane chose is told by its geometry word and, for a quad against a sphere, by the state."""
    res = results
    n = len(res["cases"])
    got = res["out"][np.argsort(res["order"][:n])]
    f, cls = res["flags"], res["cls"]
    assert np.array_equal(got[:, 10] == 1, f["live"])
    edge = np.flatnonzero(cls == "edge_of_q")
    at, above = edge[0::2], edge[1::2]                                      # q = u1, q = the next float: alias, slot
    assert f["took_alias"][at].all() and not f["took_alias"][above].any() and (f["slot"][at] == f["slot"][above]).all()
    assert (f["e"][at] == (f["slot"][at] + 1) % 3).all() and (f["e"][above] == f["slot"][above]).all()
    assert (got[at, 13:15] != got[above, 13:15]).any(axis=1).sum() >= 12    # a quad against a sphere: another number of draws
    assert (got[at, 0:12] != got[above, 0:12]).any(axis=1).all()
    for name, takes in (("q_0", True), ("q_nan", True), ("q_1", False)):
        assert (f["took_alias"][cls == name] == takes).all(), name
    assert (f["e"][cls == "alias_clamped"] == 2).all() and f["live"][cls == "alias_clamped"].any()
    for name in ("prob_0", "prob_overflow"):
        assert not f["live"][cls == name].any() and not (got[cls == name, 10] == 1).any()
    sub = cls == "prob_subnormal"
    wgt = got[sub, 11].view(np.float32)
    assert f["live"][sub].sum() > 20 and np.isfinite(wgt[f["live"][sub]]).all() and wgt[f["live"][sub]].max() > 1e30      # denormals are kept
    assert (f["e"][cls == "table_of_one"] == 0).all()
    big = np.flatnonzero(cls == "f32_slot")
    assert len(big) == 4
    for r in big:
        u0 = P.draws(orc, P.SEED, res["cases"][r]["j"], 1)[0]
        assert f["slot"][r] == int(u0 * np.float32(65521)) == int(float(u0) * 65521) + 1
