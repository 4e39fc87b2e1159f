"""trt_emitter_pick_build (tinyrt.h) without a GPU: the alias table over an emitter table.

Tables of E = 1, 2, 3, 61, 4096 and 2^20 records (a short period repeated), with weights that span 1 : 10^6 with zeros among them, with
all weights equal, and with the emitters' own powers.  For every table: the probability the alias structure implies equals w_k / sum(w),
prob has the bits of the header's rule, a zero-weight emitter is never chosen, two builds give the same bytes, and a second statement of
Vose's construction (direct_pick_cases.build: Python lists as stacks, written apart from the library's code) gives the same bytes.

The bound on the implied probability, 1e-6 relative.  The construction runs in double, so before q is rounded the implied probability
of emitter k is w_k / sum(w) to a few double roundings per step it takes part in (2^-53 each: nothing beside what follows).  Each q is
then rounded to f32, a relative error of at most 2^-24.  Emitter k's implied probability is
    P_k = (q_k + sum over the other slots j with alias_j = k of (1 - q_j)) / E,
so the roundings move it by at most 2^-24 * (q_k + sum_j q_j) / E, and relative to P_k by at most
    2^-24 * A_k,   A_k = (q_k + sum_j q_j) / (q_k + sum_j (1 - q_j)).
A slot that keeps itself only (nothing aliases to it) has A_k = 1; a slot of weight 0 that gives everything away has q_j = 0 and adds
nothing to the numerator.  A_k is large only where many slots with q_j close to 1 give slivers to one emitter; the test computes A_k
for every table it builds and asserts max A_k <= 16, the margin: 16 * 2^-24 = 9.5e-7 <= 1e-6."""
import numpy as np
import pytest

import direct_cases as D
import direct_pick_cases as P

REL = 1e-6
MARGIN = 16.0


def _table(orc, E):
    """E records, quads and spheres in turn, colours and sizes from a short period: powers differ, none is zero."""
    period = [D.quad_record(orc, (0.0, 10.0, 0.0), (1.0 + i, 0.0, 0.0), (0.0, 0.0, 2.0), (1.0 + i, 2.0, 0.5 * i)) if i % 2 == 0 else
              D.sphere_record((i, 5.0, 0.0), 0.25 * (1 + i), (0.5 * i, 0.25, 3.0)) for i in range(7)]
    period = np.concatenate(period)
    return np.ascontiguousarray(period[np.arange(E) % len(period)])


def _weights(E, which):
    if which == "equal":
        return np.full(E, 2.5, np.float32)
    if which == "power":
        return None
    # 1 : 10^6 over a period of 13, zeros among them (every fifth; never all)
    w = np.float32(10.0) ** (np.arange(E) % 13 * np.float32(0.5))
    w[np.arange(E) % 5 == 3] = 0.0
    return w.astype(np.float32)


SIZES = (1, 2, 3, 61, 4096, 2 ** 20)
CASES = [(E, which) for E in SIZES for which in ("spread", "equal", "power")]


@pytest.mark.parametrize("E,which", CASES, ids=["%d-%s" % c for c in CASES])
def test_the_table(trt, orc, E, which):
    table = _table(orc, E)
    weights = _weights(E, which)
    pick, total = trt.lights.pick_table(table, weights)
    again, total2 = trt.lights.pick_table(table.copy(), None if weights is None else weights.copy())
    assert pick.tobytes() == again.tobytes() and total == total2            # deterministic
    # the header's rules, bit for bit
    w = P.powers(table) if weights is None else weights
    assert total == np.float32(sum(float(x) for x in w))                   # double, in table order, rounded once
    with np.errstate(all="ignore"):
        assert pick["prob"].tobytes() == (w / total).astype(np.float32).tobytes()
    assert (pick["reserved"] == 0).all() and (pick["alias"] < E).all()
    assert (pick["q"] >= 0).all() and (pick["q"] <= 1).all()
    # the structure implies w_k / sum(w)
    implied = P.implied(pick)
    exact = w.astype(np.float64) / w.astype(np.float64).sum()
    live = w > 0
    assert live.any()
    # the premise of the bound (the docstring's A_k) holds for this table
    others = pick["alias"] != np.arange(E)
    qd = pick["q"].astype(np.float64)
    num, den = qd.copy(), qd.copy()
    np.add.at(num, pick["alias"][others], qd[others])
    np.add.at(den, pick["alias"][others], 1.0 - qd[others])
    assert (num[live] / den[live]).max() <= MARGIN and MARGIN * 2.0 ** -24 <= REL
    rel = np.abs(implied[live] - exact[live]) / exact[live]
    print(E, which, "largest relative error of the implied probability", rel.max())
    assert rel.max() <= REL, (E, which, rel.max())
    # an emitter of weight 0: q = 0, nobody's alias, implied probability exactly 0
    dead = ~live
    assert (implied[dead] == 0.0).all() and (pick["q"][dead] == 0.0).all() and (pick["prob"][dead] == 0.0).all()
    assert not np.isin(pick["alias"][pick["q"] < 1], np.nonzero(dead)[0]).any()
    if which == "spread" and E >= 5:
        assert dead.any()
    if which == "equal":
        assert (pick["q"] == 1.0).all() and (pick["alias"] == np.arange(E)).all()
    # a second, independent statement of the construction
    want, wtotal = P.build(table, weights)
    assert wtotal == total
    assert pick.tobytes() == want.tobytes(), (E, which, int((pick.view(np.uint8).reshape(E, 16) != want.view(np.uint8).reshape(E, 16)).any(axis=1).sum()))


def test_powers_are_the_headers_rule(trt, orc):
    """weights == NULL: ((0.2126 r + 0.7152 g) + 0.0722 b) * area in f32, which another parenthesisation does not give for every colour."""
    table = _table(orc, 61)
    pick, total = trt.lights.pick_table(table)
    w = P.powers(table)
    assert pick.tobytes() == trt.lights.pick_table(table, w)[0].tobytes()
    other = np.array([P.luminance(r["color"], "luminance_parens") * r["area"] for r in table], np.float32)
    assert (other != w).any()


def test_an_underflowing_probability_is_never_chosen(trt, orc):
    """A weight so small beside the others that w / total is 0 in f32: the emitter is built as if its weight were 0, so the table passes
    trt_direct_pick's own check (no emitter that can be chosen has prob 0)."""
    table = _table(orc, 3)
    w = np.array([1e-30, 3e38 / 4, 1.0], np.float32)
    pick, total = trt.lights.pick_table(table, w)
    assert pick["prob"][0] == 0.0 and pick["q"][0] == 0.0 and pick["alias"][0] == 1
    assert P.implied(pick)[0] == 0.0
    assert pick.tobytes() == P.build(table, w)[0].tobytes()
