"""The interval cache of the per-scene box phase (tiny-raytracer_amd/csrc/flat_literal.h flat_literal_cached_asm), without a GPU.  The native
checker (tests/native/flat_cache_check.cpp, compiled with g++) writes the text for a leaf list and a setting (interval pairs 3 ... 8, plane
registers 0 ... 8), and the cached stream - what a ray entering at i == 0 runs - is executed here SYMBOLICALLY: per register, which plane
distance (axis, plane bits) or which interval (axis, lo bits, hi bits, made by med3 with t_min / t_best or by min / max) it holds.  Every
box must combine exactly its leaf's three intervals, the x one in med3 form; a register read after something else was written to it, or
before anything was, fails the run.  The numbers of computed intervals and plane distances must equal the generator's statistics and an
independent restatement of the eviction rule (farthest next use) below.  Behind the cached stream stands flat_literal_asm's text, whole:
that is where an entry at i > 0 goes.  The checker's self test runs plain and under AddressSanitizer + UBSan (stand-alone)."""
import os
import re
import subprocess

import numpy as np
import pytest
from test_flat_literal_gen import leaves_of, random_lists, reuse_numpy, sections

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tiny-raytracer_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")
NEVER = 1 << 30
BASE_OPERANDS = {"i", "top", "m", "t0", "t1", "xe", "xx", "ye", "yx", "ze", "zx", "st", "lk", "lim", "ox", "oy", "oz", "ix", "iy", "iz", "tb", "tmin"}
AXIS = "xyz"


def build(d, source, name, *flags):
    exe = d / name
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags, "-I" + CSRC, os.path.join(NATIVE, source), "-o", str(exe)],
                   check=True, timeout=300)
    return str(exe)


@pytest.fixture(scope="module")
def gen(tmp_path_factory):
    """gen(words, pairs, planes) -> (masks, stats dict, text) or None if refused; gen.plain(words) -> flat_literal_asm's text for the list."""
    d = tmp_path_factory.mktemp("flat_cache")
    exe, old = build(d, "flat_cache_check.cpp", "cache"), build(d, "flat_literal_check.cpp", "literal")
    files = {}

    def leaf_file(words):
        words = np.ascontiguousarray(words, np.uint32).reshape(-1, 8)
        key = words.tobytes()
        if key not in files:
            files[key] = d / ("leaves%d.bin" % len(files))
            files[key].write_bytes(key)
        return words, str(files[key])

    def run(words, pairs, planes, n=None, reuse=True):
        words, f = leaf_file(words)
        out = subprocess.run([exe, f, str(len(words) if n is None else n), "1" if reuse else "0", str(pairs), str(planes)], capture_output=True, text=True, timeout=60)
        if out.returncode == 2:
            assert out.stdout.strip() == "refused"
            return None
        assert out.returncode == 0, out.stderr
        masks, stats, text = out.stdout.split("\n", 2)
        v = [int(x) for x in stats.split()[1:]]
        return tuple(int(x) for x in masks.split()[1:]), dict(intervals=v[0], planes=v[1], evictions=v[2], far=v[3], extra=v[4], cached=bool(v[5])), text

    def plain(words, reuse=True):
        words, f = leaf_file(words)
        out = subprocess.run([old, f, str(len(words)), "1" if reuse else "0"], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr
        return out.stdout.split("\n", 1)[1]
    run.plain, run.dir = plain, d
    return run


# ---- the eviction rule, restated ----
def finite(b):
    return (int(b) & 0x7F800000) != 0x7F800000


def expected_counts(w, pairs, planes):
    """(intervals computed, plane distances computed, live evictions, distinct shareable intervals + unshareable ones) for a ray that
    enters at leaf 0.  Requests come in the order x, y, z of leaf 0, x of leaf 1, ...; a request hits if its (axis, lo, hi) is resident
    and both planes are finite; a miss takes the place of the resident requested farthest in the future (never: farthest of all), but
    not of one that the same leaf requests."""
    n = len(w)
    req = [(k, a, (a, int(w[k, a]), int(w[k, 3 + a])) if finite(w[k, a]) and finite(w[k, 3 + a]) else ("unshared", k, a)) for k in range(n) for a in range(3)]

    def nxt(seq, key, pos):
        return next((j for j in range(pos + 1, len(seq)) if seq[j] == key), NEVER)
    keys = [r[2] for r in req]
    resident, computed, evicted, plane_seq = [], 0, 0, []
    for pos, (k, a, key) in enumerate(req):
        if key in resident:
            continue
        computed += 1
        plane_seq += [(a, int(w[k, a])) if finite(w[k, a]) else ("unshared", pos, 0), (a, int(w[k, 3 + a])) if finite(w[k, 3 + a]) else ("unshared", pos, 1)]
        if len(resident) < pairs:
            resident.append(key)
            continue
        mine = set(keys[3 * k:3 * k + 3])
        victim = max((r for r in resident if r not in mine), key=lambda r: nxt(keys, r, pos))
        evicted += nxt(keys, victim, pos) != NEVER
        resident[resident.index(victim)] = key
    held, distances = [], 0
    for pos, key in enumerate(plane_seq):
        if planes and key in held:
            continue
        distances += 1
        mine = nxt(plane_seq, key, pos)
        if not planes or mine == NEVER:
            continue
        if len(held) < planes:
            held.append(key)
            continue
        partner = plane_seq[pos - 1] if pos & 1 else None                # the lo plane of the same interval is read together with this one
        cands = [h for h in held if h != partner]
        if not cands:
            continue
        victim = max(cands, key=lambda h: nxt(plane_seq, h, pos))
        if nxt(plane_seq, victim, pos) > mine:
            held[held.index(victim)] = key
    return computed, distances, evicted, len(set(keys))


# ---- the symbolic run ----
def run_cached_stream(w, text, pairs, planes, extra):
    """Executes the cached stream's leaves 0 ... n-1 on symbols.  Returns (intervals computed, plane distances computed)."""
    n = len(w)
    head, _, rest = text.partition("1000:\n")
    sec = sections(head)
    assert sec[None] == ["s_cmp_lg_u32 %[i], 0", "s_cbranch_scc1 1000f"]
    assert sorted(k for k in sec if k is not None) == [1200 + k for k in range(n)]
    names = set(re.findall(r"%\[(\w+)\]", head))
    declared = BASE_OPERANDS | {"c%d" % j for j in range(extra)}
    assert names <= declared, names - declared
    pair_regs = [("xe", "xx"), ("ye", "yx"), ("ze", "zx")] + [("c%d" % (2 * j), "c%d" % (2 * j + 1)) for j in range(pairs - 3)]
    los, his = {p[0] for p in pair_regs}, {p[1] for p in pair_regs}
    plane_regs = {"t0", "t1"} | {"c%d" % (2 * (pairs - 3) + j) for j in range(planes)}
    assert not (los | his) & plane_regs
    reg, intervals, distances = {}, 0, 0
    R = r"%\[(\w+)\]"
    H = r"(0x[0-9a-f]{8})"
    for k in range(n):
        lines = sec[1200 + k]
        i = 0
        while not lines[i].startswith("v_max3_f32"):
            line = lines[i]
            i += 1
            m = re.fullmatch(rf"v_sub_f32_e32 {R}, {H}, %\[o([xyz])\]", line)
            if m:
                assert m.group(1) in plane_regs
                reg[m.group(1)] = ("sub", AXIS.index(m.group(3)), int(m.group(2), 16))
                distances += 1
                continue
            m = re.fullmatch(rf"v_mul_f32_e32 {R}, %\[i([xyz])\], {R}", line)
            if m:
                assert m.group(1) == m.group(3) and reg[m.group(1)][0] == "sub" and reg[m.group(1)][1] == AXIS.index(m.group(2)), line
                reg[m.group(1)] = ("plane",) + reg[m.group(1)][1:]
                continue
            m = re.fullmatch(rf"v_med3_f32 {R}, {R}, {R}, %\[(tmin|tb)\]", line) or re.fullmatch(rf"v_(min|max)_f32_e32 {R}, {R}, {R}", line)
            assert m, line
            if line.startswith("v_med3"):
                dst, a, b, end, form = m.group(1), m.group(2), m.group(3), "lo" if m.group(4) == "tmin" else "hi", "med3"
            else:
                dst, a, b, end, form = m.group(2), m.group(3), m.group(4), "lo" if m.group(1) == "min" else "hi", "minmax"
            pa, pb = reg[a], reg[b]
            assert pa[0] == pb[0] == "plane" and pa[1] == pb[1] and (pa[1] == 0) == (form == "med3"), line
            assert dst in (los if end == "lo" else his), line
            reg[dst] = (end, pa[1], pa[2], pb[2], form)
            intervals += end == "lo"
        m3 = re.fullmatch(rf"v_max3_f32 %\[st\], {R}, {R}, {R}", lines[i])
        n3 = re.fullmatch(rf"v_min3_f32 %\[t0\], {R}, {R}, {R}", lines[i + 1])
        assert m3 and n3, lines[i:i + 2]
        for a in range(3):
            form = "med3" if a == 0 else "minmax"
            lo, hi = m3.group(1 + a), n3.group(1 + a)
            assert (lo, hi) in pair_regs, (k, a, lo, hi)
            assert reg[lo] == ("lo", a, int(w[k, a]), int(w[k, 3 + a]), form), (k, a, reg[lo])
            assert reg[hi] == ("hi", a, int(w[k, a]), int(w[k, 3 + a]), form), (k, a, reg[hi])
        reg["st"], reg["t0"] = ("start",), ("end",)
        assert lines[i + 2:i + 4] == ["v_cmp_nle_f32_e32 vcc, %[t0], %[st]", "s_and_saveexec_b64 %[m], vcc"]
        assert lines[i + 4] == "v_mov_b32_e32 %%[lk], 0x%08x" % int(w[k, 7]), "links and push order are the list's"
        assert lines[i + 5:i + 8] == ["ds_write2_b32 %[top], %[lk], %[st] offset1:1", "v_add_u32_e32 %[top], 0x200, %[top]", "s_mov_b64 exec, %[m]"]
        tail = lines[i + 8:]
        if k == n - 1:
            assert tail == ["s_mov_b32 %%[i], 0x%08x" % n, "s_branch 990f"]
        elif k & 1:                                                          # the stack-full ballot; its exit is flat_literal_asm's own
            assert tail == ["v_cmp_gt_u32_e32 vcc, %[top], %[lim]", "s_cbranch_vccnz %df" % (400 + k + 1)]
            assert sections(rest)[400 + k + 1] == ["s_mov_b32 %%[i], 0x%08x" % (k + 1), "s_branch 990f"]
        else:
            assert tail == []
    assert not re.search(r"\d\.\d|e[+-]\d", head), "a decimal constant"
    literals = {int(v, 16) for v in re.findall(r"0x[0-9a-f]+", head)} - {0x200, n}
    assert literals <= {int(v) for v in w[:, [0, 1, 2, 3, 4, 5, 7]].ravel()} and all(len(v) == 10 for v in re.findall(r"0x[0-9a-f]+", head) if v != "0x200")
    return intervals, distances


def check(gen, w, pairs, planes, reuse=True):
    masks, st, text = gen(w, pairs, planes, reuse=reuse)
    plain = gen.plain(w, reuse=reuse)
    assert masks == (reuse_numpy(w) if reuse else (0, 0, 0))
    plain_intervals = 3 * len(w) - sum(bin(v).count("1") for v in masks)
    want = expected_counts(w, pairs, planes)
    if (pairs, planes) == (3, 0) or (want[0] >= plain_intervals and want[1] >= 2 * plain_intervals):
        assert text == plain and not st["cached"] and st["extra"] == 0        # no scene grows code for nothing
        assert (st["intervals"], st["planes"]) == (plain_intervals, 2 * plain_intervals)
        return st
    assert st["cached"] and st["extra"] == 2 * (pairs - 3) + planes
    assert text.partition("1000:\n")[2] == plain, "an entry at i > 0 reaches flat_literal_asm's text"
    got = run_cached_stream(w, text, pairs, planes, st["extra"])
    assert got == (st["intervals"], st["planes"]) == want[:2], (got, st, want)
    assert st["evictions"] == want[2]
    if all(finite(v) for v in w[:, :6].ravel()):
        assert st["intervals"] == want[3] + st["evictions"]                  # every interval once, and once more per live eviction
    return st


SETTINGS = [(p, q) for p in range(3, 9) for q in range(0, 9)]


@pytest.mark.parametrize("n", [1, 2, 3, 32])
def test_lists_of_1_2_3_and_32_leaves_at_every_setting(gen, n):
    for seed in range(2):
        w = leaves_of(random_lists(n, 10 * n + seed))
        for pairs, planes in SETTINGS:
            check(gen, w, pairs, planes)
        check(gen, w, 8, 6, reuse=False)                                     # zero masks: the cached stream is the same, the text behind it is in full
    assert gen(w, 4, 2) == gen(w, 4, 2)                                      # deterministic


@pytest.fixture(scope="module")
def cornell_leaves(trt):
    s = trt.Scene(trt.world_from_description(trt.scenes.cornell(64, 64))[0])
    box, prim, _ = s.nodes()
    w = leaves_of(box[prim >= 0])
    assert len(w) == 18
    return w


def test_cornell_counts(gen, cornell_leaves):
    """The product's own 18 leaves: 54 interval uses, 26 distinct; 39 / 32 / 29 / 28 / 26 computed with 3 / 4 / 5 / 6 / 8 pairs."""
    w = cornell_leaves
    distinct = {(a, int(w[k, a]), int(w[k, 3 + a])) for k in range(18) for a in range(3)}
    assert len(distinct) == 26 and [sum(1 for d in distinct if d[0] == a) for a in range(3)] == [10, 7, 9]
    assert len({(a, int(w[k, a + 3 * h])) for k in range(18) for a in range(3) for h in range(2)}) == 34
    got = {pairs: check(gen, w, pairs, 0) for pairs in range(3, 9)}
    assert [got[p]["intervals"] for p in (3, 4, 5, 6, 7, 8)] == [39, 32, 29, 28, CORNELL_7_PAIRS, 26]
    assert all(got[p]["planes"] == 2 * got[p]["intervals"] for p in got)
    assert got[8]["evictions"] == 0 and got[4]["evictions"] == 32 - 26
    for planes in range(1, 9):
        st = check(gen, w, 8, planes)
        assert st["intervals"] == 26 and st["planes"] == CORNELL_8_PAIRS_PLANES[planes]


# found on the product's list: 34 distinct planes, reached with seven plane registers; 35 with six
CORNELL_7_PAIRS = 27
CORNELL_8_PAIRS_PLANES = {1: 48, 2: 44, 3: 41, 4: 38, 5: 36, 6: 35, 7: 34, 8: 34}


def test_seeded_random_lists(gen):
    for seed in range(12):
        n = 4 + 5 * (seed % 6)
        w = leaves_of(random_lists(n, 1000 + seed))
        for pairs, planes in ((4, 0), (5, 3), (6, 0), (8, 6), (8, 8), (3, 4)):
            check(gen, w, pairs, planes)


def test_more_live_intervals_than_pairs_evicts(gen):
    """Six boxes A ... F, different on every axis, walked A B C D E F A B C D E F: 18 distinct intervals, all live until the second
    round, and at most 8 pairs: intervals named again are dropped at every setting, fewer with every further pair.  (check() holds the
    counts against the restated rule, and computed == 18 + evictions.)"""
    base = np.arange(6, dtype=np.float32)[:, None] * 3.0 + np.array([0.0, 0.25, 0.5], np.float32)
    boxes = np.concatenate([base, base + 2.0], axis=1)
    w = leaves_of(boxes[list(range(6)) * 2])
    computed = [36]
    for pairs in range(4, 9):
        st = check(gen, w, pairs, 0)
        assert st["cached"] and st["evictions"] > 0 and st["far"] > 0 and st["intervals"] < computed[-1], (pairs, st)
        computed.append(st["intervals"])
    assert not check(gen, w, 3, 0)["cached"]


def test_signed_zero_inf_and_nan_planes(gen):
    nan, inf = float("nan"), float("inf")
    a = [0.0, 0.0, -1.0, 1.0, 1.0, -0.0]
    b = [-0.0, 0.0, -1.0, 1.0, 1.0, 0.0]                                      # x lo and z hi change sign only
    c = [-0.0, 0.0, -1.0, inf, 1.0, 0.0]
    e = [-0.0, nan, -1.0, inf, 1.0, 0.0]
    w = leaves_of([a, b, a, c, c, e, e, b, a])
    w[5, 1] = w[6, 1] = 0x7FC12345                                           # a NaN with a payload
    for pairs, planes in ((4, 0), (8, 0), (8, 6), (5, 8)):
        st = check(gen, w, pairs, planes)
        assert st["cached"]
    masks, st, text = gen(w, 8, 0)
    head = text.partition("1000:\n")[0]
    # x: a's (+0, 1) and b's (-0, 1) once each although they alternate; c's (-0, inf) at each of its four leaves
    assert head.count("v_med3_f32") == 2 * (2 + 4)
    # y: (0, 1) once, the NaN interval at both of its leaves
    assert head.count("0x7fc12345, %[oy]") == 2
    # z: (-1, -0) and (-1, +0) once each
    assert head.count("v_sub_f32_e32 %[t1], 0x80000000, %[oz]") == 1 and head.count("v_sub_f32_e32 %[t1], 0x00000000, %[oz]") == 1


def test_refusals(gen):
    w = leaves_of(random_lists(33, 5))
    assert gen(w, 4, 0) is None and gen(w, 4, 0, n=0) is None
    assert gen(w[:32], 2, 0) is None and gen(w[:32], 9, 0) is None and gen(w[:32], 4, 9) is None
    assert gen(w[:32], 8, 8) is not None


def test_nothing_to_cache_gives_the_plain_text(gen):
    boxes = np.arange(5 * 6, dtype=np.float32).reshape(5, 6)
    w = leaves_of(boxes)
    for pairs, planes in ((3, 0), (4, 0), (8, 8)):
        masks, st, text = gen(w, pairs, planes)
        assert text == gen.plain(w) and not st["cached"] and st["extra"] == 0


def test_native_self_check_plain_and_under_sanitizers(gen):
    plain = subprocess.run([build(gen.dir, "flat_cache_check.cpp", "self_plain"), "--self"], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and "self check ok" in plain.stdout, plain.stdout + plain.stderr
    exe = build(gen.dir, "flat_cache_check.cpp", "self_san", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    san = subprocess.run([exe, "--self"], capture_output=True, text=True, timeout=300)
    assert san.returncode == 0 and "self check ok" in san.stdout, san.stdout + san.stderr
