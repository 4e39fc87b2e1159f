"""The generator of the per-scene box phase (tiny-raytracer_amd/csrc/flat_literal.h), without a GPU: the native checker
(tests/native/flat_literal_check.cpp, compiled with g++) writes the asm text for leaf lists of 1, 2, 3, 18 (Cornell's own, from the
product) and 32 leaves and for lists with signed-zero, inf and NaN planes, and the text is taken apart here: every plane is there as its
exact bit pattern, the axes left out are exactly those of flat_reuse_masks, every leaf the loop can be entered at (the even ones: the loop
is left only behind the second leaf of a pair) has an entry that computes all three axes, the links are the list's.  The checker's own
self test runs plain and under AddressSanitizer + UBSan (a stand-alone program: nothing is preloaded)."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tiny-raytracer_amd", "csrc")
CHECK = os.path.join(ROOT, "tests", "native", "flat_literal_check.cpp")
AXIS_OF = {"%[ox]": 0, "%[oy]": 1, "%[oz]": 2}


def build(d, name, *flags):
    exe = d / name
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags, "-I" + CSRC, CHECK, "-o", str(exe)], check=True, timeout=300)
    return str(exe)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("flat_literal")
    exe = build(d, "check")
    count = [0]

    def run(words, n=None, reuse=True):
        """words: (k, 8) uint32 leaves in walk order.  Returns (masks, asm text), or None if the list is refused."""
        words = np.ascontiguousarray(words, np.uint32).reshape(-1, 8)
        count[0] += 1
        f = d / ("leaves%d.bin" % count[0])
        f.write_bytes(words.tobytes())
        out = subprocess.run([exe, str(f), str(len(words) if n is None else n), "1" if reuse else "0"], capture_output=True, text=True, timeout=60)
        if out.returncode == 2:
            assert out.stdout.strip() == "refused"
            return None
        assert out.returncode == 0, out.stderr
        head, text = out.stdout.split("\n", 1)
        return tuple(int(v) for v in head.split()[1:]), text
    run.dir = d
    return run


def leaves_of(boxes, links=None):
    box = np.asarray(boxes, np.float32).reshape(-1, 6)
    w = np.zeros((len(box), 8), np.uint32)
    w[:, :6] = box.view(np.uint32)
    w[:, 6] = np.arange(1, len(box) + 1)
    w[:, 7] = (np.arange(len(box)) * 5 + 2) | 0x40000000 if links is None else links
    return w


def reuse_numpy(w):
    """flat_reuse_masks restated (tests/test_flat_reuse_masks.py): bit i of axis k iff leaf i's two planes are leaf i-1's bits, both finite."""
    fin = (w & 0x7F800000) != 0x7F800000
    out = []
    for k in range(3):
        m = 0
        for i in range(1, len(w)):
            if w[i, k] == w[i - 1, k] and w[i, k + 3] == w[i - 1, k + 3] and fin[i, k] and fin[i, k + 3]:
                m |= 1 << i
        out.append(m)
    return tuple(out)


def sections(text):
    """label number -> the instructions behind it up to the next label; None -> those before the first label."""
    out, cur = {None: []}, None
    for line in text.splitlines():
        m = re.fullmatch(r"(\d+):", line)
        if m:
            cur = int(m.group(1))
            assert cur not in out, "label defined twice"
            out[cur] = []
        else:
            out[cur].append(line)
    return out


def box_of(lines):
    """One box's instructions -> ({axis: (lo bits, hi bits)}, link bits, the lines behind the push)."""
    axes, i = {}, 0
    while lines[i].startswith("v_sub_f32_e32"):
        a = re.fullmatch(r"v_sub_f32_e32 %\[t0\], (0x[0-9a-f]{8}), (%\[o[xyz]\])", lines[i])
        b = re.fullmatch(r"v_sub_f32_e32 %\[t1\], (0x[0-9a-f]{8}), (%\[o[xyz]\])", lines[i + 1])
        assert a and b and a.group(2) == b.group(2), lines[i:i + 2]
        k = AXIS_OF[a.group(2)]
        inv = "%[i" + "xyz"[k] + "]"
        assert lines[i + 2:i + 4] == [f"v_mul_f32_e32 %[t0], {inv}, %[t0]", f"v_mul_f32_e32 %[t1], {inv}, %[t1]"]
        if k == 0:
            assert lines[i + 4:i + 6] == ["v_med3_f32 %[xe], %[t0], %[t1], %[tmin]", "v_med3_f32 %[xx], %[t0], %[t1], %[tb]"]
        else:
            c = "xyz"[k]
            assert lines[i + 4:i + 6] == [f"v_min_f32_e32 %[{c}e], %[t0], %[t1]", f"v_max_f32_e32 %[{c}x], %[t0], %[t1]"]
        assert k not in axes
        axes[k] = (int(a.group(1), 16), int(b.group(1), 16))
        i += 6
    assert lines[i:i + 4] == ["v_max3_f32 %[st], %[xe], %[ye], %[ze]", "v_min3_f32 %[t0], %[xx], %[yx], %[zx]", "v_cmp_nle_f32_e32 vcc, %[t0], %[st]",
                              "s_and_saveexec_b64 %[m], vcc"]
    link = re.fullmatch(r"v_mov_b32_e32 %\[lk\], (0x[0-9a-f]{8})", lines[i + 4])
    assert link and lines[i + 5:i + 8] == ["ds_write2_b32 %[top], %[lk], %[st] offset1:1", "v_add_u32_e32 %[top], 0x200, %[top]", "s_mov_b64 exec, %[m]"]
    return axes, int(link.group(1), 16), lines[i + 8:]


def check_text(w, masks, text):
    n = len(w)
    sec = sections(text)
    assert sec[None] == ["s_cmp_lg_u32 %[i], 0", "s_cbranch_scc1 900f"]
    reused = lambda k: 0 if k == 0 else sum(((masks[a] >> k) & 1) << a for a in range(3))
    for k in range(n):                                                       # the main stream, in walk order
        axes, link, tail = box_of(sec[200 + k])
        assert set(axes) == {a for a in range(3) if not (reused(k) >> a) & 1}, (k, axes, masks)
        for a, (lo, hi) in axes.items():
            assert (lo, hi) == (int(w[k, a]), int(w[k, 3 + a])), (k, a)
        assert link == int(w[k, 7])
        if k == n - 1:
            assert tail == ["s_mov_b32 %%[i], 0x%08x" % n, "s_branch 990f"]
        elif k & 1:                                                          # behind a pair: the stack-full ballot, exit with i = k + 1
            assert tail == ["v_cmp_gt_u32_e32 vcc, %[top], %[lim]", "s_cbranch_vccnz %df" % (400 + k + 1)]
            assert sec[400 + k + 1] == ["s_mov_b32 %%[i], 0x%08x" % (k + 1), "s_branch 990f"]
        else:
            assert tail == []
    assert 200 + n not in sec
    rows = [r for r in sec[900] if r.startswith("s_branch")]                 # the entry table: one row per even leaf
    assert sec[900][:6] == ["s_lshl_b32 s38, %[i], 1", "s_add_u32 s38, s38, 12", "s_getpc_b64 s[36:37]", "s_add_u32 s36, s36, s38",
                            "s_addc_u32 s37, s37, 0", "s_setpc_b64 s[36:37]"] and sec[900][6:] == rows
    assert len(rows) == (n + 1) // 2 and sec[990] == []
    for j, row in enumerate(rows):
        k = 2 * j
        if reused(k) == 0:                                                   # the main-stream box computes every axis: it is the entry
            assert row == "s_branch %db" % (200 + k) and 100 + k not in sec
            continue
        assert row == "s_branch %db" % (100 + k)
        axes, link, tail = box_of(sec[100 + k])                              # the fresh copy: all three axes, then on into the main stream
        assert axes == {a: (int(w[k, a]), int(w[k, 3 + a])) for a in range(3)} and link == int(w[k, 7])
        assert tail == (["s_branch %db" % (200 + k + 1)] if k + 1 < n else ["s_mov_b32 %%[i], 0x%08x" % n, "s_branch 990f"])
    assert not any(100 + k in sec for k in range(1, 33, 2)), "odd leaves are never entered at"
    assert not re.search(r"\d\.\d|e[+-]\d", text), "a decimal constant"


def random_lists(n, seed):
    """n leaves over a few plane values per axis, so that neighbours share planes on some axes and not on others."""
    rng = np.random.default_rng(seed)
    lo = rng.integers(0, 3, (n, 3)).astype(np.float32) * 1.25 - 2.0
    return np.concatenate([lo, lo + rng.integers(1, 3, (n, 3)).astype(np.float32)], axis=1)


@pytest.mark.parametrize("n", [1, 2, 3, 32])
def test_lists_of_1_2_3_and_32_leaves(checker, n):
    for seed in range(3):
        w = leaves_of(random_lists(n, 10 * n + seed))
        masks, text = checker(w)
        assert masks == reuse_numpy(w)
        check_text(w, masks, text)
        assert checker(w) == (masks, text)                                   # deterministic
        off, plain = checker(w, reuse=False)                                 # the schedule switched off: every box in full, no fresh copies
        assert off == (0, 0, 0)
        check_text(w, off, plain)


def test_identical_leaves_reuse_everything_but_the_entries(checker):
    w = leaves_of([[1.0, 2.0, 3.0, 4.0, 5.0, 6.0]] * 7)
    masks, text = checker(w)
    assert masks == (0b1111110,) * 3
    check_text(w, masks, text)
    assert text.count("v_sub_f32_e32") == 6 * (1 + 3)                        # leaf 0 and the fresh copies of leaves 2, 4, 6


def test_cornell_leaf_list(trt, checker):
    """Cornell's 18 leaves as the product packs them: 15 of the 54 intervals reused, as tests/test_flat_reuse_masks.py counts."""
    s = trt.Scene(trt.world_from_description(trt.scenes.cornell(64, 64))[0])
    box, prim, _ = s.nodes()
    w = leaves_of(box[prim >= 0])
    assert len(w) == 18
    masks, text = checker(w)
    assert masks == reuse_numpy(w) and sum(bin(v).count("1") for v in masks) == 15
    check_text(w, masks, text)


def test_empty_and_overlong_lists_are_refused(checker):
    w = leaves_of(random_lists(33, 5))
    assert checker(w) is None
    assert checker(w, n=0) is None
    assert checker(w[:32]) is not None


def test_signed_zero_inf_and_nan_planes_keep_their_bits(checker):
    nan, inf = float("nan"), float("inf")
    a = [0.0, 0.0, -1.0, 1.0, 1.0, -0.0]
    b = [-0.0, 0.0, -1.0, 1.0, 1.0, 0.0]                                      # x lo and z hi change sign only: no reuse on x or z
    c = [-0.0, 0.0, -1.0, inf, 1.0, 0.0]
    d = [-0.0, 0.0, -1.0, inf, 1.0, 0.0]                                      # the same inf plane: still computed
    e = [-0.0, nan, -1.0, inf, 1.0, 0.0]
    w = leaves_of([a, b, c, d, e, e])
    w[5, 1] = w[4, 1] = 0x7FC12345                                           # a NaN with a payload
    masks, text = checker(w)
    assert masks == reuse_numpy(w)
    assert masks[0] == 0 and (masks[2] >> 1) & 1 == 0 and (masks[1] >> 5) & 1 == 0
    check_text(w, masks, text)
    for bits in ("0x80000000", "0x00000000", "0x7f800000", "0x7fc12345"):
        assert f"v_sub_f32_e32 %[t0], {bits}," in text or f"v_sub_f32_e32 %[t1], {bits}," in text


def test_native_self_check_plain_and_under_sanitizers(checker):
    plain = subprocess.run([build(checker.dir, "self_plain"), "--self"], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and "self check ok" in plain.stdout, plain.stdout + plain.stderr
    exe = build(checker.dir, "self_san", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    san = subprocess.run([exe, "--self"], capture_output=True, text=True, timeout=120)
    assert san.returncode == 0 and "self check ok" in san.stdout, san.stdout + san.stderr
