"""Scene facts (tiny-raytracer_amd/csrc/scene_facts.h; TRT_SCENE_FACTS) without a GPU: what the handle of each test scene claims, what is
refused, the #defines of the unit and its text with the facts switched off, and the unit itself compiled on the host by hiprtc for every
scene with facts on and off - it compiles, has no scratch and no spills, and needs at most the registers of the unit without facts.  The
native checker (tests/native/scene_facts_check.cpp) runs plain and as a stand-alone AddressSanitizer + UBSan program.  README_scene_facts.md
has the table of scenes."""
import json
import os
import subprocess
import sys

import pytest
import scene_facts_scenes as S
from test_flat_literal_gen import leaves_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tiny-raytracer_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")
sys.path.insert(0, os.path.join(ROOT, "tools"))


def gxx(out, source, *flags):
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags, "-I" + CSRC, source, "-o", str(out)], check=True, timeout=300)
    return str(out)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return gxx(tmp_path_factory.mktemp("scene_facts") / "check", os.path.join(NATIVE, "scene_facts_check.cpp"))


def test_native_cases_plain_and_under_sanitizers(checker, tmp_path):
    plain = subprocess.run([checker, "--self"], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and "self check ok" in plain.stdout, plain.stdout + plain.stderr
    exe = gxx(tmp_path / "san", os.path.join(NATIVE, "scene_facts_check.cpp"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    san = subprocess.run([exe, "--self"], capture_output=True, text=True, timeout=120)
    assert san.returncode == 0 and "self check ok" in san.stdout, san.stdout + san.stderr


def facts_of(trt, desc):
    return int(trt.lib.trt_scene_facts(trt.world_from_description(desc)[0].get_bvh()._h))


@pytest.mark.parametrize("scene", sorted(S.SCENES))
def test_each_scene_claims_its_facts_and_no_more(trt, scene):
    got = facts_of(trt, S.SCENES[scene](trt))
    assert got == S.FACTS[scene], (scene, hex(got), hex(S.FACTS[scene]))


def test_the_table_of_the_issue(trt):
    f = S.FACTS
    assert f["cornell"] == 0x91F                                                              # every fact
    assert not f["quads_and_a_sphere"] & (S.NO_SPHERE | S.AXIS_EXACT | S.NEAREST_FIRST | S.STRAIGHT)
    assert f["metal_room"] & S.METAL and f["three_quads"] & S.METAL and not f["metal_room"] & S.STRAIGHT
    assert not f["tilted_quad"] & (S.AXIS_EXACT | S.NEAREST_FIRST) and f["tilted_quad"] & S.NO_SPHERE
    assert f["closed_room"] & S.LAMBERTIAN and not f["closed_room"] & S.LIGHT
    assert facts_of(trt, S.thirty_three_quads(trt)) == 0                                      # more than 32 leaves: nothing claimed
    assert int(trt.lib.trt_scene_facts(None)) == 0


def test_switched_off_claims_nothing_and_constants_alone_leave_the_shade(tmp_path):
    code = ("import sys; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests'); trt = __import__('tiny-raytracer_amd');"
            "import scene_facts_scenes as S; print(*[int(trt.lib.trt_scene_facts(trt.world_from_description(S.SCENES[n](trt))[0].get_bvh()._h)) for n in sorted(S.SCENES)])")
    # ("all": not a number - like every value but 0 and 1 it means everything)
    for value, want in (("0", [0] * len(S.SCENES)), ("1", [S.FACTS[n] & ~S.STRAIGHT for n in sorted(S.SCENES)]), ("all", [S.FACTS[n] for n in sorted(S.SCENES)])):
        r = subprocess.run([sys.executable, "-c", code, ROOT], env=dict(os.environ, TRT_SCENE_FACTS=value), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert [int(v) for v in r.stdout.split()] == want, value


def defines_of(word):
    """scene_facts_defines, restated: the facts device code reads."""
    return (("#define TRT_FACT_NO_SPHERE 1\n" if word & S.NO_SPHERE else "") + ("#define TRT_FACT_KINDS 0x%x\n" % (word >> 8) if word >> 8 else "") +
            ("#define TRT_FACT_STRAIGHT_SHADE 1\n" if word & S.STRAIGHT else ""))


def test_without_facts_the_units_text_is_the_one_before_them(checker):
    off = subprocess.run([checker, "source", "0"], capture_output=True, text=True, check=True).stdout
    on = subprocess.run([checker, "source", hex(S.FACTS["cornell"])], capture_output=True, text=True, check=True).stdout
    tail = '#define TRT_FLAT_LITERAL_EXTRA 0\n#include "stream_pool.h"\n'
    assert off.startswith('#define TRT_FLAT_LITERAL_ASM \\\n"s_cmp_lg_u32 %[i], 0\\n" \\\n') and off.endswith('""\n' + tail) and "TRT_FACT" not in off
    assert on == off[:-len('#include "stream_pool.h"\n')] + defines_of(S.FACTS["cornell"]) + '#include "stream_pool.h"\n'


# ---- the unit, compiled on the host ----
@pytest.fixture(scope="module")
def report(trt, tmp_path_factory):
    """report(scene, facts word) -> resource usage and static counts of the unit hiprtc compiles for the scene's own leaf list."""
    import literal_isa_counts
    if not os.path.exists(os.path.join(CSRC, "rtc_headers.inc")):                          # a build product of the library's Makefile: made here if a
        subprocess.run(["make", "-C", CSRC, "--no-print-directory", "rtc_headers.inc"], check=True, timeout=300)      # prebuilt library came without it
    d = tmp_path_factory.mktemp("scene_facts_units")
    exe = d / "literal_report"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + CSRC, os.path.join(ROOT, "tools", "literal_report.cpp"), "-ldl", "-o", str(exe)], check=True, timeout=300)
    cache = {}

    def get(scene, word):
        if (scene, word) not in cache:
            box, prim, _ = trt.Scene(trt.world_from_description(S.SCENES[scene](trt))[0]).nodes()
            w = leaves_of(box[prim >= 0])
            f = d / (scene + ".bin")
            f.write_bytes(w.tobytes())
            prefix = str(d / ("%s_%x" % (scene, word)))
            r = subprocess.run([str(exe), str(f), str(len(w)), "8", "6", prefix, "6", hex(word)], capture_output=True, text=True, timeout=300)
            if r.returncode == 1 and "hiprtc not found" in r.stderr:
                pytest.skip("no hiprtc on this machine")
            assert r.returncode == 0, r.stderr[-3000:]
            out = json.loads(r.stdout)
            assert out["facts"]["word"] == word
            cache[scene, word] = dict(literal_isa_counts.report(prefix + ".co"), source=open(prefix + ".hip").read(), extra_operands=out["extra_operands"])
        return cache[scene, word]
    return get


UNIT_SCENES = ["cornell", "quads_and_a_sphere", "metal_room", "tilted_quad", "closed_room", "lights_only"]


@pytest.mark.parametrize("scene", UNIT_SCENES)
def test_the_unit_compiles_with_facts_on_and_off_without_scratch_in_no_more_registers(report, scene):
    off, on = report(scene, 0), report(scene, S.FACTS[scene])
    assert "TRT_FACT" not in off["source"] and "TRT_FACT" in on["source"]
    for r in (off, on):
        assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0, r
    print(scene, {k: (off[k], on[k]) for k in ("vgprs", "sgprs", "kernel_valu", "kernel_vgpr_copies", "loop_valu", "loop_vgpr_copies", "code_object_bytes")})
    assert on["vgprs"] <= off["vgprs"], (scene, on["vgprs"], off["vgprs"])
    # the unit's text, from the real flat_literal_source: without facts the text before them - box text, operand count, include - and with
    # facts that text with the defines in front of the include and nothing else changed
    include = '#include "stream_pool.h"\n'
    assert off["source"].startswith('#define TRT_FLAT_LITERAL_ASM \\\n"s_cmp_lg_u32 %[i], 0\\n" \\\n') and off["source"].endswith(include)
    head = off["source"][:-len(include)]
    assert head.endswith('""\n#define TRT_FLAT_LITERAL_EXTRA %d\n' % on["extra_operands"]) and head.count("#define") == 2
    assert on["source"] == head + defines_of(S.FACTS[scene]) + include
    # device code reads "no sphere" in the general kernel and the kinds in the straight-line shade: a scene that claims neither compiles to
    # the same instructions, one that claims "no sphere" to fewer (a fact that removed nothing would be a bug in the plumbing)
    if S.FACTS[scene] & S.NO_SPHERE:
        assert on["kernel_valu"] < off["kernel_valu"]
    else:
        assert on["kernel_valu"] == off["kernel_valu"] and "TRT_FACT_NO_SPHERE" not in on["source"]
