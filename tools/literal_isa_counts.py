#!/usr/bin/env python3
"""Static instruction counts of a code object that tools/literal_report.cpp wrote (no device needed):

  python tools/literal_isa_counts.py build/lit_on.co [build/lit_off.co ...]

Per file, one JSON line: VALU instructions (v_*) and VGPR-to-VGPR v_mov_b32 of the whole kernel and of its round loop, SALU instructions
of the loop, and the kernel descriptor's VGPRs, SGPRs, spills and scratch (llvm-readelf --notes).  The round loop is the span of the
backward branch that covers the most instructions: stream_pool_kernel's `for (;;)` over rounds encloses every other loop.  The counts are
static - every instruction once, whatever branch it sits behind - so they bound what a round issues, they are not what it issues.
The loop's span follows the compiler's block layout: cold blocks of the loop may be placed behind the back edge in one build and inside the
span in another (loop_instructions says how much was caught), so the loop columns of two builds compare only where their spans agree; the
kernel columns always compare."""
import json
import os
import re
import subprocess
import sys

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")


def disassemble(path):
    out = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", path], capture_output=True, text=True, check=True).stdout
    ins = []                                                       # (address, mnemonic, operands)
    for line in out.splitlines():
        m = re.match(r"\s+(\w+)\s+(.*?)\s*//\s*([0-9A-Fa-f]+):", line)
        if m:
            ins.append((int(m.group(3), 16), m.group(1), m.group(2)))
    return ins


def counts(ins):
    valu = sum(1 for _, op, _ in ins if op.startswith("v_"))
    copies = sum(1 for _, op, args in ins if op.startswith("v_mov_b32") and re.fullmatch(r"v\d+, v\d+", args.strip()))
    salu = sum(1 for _, op, _ in ins if op.startswith("s_") and not op.startswith(("s_waitcnt", "s_nop", "s_load", "s_buffer_load")))
    return valu, copies, salu


def round_loop(ins):
    addr = {a: k for k, (a, _, _) in enumerate(ins)}
    best = (0, 0)
    for k, (a, op, args) in enumerate(ins):
        if not (op.startswith("s_cbranch") or op == "s_branch"):
            continue
        m = re.match(r"(-?\d+)", args.strip())
        if not m:
            continue
        simm = int(m.group(1))
        if simm >= 32768:
            simm -= 65536
        target = a + 4 + 4 * simm
        if target in addr and addr[target] <= k and k - addr[target] > best[1] - best[0]:
            best = (addr[target], k + 1)
    return ins[best[0]:best[1]]


def notes(path):
    out = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", path], capture_output=True, text=True, check=True).stdout
    get = lambda key: next((int(m.group(1)) for m in [re.search(r"\." + key + r":\s+(\d+)", out)] if m), None)  # noqa: E731
    return dict(vgprs=get("vgpr_count"), sgprs=get("sgpr_count"), vgpr_spills=get("vgpr_spill_count"), sgpr_spills=get("sgpr_spill_count"),
                scratch_bytes=get("private_segment_fixed_size"), lds_static_bytes=get("group_segment_fixed_size"))


def report(path):
    ins = disassemble(path)
    loop = round_loop(ins)
    kv, kc, _ = counts(ins)
    lv, lc, ls = counts(loop)
    r = dict(file=os.path.basename(path), instructions=len(ins), kernel_valu=kv, kernel_vgpr_copies=kc, loop_instructions=len(loop), loop_valu=lv,
             loop_vgpr_copies=lc, loop_salu=ls, code_object_bytes=os.path.getsize(path))
    r.update(notes(path))
    return r


if __name__ == "__main__":
    for p in sys.argv[1:]:
        print(json.dumps(report(p)))
