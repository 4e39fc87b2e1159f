#!/usr/bin/env python3
"""Are the kernels of one gfx950 assembly file (make asm: build/<unit>-hip-amdgcn-amd-amdhsa-gfx950.s) line for line those of another?

  python tools/asm_same_kernels.py parent/build/direct-hip-amdgcn-amd-amdhsa-gfx950.s build/direct-hip-amdgcn-amd-amdhsa-gfx950.s

For a unit that gained kernels or whose kernels gained a trailing template parameter: every kernel of the first file must have exactly
one partner in the second - the same function name and template integers, or those followed by one more `false` - with the same
instructions.  Dropped before comparing: __hip_cuid_ lines, the numbers of local labels, mangled names, and comments (they name IR blocks
by a running number that moves with any code added to the unit).  A unit that gained nothing is compared with diff, less the
__hip_cuid_ line.  Exit status 1 if any kernel differs or has no partner."""
import re
import sys


def bodies(path):
    out, name, cur = {}, None, []
    for line in open(path):
        if "__hip_cuid_" in line:
            continue
        m = re.match(r"^(_Z\w+):\s", line)
        if m and name is None:
            name, cur = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = cur
                name = None
                continue
            line = re.sub(r"\.LBB\d+_\d+", ".LBB", line)
            line = re.sub(r"_Z\w+", "SYM", line)
            line = re.sub(r"\s*;.*$", "", line)
            cur.append(line)
    return out


def key(name):
    m = re.search(r"(\d+[A-Za-z_]\w*?)I((?:L[ib]\d+E)+)E", name)
    return (m.group(1), m.group(2)) if m else (name, "")


def main():
    old, new = bodies(sys.argv[1]), bodies(sys.argv[2])
    bad = 0
    for n, b in old.items():
        k = key(n)
        partners = [m for m in new if key(m) == k or key(m) == (k[0], k[1] + "Lb0E")]
        if len(partners) != 1:
            print("NO PARTNER", n, partners)
            bad += 1
            continue
        same = new[partners[0]] == b
        print("same" if same else "DIFFERENT", len(b), "lines", k)
        bad += not same
    print("kernels: first file", len(old), "second file", len(new), "differing or without partner", bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
