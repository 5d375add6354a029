#!/usr/bin/env python3
"""Compare the gfx950 kernels of two sets of assembly files, symbol by symbol (plain text diffing, nothing more).

    hipcc <library flags> --cuda-device-only -S csrc/X.hip -o before/X.s     (likewise after/)
    python tools/asm_kernel_diff.py before/ after/

For every .amdhsa_kernel symbol found in either directory the instruction text from the symbol's label to its .Lfunc_end and
the .amdhsa_* block (register counts, scratch, LDS, occupancy inputs) are compared.  Kernels may move between files.  Two
normalisations: the per-translation-unit __hip_cuid_* symbol and the function ordinal inside local labels (.LBB<n>_<m>, also
where the compiler's block comments quote them; runs of blanks count as one).
Exit status 0: same set of kernels, same text for each."""
from __future__ import annotations

import difflib
import glob
import os
import re
import sys


def _norm(line: str) -> str:
    line = re.sub(r"__hip_cuid_\w+", "__hip_cuid", line)
    line = re.sub(r"\.L([A-Za-z_]+?)\d+_(\d+)", r".L\1_\2", line)
    line = re.sub(r"\bBB\d+_(\d+)", r"BB_\1", line)  # the same ordinal inside the compiler's block comments
    line = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", line)
    return " ".join(line.split())  # comment columns move with the label width


def kernels(directory: str) -> dict:
    """symbol -> (file, normalised body lines, normalised .amdhsa block lines)"""
    out = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        lines = open(path).read().split("\n")
        names = [l.split()[1] for l in lines if l.lstrip().startswith(".amdhsa_kernel ")]
        for name in names:
            start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
            end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
            d0 = next(i for i, l in enumerate(lines) if l.split() == [".amdhsa_kernel", name])
            d1 = next(i for i in range(d0, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
            assert name not in out, f"{name} defined twice ({out.get(name, ('',))[0]}, {path})"
            out[name] = (os.path.basename(path), [_norm(l) for l in lines[start:end + 1]], [_norm(l) for l in lines[d0:d1 + 1]])
    return out


def main() -> int:
    if len(sys.argv) != 3:
        print(__doc__)
        return 2
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for name in sorted(set(a) - set(b)):
        print(f"ONLY BEFORE  {name}  ({a[name][0]})")
        bad += 1
    for name in sorted(set(b) - set(a)):
        print(f"ONLY AFTER   {name}  ({b[name][0]})")
        bad += 1
    for name in sorted(set(a) & set(b)):
        for what, x, y in (("code", a[name][1], b[name][1]), ("descriptor", a[name][2], b[name][2])):
            if x != y:
                bad += 1
                d = list(difflib.unified_diff(x, y, lineterm="", n=0))
                changed = sum(1 for l in d if l[:1] in "+-" and l[:3] not in ("+++", "---"))
                print(f"DIFFERS      {name}  {what}: {len(x)} -> {len(y)} lines, {changed} changed  ({a[name][0]} -> {b[name][0]})")
                for l in d[:12]:
                    print("    " + l)
    print(f"{len(a)} kernels before, {len(b)} after, {bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
