#!/usr/bin/env python3
"""Per-kernel resources of two device-only assembly files of one source, side by side (profiles/README.md, "Q1 group frame").

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -Iplan_amd/csrc --cuda-device-only -S plan_amd/csrc/scan_kernels.hip -o new.s
    python scripts/kernel_resources.py parent.s new.s [OLD_NAME=NEW_NAME ...] > profiles/<name>_kernel_resources.txt

A kernel is matched by its demangled name, or through an OLD_NAME=NEW_NAME pair when the change renamed it. VGPR, SGPR, LDS and scratch
are the compiler's own "Kernel info" lines; "insts" counts the instruction lines of the kernel's text. The last column says whether the
two texts are the same multiset of instruction lines (registers included; labels without the function's number), i.e. differ by order only.
"""
import collections
import re
import subprocess
import sys

INFO = {"vgpr": r"; TotalNumVgprs: (\d+)", "sgpr": r"; TotalNumSgprs: (\d+)", "lds": r"; LDSByteSize: (\d+)", "scratch": r"; ScratchSize: (\d+)"}


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return [re.sub(r"^void |\([^()]*\)$|ph::| (?=>)", "", n) for n in out.splitlines()]   # the name and its template arguments


def kernels(path):
    """{demangled name: (resources, Counter of instruction lines)} of every kernel of the file"""
    text = open(path).read()
    found = []
    for m in re.finditer(r"^(\w+):.*?\n(.*?)^\.Lfunc_end\d+:\n.*?^; Kernel info:\n(.*?)^; COMPUTE_PGM", text, re.M | re.S):
        insts = [re.sub(r"\.LBB\d+_", ".LBB_", ln.split(";")[0].strip()) for ln in m.group(2).splitlines() if re.match(r"\t[a-z]", ln)]
        res = {k: int(re.search(p, m.group(3)).group(1)) for k, p in INFO.items()}
        res["insts"] = len(insts)
        found.append((m.group(1), res, collections.Counter(insts)))
    return {n: (r, c) for n, (_, r, c) in zip(demangle([f[0] for f in found]), found)}


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    renamed = dict(a.split("=", 1) for a in sys.argv[3:])
    cols = ["vgpr", "sgpr", "lds", "scratch", "insts"]
    print(f"{len(old)} kernels in {sys.argv[1]}, {len(new)} in {sys.argv[2]}; parent -> branch")
    print("  ".join(f"{c:>12}" for c in cols) + "  same multiset  kernel")
    for name, (r0, c0) in old.items():
        to = renamed.get(name, name)
        r1, c1 = new[to]
        cells = "  ".join(f"{str(r0[c]) + ' -> ' + str(r1[c]):>12}" for c in cols)
        print(f"{cells}  {'yes' if c0 == c1 else 'no':>13}  {name}" + (f"  (now {to})" if to != name else ""))
    left = set(new) - {renamed.get(n, n) for n in old}
    assert not left, left


if __name__ == "__main__":
    main()
