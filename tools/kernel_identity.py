#!/usr/bin/env python3
"""Are the kernels of two builds the same instructions?  Reads the device assembly of one kernel file from two builds -- any pair of
.s files: kernels.s, transpose.s, value_grad.s, tts_transpose.s, spmm.s, spmm_bf16.s, spmm_grad.s, spmm_grad_bf16.s (`make -C hispmv_amd/csrc
asm-all`) -- and
compares, per kernel symbol, the function text and the .amdhsa_kernel descriptor block -- comments, .loc / .file lines and blank lines
stripped, label numbers (.LBB<n>_, .Ltmp<n>, .Lfunc_*<n>) normalised.  Per symbol, not with diff: the order in which the
instantiations are emitted follows the host code.  Exit status 1 if a kernel changed, appeared or went.
Usage: tools/kernel_identity.py before/spmm.s after/spmm.s"""
import re
import sys
from pathlib import Path


def kernels(path):
    txt = Path(path).read_text().split("\n")
    names = {l.split()[-1] for l in txt if l.strip().startswith(".amdhsa_kernel ")}
    out = {n: [] for n in names}
    lines = 0
    cur, desc = None, None
    for l in txt:
        m = re.match(r"^(\S+):\s*;\s*@", l)
        if m and m.group(1) in names:
            cur = m.group(1)
        if l.strip().startswith(".amdhsa_kernel "):
            desc = l.split()[-1]
        for name in {cur, desc} - {None}:
            s = l.split(";")[0].strip()
            if not s or s.startswith((".loc", ".file", ".cfi_")):
                continue
            s = re.sub(r"\.LBB\d+_", ".LBB_", s)
            s = re.sub(r"\.(Ltmp|Lfunc_begin|Lfunc_end)\d+", r".\1", s)
            out[name].append(s)
            lines += name == cur and not s.endswith(":") and not s.startswith(".")
        if cur and re.match(r"^\.Lfunc_end\d+:", l):
            cur = None
        if l.strip() == ".end_amdhsa_kernel":
            desc = None
    return out, lines


a, la = kernels(sys.argv[1])
b, lb = kernels(sys.argv[2])
changed = sorted(n for n in a.keys() & b.keys() if a[n] != b[n])
new, gone = sorted(b.keys() - a.keys()), sorted(a.keys() - b.keys())
print(f"kernel symbols: {len(a)} before, {len(b)} after; instruction lines: {la} before, {lb} after")
print(f"{len(changed)} changed, {len(new)} new, {len(gone)} gone")
for tag, ns in (("changed", changed), ("new", new), ("gone", gone)):
    for n in ns:
        print(f"  {tag}: {n}")
sys.exit(1 if changed or new or gone else 0)
