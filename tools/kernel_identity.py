#!/usr/bin/env python3
r"""Are the kernels of two builds the same instructions?  Reads the device assembly of one kernel file from two builds -- .s files of
`make -C hispmv_amd/csrc asm-all`: kernels.s, transpose.s, value_grad.s, tts_transpose.s, spmm.s, spmm_grad.s, krylov.s, krylov_multi.s, gmres.s, lanczos.s,
block_jacobi.s -- and
compares, per kernel symbol, the function text and the .amdhsa_kernel descriptor block -- comments, .loc / .file lines and blank lines
stripped, label numbers (.LBB<n>_, .Ltmp<n>, .Lfunc_*<n>) normalised.  Per symbol, not with diff: the order in which the
instantiations are emitted follows the host code.  Exit status 1 if a kernel changed, appeared or went.
Several files may stand for the "before" side (two kernel files that became one): every file but the last is "before".  Where a kernel
changed its NAME -- two templates that became one over a further parameter -- `--rename PATTERN REPLACEMENT` (re.sub, may be repeated)
rewrites the mangled symbols of the "before" side, in the text as well, ahead of the comparison.
Usage: tools/kernel_identity.py before/transpose.s after/transpose.s
       tools/kernel_identity.py --rename '23spmm_grad_slices_kernelIL(\w*?)NS_16SpmmGradOperandsE' '23spmm_grad_slices_kernelIfL\1NS_18SpmmGradOperandsOfIT_EE' \
           --rename '28spmm_grad_bf16_slices_kernelIL(\w*?)NS_20SpmmGradBf16OperandsE' '23spmm_grad_slices_kernelItL\1NS_18SpmmGradOperandsOfIT_EE' \
           before/spmm_grad.s before/spmm_grad_bf16.s after/spmm_grad.s"""
import argparse
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


def renamed(ks, rules):
    def sub(s):
        for pat, repl in rules:
            s = re.sub(pat, repl, s)
        return s
    out = {}
    for n, body in ks.items():
        assert sub(n) not in out, f"two kernels are renamed to {sub(n)}"
        out[sub(n)] = [sub(l) for l in body]
    return out


ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
ap.add_argument("--rename", nargs=2, action="append", default=[], metavar=("PATTERN", "REPLACEMENT"))
ap.add_argument("files", nargs="+", help="BEFORE.s [BEFORE.s ...] AFTER.s")
args = ap.parse_args()
if len(args.files) < 2:
    ap.error("at least one file before and one after")
a, la = {}, 0
for f in args.files[:-1]:
    ks, n = kernels(f)
    assert not a.keys() & ks.keys(), f"{f} defines a kernel an earlier file has"
    a.update(ks)
    la += n
a = renamed(a, args.rename)
b, lb = kernels(args.files[-1])
changed = sorted(n for n in a.keys() & b.keys() if a[n] != b[n])
new, gone = sorted(b.keys() - a.keys()), sorted(a.keys() - b.keys())
print(f"kernel symbols: {len(a)} before, {len(b)} after; instruction lines: {la} before, {lb} after")
print(f"{len(changed)} changed, {len(new)} new, {len(gone)} gone")
for tag, ns in (("changed", changed), ("new", new), ("gone", gone)):
    for n in ns:
        print(f"  {tag}: {n}")
sys.exit(1 if changed or new or gone else 0)
