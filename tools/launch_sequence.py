#!/usr/bin/env python3
"""The kernel launches of a fixed list of multi-vector and Krylov calls, to compare two builds of the library launch for launch.

    rocprofv3 --kernel-trace --output-format csv -d A -- python tools/launch_sequence.py run      # HISPMV_LIB = the one build
    rocprofv3 --kernel-trace --output-format csv -d B -- python tools/launch_sequence.py run      # ... the other, a process of its own
    python tools/launch_sequence.py compare A B [report.txt]

`run` issues, on small matrices and with a hispmv_synchronize behind every call:
  linear_device    on a one-part slice stream, a slice stream of 8 column parts, a tile stream and a dense handle;
  linear_device_t  on handles whose stored transpose is a one-part slice stream, 8 column parts and a tile stream;
                   both for B in 1, 2, 3, 5, 9, beta 0 and 1, d_x aligned and moved by one float, _t with a shared and a per-vector bias;
  spmm_device, spmm_device_t and their bf16 forms (5 and 130 vectors), value_grad_device on a slice stream and a dense handle;
  the Krylov layer on tridiagonal systems of n = 1025 (two chunks, a one-element tail) and 4099: cg_device without and with minv,
                   bicgstab_device, cgls_device over a stored transpose, and cg_multi_device without and with minv and
                   bicgstab_multi_device for 5 and 65 right-hand sides (a second column tile of one column), each with rtol = 0 and
                   (max_iters, check_every) = (4, 0), (4, 3) -- a look inside the loop and one behind it -- and (3, 3) -- the last look
                   is the loop's; every entry once with b = 0 and check_every = 3 (the early return: no product); dot_device and
                   dot_multi_device at n = 1025.
It asserts that every handle got the kind it is listed under.  `compare` reads the kernel traces (the CSV columns tools/trace_seq.py
reads), keeps the library's kernels in dispatch order and compares (kernel name, grid, workgroup, LDS bytes) line by line; exit
status 1 on a difference."""
from __future__ import annotations

import csv
import glob
import os
import sys
from contextlib import contextmanager
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

HW = ("launch_sequence.xclbin", 0, 24, 1, 1, 2, 5, True, False, True)
BS = (1, 2, 3, 5, 9)
SLICES = {"HISPMV_FORMAT": "slices"}
COLTILES = {"HISPMV_FORMAT": "slices", "HISPMV_COL_TILE_BYTES": "65536"}
AUTO = {"HISPMV_FORMAT": "auto", "HISPMV_TTS_MIN_NNZ": "20000"}


@contextmanager
def environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def uniform(rows, cols, nnz, seed, heavy_row=None):
    """nnz entries anywhere; heavy_row = (row, share): that share of them in one row, which the packer then cuts."""
    rng = np.random.default_rng(seed)
    r, c = rng.integers(0, rows, nnz), rng.integers(0, cols, nnz)
    if heavy_row is not None:
        r[: int(nnz * heavy_row[1])] = heavy_row[0]
    return dict(rows=rows, cols=cols, r=r.astype(np.int32), c=c.astype(np.int32), v=rng.random(nnz, dtype=np.float32) - np.float32(0.5))


def T(m):
    return dict(m, rows=m["cols"], cols=m["rows"], r=m["c"], c=m["r"])


def tridiag(n):
    """2.5 on the diagonal, -1 beside it: the system of tests/krylov_model.py"""
    i = np.arange(n, dtype=np.int32)
    return dict(rows=n, cols=n, r=np.concatenate([i, i[1:], i[:-1]]), c=np.concatenate([i, i[:-1], i[1:]]),
                v=np.concatenate([np.full(n, 2.5), np.full(2 * (n - 1), -1.0)]).astype(np.float32))


KRYLOV_NS = (1025, 4099)
KRYLOV_MS = (5, 65)
KRYLOV_LOOPS = ((4, 0), (4, 3), (3, 3))          # (max_iters, check_every)


def run():
    import torch
    import pyhispmv
    dev = torch.device("cuda", 0)

    def buffers(n):
        host = np.random.default_rng(1).random(n + 8, dtype=np.float32)
        return [torch.from_numpy(host).to(dev) for _ in range(3)]          # (copies: no kernel of torch's in between)

    def linear_calls(h, k, info, transposed):
        n = 9 * max(info["rows"], info["cols"])
        x, b, y = buffers(n)
        for B in BS:
            for beta in (0.0, 1.0):
                for shift in (0, 4):
                    if not transposed:
                        h.linear_device(k, x.data_ptr() + shift, B, b.data_ptr(), y.data_ptr(), 1.0, beta)
                        h.synchronize()
                        continue
                    for stride in (0, info["cols"]):
                        h.linear_device_t(k, x.data_ptr() + shift, B, b.data_ptr(), y.data_ptr(), 1.0, beta, bias_stride=stride)
                        h.synchronize()

    def context(env, make):
        with environment(env):
            h = pyhispmv.FpgaHandle(*HW)
            kinds = make(h)
            h.load_matrices()
        return h, kinds

    def sparse(h, m):
        return h.create_sparse_handle(m["r"], m["c"], m["v"], m["rows"], m["cols"])

    small = uniform(300, 252, 4000, 3, heavy_row=(7, 0.3))
    tiled = uniform(3000, 200000, 60000, 42, heavy_row=(7, 1.0 / 3))
    scattered = uniform(3000, 400000, 60000, 32)

    # ---- slice streams of one part, a dense handle, the wide batch and the value gradients
    def make_small(h):
        k = dict(slices=sparse(h, small), dense=h.create_dense_handle(np.arange(17 * 33, dtype=np.float32) / 100, 17, 33))
        h.set_transposable("companion")
        k["stored"] = sparse(h, small)
        h.set_transposable(0)
        h.set_value_updates(True)
        k["updatable"] = sparse(h, small)
        k["updatable_dense"] = h.create_dense_handle(np.arange(17 * 33, dtype=np.float32) / 100, 17, 33)
        return k
    h, k = context(SLICES, make_small)
    info = {name: h.matrix_info(i) for name, i in k.items()}
    ci = h.companion_info(k["stored"])
    assert info["slices"]["format"] == 0 and info["slices"]["col_tiles"] == 1 and ci["has"] and ci["format"] == 0 and ci["parts"] == 1, (info, ci)
    linear_calls(h, k["slices"], info["slices"], False)
    linear_calls(h, k["dense"], info["dense"], False)
    linear_calls(h, k["stored"], info["stored"], True)
    for nv in (5, 130):
        x, b, y = buffers(nv * 300)
        work = torch.zeros(1 << 20, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        for beta in (0.0, 1.0):
            for call in (h.spmm_device, h.spmm_device_t, h.spmm_device_bf16, h.spmm_device_t_bf16):
                call(k["stored"], x.data_ptr(), nv, b.data_ptr(), y.data_ptr(), 1.0, beta, work=work.data_ptr(), work_bytes=4 * work.numel())
                h.synchronize()
    for name in ("updatable", "updatable_dense"):
        n = h.value_update_info(k[name])["n"]
        x, gy, _ = buffers(9 * 300)
        grad = torch.zeros(n, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        for B in BS:
            for alpha, beta in ((1.0, 0.0), (0.5, 1.0), (0.0, 2.0)):
                h.value_grad_device(k[name], gy.data_ptr(), x.data_ptr(), B, grad.data_ptr(), alpha, beta)
                h.synchronize()
    h.close()

    # ---- eight column parts, forward and as a stored transpose
    def make_tiled(h):
        k = dict(slices=sparse(h, tiled))
        h.set_transposable("companion")
        k["stored"] = sparse(h, T(tiled))
        return k
    h, k = context(COLTILES, make_tiled)
    info = {name: h.matrix_info(i) for name, i in k.items()}
    ci = h.companion_info(k["stored"])
    assert info["slices"]["format"] == 0 and info["slices"]["col_tiles"] == 8 and ci["format"] == 0 and ci["parts"] == 8, (info, ci)
    linear_calls(h, k["slices"], info["slices"], False)
    linear_calls(h, k["stored"], info["stored"], True)
    h.close()

    # ---- a tile stream, forward and as a stored transpose
    def make_tts(h):
        k = dict(tile_stream=sparse(h, scattered))
        h.set_transposable("companion")
        k["stored"] = sparse(h, T(scattered))
        return k
    h, k = context(AUTO, make_tts)
    info = {name: h.matrix_info(i) for name, i in k.items()}
    ci = h.companion_info(k["stored"])
    assert info["tile_stream"]["format"] == 1 and info["tile_stream"]["col_tiles"] == 1 and ci["format"] == 1 and ci["parts"] == 1, (info, ci)
    linear_calls(h, k["tile_stream"], info["tile_stream"], False)
    linear_calls(h, k["stored"], info["stored"], True)
    h.close()

    # ---- the Krylov layer: square slice streams for CG and BiCGSTAB, single and multi, and one with a stored transpose for CGLS
    def make_krylov(h):
        k = {("square", n): sparse(h, tridiag(n)) for n in KRYLOV_NS}
        h.set_transposable("companion")
        k.update({("stored", n): sparse(h, tridiag(n)) for n in KRYLOV_NS})
        return k
    h, k = context(SLICES, make_krylov)

    def device(a):
        return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)

    def workspace(nbytes):
        return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    for n in KRYLOV_NS:
        mmax = max(KRYLOV_MS)
        host = np.random.default_rng(1).uniform(-1, 1, n * mmax)
        bs = {"b": device(host), "0": device(np.zeros(n * mmax))}
        minv, x = device(np.full(n, 0.4)), device(np.zeros(n * mmax))
        singles = [("cg", h.cg_device, ("square", n), {}), ("cg", h.cg_device, ("square", n), dict(d_minv=minv.data_ptr())),
                   ("bicgstab", h.bicgstab_device, ("square", n), {}), ("cgls", h.cgls_device, ("stored", n), {})]
        multis = [("cg", h.cg_multi_device, {}), ("cg", h.cg_multi_device, dict(d_minv=minv.data_ptr())), ("bicgstab", h.bicgstab_multi_device, {})]

        def solve(call, idx, work, loops, b, **kw):
            for max_iters, check_every in loops:
                x.zero_()
                torch.cuda.synchronize()
                call(idx, bs[b].data_ptr(), x.data_ptr(), rtol=0.0, max_iters=max_iters, check_every=check_every, work=work.data_ptr(),
                     work_bytes=work.numel(), **kw)
                h.synchronize()
        for solver, call, key, kw in singles:
            info = h.krylov_info(k[key], solver)
            assert info["accepted"], (solver, key, info)
            work = workspace(info["work_bytes"])
            solve(call, k[key], work, KRYLOV_LOOPS, "b", **kw)
            if not kw:
                solve(call, k[key], work, ((4, 3),), "0")
        for m in KRYLOV_MS:
            for solver, call, kw in multis:
                info = h.krylov_multi_info(k["square", n], solver, m)
                assert info["accepted"], (solver, m, info)
                work = workspace(info["work_bytes"])
                solve(call, k["square", n], work, KRYLOV_LOOPS, "b", num_vecs=m, **kw)
                if not kw and m == KRYLOV_MS[0]:
                    solve(call, k["square", n], work, ((4, 3),), "0", num_vecs=m)
    n = KRYLOV_NS[0]
    out, work = torch.zeros(max(KRYLOV_MS), dtype=torch.float64, device=dev), workspace(8 * 2 * 68)          # 2 chunks x ld 68
    for m in (0,) + KRYLOV_MS:          # 0: dot_device
        a = device(np.random.default_rng(2).uniform(-1, 1, n * max(m, 1)))
        torch.cuda.synchronize()
        if m:
            h.dot_multi_device(n, m, a.data_ptr(), a.data_ptr(), out.data_ptr(), work.data_ptr(), work.numel())
        else:
            h.dot_device(n, a.data_ptr(), a.data_ptr(), out.data_ptr(), work.data_ptr(), work.numel())
        h.synchronize()
    h.close()
    print("launch_sequence: all calls issued")


def launches(src):
    """The library's kernels of a trace directory (or CSV file) in dispatch order -> [(name, grid, workgroup, LDS bytes)]."""
    files = [src] if src.endswith(".csv") else sorted(glob.glob(src + "/**/*kernel_trace.csv", recursive=True))
    assert files, f"no kernel trace under {src}"
    rows = [r for f in files for r in csv.DictReader(open(f))]
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    return [(r["Kernel_Name"], tuple(int(r[f"Grid_Size_{a}"]) for a in "XYZ"), tuple(int(r[f"Workgroup_Size_{a}"]) for a in "XYZ"), int(r["LDS_Block_Size"]))
            for r in rows if "hispmv" in r["Kernel_Name"]]


def compare(a, b, report=None):
    la, lb = launches(a), launches(b)
    lines = [f"launches compared: {len(la)} against {len(lb)}"]
    diff = [(i, x, y) for i, (x, y) in enumerate(zip(la, lb)) if x != y]
    for i, x, y in diff[:20]:
        lines += [f"launch {i}:", f"  {a}: {x}", f"  {b}: {y}"]
    same = not diff and len(la) == len(lb) and len(la) > 0
    lines.append("result: identical (kernel name, grid, workgroup, LDS bytes, in dispatch order)" if same else f"result: DIFFERENT ({len(diff)} of the common launches differ)")
    kinds = sorted({x[0].split("<")[0].replace("void ", "") for x in la})
    lines.append(f"distinct kernels: {len(kinds)}: " + ", ".join(kinds))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if report:
        Path(report).write_text(text)
    return 0 if same else 1


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) >= 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else None))
    else:
        sys.exit(__doc__)
