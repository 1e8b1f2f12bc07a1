"""Per-iteration time of the device-resident Krylov solvers against the same loops written in torch (not part of bench.py).

Per system and solver (cg, bicgstab, cgls), `--iters` iterations from x = 0 with rtol = 0 (nothing stops early), wall clock from the
first enqueue to the end of a final synchronisation, `--rounds` times, alternately, medians and spread:
  ours8   hispmv_amd.solvers with check_every = 8      (the default: the host looks every 8 iterations)
  ours0   check_every = 0                               (everything enqueued, one synchronisation at the end)
  (a)     the loop in torch: spmv_device / spmv_device_t for the products, torch ops for the vectors, fp32 dot products, and a
          .item() on the residual norm every iteration -- what a user writes today with a stopping rule
  (b)     the same loop without any stop test: no host synchronisation until the end
  prod    the products of an iteration alone, back to back
Reported per solver: microseconds per iteration of each, ours8 / (a), ours0 / (b), and the share of an ours0 iteration that is not
product time, 1 - prod / ours0.  `spread` is the largest (max - min) / median among the timings a ratio is made of: a ratio closer to
1 than that is not a difference.  `iterations` is what the layer reports it applied: fewer than --iters means it froze (breakdown or
an exact zero residual) and the row says so.

Systems: the small tridiagonal system of the tests (n = 4099) and stand-ins of hispmv_amd/matrices.py with a dominant diagonal added
(the stand-ins carry random values; the diagonal makes them systems a Krylov method can be timed on -- "spd" rows are the symmetric
part's positive definite kind, not symmetrised).  CGLS runs over a stored transpose (set_transposable("companion")).

    python tools/krylov_bench.py [--iters 48] [--rounds 5] [--systems a,b] [--out profiles/krylov_bench.json]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

STANDINS = ("poli_large", "hangGlider_3", "c-52", "lowThrust_7", "ford2", "trans5")


def systems():
    from hispmv_amd import matrices
    n = 4099
    i = np.arange(n)
    r = np.concatenate([i, i[1:], i[:-1]])
    c = np.concatenate([i, i[:-1], i[1:]])
    v = np.concatenate([np.full(n, 2.5), np.full(2 * (n - 1), -1.0)]).astype(np.float32)
    yield "tridiag_4099", n, r, c, v
    for name in STANDINS:
        rows, cols, rp, ci, va, _ = matrices.suitesparse_standin(name)
        rr = np.repeat(np.arange(rows), np.diff(rp))
        dom = np.bincount(rr, weights=np.abs(va), minlength=rows).astype(np.float32) + np.float32(1.0)
        yield name, rows, np.concatenate([rr, np.arange(rows)]), np.concatenate([ci, np.arange(rows)]), np.concatenate([va, dom]).astype(np.float32)


def torch_loop(torch, h, idx, solver, b, iters, stop_test):
    """The solver written with the library's products and torch vector ops on the current stream; returns x."""
    s = torch.cuda.current_stream().cuda_stream
    n = b.numel()

    def mv(x, y):
        h.spmv_device(idx, x.data_ptr(), 0, y.data_ptr(), 1.0, 0.0, s)

    def mvt(x, y):
        h.spmv_device_t(idx, x.data_ptr(), 0, y.data_ptr(), 1.0, 0.0, s)
    x = torch.zeros_like(b)
    r = torch.empty_like(b)
    h.spmv_device(idx, x.data_ptr(), b.data_ptr(), r.data_ptr(), -1.0, 1.0, s)
    q = torch.empty_like(b)
    bb = torch.dot(b, b)
    if solver == "cg":
        p = r.clone()
        rz = torch.dot(r, r)
        for _ in range(iters):
            mv(p, q)
            alpha = rz / torch.dot(p, q)
            x.add_(alpha * p)
            r.sub_(alpha * q)
            rz_new = torch.dot(r, r)
            if stop_test and (rz_new / bb).item() < 0.0:
                break
            p.mul_(rz_new / rz).add_(r)
            rz = rz_new
    elif solver == "bicgstab":
        rhat, p, t = r.clone(), r.clone(), torch.empty_like(b)
        rho = torch.dot(rhat, r)
        for _ in range(iters):
            mv(p, q)
            alpha = rho / torch.dot(rhat, q)
            r.sub_(alpha * q)
            mv(r, t)
            omega = torch.dot(t, r) / torch.dot(t, t)
            x.add_(alpha * p).add_(omega * r)
            r.sub_(omega * t)
            if stop_test and (torch.dot(r, r) / bb).item() < 0.0:
                break
            rho_new = torch.dot(rhat, r)
            p.sub_(omega * q).mul_((rho_new / rho) * (alpha / omega)).add_(r)
            rho = rho_new
    else:
        sv = torch.empty(n, dtype=b.dtype, device=b.device)
        mvt(r, sv)
        p = sv.clone()
        gamma = torch.dot(sv, sv)
        g0 = gamma.clone()
        for _ in range(iters):
            mv(p, q)
            alpha = gamma / torch.dot(q, q)
            x.add_(alpha * p)
            r.sub_(alpha * q)
            mvt(r, sv)
            g_new = torch.dot(sv, sv)
            if stop_test and (g_new / g0).item() < 0.0:
                break
            p.mul_(g_new / gamma).add_(sv)
            gamma = g_new
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--systems", default="")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "krylov_bench.json"))
    args = ap.parse_args()
    import torch
    import pyhispmv
    from hispmv_amd import solvers
    dev = torch.device("cuda", 0)
    K = args.iters
    only = set(filter(None, args.systems.split(",")))
    results = []
    for name, n, r, c, v in systems():
        if only and name not in only:
            continue
        h = pyhispmv.FpgaHandle("bench.xclbin", 0, 24, 1, 1, 2, 5, True, False, True)
        h.set_transposable("companion")
        idx = h.create_sparse_handle(r, c, v, n, n)
        h.load_matrices()
        info = h.matrix_info(idx)
        b = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, n).astype(np.float32)).to(dev)
        y = torch.empty_like(b)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream(device=dev)
        row = dict(system=name, n=n, nnz=int(info["nnz"]), format=int(info["format"]), parts=int(info["col_tiles"]), solvers={})
        with torch.cuda.stream(stream):
            for solver in ("cg", "bicgstab", "cgls"):
                fn = getattr(solvers, solver)
                ki = h.krylov_info(idx, solver)
                work = solvers.workspace(h, idx, solver, dev)
                applied = {}

                def ours(ce):
                    x, out = fn(h, idx, b, rtol=0.0, max_iters=K, check_every=ce, work=work)
                    if ce == 0:
                        out = h.krylov_status(work.data_ptr(), stream.cuda_stream)
                    applied[ce] = (out["status"], out["iterations"])

                def products():
                    for _ in range(K):
                        for _ in range(ki["products_per_iteration"]):
                            h.spmv_device(idx, b.data_ptr(), 0, y.data_ptr(), 1.0, 0.0, stream.cuda_stream)
                        for _ in range(ki["products_t_per_iteration"]):
                            h.spmv_device_t(idx, b.data_ptr(), 0, y.data_ptr(), 1.0, 0.0, stream.cuda_stream)
                calls = {"ours8": lambda: ours(8), "ours0": lambda: ours(0), "a": lambda: torch_loop(torch, h, idx, solver, b, K, True),
                         "b": lambda: torch_loop(torch, h, idx, solver, b, K, False), "prod": products}
                t = {k: [] for k in calls}
                for f in calls.values():
                    f()
                stream.synchronize()
                for _ in range(args.rounds):
                    for k, f in calls.items():
                        t0 = time.perf_counter()
                        f()
                        stream.synchronize()
                        t[k].append((time.perf_counter() - t0) * 1e6 / K)
                med = {k: float(np.median(x)) for k, x in t.items()}
                spread = max(float((max(x) - min(x)) / np.median(x)) for x in t.values())
                row["solvers"][solver] = dict(us_per_iteration=med, ours8_over_a=med["ours8"] / med["a"], ours0_over_b=med["ours0"] / med["b"],
                                              ours8_over_b=med["ours8"] / med["b"], not_product_share=1.0 - med["prod"] / med["ours0"], spread=spread,
                                              applied=applied, launches_per_iteration=ki["launches_per_iteration"])
                print(f'{name:14s} {solver:9s} us/iter ours8 {med["ours8"]:8.1f} ours0 {med["ours0"]:8.1f} (a) {med["a"]:8.1f} (b) {med["b"]:8.1f} prod {med["prod"]:8.1f} '
                      f'| ours8/(a) {med["ours8"] / med["a"]:.2f} ours0/(b) {med["ours0"] / med["b"]:.2f} not-product {1.0 - med["prod"] / med["ours0"]:.2f} '
                      f'spread {spread:.2f} applied {applied}', flush=True)
        torch.cuda.synchronize()
        h.close()
        results.append(row)
    line = json.dumps(dict(tool="krylov_bench", iters=K, rounds=args.rounds, device=torch.cuda.get_device_name(0), results=results))
    print(line)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
