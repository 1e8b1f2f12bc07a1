"""Per-inner-iteration time of restarted GMRES(m) on loaded handles against the same loop in torch and against BiCGSTAB per product
(not part of bench.py).

Per system of tools/krylov_bench.py (non-symmetric as they stand: random values under a dominant diagonal) and restart 10 and 30,
`--iters` inner iterations from x = 0 with rtol = 0 (nothing stops early), wall clock from the first enqueue to the end of a final
synchronisation, `--rounds` times, alternately, medians and spread:
  gmres8  solvers.gmres with check_every = 8
  gmres0  check_every = 0 (everything enqueued, one synchronisation at the end)
  (a)     the same CGS2 loop in torch: spmv_device for the product, h = V @ w and w -= V.T @ h twice, the norm, and the Givens
          rotations on the host (one .cpu() per inner iteration)
  (b)     bicgstab_device, check_every = 0, --iters / 2 iterations: the same number of products
  prod    the products alone, back to back
Reported: microseconds per inner iteration (for (b): per product), gmres8 / (a), gmres0 / (a), gmres0 / (b), and the share of a gmres0
iteration that is not product time, 1 - prod / gmres0.  `spread` is the largest (max - min) / median among the timings.
Per system also, for j = 1, 10, 30, 63: `step` = the time of inner iteration j, from the difference of two check_every = 0 solves of
j + 1 and j iterations at restart 64; `multi_dot` = dot_basis_device over j + 1 vectors (the multi-dot kernel and its one-workgroup
finish); `rest` = step - one product - multi_dot: the two subtract-and-dot passes and the rotate kernel.

    python tools/gmres_bench.py [--iters 60] [--rounds 5] [--systems a,b] [--out profiles/gmres_bench.json]
"""
from __future__ import annotations

import argparse
import json
import math
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

STEPS = (1, 10, 30, 63)


def torch_gmres(torch, h, idx, b, iters, restart):
    """GMRES(restart) with CGS2 written with the library's product and torch ops on the current stream; returns x."""
    s = torch.cuda.current_stream().cuda_stream
    n = b.numel()
    x = torch.zeros_like(b)
    V = torch.empty(restart + 1, n, dtype=b.dtype, device=b.device)
    it = 0
    while it < iters:
        m = min(restart, iters - it)
        h.spmv_device(idx, x.data_ptr(), b.data_ptr(), V[0].data_ptr(), -1.0, 1.0, s)
        beta = torch.linalg.vector_norm(V[0])
        V[0].div_(beta)
        g = np.zeros(m + 1)
        g[0] = float(beta)
        R = np.zeros((m + 1, m))
        cs, sn = np.zeros(m), np.zeros(m)
        for j in range(m):
            w = V[j + 1]
            h.spmv_device(idx, V[j].data_ptr(), 0, w.data_ptr(), 1.0, 0.0, s)
            B = V[:j + 1]
            h1 = B @ w
            w.sub_(B.T @ h1)
            h2 = B @ w
            w.sub_(B.T @ h2)
            hn = torch.linalg.vector_norm(w)
            col = torch.cat([h1 + h2, hn.reshape(1)]).double().cpu().numpy()          # the host's look of this loop
            w.div_(hn)
            for i in range(j):
                col[i], col[i + 1] = cs[i] * col[i] + sn[i] * col[i + 1], cs[i] * col[i + 1] - sn[i] * col[i]
            d = math.hypot(col[j], col[j + 1])
            cs[j], sn[j] = col[j] / d, col[j + 1] / d
            col[j], col[j + 1] = d, 0.0
            g[j + 1] = -sn[j] * g[j]
            g[j] = cs[j] * g[j]
            R[:j + 2, j] = col
            it += 1
        y = np.linalg.solve(np.triu(R[:m, :m]), g[:m])
        x.add_(V[:m].T @ torch.from_numpy(y.astype(np.float32)).to(b.device))
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--systems", default="")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "gmres_bench.json"))
    args = ap.parse_args()
    import torch
    import pyhispmv
    from hispmv_amd import prep, solvers
    from krylov_bench import systems
    dev = torch.device("cuda", 0)
    K = args.iters
    only = set(filter(None, args.systems.split(",")))
    results = []
    for name, n, r, c, v in systems():
        if only and name not in only:
            continue
        h = pyhispmv.FpgaHandle("bench.xclbin", 0, 24, 1, 1, 2, 5, True, False, True)
        idx = h.create_sparse_handle(r, c, v, n, n)
        h.load_matrices()
        info = h.matrix_info(idx)
        b = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, n).astype(np.float32)).to(dev)
        y = torch.empty_like(b)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream(device=dev)
        sid = stream.cuda_stream
        row = dict(system=name, n=n, nnz=int(info["nnz"]), format=int(info["format"]), parts=int(info["col_tiles"]), restarts={}, steps={})

        def timed(calls, per):
            t = {k: [] for k in calls}
            for f in calls.values():
                f()
            stream.synchronize()
            for _ in range(args.rounds):
                for k, f in calls.items():
                    t0 = time.perf_counter()
                    f()
                    stream.synchronize()
                    t[k].append((time.perf_counter() - t0) * 1e6 / per[k])
            med = {k: float(np.median(x)) for k, x in t.items()}
            return med, max(float((max(x) - min(x)) / np.median(x)) for x in t.values())

        with torch.cuda.stream(stream):
            bwork = solvers.workspace(h, idx, "bicgstab", dev)
            for restart in (10, 30):
                work = solvers.workspace_gmres(h, idx, restart, False, dev)
                applied = {}

                def ours(ce):
                    x, out = solvers.gmres(h, idx, b, restart=restart, rtol=0.0, max_iters=K, check_every=ce, work=work)
                    if ce == 0:
                        out = h.krylov_status(work.data_ptr(), sid)
                    applied[ce] = (out["status"], out["iterations"])

                def products():
                    for _ in range(K):
                        h.spmv_device(idx, b.data_ptr(), 0, y.data_ptr(), 1.0, 0.0, sid)
                calls = {"gmres8": lambda: ours(8), "gmres0": lambda: ours(0), "a": lambda: torch_gmres(torch, h, idx, b, K, restart),
                         "b": lambda: solvers.bicgstab(h, idx, b, rtol=0.0, max_iters=K // 2, check_every=0, work=bwork), "prod": products}
                med, spread = timed(calls, {"gmres8": K, "gmres0": K, "a": K, "b": 2 * (K // 2), "prod": K})
                row["restarts"][str(restart)] = dict(us_per_inner_iteration=med, gmres8_over_a=med["gmres8"] / med["a"], gmres0_over_a=med["gmres0"] / med["a"],
                                                     gmres0_over_b=med["gmres0"] / med["b"], not_product_share=1.0 - med["prod"] / med["gmres0"],
                                                     spread=spread, applied=applied)
                print(f'{name:14s} m={restart:2d} us/inner gmres8 {med["gmres8"]:7.1f} gmres0 {med["gmres0"]:7.1f} (a) {med["a"]:7.1f} (b)/product {med["b"]:7.1f} '
                      f'prod {med["prod"]:7.1f} | gmres8/(a) {med["gmres8"] / med["a"]:.2f} gmres0/(a) {med["gmres0"] / med["a"]:.2f} gmres0/(b) {med["gmres0"] / med["b"]:.2f} '
                      f'not-product {1.0 - med["prod"] / med["gmres0"]:.2f} spread {spread:.2f} applied {applied}', flush=True)
            # one inner iteration at depth j
            work = solvers.workspace_gmres(h, idx, 64, False, dev)
            stride, groups = (n + 3) // 4 * 4, prep.krylov_groups(n)
            basis = torch.randn(65 * stride, dtype=torch.float32, device=dev)
            out = torch.empty(65, dtype=torch.float64, device=dev)
            dwork = torch.empty(8 * 65 * groups + 16, dtype=torch.uint8, device=dev)
            reps = 20
            for j in STEPS:
                def solve(iters):
                    solvers.gmres(h, idx, b, restart=64, rtol=0.0, max_iters=iters, check_every=0, work=work)

                def dots():
                    for _ in range(reps):
                        h.dot_basis_device(n, j + 1, basis.data_ptr(), b.data_ptr(), out.data_ptr(), dwork.data_ptr(), dwork.numel(), ld_v=stride, stream=sid)

                def one_product():
                    for _ in range(reps):
                        h.spmv_device(idx, b.data_ptr(), 0, y.data_ptr(), 1.0, 0.0, sid)
                med, spread = timed({"upto": lambda: solve(j + 1), "before": lambda: solve(j), "multi_dot": dots, "prod": one_product},
                                    {"upto": 1, "before": 1, "multi_dot": reps, "prod": reps})
                step = med["upto"] - med["before"]
                row["steps"][str(j)] = dict(step_us=step, multi_dot_us=med["multi_dot"], product_us=med["prod"], rest_us=step - med["prod"] - med["multi_dot"],
                                            spread=spread)
                print(f'{name:14s} j={j:2d} step {step:7.1f} us: product {med["prod"]:6.1f}, multi-dot {med["multi_dot"]:6.1f}, '
                      f'subtract twice + rotate {step - med["prod"] - med["multi_dot"]:6.1f} (spread {spread:.2f})', flush=True)
        torch.cuda.synchronize()
        h.close()
        results.append(row)
    line = json.dumps(dict(tool="gmres_bench", iters=K, rounds=args.rounds, device=torch.cuda.get_device_name(0), results=results))
    print(line)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
