"""Per-iteration time of the multi-right-hand-side Krylov entries against m consecutive single-vector solves (not part of bench.py).

Per system of tools/krylov_bench.py, solver (cg, bicgstab) and m in {1, 2, 4, ..., 256}: `--iters` iterations from X = 0 with rtol = 0
(nothing stops early), wall clock from the first enqueue to the end of a final synchronisation, `--rounds` times, alternately, medians:
  multi0 / multi8    hispmv_amd.solvers.cg_multi / bicgstab_multi on B [n, m], check_every = 0 / 8
  single0 / single8  m consecutive hispmv_amd.solvers.cg / bicgstab solves on the same handle, one per column, same check_every --
                     the only route without the multi entries
  prod               the spmm_device calls of the multi iterations alone, back to back
Reported: microseconds per iteration of each (single: of all m solves together), the ratios multi / single, microseconds per vector
kernel of the multi entry = (multi0 - prod) / launches per iteration, and per system and solver the smallest m from which the multi
entry wins.  `spread` is the largest (max - min) / median among the timings of a row: a ratio closer to 1 than that is not a
difference.

    python tools/krylov_multi_bench.py [--iters 48] [--rounds 5] [--systems a,b] [--out profiles/krylov_multi_bench.json]
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
sys.path.insert(0, str(ROOT / "tools"))

WIDTHS = (1, 2, 4, 8, 16, 32, 64, 128, 256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--systems", default="")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "krylov_multi_bench.json"))
    args = ap.parse_args()
    import torch
    import pyhispmv
    from hispmv_amd import solvers
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
        Ball = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, (n, WIDTHS[-1])).astype(np.float32)).to(dev)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream(device=dev)
        row = dict(system=name, n=n, nnz=int(info["nnz"]), parts=int(info["col_tiles"]), solvers={})
        with torch.cuda.stream(stream):
            for solver in ("cg", "bicgstab"):
                multi, single = getattr(solvers, solver + "_multi"), getattr(solvers, solver)
                work1 = solvers.workspace(h, idx, solver, dev)
                per_m, wins_from = {}, None
                for m in WIDTHS:
                    B = Ball[:, :m].contiguous()
                    cols = [B[:, j].contiguous() for j in range(m)]
                    ki = h.krylov_multi_info(idx, solver, m)
                    work = solvers.workspace_multi(h, idx, solver, m, dev)
                    P, Q = torch.zeros(n, ki["ld"], dtype=torch.float32, device=dev), torch.empty(n, ki["ld"], dtype=torch.float32, device=dev)
                    pw = torch.empty(max(h.spmm_info(idx, m, ki["ld"])["work_bytes"], 16), dtype=torch.uint8, device=dev)
                    applied = {}

                    def run_multi(ce):
                        X, out = multi(h, idx, B, rtol=0.0, max_iters=K, check_every=ce, work=work)
                        its = out["iterations"] if ce else [q["iterations"] for q in h.krylov_multi_status(work.data_ptr(), m, stream.cuda_stream)]
                        applied[ce] = int(min(its))

                    def run_single(ce):
                        for b in cols:
                            single(h, idx, b, rtol=0.0, max_iters=K, check_every=ce, work=work1)

                    def products():
                        for _ in range(K * ki["products_per_iteration"]):
                            h.spmm_device(idx, P.data_ptr(), m, 0, Q.data_ptr(), 1.0, 0.0, ld_x=ki["ld"], ld_y=ki["ld"], work=pw.data_ptr(),
                                          work_bytes=pw.numel(), stream=stream.cuda_stream)
                    calls = {"multi0": lambda: run_multi(0), "multi8": lambda: run_multi(8), "single0": lambda: run_single(0),
                             "single8": lambda: run_single(8), "prod": products}
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
                    r0, r8 = med["multi0"] / med["single0"], med["multi8"] / med["single8"]
                    per_kernel = (med["multi0"] - med["prod"]) / ki["launches_per_iteration"]
                    per_m[m] = dict(us_per_iteration=med, multi0_over_single0=r0, multi8_over_single8=r8, us_per_vector_kernel=per_kernel, spread=spread,
                                    applied=applied)
                    if max(r0, r8) < 1.0:
                        wins_from = m if wins_from is None else wins_from
                    else:
                        wins_from = None
                    print(f'{name:14s} {solver:9s} m {m:3d} us/iter multi0 {med["multi0"]:8.1f} multi8 {med["multi8"]:8.1f} single0 {med["single0"]:9.1f} '
                          f'single8 {med["single8"]:9.1f} prod {med["prod"]:8.1f} | multi/single {r0:.3f} {r8:.3f} us/kernel {per_kernel:6.1f} '
                          f'spread {spread:.2f} applied {applied}', flush=True)
                    del work, P, Q, pw, B, cols
                row["solvers"][solver] = dict(widths=per_m, wins_from=wins_from)
        torch.cuda.synchronize()
        h.close()
        del Ball
        results.append(row)
    line = json.dumps(dict(tool="krylov_multi_bench", iters=K, rounds=args.rounds, device=torch.cuda.get_device_name(0), results=results))
    print(line)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
