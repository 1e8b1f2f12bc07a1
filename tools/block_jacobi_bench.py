"""What the block-Jacobi preconditioner costs and what it buys, per system (not part of bench.py).

Systems: the seven of tools/krylov_bench.py (a small tridiagonal system and six stand-ins with random values under a dominant
diagonal), plus the two systems the preconditioner was built for, at sizes a user would run: `multidof` (tests/block_jacobi_model.py:
`--nodes` nodes of 8 unknowns, symmetric positive definite, ill-conditioned inside a node) and `convdiff` (tests/gmres_model.py:
convection-diffusion on a `--grid` x `--grid` grid at Peclet number 1000, strongly coupled along a grid line).

Per system, on a torch side stream, wall clock from the first enqueue to the end of a final synchronisation, `--rounds` rounds in which
every variant takes its turn (so drift hits all alike), medians and spread ((max - min) / median, the largest among the timings):
  setup     per block size: the extraction alone, the inversion alone (`--reps` calls back to back, per call)
  apply     per block size: one multiply z = M^-1 r (`--reps` calls back to back, per call)
  iteration CG, GMRES(10) and GMRES(30) with no preconditioner, with minv = 1 / diag, and with blocks of 4, 8, 16, 32: `--iters`
            iterations from x = 0 with rtol = 0 and check_every = 0 (nothing stops early, one synchronisation), microseconds per iteration
  solve     the same variants to `--rtol` with check_every = 8 and a budget of `--budget` iterations: status, iterations, milliseconds
A CG row on a system that is not symmetric positive definite (the stand-ins) says what CG does there, breakdown included; it is
recorded, not hidden.

    python tools/block_jacobi_bench.py [--iters 48] [--rounds 5] [--systems a,b] [--out profiles/block_jacobi_bench.json]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "tools", ROOT / "tests"):
    sys.path.insert(0, str(p))

SIZES = (4, 8, 16, 32)


def all_systems(nodes, grid):
    from krylov_bench import systems
    import block_jacobi_model as bj
    import gmres_model as gm
    yield from systems()
    for name, A in ((f"multidof_{nodes}x8", bj.multidof(nodes, 8)), (f"convdiff_{grid}_pe1000", gm.convdiff(grid, 1000))):
        A = A.tocoo()
        yield name, A.shape[0], A.row, A.col, A.data.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rtol", type=float, default=1e-6)
    ap.add_argument("--budget", type=int, default=600)
    ap.add_argument("--nodes", type=int, default=16000)
    ap.add_argument("--grid", type=int, default=384)
    ap.add_argument("--systems", default="")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "block_jacobi_bench.json"))
    args = ap.parse_args()
    import scipy.sparse as sp
    import torch
    import pyhispmv
    from hispmv_amd import prep, solvers
    dev = torch.device("cuda", 0)
    K = args.iters
    only = set(filter(None, args.systems.split(",")))
    results = []
    for name, n, r, c, v in all_systems(args.nodes, args.grid):
        if only and name not in only:
            continue
        h = pyhispmv.FpgaHandle("bench.xclbin", 0, 24, 1, 1, 2, 5, True, False, True)
        idx = h.create_sparse_handle(r, c, v, n, n)
        h.load_matrices()
        info = h.matrix_info(idx)
        row = dict(system=name, n=n, nnz=int(info["nnz"]), format=int(info["format"]), parts=int(info["col_tiles"]))
        if not h.block_jacobi_info(idx, 8)["accepted"]:          # a tile stream: the extraction refuses it
            row["refused"] = True
            results.append(row)
            print(f"{name:22s} refused (format {info['format']})", flush=True)
            h.close()
            continue
        b = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, n).astype(np.float32)).to(dev)
        diag = sp.coo_matrix((v, (r, c)), shape=(n, n)).tocsr().diagonal()
        minv = torch.from_numpy((1.0 / diag).astype(np.float32)).to(dev)
        z = torch.empty_like(b)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream(device=dev)
        sid = stream.cuda_stream

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
            pre = {bs: solvers.block_jacobi(h, idx, bs) for bs in SIZES}
            row["singular_blocks"] = {str(bs): pre[bs].singular_blocks() for bs in SIZES}
            # setup and apply
            calls, per = {}, {}
            for bs in SIZES:
                p = pre[bs]
                nb = prep.block_jacobi(n, bs)["n_blocks"]
                scratch = torch.empty_like(p.buffer)

                def extract(p=p, bs=bs, scratch=scratch):
                    for _ in range(args.reps):
                        h.block_jacobi_extract_device(idx, bs, scratch.data_ptr(), scratch.numel(), sid)

                def invert(bs=bs, scratch=scratch, nb=nb):          # (inverting an inverse: the same work on other values)
                    for _ in range(args.reps):
                        h.block_invert_device(scratch.data_ptr(), nb, bs, sid)

                def apply(p=p, bs=bs):
                    for _ in range(args.reps):
                        h.block_jacobi_apply_device(p.buffer.data_ptr(), n, bs, b.data_ptr(), z.data_ptr(), sid)
                for key, f in (("extract", extract), ("invert", invert), ("apply", apply)):
                    calls[f"{key}_{bs}"], per[f"{key}_{bs}"] = f, args.reps
            med, spread = timed(calls, per)
            row["setup_apply_us"] = dict(med, spread=spread)
            print(f"{name:22s} n {n:8d} us per call  " + "  ".join(f"bs {bs}: extract {med[f'extract_{bs}']:.1f} invert {med[f'invert_{bs}']:.1f} "
                                                                     f"apply {med[f'apply_{bs}']:.1f}" for bs in SIZES) + f"  spread {spread:.2f}", flush=True)
            # iterations and solves
            variants = [("none", {}), ("minv", dict(minv=minv))] + [(f"bs{bs}", dict(precond=pre[bs])) for bs in SIZES]
            row["solvers"] = {}
            for sname, solve, extra, with_z in (("cg", solvers.cg, {}, None), ("gmres10", solvers.gmres, dict(restart=10), 10), ("gmres30", solvers.gmres, dict(restart=30), 30)):
                works = {}
                for vname, kw in variants:
                    works[vname] = solvers.workspace(h, idx, "cg", dev) if with_z is None else solvers.workspace_gmres(h, idx, with_z, bool(kw), dev)
                outcome = {}

                def iterate(vname, kw):
                    solve(h, idx, b, rtol=0.0, max_iters=K, check_every=0, work=works[vname], **extra, **kw)

                def to_rtol(vname, kw):
                    _, out = solve(h, idx, b, rtol=args.rtol, max_iters=args.budget, check_every=8, work=works[vname], **extra, **kw)
                    outcome[vname] = (out["status"], out["iterations"], out["relres"])
                med_i, spread_i = timed({vn: (lambda vn=vn, kw=kw: iterate(vn, kw)) for vn, kw in variants}, {vn: K for vn, _ in variants})
                med_s, spread_s = timed({vn: (lambda vn=vn, kw=kw: to_rtol(vn, kw)) for vn, kw in variants}, {vn: 1000.0 for vn, _ in variants})
                row["solvers"][sname] = dict(us_per_iteration=med_i, iteration_spread=spread_i, solve_ms=med_s, solve_spread=spread_s,
                                             outcome={k: dict(status=o[0], iterations=o[1], relres=o[2]) for k, o in outcome.items()})
                print(f"{name:22s} {sname:8s} " + "  ".join(f"{vn}: {med_i[vn]:.1f} us/it, {outcome[vn][0][:4]} {outcome[vn][1]} it {med_s[vn]:.2f} ms"
                                                           for vn, _ in variants) + f"  spread {spread_i:.2f} / {spread_s:.2f}", flush=True)
        torch.cuda.synchronize()
        h.close()
        results.append(row)
    line = json.dumps(dict(tool="block_jacobi_bench", iters=K, rounds=args.rounds, reps=args.reps, rtol=args.rtol, budget=args.budget,
                           device=torch.cuda.get_device_name(0), results=results))
    print(line)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
