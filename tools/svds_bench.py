"""Times of the thick-restart Golub-Kahan singular-value solver on loaded handles (not part of bench.py).

Matrices: the rectangular model layers (1024 x 8192 and 8192 x 8192 at density 0.1, random pattern, standard normal values scaled by
1 / sqrt(density * cols)), each created twice -- under set_transposable("companion") (both products in a fixed order) and under
set_transposable(True) (the transposed product through atomics) -- and the first two systems of tools/krylov_bench.py (companion).
Wall clock from the first enqueue to the end of a final synchronisation on a side stream, `--rounds` times, alternately, medians and
spread:
  steps    one Golub-Kahan step (two products, CGS2 on both sides) at depth j = 20 and 63.  `gk_us`: step j alone, enqueued 20 times back
           to back on the state steps 0 .. j - 1 left (gk_steps_device(64, j, j + 1)), divided by 20.  `torch_us` = the same step in
           torch, 20 times back to back (spmv_device and spmv_device_t for the products, g = W @ w and w -= W.T @ g twice per side, the
           norm and the division; no host look)
  svds     solvers.svds with k = 4, the default ncv and tol, against `torch_svds`: the same thick-restart loop with those torch steps,
           numpy's SVD of the projected matrix and torch.matmul for the rotations, one host look per cycle -- seconds, products,
           cycles and status of both
`spread` is the largest (max - min) / median among the timings of a row.  The first matrix is timed once before anything is recorded.

    python tools/svds_bench.py [--rounds 5] [--only a,b] [--out profiles/svds_bench.json]
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

DEPTHS = (20, 63)
STEP_REPS = 20
DENSITY = 0.1


def layer(rows, cols, seed):
    rng = np.random.default_rng(seed)
    r, c = np.nonzero(rng.random((rows, cols), dtype=np.float32) < DENSITY)
    return r, c, (rng.standard_normal(len(r)) / np.sqrt(DENSITY * cols)).astype(np.float32)


def matrices():
    from krylov_bench import systems
    for rows, cols in ((1024, 8192), (8192, 8192)):
        r, c, v = layer(rows, cols, rows + cols)
        for mode in ("companion", True):
            yield f"layer_{rows}x{cols}_{'companion' if mode == 'companion' else 'atomics'}", rows, cols, r, c, v, mode
    for k, (name, n, r, c, v) in enumerate(systems()):
        if k < 2:
            yield name, n, n, r, c, v, "companion"


def torch_svds(torch, h, idx, rows, cols, v0, k, ncv, tol, max_products, sid):
    """Thick-restart Golub-Kahan with the library's products and torch vector ops on the current stream: (s, info)."""
    dev = v0.device
    V = torch.zeros(ncv + 1, cols, dtype=torch.float32, device=dev)
    U = torch.zeros(ncv, rows, dtype=torch.float32, device=dev)
    V[0] = v0 / torch.linalg.vector_norm(v0)
    B = np.zeros((ncv, ncv))
    G = torch.zeros(ncv, ncv, dtype=torch.float32, device=dev)          # column j: the U-side coefficients of step j
    ab = torch.zeros(2, ncv, dtype=torch.float32, device=dev)
    j0 = products = cycles = 0
    keep = min(k + (ncv - k) // 2, ncv - 1)
    while True:
        for j in range(j0, ncv):
            u, w = U[j], V[j + 1]
            h.spmv_device(idx, V[j].data_ptr(), 0, u.data_ptr(), 1.0, 0.0, sid)
            if j:
                W = U[:j]
                g1 = W @ u
                u.sub_(W.T @ g1)
                g2 = W @ u
                u.sub_(W.T @ g2)
                G[:j, j] = g1 + g2
            ab[0, j] = torch.linalg.vector_norm(u)
            u.div_(ab[0, j])
            h.spmv_device_t(idx, u.data_ptr(), 0, w.data_ptr(), 1.0, 0.0, sid)
            W = V[:j + 1]
            w.sub_(W.T @ (W @ w))
            w.sub_(W.T @ (W @ w))
            ab[1, j] = torch.linalg.vector_norm(w)
            w.div_(ab[1, j])
        products += 2 * (ncv - j0)
        cycles += 1
        Gh, abh = G.cpu().numpy().astype(np.float64), ab.cpu().numpy().astype(np.float64)          # the host look
        for j in range(j0, ncv):
            B[:j, j] = Gh[:j, j]
            B[j, j] = abh[0, j]
        P, s, Qt = np.linalg.svd(B)
        res = abh[1, ncv - 1] * np.abs(P[ncv - 1, :k])
        if (res <= tol * s[0]).all() or products >= max_products:
            return s[:k], dict(status="CONVERGED" if (res <= tol * s[0]).all() else "MAX_ITERS", products=products, cycles=cycles)
        last = V[ncv].clone()
        U[:keep] = torch.from_numpy(P[:, :keep].T.astype(np.float32)).to(dev) @ U[:ncv]
        V[:keep] = torch.from_numpy(Qt[:keep].astype(np.float32)).to(dev) @ V[:ncv]
        V[keep] = last
        B[:] = 0.0
        B[np.arange(keep), np.arange(keep)] = s[:keep]
        j0 = keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "svds_bench.json"))
    args = ap.parse_args()
    import torch
    import pyhispmv
    from hispmv_amd import solvers
    dev = torch.device("cuda", 0)
    only = set(filter(None, args.only.split(",")))
    todo = [m for m in matrices() if not only or m[0] in only]
    results = []
    for warm, (name, rows, cols, r, c, v, mode) in [(True, todo[0])] + [(False, m) for m in todo]:
        h = pyhispmv.FpgaHandle("bench.xclbin", 0, 24, 1, 1, 2, 5, True, False, True)
        h.set_transposable(mode)
        idx = h.create_sparse_handle(r, c, v, rows, cols)
        h.load_matrices()
        info = h.matrix_info(idx)
        v0 = torch.from_numpy(np.random.default_rng(1).standard_normal(cols).astype(np.float32)).to(dev)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream(device=dev)
        sid = stream.cuda_stream
        row = dict(matrix=name, rows=rows, cols=cols, nnz=int(info["nnz"]), format=int(info["format"]), companion=mode == "companion", steps={})

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
            return {k: float(np.median(x)) for k, x in t.items()}, max(float((max(x) - min(x)) / np.median(x)) for x in t.values())

        with torch.cuda.stream(stream):
            gi = h.gk_info(idx, 64)
            work = torch.empty(gi["work_bytes"], dtype=torch.uint8, device=dev)
            Vb = torch.randn(65, cols, dtype=torch.float32, device=dev)
            Ub = torch.randn(64, rows, dtype=torch.float32, device=dev)
            Vb /= torch.linalg.vector_norm(Vb, dim=1, keepdim=True)
            Ub /= torch.linalg.vector_norm(Ub, dim=1, keepdim=True)
            for j in DEPTHS:
                def gk_step():
                    for _ in range(STEP_REPS):
                        h.gk_steps_device(idx, 64, j, j + 1, False, 0, work.data_ptr(), gi["work_bytes"], sid)

                def torch_step():
                    for _ in range(STEP_REPS):
                        u, w = Ub[j], Vb[j + 1]
                        h.spmv_device(idx, Vb[j].data_ptr(), 0, u.data_ptr(), 1.0, 0.0, sid)
                        W = Ub[:j]
                        u.sub_(W.T @ (W @ u))
                        u.sub_(W.T @ (W @ u))
                        u.div_(torch.linalg.vector_norm(u))
                        h.spmv_device_t(idx, u.data_ptr(), 0, w.data_ptr(), 1.0, 0.0, sid)
                        W = Vb[:j + 1]
                        w.sub_(W.T @ (W @ w))
                        w.sub_(W.T @ (W @ w))
                        w.div_(torch.linalg.vector_norm(w))
                h.gk_steps_device(idx, 64, 0, j, True, v0.data_ptr(), work.data_ptr(), gi["work_bytes"], sid)          # the state gk_step repeats step j on
                stream.synchronize()
                med, spread = timed({"gk": gk_step, "torch": torch_step}, {"gk": STEP_REPS, "torch": STEP_REPS})
                row["steps"][str(j)] = dict(gk_us=med["gk"], torch_us=med["torch"], gk_over_torch=med["gk"] / med["torch"], spread=spread,
                                            status=h.gk_status(work.data_ptr(), sid))
                print(f'{name:32s} j={j:2d} step: gk {med["gk"]:7.1f} us, torch {med["torch"]:7.1f} us (spread {spread:.2f})', flush=True)
            ncv = 20
            budget = min(max(20 * max(rows, cols), 2000), 20000)
            times = {"ours": [], "torch": []}
            for _ in range(args.rounds + 1):
                stream.synchronize()
                t0 = time.perf_counter()
                s, _, _, out = solvers.svds(h, idx, 4, v0=v0, max_products=budget)
                stream.synchronize()
                times["ours"].append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                ts, tout = torch_svds(torch, h, idx, rows, cols, v0, 4, ncv, 1e-5, budget, sid)
                stream.synchronize()
                times["torch"].append(time.perf_counter() - t0)
            med = {k: float(np.median(x[1:])) for k, x in times.items()}
            row["svds"] = dict(seconds=med["ours"], torch_seconds=med["torch"], ours_over_torch=med["ours"] / med["torch"],
                               spread=max(float((max(x[1:]) - min(x[1:])) / np.median(x[1:])) for x in times.values()), status=out["status"],
                               found=out["found"], products=out["products"], cycles=out["cycles"], s=[float(x) for x in s], torch_status=tout["status"],
                               torch_products=tout["products"], torch_cycles=tout["cycles"], torch_s=[float(x) for x in ts])
            print(f'{name:32s} svds k=4: {med["ours"] * 1e3:8.2f} ms, {out["status"]}, {out["products"]} products, {out["cycles"]} cycles; torch loop '
                  f'{med["torch"] * 1e3:8.2f} ms, {tout["status"]}, {tout["products"]} products', flush=True)
        torch.cuda.synchronize()
        h.close()
        if not warm:
            results.append(row)
    line = json.dumps(dict(tool="svds_bench", rounds=args.rounds, device=torch.cuda.get_device_name(0), results=results))
    print(line)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
