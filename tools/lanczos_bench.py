"""Times of the thick-restart Lanczos eigensolver on loaded handles (not part of bench.py).

Per system of tools/krylov_bench.py, symmetrised (A + A^T, duplicates summed: Lanczos needs a symmetric matrix), wall clock from the
first enqueue to the end of a final synchronisation on a side stream, `--rounds` times, alternately, medians and spread:
  steps    one Lanczos step at depth j = 5, 20, 63, two ways.  `lanczos_us`: step j alone, enqueued 50 times back to back on the state
           steps 0 .. j - 1 left (lanczos_steps_device(j, j + 1): the same product, dots, subtractions and normalisation each time),
           divided by 50.  `lanczos_diff_us`: the difference of two runs over steps 0 .. j and 0 .. j - 1, the median of the rounds'
           own differences -- a few percent of either timing, so the less steady figure, kept because the comparator can only be
           measured this way: `gmres_us` = gmres_device's inner iteration at the same depth, the same difference of two
           check_every = 0 solves of j + 1 and j iterations at restart 64.  `torch_us` = the same CGS2 step in torch, 20 times back
           to back (spmv_device for the product, h = V @ w and w -= V.T @ h twice, the norm and the division; no host look)
  rotate   basis_rotate_device in place for (m, keep) = (20, 12) and (64, 36) against torch.matmul on the same operands (out of place:
           torch has no in-place product)
  eigsh    solvers.eigsh with k = 4, LA, the default ncv and tol: seconds, products, cycles and status
`spread` is the largest (max - min) / median among the timings of a row.  The first system is timed once before anything is recorded.

    python tools/lanczos_bench.py [--rounds 9] [--systems a,b] [--out profiles/lanczos_bench.json]
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

DEPTHS = (5, 20, 63)
STEP_REPS = 50
ROTATIONS = ((20, 12), (64, 36))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--systems", default="")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "lanczos_bench.json"))
    args = ap.parse_args()
    import scipy.sparse as sp
    import torch
    import pyhispmv
    from hispmv_amd import solvers
    from krylov_bench import systems
    dev = torch.device("cuda", 0)
    only = set(filter(None, args.systems.split(",")))
    results = []
    todo = [sy for sy in systems() if not only or sy[0] in only]
    for warm, (name, n, r, c, v) in [(True, todo[0])] + [(False, sy) for sy in todo]:
        A = sp.coo_matrix((v, (r, c)), shape=(n, n)).tocsr()
        A = (A + A.T).tocoo()
        h = pyhispmv.FpgaHandle("bench.xclbin", 0, 24, 1, 1, 2, 5, True, False, True)
        idx = h.create_sparse_handle(A.row, A.col, A.data.astype(np.float32), n, n)
        h.load_matrices()
        info = h.matrix_info(idx)
        b = torch.from_numpy(np.random.default_rng(1).standard_normal(n).astype(np.float32)).to(dev)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream(device=dev)
        sid = stream.cuda_stream
        row = dict(system=name, n=n, nnz=int(info["nnz"]), format=int(info["format"]), steps={}, rotate={})

        def timed(calls, per, diffs=()):
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
            for a, b in diffs:          # a step: the median of the rounds' own differences, which a drift between rounds cancels out of
                med[a + "-" + b] = float(np.median(np.array(t[a]) - np.array(t[b])))
            return med, max(float((max(x) - min(x)) / np.median(x)) for x in t.values())

        with torch.cuda.stream(stream):
            li = h.lanczos_info(idx, 64)
            stride = li["stride"]
            lwork = torch.empty(li["work_bytes"], dtype=torch.uint8, device=dev)
            gwork = solvers.workspace_gmres(h, idx, 64, False, dev)
            basis = torch.randn(65, stride, dtype=torch.float32, device=dev)
            basis /= torch.linalg.vector_norm(basis, dim=1, keepdim=True)
            reps = 20
            for j in DEPTHS:
                def lanczos(upto):
                    h.lanczos_steps_device(idx, 0, upto, True, b.data_ptr(), lwork.data_ptr(), li["work_bytes"], sid)

                def gmres(iters):
                    solvers.gmres(h, idx, b, restart=64, rtol=0.0, max_iters=iters, check_every=0, work=gwork)

                def torch_step():
                    B, w = basis[:j + 1], basis[j + 1]
                    for _ in range(reps):
                        h.spmv_device(idx, basis[j].data_ptr(), 0, w.data_ptr(), 1.0, 0.0, sid)
                        h1 = B @ w
                        w.sub_(B.T @ h1)
                        h2 = B @ w
                        w.sub_(B.T @ h2)
                        w.div_(torch.linalg.vector_norm(w))
                def one_step():
                    for _ in range(STEP_REPS):
                        h.lanczos_steps_device(idx, j, j + 1, False, 0, lwork.data_ptr(), li["work_bytes"], sid)
                lanczos(j)          # the state one_step repeats step j on
                stream.synchronize()
                direct, direct_spread = timed({"step": one_step}, {"step": STEP_REPS})
                calls = {"l_upto": lambda: lanczos(j + 1), "l_before": lambda: lanczos(j), "g_upto": lambda: gmres(j + 1), "g_before": lambda: gmres(j),
                         "torch": torch_step}
                med, spread = timed(calls, {"l_upto": 1, "l_before": 1, "g_upto": 1, "g_before": 1, "torch": reps}, (("l_upto", "l_before"), ("g_upto", "g_before")))
                ours, diff, theirs = direct["step"], med["l_upto-l_before"], med["g_upto-g_before"]
                row["steps"][str(j)] = dict(lanczos_us=ours, lanczos_spread=direct_spread, lanczos_diff_us=diff, gmres_us=theirs, torch_us=med["torch"],
                                            lanczos_over_gmres=ours / theirs if theirs > 0 else None, lanczos_over_torch=ours / med["torch"], spread=spread,
                                            status=h.lanczos_status(lwork.data_ptr(), sid))
                print(f'{name:14s} j={j:2d} step: lanczos {ours:7.1f} us (spread {direct_spread:.2f}; by difference {diff:7.1f}), gmres by difference {theirs:7.1f} us, '
                      f'torch {med["torch"]:7.1f} us (spread {spread:.2f})', flush=True)
            for m, keep in ROTATIONS:
                Yt = torch.linalg.qr(torch.randn(m, m, dtype=torch.float32, device=dev))[0][:keep].contiguous()
                V = basis[:m + 1].clone()
                out = torch.empty(keep, stride, dtype=torch.float32, device=dev)

                def ours_rotate():
                    for _ in range(reps):
                        h.basis_rotate_device(n, m, keep, V.data_ptr(), Yt.data_ptr(), V.data_ptr(), ld_v=stride, ld_out=stride, stream=sid)

                def torch_rotate():
                    for _ in range(reps):
                        torch.matmul(Yt, V[:m], out=out)
                med, spread = timed({"ours": ours_rotate, "torch": torch_rotate}, {"ours": reps, "torch": reps})
                gbs = (m + keep) * n * 4 / med["ours"] / 1e3
                row["rotate"][f"{m},{keep}"] = dict(ours_us=med["ours"], torch_us=med["torch"], ours_over_torch=med["ours"] / med["torch"], ours_gb_per_s=gbs,
                                                    spread=spread)
                print(f'{name:14s} rotate ({m}, {keep}): ours {med["ours"]:7.1f} us ({gbs:6.0f} GB/s), torch.matmul {med["torch"]:7.1f} us (spread {spread:.2f})',
                      flush=True)
            times, last = [], None
            for _ in range(args.rounds + 1):
                stream.synchronize()
                t0 = time.perf_counter()
                vals, vecs, out = solvers.eigsh(h, idx, 4, which="LA", v0=b, max_products=4000)
                stream.synchronize()
                times.append(time.perf_counter() - t0)
                last = out
            row["eigsh"] = dict(seconds=float(np.median(times[1:])), spread=float((max(times[1:]) - min(times[1:])) / np.median(times[1:])), status=last["status"],
                                found=last["found"], products=last["products"], cycles=last["cycles"], vals=[float(x) for x in vals])
            print(f'{name:14s} eigsh k=4 LA: {row["eigsh"]["seconds"] * 1e3:8.2f} ms, {last["status"]}, {last["products"]} products, {last["cycles"]} cycles', flush=True)
        torch.cuda.synchronize()
        h.close()
        if not warm:
            results.append(row)
    line = json.dumps(dict(tool="lanczos_bench", rounds=args.rounds, device=torch.cuda.get_device_name(0), results=results))
    print(line)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
