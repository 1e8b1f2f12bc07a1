"""Several vectors per pass on device pointers against one call per vector, and against the host-pointer `linear` (not part of bench.py).

Per matrix and B in --vecs, timed with HIP events around `--reps` back-to-back calls on one stream after warm-up, `--rounds` times,
alternately (medians and spread):
  (a)  linear_device    (B vectors)   against  (a1) B calls of spmv_device       y = A x + bias      (alpha = beta = 1);
  (b)  linear_device_t  (B vectors)   against  (b1) B calls of spmv_device_t     y = A^T x           (alpha = 1, beta = 0);
  (c)  linear           (B host vectors, the activations cross PCIe twice): host clock around calls that return synchronised.
(a1) and (b1) run the single-vector entries only, so they are the times of the library before the multi-vector entries existed.
Matrices: the two seeded sparse layers and the dense layer of examples/model_check.py (hispmv_amd.matrices.model_test_layers; the
sparse ones created with set_transposable on; the 8192 x 8192 one gets a window, the 1024 x 8192 one does not), the 8192 x 8192 layer
again with bf16 values (half groups), and the scattered analytics stand-in, whose plan has no window -- every plan class of the
transposed pass (window, half, no window, dense) is there.
`spread` is the largest (max - min) / median over the rounds of the two timings a ratio is made of: a ratio closer to 1 than that is
not a difference.  Prints a table and one JSON line, and writes the line to --out.

    python tools/linear_device_bench.py [--rounds 5] [--reps 10] [--vecs 1,2,4,8,32] [--out profiles/linear_device_bench.json]
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


def time_calls(torch, stream, call, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps          # microseconds per call


def plan_class(info, storage):
    if info["is_dense"]:
        return "dense"
    if info["lds_bytes"] == 0:
        return "no window"
    return "half" if storage["storage"] == "bf16" and storage["slots_2byte"] > 0 else "window"


def measure(torch, h, name, idx, B, rounds, reps):
    dev = torch.device("cuda", 0)
    info = h.matrix_info(idx)
    rows, cols = info["rows"], info["cols"]
    xc = torch.rand((B, cols), dtype=torch.float32, device=dev)
    xr = torch.rand((B, rows), dtype=torch.float32, device=dev)
    bias = torch.rand(rows, dtype=torch.float32, device=dev)
    yr = torch.empty((B, rows), dtype=torch.float32, device=dev)
    yc = torch.empty((B, cols), dtype=torch.float32, device=dev)
    yr1, yc1 = torch.empty_like(yr), torch.empty_like(yc)
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream
    px, pr, pb = xc.data_ptr(), xr.data_ptr(), bias.data_ptr()

    def a1():
        for v in range(B):
            h.spmv_device(idx, px + 4 * v * cols, pb, yr1.data_ptr() + 4 * v * rows, 1.0, 1.0, s)

    def b1():
        for v in range(B):
            h.spmv_device_t(idx, pr + 4 * v * rows, 0, yc1.data_ptr() + 4 * v * cols, 1.0, 0.0, s)

    calls = dict(a=lambda: h.linear_device(idx, px, B, pb, yr.data_ptr(), 1.0, 1.0, s), a1=a1,
                 b=lambda: h.linear_device_t(idx, pr, B, 0, yc.data_ptr(), 1.0, 0.0, 0, s), b1=b1)
    torch.cuda.synchronize()
    t = {k: [] for k in calls}
    for f in calls.values():
        time_calls(torch, stream, f, 3)
    for _ in range(rounds):
        for k, f in calls.items():
            t[k].append(time_calls(torch, stream, f, reps))
    torch.cuda.synchronize()
    # the results of the timed calls: multi-vector against per-vector, on the scale of the largest entry
    diff_a = float((yr - yr1).abs().max() / yr1.abs().max().clamp_min(1e-30))
    diff_b = float((yc - yc1).abs().max() / yc1.abs().max().clamp_min(1e-30))
    xh, bh = xc.cpu().numpy().reshape(-1), bias.cpu().numpy()
    h.linear(idx, xh, bh)
    host = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(reps):
            h.linear(idx, xh, bh)
        host.append((time.perf_counter() - t0) * 1e6 / reps)
    med = {k: float(np.median(v)) for k, v in t.items()}
    rel = {k: float((max(v) - min(v)) / np.median(v)) for k, v in t.items()}
    return dict(name=name, plan_class=plan_class(info, h.value_storage_info(idx)), rows=rows, cols=cols, nnz=info["nnz"], B=B,
                block_threads=info["block_threads"], lds_bytes=info["lds_bytes"], parts=info["col_tiles"], linear_info=h.linear_info(idx, B),
                linear_device_us=med["a"], spmv_device_x_B_us=med["a1"], linear_device_t_us=med["b"], spmv_device_t_x_B_us=med["b1"],
                linear_host_us=float(np.median(host)), speedup_forward=med["a1"] / med["a"], speedup_transposed=med["b1"] / med["b"],
                spread_forward=max(rel["a"], rel["a1"]), spread_transposed=max(rel["b"], rel["b1"]),
                range_us={k: [float(min(v)), float(max(v))] for k, v in t.items()}, max_rel_diff_forward=diff_a, max_rel_diff_transposed=diff_b)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--vecs", default="1,2,4,8,32")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    vecs = [int(v) for v in a.vecs.split(",")]
    import torch
    import pyhispmv
    from hispmv_amd import matrices as M

    h = pyhispmv.FpgaHandle("bench.xclbin", 0, 24, 1, 1, 2, 5, True, False, True)
    h.set_arena_bytes(64 << 30)
    todo = []
    try:
        h.set_transposable(True)
        layers = M.model_test_layers()
        for kind, w, rows, cols, _b in layers[1:]:
            todo.append((f"sparse layer {rows} x {cols}", h.create_sparse_handle(*w, rows, cols)))
        kind, w, rows, cols, _b = layers[1]
        h.set_value_storage("bf16")
        todo.append((f"sparse layer {rows} x {cols}, bf16", h.create_sparse_handle(*w, rows, cols)))
        h.set_value_storage("fp32")
        kind, W, rows, cols, _b = layers[0]
        todo.append((f"dense layer {rows} x {cols}", h.create_dense_handle(W.reshape(-1), rows, cols)))
        rows, cols, rp, ci, va, _src = M.suitesparse_standin("analytics")
        r = np.repeat(np.arange(rows, dtype=np.int32), np.diff(rp).astype(np.int64))
        todo.append(("scattered, no window (analytics stand-in)", h.create_sparse_handle(r, np.asarray(ci, np.int32), np.asarray(va, np.float32), rows, cols)))
        assert all(i >= 0 for _n, i in todo), todo
        h.load_matrices()
        out = [measure(torch, h, name, i, B, a.rounds, a.reps) for name, i in todo for B in vecs]
    finally:
        h.close()
    print(f"{'matrix':42s} {'class':>9s} {'B':>3s} {'w':>2s} {'wT':>2s} {'(a) us':>9s} {'B x spmv':>9s} {'a1/a':>5s} {'spread':>6s} {'(b) us':>9s} {'B x spmvT':>9s} {'b1/b':>5s} "
          f"{'spread':>6s} {'(c) us':>9s}")
    for q in out:
        li = q["linear_info"]
        print(f"{q['name'][:42]:42s} {q['plan_class']:>9s} {q['B']:3d} {li['width']:2d} {li['width_t']:2d} {q['linear_device_us']:9.1f} {q['spmv_device_x_B_us']:9.1f} "
              f"{q['speedup_forward']:5.2f} {q['spread_forward']:6.2f} {q['linear_device_t_us']:9.1f} {q['spmv_device_t_x_B_us']:9.1f} {q['speedup_transposed']:5.2f} "
              f"{q['spread_transposed']:6.2f} {q['linear_host_us']:9.1f}")
    line = json.dumps({"linear_device_bench": out, "rounds": a.rounds, "reps": a.reps, "device": torch.cuda.get_device_name(0)})
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
