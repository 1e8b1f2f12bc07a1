"""The value gradient on device pointers beside the forward and transposed products of the same handle, and beside the torch route
(not part of bench.py; built the way tools/linear_device_bench.py measures).

Per matrix and B in --vecs, timed with HIP events around `--reps` back-to-back calls on one stream after warm-up, `--rounds` times,
alternately (medians and spread):
  (g)  value_grad_device  (B vectors, alpha = 1, beta = 0)       grad[k] = sum_v gy[v, r_k] x[v, c_k]
  (a)  linear_device      (B vectors, alpha = beta = 1)          the forward product of the same handle: a yardstick
  (b)  linear_device_t    (B vectors, alpha = 1, beta = 0)       the transposed product of the same handle: a yardstick
  (t)  torch              (gy.T @ x)[r, c]                       the dense rows x cols product and a gather, the only route without (g)
Matrices: the two seeded sparse layers of examples/model_check.py (hispmv_amd.matrices.model_test_layers; created with
set_transposable and set_value_updates on) and one dense shape, 1024 x 4096.
--bf16: every matrix a second time with bf16 value storage (set_value_updates("any_storage")), measured in the same run beside its
fp32 twin (rows named `... bf16`); the gradient reads no values, so what differs is the slice stride and the 8-of-16-byte meta pieces.
`spread` is the largest (max - min) / median over the rounds of (g): a ratio closer to 1 than that is not a difference.  Prints a
table and one JSON line, and writes the line to --out.

    python tools/value_grad_bench.py [--rounds 5] [--reps 10] [--vecs 1,4,16,64] [--bf16] [--out profiles/value_grad_bench.json]
"""
from __future__ import annotations

import argparse
import json
import sys
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


def measure(torch, h, name, idx, r, c, B, rounds, reps):
    dev = torch.device("cuda", 0)
    info = h.matrix_info(idx)
    rows, cols = info["rows"], info["cols"]
    n = h.value_update_info(idx)["n"]
    x = torch.rand((B, cols), dtype=torch.float32, device=dev)
    gy = torch.rand((B, rows), dtype=torch.float32, device=dev)
    bias = torch.rand(rows, dtype=torch.float32, device=dev)
    y = torch.empty((B, rows), dtype=torch.float32, device=dev)
    gx = torch.empty((B, cols), dtype=torch.float32, device=dev)
    grad = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
    ri, ci = torch.from_numpy(r.astype(np.int64)).to(dev), torch.from_numpy(c.astype(np.int64)).to(dev)
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream
    keep = {}

    def t_route():
        keep["t"] = (gy.T @ x)[ri, ci]

    calls = dict(g=lambda: h.value_grad_device(idx, gy.data_ptr(), x.data_ptr(), B, grad.data_ptr(), 1.0, 0.0, s),
                 a=lambda: h.linear_device(idx, x.data_ptr(), B, bias.data_ptr(), y.data_ptr(), 1.0, 1.0, s),
                 b=lambda: h.linear_device_t(idx, gy.data_ptr(), B, 0, gx.data_ptr(), 1.0, 0.0, 0, s), t=t_route)
    torch.cuda.synchronize()
    t = {k: [] for k in calls}
    for f in calls.values():
        time_calls(torch, stream, f, 3)
    for _ in range(rounds):
        for k, f in calls.items():
            t[k].append(time_calls(torch, stream, f, reps))
    torch.cuda.synchronize()
    # the result of the timed calls against the torch route, on the scale of the largest entry
    diff = float((grad - keep["t"]).abs().max() / keep["t"].abs().max().clamp_min(1e-30))
    med = {k: float(np.median(v)) for k, v in t.items()}
    spread = float((max(t["g"]) - min(t["g"])) / med["g"])
    # bytes the gradient kernel moves per call: metas + map + grad written per stored slot and pass (sparse), grad written (dense)
    gi = h.value_grad_info(idx, B)
    if info["is_dense"]:
        moved = 4 * n
    else:
        slots = info["n_slices"] * 1024
        meta = 2 * info["compact_slices"] * 1024 + 4 * (info["n_slices"] - info["compact_slices"]) * 1024
        moved = gi["passes"] * (meta + 4 * slots + 4 * n) + (gi["passes"] - 1) * 4 * n
    return dict(name=name, rows=rows, cols=cols, n=n, B=B, dense=bool(info["is_dense"]), block_threads=info["block_threads"], lds_bytes=info["lds_bytes"],
                parts=info["col_tiles"], value_grad_info=gi, value_grad_us=med["g"], linear_device_us=med["a"], linear_device_t_us=med["b"], torch_us=med["t"],
                grad_over_forward=med["g"] / med["a"], grad_over_transposed=med["g"] / med["b"], torch_over_grad=med["t"] / med["g"], spread=spread,
                gbytes_per_s=moved / med["g"] * 1e-3, range_us={k: [float(min(v)), float(max(v))] for k, v in t.items()}, max_rel_diff_torch=diff)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--vecs", default="1,4,16,64")
    ap.add_argument("--bf16", action="store_true", help="also measure every matrix with bf16 value storage, in the same run")
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
        h.set_value_updates("any_storage" if a.bf16 else True)
        rows_d, cols_d = 1024, 4096
        W = (np.random.default_rng(3).random((rows_d, cols_d), dtype=np.float32) - np.float32(0.5)) * np.float32(0.05)
        k = np.arange(rows_d * cols_d, dtype=np.int64)
        for storage in ("fp32", "bf16") if a.bf16 else ("fp32",):
            h.set_value_storage(storage)
            tag = " bf16" if storage == "bf16" else ""
            for kind, w, rows, cols, _b in M.model_test_layers()[1:]:
                todo.append((f"sparse layer {rows} x {cols}{tag}", h.create_sparse_handle(*w, rows, cols), w[0], w[1]))
            todo.append((f"dense {rows_d} x {cols_d}{tag}", h.create_dense_handle(W.reshape(-1), rows_d, cols_d), k // cols_d, k % cols_d))
        assert all(q[1] >= 0 for q in todo), todo
        h.load_matrices()
        out = [measure(torch, h, name, i, r, c, B, a.rounds, a.reps) for name, i, r, c in todo for B in vecs]
    finally:
        h.close()
    print(f"{'matrix':28s} {'B':>3s} {'w':>2s} {'pass':>4s} {'(g) us':>9s} {'spread':>6s} {'GB/s':>7s} {'(a) us':>9s} {'g/a':>5s} {'(b) us':>9s} {'g/b':>5s} {'(t) us':>9s} {'t/g':>6s}")
    for q in out:
        gi = q["value_grad_info"]
        print(f"{q['name'][:28]:28s} {q['B']:3d} {gi['width']:2d} {gi['passes']:4d} {q['value_grad_us']:9.1f} {q['spread']:6.2f} {q['gbytes_per_s']:7.0f} "
              f"{q['linear_device_us']:9.1f} {q['grad_over_forward']:5.2f} {q['linear_device_t_us']:9.1f} {q['grad_over_transposed']:5.2f} "
              f"{q['torch_us']:9.1f} {q['torch_over_grad']:6.2f}")
    line = json.dumps({"value_grad_bench": out, "rounds": a.rounds, "reps": a.reps, "device": torch.cuda.get_device_name(0)})
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
