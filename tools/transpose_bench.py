"""The transposed product against the forward product and against today's workaround (not part of bench.py).

Per matrix, timed with HIP events around `--reps` back-to-back launches on one stream after warm-up, `--rounds` times, alternately
(medians and spread):
  (a) spmv_device            y[rows] = A x        on the handle;
  (b) spmv_device_t          y[cols] = A^T x      on the SAME handle (hispmv_spmv_device_t);
  (c) spmv_device            on a second handle created from the swapped COO under the default switches -- what a user has to do
                             without (b): a second copy of the matrix in the arena and a second preprocessing run.
Matrices (generators of hispmv_amd/matrices.py): a windowed band (the crankseg_2 stand-in, all groups compact), the same band with
2 % of its entries re-drawn at random columns (stray slots or a stray split, as the loader decides), a scattered matrix whose
plan has no window (the analytics stand-in, created with set_transposable on: every element adds to y directly), and the
1024 x 8192 layer of model_test_layers as a dense handle -- with fp32 and with bf16 values, whole and less its last column (odd cols:
the element-load kernels).
Next to the times: what transpose_info reports, the arena bytes (c) costs, and the simple floor of (b): stream bytes / 5.6 TB/s
(what the step kernel reaches) + atomic bytes / 1.3 TB/s (the chip-wide rate of float atomic adds).
Prints one JSON line and writes it to --out.

    python tools/transpose_bench.py [--rounds 7] [--reps 20] [--out profiles/transpose_bench.json]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SLICE_BYTES = {"half": 4096, "compact": 6144, "wide": 8192}
STREAM_TBPS, ATOMIC_TBPS = 5.6, 1.3


def stream_bytes(info, storage):
    """Bytes one product streams from the handle's matrix layout (values + metas), by the handle's value storage."""
    bf16 = storage["storage"] == "bf16"
    if info["is_dense"]:
        return info["rows"] * info["cols"] * (2 if bf16 else 4)
    if info["format"] == 1:
        return info["n_slices"] * SLICE_BYTES["wide"]
    compact = info["compact_slices"]
    return compact * SLICE_BYTES["half" if bf16 else "compact"] + (info["n_slices"] - compact) * SLICE_BYTES["wide"]


def coo_of_csr(rp, ci, va):
    rows = rp.size - 1
    return np.repeat(np.arange(rows, dtype=np.int32), np.diff(rp).astype(np.int64)), np.asarray(ci, np.int32), np.asarray(va, np.float32)


def time_calls(torch, stream, call, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps          # microseconds per call


def measure(torch, h, name, i_fwd, i_swapped, swapped_bytes, rounds, reps):
    dev = torch.device("cuda", 0)
    info, ti = h.matrix_info(i_fwd), h.transpose_info(i_fwd)
    rows, cols = info["rows"], info["cols"]
    xc = torch.rand(cols, dtype=torch.float32, device=dev)
    xr = torch.rand(rows, dtype=torch.float32, device=dev)
    yr = torch.empty(rows, dtype=torch.float32, device=dev)
    yc = torch.empty(cols, dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream
    calls = dict(a=lambda: h.spmv_device(i_fwd, xc.data_ptr(), 0, yr.data_ptr(), 1.0, 0.0, s),
                 b=lambda: h.spmv_device_t(i_fwd, xr.data_ptr(), 0, yc.data_ptr(), 1.0, 0.0, s),
                 c=lambda: h.spmv_device(i_swapped, xr.data_ptr(), 0, yc.data_ptr(), 1.0, 0.0, s))
    torch.cuda.synchronize()
    t = {k: [] for k in calls}
    for k, f in calls.items():
        time_calls(torch, stream, f, 3)
    for _ in range(rounds):
        for k, f in calls.items():
            t[k].append(time_calls(torch, stream, f, reps))
    # (b) against (c) once: the two must agree within the 1e-5 gate's scale
    calls["b"]()
    yb = yc.clone()
    calls["c"]()
    torch.cuda.synchronize()
    diff = float((yb - yc).abs().max() / yc.abs().max().clamp_min(1e-30))
    med = {k: float(np.median(v)) for k, v in t.items()}
    sb = stream_bytes(info, h.value_storage_info(i_fwd))
    floor = sb / (STREAM_TBPS * 1e12) * 1e6 + ti["atomic_bytes"] / (ATOMIC_TBPS * 1e12) * 1e6
    sw = h.matrix_info(i_swapped)
    return dict(name=name, rows=rows, cols=cols, nnz=info["nnz"], is_dense=info["is_dense"], format=info["format"], tile_kind=info["tile_kind"],
                parts=info["col_tiles"], block_threads=info["block_threads"], lds_bytes=info["lds_bytes"], n_slices=info["n_slices"],
                compact_slices=info["compact_slices"], swapped_format=sw["format"], transpose_info=ti,
                forward_us=med["a"], transposed_us=med["b"], swapped_us=med["c"],
                spread_us={k: [float(min(v)), float(max(v))] for k, v in t.items()},
                b_over_a=med["b"] / med["a"], b_over_c=med["b"] / med["c"], swapped_arena_bytes=int(swapped_bytes),
                stream_bytes=int(sb), floor_us=floor, b_over_floor=med["b"] / floor, max_rel_diff_b_c=diff)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import pyhispmv
    from hispmv_amd import matrices as M

    h = pyhispmv.FpgaHandle("bench.xclbin", 0, 24, 1, 1, 2, 5, True, False, True)
    h.set_arena_bytes(64 << 30)
    todo = []

    def sparse(name, r, c, v, rows, cols, transposable):
        h.set_transposable(transposable)
        i = h.create_sparse_handle(r, c, v, rows, cols)
        h.set_transposable(False)
        before = h.arena_bytes_used()
        j = h.create_sparse_handle(c, r, v, cols, rows)          # (c): the swapped COO, default switches
        assert i >= 0 and j >= 0, name
        todo.append((name, i, j, h.arena_bytes_used() - before))

    try:
        _r, _c, rp, ci, va = M.standin_variant("crankseg_2", "base")
        sparse("windowed band (crankseg_2 stand-in)", *coo_of_csr(rp, ci, va), _r, _c, False)
        _r, _c, rp, ci, va = M.standin_variant("crankseg_2", "stray2")
        sparse("stray band (crankseg_2 stand-in, 2 % re-drawn)", *coo_of_csr(rp, ci, va), _r, _c, False)
        _r, _c, rp, ci, va, _src = M.suitesparse_standin("analytics")      # (always the seeded stand-in, also where a real file exists)
        sparse("scattered, no window (analytics stand-in)", *coo_of_csr(rp, ci, va), _r, _c, True)
        kind, (r, c, v), rows, cols, _b = M.model_test_layers()[2]
        W = np.zeros((rows, cols), np.float32)
        W[r, c] = v
        # the four dense kernels of (b): fp32 and bf16 W, vector loads (cols % 4 == 0) and element loads (the layer less its last column)
        for storage in ("fp32", "bf16"):
            for Wd in (W, np.ascontiguousarray(W[:, :-1])):
                h.set_value_storage(storage)
                i = h.create_dense_handle(Wd.reshape(-1), *Wd.shape)
                before = h.arena_bytes_used()
                j = h.create_dense_handle(np.ascontiguousarray(Wd.T).reshape(-1), *Wd.shape[::-1])
                tag = "" if storage == "fp32" else " bf16"
                todo.append((f"dense layer {Wd.shape[0]} x {Wd.shape[1]}{tag}", i, j, h.arena_bytes_used() - before))
        h.set_value_storage("fp32")
        del W
        h.load_matrices()
        out = [measure(torch, h, name, i, j, nbytes, a.rounds, a.reps) for name, i, j, nbytes in todo]
    finally:
        h.close()
    print(f"{'matrix':50s} {'(a) us':>8s} {'(b) us':>8s} {'(c) us':>8s} {'b/a':>6s} {'b/c':>6s} {'floor':>7s} {'direct':>9s} {'atomic MB':>9s} {'(c) MB':>7s}")
    for q in out:
        ti = q["transpose_info"]
        print(f"{q['name'][:50]:50s} {q['forward_us']:8.1f} {q['transposed_us']:8.1f} {q['swapped_us']:8.1f} {q['b_over_a']:6.2f} {q['b_over_c']:6.2f} "
              f"{q['floor_us']:7.1f} {ti['direct_elems']:9d} {ti['atomic_bytes'] / 1e6:9.1f} {q['swapped_arena_bytes'] / 1e6:7.1f}")
    line = json.dumps({"transpose_bench": out, "rounds": a.rounds, "reps": a.reps, "device": torch.cuda.get_device_name(0)})
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
