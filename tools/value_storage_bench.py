"""bf16 value storage against fp32 storage (hispmv_set_value_storage; not part of bench.py).

An fp32 and a bf16 handle of the same matrix in ONE context, timed alternately with hispmv_time_device (several rounds; medians
and spread), for:
  * the three layers of examples/model_check.py as hispmv_amd.matrices.model_test_layers seeds them: dense 8192 x 4096, sparse
    8192 x 8192 (density 0.1), sparse 1024 x 8192 (density 0.25);
  * an all-compact band matrix whose fp32 stream (>= 512 MiB) does not stay in the 256 MB last-level cache;
  * two stand-ins of the benchmark set: a mesh matrix whose groups are compact, and a tile-stream matrix as the control that
    must not move.
Next to every measured time ratio stands the BYTE RATIO computed from the layouts (stream bytes bf16 / fp32: the floor the time
ratio can approach -- 4/6 for an all-compact matrix, 1/2 for dense, 1 for the control).  Prints one JSON line and writes it to --out.

    python tools/value_storage_bench.py [--rounds 9] [--reps 20] [--big-rows 6000000] [--out profiles/value_storage.json]
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


def band(rows, per_row, half, seed=3):
    rng = np.random.default_rng(seed)
    r = np.repeat(np.arange(rows, dtype=np.int64), per_row)
    c = np.clip(r + rng.integers(-half, half + 1, size=r.size), 0, rows - 1)
    return r.astype(np.int32), c.astype(np.int32)


def stream_bytes(info, storage):
    """Bytes one SpMV streams from the handle's matrix layout (values + metas; headers, x and y left out on both sides)."""
    if info["is_dense"]:
        return info["rows"] * info["cols"] * (2 if storage["storage"] == "bf16" else 4)
    if info["format"] == 1:
        return info["n_slices"] * SLICE_BYTES["wide"]
    compact = info["compact_slices"]
    return compact * SLICE_BYTES["half" if storage["storage"] == "bf16" else "compact"] + (info["n_slices"] - compact) * SLICE_BYTES["wide"]


def measure(torch, h, name, i_fp32, i_bf16, rounds, reps):
    dev = torch.device("cuda", 0)
    info = h.matrix_info(i_fp32)
    dx = torch.rand(info["cols"], dtype=torch.float32, device=dev)
    db = torch.rand(info["rows"], dtype=torch.float32, device=dev)
    dy = torch.empty(info["rows"], dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    t = {i_fp32: [], i_bf16: []}
    for i in (i_fp32, i_bf16):
        h.time_device(i, dx.data_ptr(), db.data_ptr(), dy.data_ptr(), 1.0, 1.0, 3)
    for _ in range(rounds):
        for i in (i_fp32, i_bf16):
            t[i].append(h.time_device(i, dx.data_ptr(), db.data_ptr(), dy.data_ptr(), 1.0, 1.0, reps) * 1e3)
    f, b = np.array(t[i_fp32]), np.array(t[i_bf16])
    bf, bb = stream_bytes(info, h.value_storage_info(i_fp32)), stream_bytes(h.matrix_info(i_bf16), h.value_storage_info(i_bf16))
    return dict(name=name, format=info["format"], tile_kind=info["tile_kind"], n_slices=info["n_slices"], compact_slices=info["compact_slices"],
                fp32_us=float(np.median(f)), fp32_us_min=float(f.min()), fp32_us_max=float(f.max()),
                bf16_us=float(np.median(b)), bf16_us_min=float(b.min()), bf16_us_max=float(b.max()),
                time_ratio=float(np.median(b) / np.median(f)), byte_ratio=bb / bf, fp32_stream_bytes=int(bf), bf16_stream_bytes=int(bb),
                fp32_tbps=bf / (float(np.median(f)) * 1e-6) / 1e12, bf16_tbps=bb / (float(np.median(b)) * 1e-6) / 1e12)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--big-rows", type=int, default=6000000, help="rows of the all-compact band matrix (16 entries per row)")
    ap.add_argument("--standins", default="crankseg_2,ASIC_680k", help="benchmark-set stand-ins: an all-compact one, a tile-stream control")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import pyhispmv
    from hispmv_amd import matrices as M

    h = pyhispmv.FpgaHandle("bench.xclbin", 0, 24, 1, 1, 2, 5, True, False, True)
    h.set_arena_bytes(64 << 30)
    pairs = []

    def both(name, create):
        idx = []
        for storage in ("fp32", "bf16"):
            h.set_value_storage(storage)
            idx.append(create())
        assert min(idx) >= 0, name
        pairs.append((name, idx[0], idx[1]))

    try:
        for k, (kind, W, rows, cols, _b) in enumerate(M.model_test_layers()):
            if kind == "dense":
                both(f"model layer {k}: dense {rows} x {cols}", lambda: h.create_dense_handle(W.reshape(-1), rows, cols))
            else:
                both(f"model layer {k}: sparse {rows} x {cols}", lambda: h.create_sparse_handle(W[0], W[1], W[2], rows, cols))
        r, c = band(a.big_rows, 16, 400)
        v = np.random.default_rng(3).random(r.size, dtype=np.float32) - np.float32(0.5)
        both(f"band {a.big_rows} x 16", lambda: h.create_sparse_handle(r, c, v, a.big_rows, a.big_rows))
        del r, c, v
        for m in M.benchmark_set(names=[n for n in a.standins.split(",") if n]):
            if "rp" in m:
                both(f"{m['name']} ({m['source']})", lambda: h.create_sparse_handle_from_csr(m["rp"], m["ci"], m["va"], m["rows"], m["cols"]))
            else:
                both(f"{m['name']} ({m['source']})", lambda: h.create_sparse_handle_from_mtx(m["path"]))
        h.load_matrices()
        rows_out = [measure(torch, h, name, i, j, a.rounds, a.reps) for name, i, j in pairs]
    finally:
        h.close()
    print(f"{'matrix':58s} {'fp32 us':>9s} {'bf16 us':>9s} {'time':>6s} {'bytes':>6s}")
    for q in rows_out:
        print(f"{q['name'][:58]:58s} {q['fp32_us']:9.1f} {q['bf16_us']:9.1f} {q['time_ratio']:6.3f} {q['byte_ratio']:6.3f}")
    line = json.dumps({"value_storage_bench": rows_out, "rounds": a.rounds, "reps": a.reps, "device": torch.cuda.get_device_name(0)})
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
