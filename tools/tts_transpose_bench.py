"""Transposed product, multi-vector transposed product and value gradient on a TILE STREAM against the same on the slice stream the
handle had to be forced into before (not part of bench.py).

For every stand-in of the benchmark set (hispmv_amd/matrices.py: suitesparse_standin) that the loader makes a transposed tile stream,
the matrix is created four times in one context:
  handle 1   set_transposable("keep_format"): the loader's own choice, a tile stream, accepted by the transposed entries;
  handle 2   set_transposable(True): the slice stream, the only remedy before;
  handles 3, 4   the same two with value updates on (the value gradient needs the map).
Timed with the method of tools/transpose_bench.py (time_calls: HIP events around `--reps` back-to-back launches on one stream after
warm-up, `--rounds` times, alternately; medians and spread):
  forward       spmv_device            on handles 1 and 2
  transposed    spmv_device_t          on handles 1 and 2
  linear_t4     linear_device_t, 4 vectors, on handles 1 and 2
  value_grad4   value_grad_device, 4 vectors, on handles 3 and 4
The figure to judge by is transposed on the tile stream against transposed on the slices of the same matrix.
Prints a table and one JSON line, and writes the line to --out.

    python tools/tts_transpose_bench.py [--names soc-Pokec,analytics] [--rounds 7] [--reps 20] [--out profiles/tts_transpose_bench.json]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from transpose_bench import coo_of_csr, time_calls  # noqa: E402

# the stand-ins without an x window in their slice plan (scattered, power-law, wide bands): the candidates for a tile stream
CANDIDATES = ("soc-Pokec", "ASIC_680k", "nxp1", "analytics", "boyd2", "language", "trans5")
VECS = 4


def measure(torch, h, name, ids, rounds, reps):
    dev = torch.device("cuda", 0)
    tile, slices, tile_u, slices_u = ids
    info = {k: h.matrix_info(i) for k, i in (("tile", tile), ("slices", slices))}
    rows, cols, n = info["tile"]["rows"], info["tile"]["cols"], h.value_update_info(tile_u)["n"]
    xc = torch.rand(VECS * cols, dtype=torch.float32, device=dev)
    xr = torch.rand(VECS * rows, dtype=torch.float32, device=dev)
    yr = torch.empty(rows, dtype=torch.float32, device=dev)
    yc = torch.empty(VECS * cols, dtype=torch.float32, device=dev)
    grad = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream
    calls = {}
    for kind, i, iu in (("tile", tile, tile_u), ("slices", slices, slices_u)):
        calls[f"forward_{kind}"] = lambda i=i: h.spmv_device(i, xc.data_ptr(), 0, yr.data_ptr(), 1.0, 0.0, s)
        calls[f"transposed_{kind}"] = lambda i=i: h.spmv_device_t(i, xr.data_ptr(), 0, yc.data_ptr(), 1.0, 0.0, s)
        calls[f"linear_t4_{kind}"] = lambda i=i: h.linear_device_t(i, xr.data_ptr(), VECS, 0, yc.data_ptr(), 1.0, 0.0, 0, s)
        calls[f"value_grad4_{kind}"] = lambda iu=iu: h.value_grad_device(iu, xr.data_ptr(), xc.data_ptr(), VECS, grad.data_ptr(), 1.0, 0.0, s)
    torch.cuda.synchronize()
    t = {k: [] for k in calls}
    for f in calls.values():
        time_calls(torch, stream, f, 3)
    for _ in range(rounds):
        for k, f in calls.items():
            t[k].append(time_calls(torch, stream, f, reps))
    # the two transposed products and the two gradients once against each other (the calls run on `stream`, the copies on torch's
    # current stream: every call is waited for before its result is copied)
    calls["transposed_tile"]()
    torch.cuda.synchronize()
    a = yc[:cols].clone()
    calls["transposed_slices"]()
    torch.cuda.synchronize()
    diff_t = float((a - yc[:cols]).abs().max() / yc[:cols].abs().max().clamp_min(1e-30))
    calls["value_grad4_tile"]()
    torch.cuda.synchronize()
    g = grad.clone()
    calls["value_grad4_slices"]()
    torch.cuda.synchronize()
    diff_g = float((g - grad).abs().max() / grad.abs().max().clamp_min(1e-30))
    med = {k: float(np.median(v)) for k, v in t.items()}
    return dict(name=name, rows=rows, cols=cols, nnz=info["tile"]["nnz"], tts_lines_per_gather=info["tile"]["tts_lines_per_gather"],
                tile=dict(format=info["tile"]["format"], group_slices=info["tile"]["group_slices"], device_bytes=info["tile"]["device_bytes"],
                          transpose_info=h.transpose_info(tile), linear_info=h.linear_info(tile, VECS), value_grad_info=h.value_grad_info(tile_u, VECS)),
                slices=dict(format=info["slices"]["format"], block_threads=info["slices"]["block_threads"], lds_bytes=info["slices"]["lds_bytes"],
                            parts=info["slices"]["col_tiles"], device_bytes=info["slices"]["device_bytes"], transpose_info=h.transpose_info(slices),
                            linear_info=h.linear_info(slices, VECS), value_grad_info=h.value_grad_info(slices_u, VECS)),
                us=med, spread_us={k: [float(min(v)), float(max(v))] for k, v in t.items()},
                tile_over_slices={k: med[f"{k}_tile"] / med[f"{k}_slices"] for k in ("forward", "transposed", "linear_t4", "value_grad4")},
                max_rel_diff_transposed=diff_t, max_rel_diff_value_grad=diff_g)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--names", default=",".join(CANDIDATES))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import pyhispmv
    from hispmv_amd import matrices as M
    from hispmv_amd import prep

    h = pyhispmv.FpgaHandle("bench.xclbin", 0, 24, 1, 1, 2, 5, True, False, True)
    h.set_arena_bytes(64 << 30)
    todo, skipped = [], []
    try:
        for name in [q for q in a.names.split(",") if q]:
            rows, cols, rp, ci, va, _src = M.suitesparse_standin(name)
            if prep.choose_format_from_csr(rp, ci, va, rows, cols, 256)["format"] != 1:
                skipped.append(name)
                continue
            r, c, v = coo_of_csr(rp, ci, va)
            ids = []
            for updates in (False, True):
                for state in ("keep_format", True):
                    h.set_value_updates(updates)
                    h.set_transposable(state)
                    ids.append(h.create_sparse_handle(r, c, v, rows, cols))
                    assert ids[-1] >= 0, name
            h.set_value_updates(False)
            h.set_transposable(False)
            assert h.matrix_info(ids[0])["format"] == 1 and h.matrix_info(ids[1])["format"] == 0, name
            todo.append((name, ids))
        h.load_matrices()
        out = [measure(torch, h, name, ids, a.rounds, a.reps) for name, ids in todo]
    finally:
        h.close()
    kinds = ("forward", "transposed", "linear_t4", "value_grad4")
    print(f"{'matrix':12s} {'lines':>6s} " + " ".join(f"{k + ' tile/slices us':>30s}" for k in kinds))
    for q in out:
        print(f"{q['name'][:12]:12s} {q['tts_lines_per_gather']:6.1f} " +
              " ".join(f"{q['us'][k + '_tile']:11.1f} /{q['us'][k + '_slices']:9.1f} ({q['tile_over_slices'][k]:4.2f})" for k in kinds))
    line = json.dumps({"tts_transpose_bench": out, "not_tile_streams": skipped, "vecs": VECS, "rounds": a.rounds, "reps": a.reps,
                       "device": torch.cuda.get_device_name(0)})
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
