"""The transposed product through a stored transpose ("companion") against the atomics route and against its yardstick (not part of bench.py).

Per matrix three handles are created from the same COO, all updatable: (b) under set_transposable(True), no companion; (k) under
set_transposable("companion"); (c) under set_transposable(False) from the SWAPPED COO -- what a user had to do before the companion
existed, and code the companion did not touch.  Per B in --vecs, timed with HIP events around `--reps` back-to-back calls on one
stream after warm-up, `--rounds` times, alternately (medians and spread), y = A^T x (alpha = 1, beta = 0):
  (b)  linear_device_t on the handle without a companion   (float atomics);
  (k)  linear_device_t on the handle with one              (forward launches over the stored transpose);
  (c)  linear_device   on the swapped handle               (beta = 0: a slice stream takes ONE vector per pass there, include/hispmv.h);
  (k1) and (c1): (k) and (c) with beta = 1 and a shared bias -- then both routes take the same passes, the same launches, and (k1)
       should equal (c1) within the spread.  With beta = 0 the companion route keeps its 4-2-1 passes and (k) undercuts (c) for B > 1.
Also per matrix: update_values_device on (b) and on (k) (one update writes both matrices of (k)), prep_seconds and device_bytes of
both, and whether (k) and (c) gave the same bits.
Matrices: the two seeded sparse layers of examples/model_check.py (8192 x 8192 with a window, 1024 x 8192 without), the 8192 x 8192
layer again with bf16 values, and the scattered analytics stand-in.
`spread` is the largest (max - min) / median over the rounds of the timings a ratio is made of: a ratio closer to 1 than that is not
a difference.  Prints a table and one JSON line, and writes the line to --out.

    python tools/companion_bench.py [--rounds 5] [--reps 10] [--vecs 1,4,32] [--out profiles/companion_bench.json]
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


def rounds_of(torch, stream, calls, rounds, reps):
    """-> medians and (max - min) / median per call, the calls timed alternately."""
    torch.cuda.synchronize()
    t = {k: [] for k in calls}
    for f in calls.values():
        time_calls(torch, stream, f, 3)
    for _ in range(rounds):
        for k, f in calls.items():
            t[k].append(time_calls(torch, stream, f, reps))
    torch.cuda.synchronize()
    return ({k: float(np.median(v)) for k, v in t.items()}, {k: float((max(v) - min(v)) / np.median(v)) for k, v in t.items()},
            {k: [float(min(v)), float(max(v))] for k, v in t.items()})


def describe(h, idx):
    info, ci = h.matrix_info(idx), h.companion_info(idx)
    return dict(format=info["format"], parts=info["col_tiles"], block_threads=info["block_threads"], lds_bytes=info["lds_bytes"],
                device_bytes=info["device_bytes"], prep_seconds=info["prep_seconds"], companion=ci, transpose_info=h.transpose_info(idx))


def measure(torch, h, name, hb, hk, hc, vecs, rounds, reps):
    dev = torch.device("cuda", 0)
    info = h.matrix_info(hb)
    rows, cols, n = info["rows"], info["cols"], h.value_update_info(hb)["n"]
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream
    out = dict(name=name, rows=rows, cols=cols, nnz=info["nnz"], without=describe(h, hb), with_companion=describe(h, hk), swapped=describe(h, hc), by_vecs=[])
    for B in vecs:
        x = torch.rand((B, rows), dtype=torch.float32, device=dev)
        yb, yk, yc = (torch.empty((B, cols), dtype=torch.float32, device=dev) for _ in range(3))
        yk1, yc1, bias = torch.empty_like(yk), torch.empty_like(yc), torch.rand(cols, dtype=torch.float32, device=dev)
        calls = dict(b=lambda: h.linear_device_t(hb, x.data_ptr(), B, 0, yb.data_ptr(), 1.0, 0.0, 0, s),
                     k=lambda: h.linear_device_t(hk, x.data_ptr(), B, 0, yk.data_ptr(), 1.0, 0.0, 0, s),
                     c=lambda: h.linear_device(hc, x.data_ptr(), B, 0, yc.data_ptr(), 1.0, 0.0, s),
                     k1=lambda: h.linear_device_t(hk, x.data_ptr(), B, bias.data_ptr(), yk1.data_ptr(), 1.0, 1.0, 0, s),
                     c1=lambda: h.linear_device(hc, x.data_ptr(), B, bias.data_ptr(), yc1.data_ptr(), 1.0, 1.0, s))
        med, rel, rng = rounds_of(torch, stream, calls, rounds, reps)
        out["by_vecs"].append(dict(B=B, atomics_us=med["b"], companion_us=med["k"], swapped_forward_us=med["c"], atomics_over_companion=med["b"] / med["k"],
                                   companion_over_swapped=med["k"] / med["c"], companion_bias_us=med["k1"], swapped_forward_bias_us=med["c1"],
                                   companion_over_swapped_bias=med["k1"] / med["c1"], spread=max(rel.values()), range_us=rng,
                                   linear_info=h.linear_info(hk, B), same_bits_as_swapped=bool(torch.equal(yk.view(torch.int32), yc.view(torch.int32)) and torch.equal(yk1.view(torch.int32), yc1.view(torch.int32))),
                                   max_rel_diff_to_atomics=float((yk - yb).abs().max() / yb.abs().max().clamp_min(1e-30))))
    v = torch.rand(n, dtype=torch.float32, device=dev) - 0.5
    med, rel, rng = rounds_of(torch, stream, dict(b=lambda: h.update_values_device(hb, v.data_ptr(), n, s), k=lambda: h.update_values_device(hk, v.data_ptr(), n, s)), rounds, reps)
    out["update"] = dict(without_us=med["b"], with_companion_us=med["k"], spread=max(rel.values()), range_us=rng,
                         written_without=h.value_update_info(hb)["written"], written_with=h.value_update_info(hk)["written"])
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--vecs", default="1,4,32")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    vecs = [int(v) for v in a.vecs.split(",")]
    import torch
    import pyhispmv
    from hispmv_amd import matrices as M

    layers = M.model_test_layers()
    inputs = []
    for kind, w, rows, cols, _b in layers[1:]:
        inputs.append((f"sparse layer {rows} x {cols}", "fp32", w[0], w[1], w[2], rows, cols))
    kind, w, rows, cols, _b = layers[1]
    inputs.append((f"sparse layer {rows} x {cols}, bf16", "bf16", w[0], w[1], w[2], rows, cols))
    rows, cols, rp, ci, va, _src = M.suitesparse_standin("analytics")
    r = np.repeat(np.arange(rows, dtype=np.int32), np.diff(rp).astype(np.int64))
    inputs.append(("scattered, no window (analytics stand-in)", "fp32", r, np.asarray(ci, np.int32), np.asarray(va, np.float32), rows, cols))

    h = pyhispmv.FpgaHandle("bench.xclbin", 0, 24, 1, 1, 2, 5, True, False, True)
    h.set_arena_bytes(64 << 30)
    try:
        h.set_value_updates("any_storage")
        todo = []
        for name, storage, r, c, v, rows, cols in inputs:
            h.set_value_storage(storage)
            h.set_transposable(True)
            hb = h.create_sparse_handle(r, c, v, rows, cols)
            h.set_transposable("companion")
            hk = h.create_sparse_handle(r, c, v, rows, cols)
            h.set_transposable(False)
            hc = h.create_sparse_handle(c, r, v, cols, rows)
            assert min(hb, hk, hc) >= 0, (name, hb, hk, hc)
            todo.append((name, hb, hk, hc))
        h.load_matrices()
        out = [measure(torch, h, name, hb, hk, hc, vecs, a.rounds, a.reps) for name, hb, hk, hc in todo]
    finally:
        h.close()
    print(f"{'matrix':42s} {'B':>3s} {'wT':>2s} {'(b) us':>9s} {'(k) us':>9s} {'(c) us':>9s} {'b/k':>6s} {'k/c':>5s} {'(k1) us':>9s} {'(c1) us':>9s} {'k1/c1':>5s} {'spread':>6s} {'bits':>5s}")
    for q in out:
        for p in q["by_vecs"]:
            print(f"{q['name'][:42]:42s} {p['B']:3d} {p['linear_info']['width_t']:2d} {p['atomics_us']:9.1f} {p['companion_us']:9.1f} {p['swapped_forward_us']:9.1f} "
                  f"{p['atomics_over_companion']:6.2f} {p['companion_over_swapped']:5.2f} {p['companion_bias_us']:9.1f} {p['swapped_forward_bias_us']:9.1f} "
                  f"{p['companion_over_swapped_bias']:5.2f} {p['spread']:6.2f} {str(p['same_bits_as_swapped']):>5s}")
    print(f"{'matrix':42s} {'bytes':>12s} {'+companion':>12s} {'prep s':>8s} {'+comp.':>8s} {'update us':>10s} {'+comp.':>8s} {'spread':>6s} {'companion is':>24s}")
    for q in out:
        w, k, u = q["without"], q["with_companion"], q["update"]
        ci = k["companion"]
        print(f"{q['name'][:42]:42s} {w['device_bytes']:12d} {k['device_bytes']:12d} {w['prep_seconds']:8.3f} {k['prep_seconds']:8.3f} {u['without_us']:10.1f} "
              f"{u['with_companion_us']:8.1f} {u['spread']:6.2f} {'format %d, %d part(s)' % (ci['format'], ci['parts']):>24s}")
    line = json.dumps({"companion_bench": out, "rounds": a.rounds, "reps": a.reps, "device": torch.cuda.get_device_name(0)})
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
