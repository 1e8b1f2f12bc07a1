"""The wide-batch value gradient on feature-major operands against the passes of 4 vectors (not part of bench.py).

Per layer and B in --vecs, timed with HIP events around `--reps` back-to-back calls on one stream after warm-up, `--rounds` times,
alternately (medians and spread), all on ONE handle in one process:
  (w)   spmm_value_grad_device   grad[n] = sum_v gyt[row, v] * xt[col, v]     (alpha = 1, beta = 0, feature-major operands)
  (w+)  the same plus the two torch transposes in front of it                  (gy [B, rows] -> gyt, x [B, cols] -> xt, both contiguous)
  (g)   value_grad_device        on gy [B, rows], x [B, cols]                  (the library as it was: passes of 4 vectors -- the yardstick)
  (f)   spmm_device              yt[rows, B] = A xt[cols, B]                    (the wide forward product: the same gathers of xt per element)
  (t)   torch                    (gy.T @ x)[r, c]                               (a dense [rows, cols] product, then a gather of the pattern)
Layers: the 8192 x 8192 (density 0.1) and 1024 x 8192 (density 0.25) sparse layers of examples/model_check.py and an 8192 x 8192 layer
of density 0.01, each with fp32 and with bf16 values, created under set_value_updates("any_storage") in a context that keeps slice
streams (HISPMV_FORMAT=slices).
`spread` is the largest (max - min) / median over the rounds of the timings: a ratio closer to 1 than that is not a difference.
`max_rel_diff` is the largest difference between (w) and (g) over all entries, relative to the largest entry of (g).  Prints a table
and one JSON line, and writes the line to --out.

    python tools/spmm_value_grad_bench.py [--rounds 5] [--reps 10] [--vecs 16,32,64,128,256] [--out profiles/spmm_value_grad_bench.json]

--bf16-activations measures the entry with bf16 operands instead, same layers and method, --vecs 16,32,64,128,256,512,1024 by default:
  (w)   spmm_value_grad_device        on the widened fp32 feature-major operands, ld = B rounded up to 4 -- the yardstick: code the bf16
                                      entry does not touch
  (wb)  spmm_value_grad_device_bf16   on the bf16 feature-major operands, ld = B rounded up to 8
  (wb4) the same with both operands moved by 8 bytes: alignment 8 caps the lanes at VB 4, so where (wb) runs one VB 8 tile this runs two
        VB 4 tiles on the same data
  (c)   the two torch copies that sparse_linear(wide_grad="bf16") saves: gy, x bf16 [B, n] -> fp32 feature-major [n, ld]
`max_rel_diff` is then (wb) against (w) on all entries.

    python tools/spmm_value_grad_bench.py --bf16-activations [--out profiles/spmm_value_grad_bf16_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
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
    rows, cols, n = info["rows"], info["cols"], h.value_update_info(idx)["n"]
    wi, si = h.spmm_value_grad_info(idx, B), h.spmm_info(idx, B)
    assert wi["accepted"] and si["accepted"], (name, wi, si)
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream
    with torch.cuda.stream(stream):
        x = torch.rand((B, cols), dtype=torch.float32, device=dev) - 0.3
        gy = torch.rand((B, rows), dtype=torch.float32, device=dev) - 0.5
        xt, gyt = x.t().contiguous(), gy.t().contiguous()
        yt = torch.empty((rows, B), dtype=torch.float32, device=dev)
        grad_w = torch.empty(n, dtype=torch.float32, device=dev)
        grad_g = torch.empty(n, dtype=torch.float32, device=dev)
        work = torch.empty(max(si["work_bytes"], 4) // 4, dtype=torch.float32, device=dev)
    keep = {}

    def wide():
        h.spmm_value_grad_device(idx, gyt.data_ptr(), xt.data_ptr(), B, grad_w.data_ptr(), 1.0, 0.0, stream=s)

    def wide_with_transposes():
        a, b = gy.t().contiguous(), x.t().contiguous()
        h.spmm_value_grad_device(idx, a.data_ptr(), b.data_ptr(), B, grad_w.data_ptr(), 1.0, 0.0, stream=s)
        keep["t"] = (a, b)

    calls = dict(w=wide, wp=wide_with_transposes,
                 g=lambda: h.value_grad_device(idx, gy.data_ptr(), x.data_ptr(), B, grad_g.data_ptr(), 1.0, 0.0, s),
                 f=lambda: h.spmm_device(idx, xt.data_ptr(), B, 0, yt.data_ptr(), 1.0, 0.0, work=work.data_ptr(), work_bytes=si["work_bytes"], stream=s),
                 t=lambda: keep.__setitem__("mm", torch.matmul(gy.t(), x)[r, c]))
    torch.cuda.synchronize()
    t = {k: [] for k in calls}
    with torch.cuda.stream(stream):          # (torch's own kernels of (w+) and (t) go to the timed stream too)
        for f in calls.values():
            time_calls(torch, stream, f, 3)
        for _ in range(rounds):
            for k, f in calls.items():
                t[k].append(time_calls(torch, stream, f, reps))
    torch.cuda.synchronize()
    wide()
    torch.cuda.synchronize()
    scale = grad_g.abs().max().clamp_min(1e-30)
    diff = float((grad_w - grad_g).abs().max() / scale)
    diff_torch = float((keep["mm"] - grad_g).abs().max() / scale)
    med = {k: float(np.median(v)) for k, v in t.items()}
    rel = {k: float((max(v) - min(v)) / np.median(v)) for k, v in t.items()}
    return dict(name=name, rows=rows, cols=cols, nnz=info["nnz"], B=B, block_threads=info["block_threads"], lds_bytes=info["lds_bytes"],
                parts=info["col_tiles"], format=info["format"], wide_info=wi, value_grad_info=h.value_grad_info(idx, B),
                wide_us=med["w"], wide_with_transposes_us=med["wp"], value_grad_us=med["g"], spmm_us=med["f"], torch_us=med["t"],
                w_over_g=med["w"] / med["g"], wp_over_g=med["wp"] / med["g"], w_over_f=med["w"] / med["f"], t_over_w=med["t"] / med["w"],
                t_over_wp=med["t"] / med["wp"], spread=max(rel.values()), spread_of=rel,
                range_us={k: [float(min(v)), float(max(v))] for k, v in t.items()}, max_rel_diff=diff, max_rel_diff_torch=diff_torch)


def measure_bf16(torch, h, name, idx, B, rounds, reps):
    dev = torch.device("cuda", 0)
    info = h.matrix_info(idx)
    rows, cols, n = info["rows"], info["cols"], h.value_update_info(idx)["n"]
    ld4, ld8 = (B + 3) & ~3, (B + 7) & ~7
    wi, bi = h.spmm_value_grad_info(idx, B, ld4), h.spmm_value_grad_bf16_info(idx, B, ld8)
    assert wi["accepted"] and bi["accepted"], (name, wi, bi)
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream

    def feature_major(a, ld, dtype, lead=0):
        """[B, n] -> [n, ld] of dtype behind `lead` elements, pad columns zero"""
        flat = torch.zeros(lead + a.shape[1] * ld, dtype=dtype, device=dev)
        at = flat[lead:].view(a.shape[1], ld)
        at[:, :B] = a.t()
        return flat, at

    with torch.cuda.stream(stream):
        x = (torch.rand((B, cols), dtype=torch.float32, device=dev) - 0.3).to(torch.bfloat16)
        gy = (torch.rand((B, rows), dtype=torch.float32, device=dev) - 0.5).to(torch.bfloat16)
        _, xt32 = feature_major(x, ld4, torch.float32)
        _, gt32 = feature_major(gy, ld4, torch.float32)
        _, xt16 = feature_major(x, ld8, torch.bfloat16)
        _, gt16 = feature_major(gy, ld8, torch.bfloat16)
        xo, xt16o = feature_major(x, ld8, torch.bfloat16, lead=4)
        go, gt16o = feature_major(gy, ld8, torch.bfloat16, lead=4)
        assert xt16.data_ptr() % 16 == 0 and gt16.data_ptr() % 16 == 0 and xt16o.data_ptr() % 16 == 8 and gt16o.data_ptr() % 16 == 8
        grad_w = torch.empty(n, dtype=torch.float32, device=dev)
        grad_b = torch.empty(n, dtype=torch.float32, device=dev)
        grad_o = torch.empty(n, dtype=torch.float32, device=dev)
    keep = {}

    def copies():
        keep["c"] = (feature_major(gy, ld4, torch.float32), feature_major(x, ld4, torch.float32))

    calls = dict(w=lambda: h.spmm_value_grad_device(idx, gt32.data_ptr(), xt32.data_ptr(), B, grad_w.data_ptr(), 1.0, 0.0, ld_gy=ld4, ld_x=ld4, stream=s),
                 wb=lambda: h.spmm_value_grad_device_bf16(idx, gt16.data_ptr(), xt16.data_ptr(), B, grad_b.data_ptr(), 1.0, 0.0, ld_gy=ld8, ld_x=ld8, stream=s),
                 wb4=lambda: h.spmm_value_grad_device_bf16(idx, gt16o.data_ptr(), xt16o.data_ptr(), B, grad_o.data_ptr(), 1.0, 0.0, ld_gy=ld8, ld_x=ld8, stream=s),
                 c=copies)
    torch.cuda.synchronize()
    t = {k: [] for k in calls}
    with torch.cuda.stream(stream):
        for f in calls.values():
            time_calls(torch, stream, f, 3)
        for _ in range(rounds):
            for k, f in calls.items():
                t[k].append(time_calls(torch, stream, f, reps))
    torch.cuda.synchronize()
    scale = grad_w.abs().max().clamp_min(1e-30)
    med = {k: float(np.median(v)) for k, v in t.items()}
    rel = {k: float((max(v) - min(v)) / np.median(v)) for k, v in t.items()}
    from hispmv_amd import prep
    return dict(name=name, rows=rows, cols=cols, nnz=info["nnz"], B=B, ld_fp32=ld4, ld_bf16=ld8, block_threads=info["block_threads"], lds_bytes=info["lds_bytes"],
                parts=info["col_tiles"], fp32_info=wi, bf16_info=bi, bf16_tiles_align8=prep.spmm_bf16_tiles(cols, B, ld8, 8),
                wide_us=med["w"], wide_bf16_us=med["wb"], wide_bf16_align8_us=med["wb4"], copies_us=med["c"],
                wb_over_w=med["wb"] / med["w"], wb_over_wb4=med["wb"] / med["wb4"], wb_over_w_plus_c=med["wb"] / (med["w"] + med["c"]),
                spread=max(rel.values()), spread_of=rel, range_us={k: [float(min(v)), float(max(v))] for k, v in t.items()},
                max_rel_diff=float((grad_b - grad_w).abs().max() / scale), max_rel_diff_align8=float((grad_o - grad_w).abs().max() / scale))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--vecs", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--bf16-activations", action="store_true", help="measure spmm_value_grad_device_bf16 against the fp32 entry on the widened operands")
    a = ap.parse_args()
    vecs = [int(v) for v in (a.vecs or ("16,32,64,128,256,512,1024" if a.bf16_activations else "16,32,64,128,256")).split(",")]
    os.environ["HISPMV_FORMAT"] = "slices"          # read when the context is created: the handles stay slice streams
    import torch
    import pyhispmv
    from hispmv_amd import matrices as M

    if not torch.cuda.is_available():
        raise SystemExit("spmm_value_grad_bench needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    h = pyhispmv.FpgaHandle("bench.xclbin", 0, 24, 1, 1, 2, 5, True, False, True)
    h.set_arena_bytes(64 << 30)
    todo = []
    try:
        h.set_transposable(True)
        h.set_value_updates("any_storage")
        layers = [(w, rows, cols) for _kind, w, rows, cols, _b in M.model_test_layers()[1:]]
        rng = np.random.default_rng(7)
        mask = rng.random((8192, 8192), dtype=np.float32) < 0.01
        r, c = np.nonzero(mask)
        thin = ((r.astype(np.int32), c.astype(np.int32), (rng.random(r.size, dtype=np.float32) - np.float32(0.5)) * np.float32(0.05) + np.float32(0.1)), 8192, 8192)
        for (w, rows, cols), dens in zip(layers + [thin], (0.1, 0.25, 0.01)):
            for storage in ("fp32", "bf16"):
                h.set_value_storage(storage)
                todo.append((f"sparse layer {rows} x {cols}, d = {dens}, {storage}", h.create_sparse_handle(*w, rows, cols), w))
        h.set_value_storage("fp32")
        assert all(t[1] >= 0 for t in todo), todo
        h.load_matrices()
        out = []
        for name, i, (r, c, _v) in todo:
            if a.bf16_activations:
                out += [measure_bf16(torch, h, name, i, B, a.rounds, a.reps) for B in vecs]
                continue
            dr, dc = torch.from_numpy(r.astype(np.int64)).to(dev), torch.from_numpy(c.astype(np.int64)).to(dev)
            out += [measure(torch, h, name, i, dr, dc, B, a.rounds, a.reps) for B in vecs]
            del dr, dc
    finally:
        h.close()
    if a.bf16_activations:
        print(f"{'layer':44s} {'B':>4s} {'VL':>2s} {'tiles':>5s} {'VB':>2s} {'tiles':>5s} {'(w) us':>9s} {'(wb) us':>9s} {'(wb4) us':>9s} {'(c) us':>9s} {'wb/w':>5s} {'wb/wb4':>6s} "
              f"{'wb/(w+c)':>8s} {'spread':>6s} {'diff':>8s}")
        for q in out:
            wi, bi = q["fp32_info"], q["bf16_info"]
            print(f"{q['name'][:44]:44s} {q['B']:4d} {wi['vl']:2d} {wi['tiles']:5d} {bi['vb']:2d} {bi['tiles']:5d} {q['wide_us']:9.1f} {q['wide_bf16_us']:9.1f} "
                  f"{q['wide_bf16_align8_us']:9.1f} {q['copies_us']:9.1f} {q['wb_over_w']:5.2f} {q['wb_over_wb4']:6.2f} {q['wb_over_w_plus_c']:8.2f} {q['spread']:6.2f} {q['max_rel_diff']:8.1e}")
        line = json.dumps({"spmm_value_grad_bf16_bench": out, "rounds": a.rounds, "reps": a.reps, "device": torch.cuda.get_device_name(0)})
        print(line)
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.out).write_text(line + "\n")
        return
    print(f"{'layer':44s} {'B':>3s} {'VL':>2s} {'tiles':>5s} {'(w) us':>9s} {'(w+) us':>9s} {'(g) us':>9s} {'(f) us':>9s} {'(t) us':>9s} {'w/g':>5s} {'w/f':>5s} {'t/w':>5s} "
          f"{'t/w+':>5s} {'spread':>6s} {'diff':>8s}")
    for q in out:
        wi = q["wide_info"]
        print(f"{q['name'][:44]:44s} {q['B']:3d} {wi['vl']:2d} {wi['tiles']:5d} {q['wide_us']:9.1f} {q['wide_with_transposes_us']:9.1f} {q['value_grad_us']:9.1f} "
              f"{q['spmm_us']:9.1f} {q['torch_us']:9.1f} {q['w_over_g']:5.2f} {q['w_over_f']:5.2f} {q['t_over_w']:5.2f} {q['t_over_wp']:5.2f} {q['spread']:6.2f} "
              f"{q['max_rel_diff']:8.1e}")
    line = json.dumps({"spmm_value_grad_bench": out, "rounds": a.rounds, "reps": a.reps, "device": torch.cuda.get_device_name(0)})
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
