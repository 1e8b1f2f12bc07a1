"""The wide-batch product on feature-major operands against the passes of 4 vectors (not part of bench.py).

Per layer and B in --vecs, timed with HIP events around `--reps` back-to-back calls on one stream after warm-up, `--rounds` times,
alternately (medians and spread), all on ONE handle in one process:
  (s)   spmm_device       yt[rows, B] = A xt[cols, B] + bias              (alpha = beta = 1, shared bias, caller's workspace)
  (s+)  spmm_device plus the two torch transposes around it               (x [B, cols] -> xt, yt -> y [B, rows], both contiguous)
  (l)   linear_device     y[B, rows]  = A x[B, cols] + bias               (the library as it was: passes of 4 vectors)
  (st)  spmm_device_t     on the handle's stored transpose                (alpha = 1, beta = 0)
  (lt)  linear_device_t   on the same handle                              (the forward passes over the stored transpose)
  (mm)  torch.matmul with the densified fp32 W, for context               (x [B, cols] @ W^T)
Layers: the 8192 x 8192 (density 0.1) and 1024 x 8192 (density 0.25) sparse layers of examples/model_check.py with fp32 and with bf16
values, and an 8192 x 8192 layer of density 0.01.  Every handle is created under set_transposable("companion") in a context that
keeps slice streams (HISPMV_FORMAT=slices), so that both wide entries accept it.
`spread` is the largest (max - min) / median over the rounds of the two timings a ratio is made of: a ratio closer to 1 than that is
not a difference.  `max_rel_diff` is the largest difference between (s) and (l) over all vectors, relative to the largest entry of
(l).  Prints a table and one JSON line, and writes the line to --out.

--bf16-activations measures something else on the same handles: (sb) spmm_device_bf16 beside (s), and (stb) spmm_device_t_bf16 beside
(st), the fp32 entries on the widened values of the same bf16 operands, alternately, with B = 1024 added; `bits` says whether (sb) is
bf16((s)) bit for bit.  The result goes to profiles/spmm_bf16_bench.json.

    python tools/spmm_bench.py [--rounds 5] [--reps 10] [--vecs 32,64,128,256,512] [--out profiles/spmm_bench.json]
    python tools/spmm_bench.py --bf16-activations --out profiles/spmm_bf16_bench.json
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


def measure(torch, h, name, idx, W, B, rounds, reps):
    dev = torch.device("cuda", 0)
    info = h.matrix_info(idx)
    rows, cols = info["rows"], info["cols"]
    si = h.spmm_info(idx, B)
    assert si["accepted"], (name, si)
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream
    with torch.cuda.stream(stream):
        x = torch.rand((B, cols), dtype=torch.float32, device=dev) - 0.3
        g = torch.rand((B, rows), dtype=torch.float32, device=dev) - 0.5
        bias = torch.rand(rows, dtype=torch.float32, device=dev)
        xt, gt = x.t().contiguous(), g.t().contiguous()
        yt = torch.empty((rows, B), dtype=torch.float32, device=dev)
        gxt = torch.empty((cols, B), dtype=torch.float32, device=dev)
        y = torch.empty((B, rows), dtype=torch.float32, device=dev)
        gx = torch.empty((B, cols), dtype=torch.float32, device=dev)
        work = torch.empty(max(si["work_bytes"], si["work_bytes_t"], 4) // 4, dtype=torch.float32, device=dev)
    keep = {}

    def spmm():
        h.spmm_device(idx, xt.data_ptr(), B, bias.data_ptr(), yt.data_ptr(), 1.0, 1.0, work=work.data_ptr(), work_bytes=si["work_bytes"], stream=s)

    def spmm_with_transposes():
        a = x.t().contiguous()
        h.spmm_device(idx, a.data_ptr(), B, bias.data_ptr(), yt.data_ptr(), 1.0, 1.0, work=work.data_ptr(), work_bytes=si["work_bytes"], stream=s)
        keep["y"] = yt.t().contiguous()

    calls = dict(s=spmm, sp=spmm_with_transposes,
                 l=lambda: h.linear_device(idx, x.data_ptr(), B, bias.data_ptr(), y.data_ptr(), 1.0, 1.0, s),
                 lt=lambda: h.linear_device_t(idx, g.data_ptr(), B, 0, gx.data_ptr(), 1.0, 0.0, 0, s))
    if si["accepted_t"]:
        calls["st"] = lambda: h.spmm_device_t(idx, gt.data_ptr(), B, 0, gxt.data_ptr(), 1.0, 0.0, work=work.data_ptr(), work_bytes=si["work_bytes_t"], stream=s)
    if W is not None:
        calls["mm"] = lambda: keep.__setitem__("mm", torch.matmul(x, W.t()))
    torch.cuda.synchronize()
    t = {k: [] for k in calls}
    with torch.cuda.stream(stream):          # (torch's own kernels of (s+) and (mm) go to the timed stream too)
        for f in calls.values():
            time_calls(torch, stream, f, 3)
        for _ in range(rounds):
            for k, f in calls.items():
                t[k].append(time_calls(torch, stream, f, reps))
    torch.cuda.synchronize()
    diff = float((yt.t() - y).abs().max() / y.abs().max().clamp_min(1e-30))
    diff_t = float((gxt.t() - gx).abs().max() / gx.abs().max().clamp_min(1e-30)) if "st" in calls else None
    med = {k: float(np.median(v)) for k, v in t.items()}
    rel = {k: float((max(v) - min(v)) / np.median(v)) for k, v in t.items()}
    return dict(name=name, rows=rows, cols=cols, nnz=info["nnz"], B=B, block_threads=info["block_threads"], lds_bytes=info["lds_bytes"],
                parts=info["col_tiles"], format=info["format"], spmm_info=si, linear_info=h.linear_info(idx, B),
                spmm_us=med["s"], spmm_with_transposes_us=med["sp"], linear_device_us=med["l"], linear_device_t_us=med["lt"],
                spmm_t_us=med.get("st"), matmul_us=med.get("mm"),
                speedup=med["l"] / med["s"], speedup_with_transposes=med["l"] / med["sp"], spread=max(rel["s"], rel["l"]),
                spread_with_transposes=max(rel["sp"], rel["l"]),
                speedup_t=(med["lt"] / med["st"]) if "st" in med else None, spread_t=max(rel["st"], rel["lt"]) if "st" in rel else None,
                range_us={k: [float(min(v)), float(max(v))] for k, v in t.items()}, max_rel_diff=diff, max_rel_diff_t=diff_t)


def measure_bf16(torch, h, name, idx, B, rounds, reps):
    """(s) spmm_device on fp32 activations against (sb) spmm_device_bf16 on the same values as bf16, and (st) against (stb) for the
    transposed entries, alternately on one handle and one stream; ld = B.  `equal_bits`: (sb) is bf16((s)) bit for bit."""
    dev = torch.device("cuda", 0)
    info = h.matrix_info(idx)
    rows, cols = info["rows"], info["cols"]
    si, sb = h.spmm_info(idx, B), h.spmm_bf16_info(idx, B)
    assert si["accepted"] and sb["accepted"], (name, si, sb)
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream
    with torch.cuda.stream(stream):
        xt16 = (torch.rand((cols, B), dtype=torch.float32, device=dev) - 0.3).to(torch.bfloat16)
        gt16 = (torch.rand((rows, B), dtype=torch.float32, device=dev) - 0.5).to(torch.bfloat16)
        xt, gt = xt16.float(), gt16.float()
        bias = torch.rand(rows, dtype=torch.float32, device=dev)
        yt, yt16 = torch.empty((rows, B), dtype=torch.float32, device=dev), torch.empty((rows, B), dtype=torch.bfloat16, device=dev)
        gxt, gxt16 = torch.empty((cols, B), dtype=torch.float32, device=dev), torch.empty((cols, B), dtype=torch.bfloat16, device=dev)
        work = torch.empty(max(si["work_bytes"], si["work_bytes_t"], sb["work_bytes"], sb["work_bytes_t"], 4) // 4, dtype=torch.float32, device=dev)
    calls = dict(
        s=lambda: h.spmm_device(idx, xt.data_ptr(), B, bias.data_ptr(), yt.data_ptr(), 1.0, 1.0, work=work.data_ptr(), work_bytes=si["work_bytes"], stream=s),
        sb=lambda: h.spmm_device_bf16(idx, xt16.data_ptr(), B, bias.data_ptr(), yt16.data_ptr(), 1.0, 1.0, work=work.data_ptr(), work_bytes=sb["work_bytes"], stream=s))
    if si["accepted_t"]:
        calls["st"] = lambda: h.spmm_device_t(idx, gt.data_ptr(), B, 0, gxt.data_ptr(), 1.0, 0.0, work=work.data_ptr(), work_bytes=si["work_bytes_t"], stream=s)
        calls["stb"] = lambda: h.spmm_device_t_bf16(idx, gt16.data_ptr(), B, 0, gxt16.data_ptr(), 1.0, 0.0, work=work.data_ptr(), work_bytes=sb["work_bytes_t"], stream=s)
    torch.cuda.synchronize()
    t = {k: [] for k in calls}
    with torch.cuda.stream(stream):
        for f in calls.values():
            time_calls(torch, stream, f, 3)
        for _ in range(rounds):
            for k, f in calls.items():
                t[k].append(time_calls(torch, stream, f, reps))
    torch.cuda.synchronize()
    equal = bool(torch.equal(yt16, yt.to(torch.bfloat16)) and ("st" not in calls or torch.equal(gxt16, gxt.to(torch.bfloat16))))
    med = {k: float(np.median(v)) for k, v in t.items()}
    rel = {k: float((max(v) - min(v)) / np.median(v)) for k, v in t.items()}
    return dict(name=name, rows=rows, cols=cols, nnz=info["nnz"], B=B, block_threads=info["block_threads"], parts=info["col_tiles"], spmm_info=si, spmm_bf16_info=sb,
                spmm_us=med["s"], spmm_bf16_us=med["sb"], speedup=med["s"] / med["sb"], spread=max(rel["s"], rel["sb"]),
                spmm_t_us=med.get("st"), spmm_t_bf16_us=med.get("stb"), speedup_t=(med["st"] / med["stb"]) if "st" in med else None,
                spread_t=max(rel["st"], rel["stb"]) if "st" in rel else None, range_us={k: [float(min(v)), float(max(v))] for k, v in t.items()}, equal_bits=equal)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--vecs", default="32,64,128,256,512")
    ap.add_argument("--out", default="")
    ap.add_argument("--bf16-activations", action="store_true",
                    help="measure spmm_device_bf16 / spmm_device_t_bf16 beside (s) / (st) on the same handle instead (B = 1024 added; profiles/spmm_bf16_bench.json)")
    a = ap.parse_args()
    vecs = [int(v) for v in a.vecs.split(",")]
    if a.bf16_activations and a.vecs == ap.get_default("vecs"):
        vecs.append(1024)
    os.environ["HISPMV_FORMAT"] = "slices"          # read when the context is created: handle and stored transpose stay slice streams
    import torch
    import pyhispmv
    from hispmv_amd import matrices as M

    if not torch.cuda.is_available():
        raise SystemExit("spmm_bench needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    h = pyhispmv.FpgaHandle("bench.xclbin", 0, 24, 1, 1, 2, 5, True, False, True)
    h.set_arena_bytes(64 << 30)
    todo = []
    try:
        h.set_transposable("companion")
        layers = [(w, rows, cols) for _kind, w, rows, cols, _b in M.model_test_layers()[1:]]
        rng = np.random.default_rng(7)
        mask = rng.random((8192, 8192), dtype=np.float32) < 0.01
        r, c = np.nonzero(mask)
        thin = ((r.astype(np.int32), c.astype(np.int32), (rng.random(r.size, dtype=np.float32) - np.float32(0.5)) * np.float32(0.05) + np.float32(0.1)), 8192, 8192)
        for (w, rows, cols), dens in zip(layers + [thin], (0.1, 0.25, 0.01)):
            for storage in (("fp32", "bf16") if dens != 0.01 else ("fp32",)):
                h.set_value_storage(storage)
                todo.append((f"sparse layer {rows} x {cols}, d = {dens}, {storage}", h.create_sparse_handle(*w, rows, cols), w, rows, cols))
        h.set_value_storage("fp32")
        assert all(t[1] >= 0 for t in todo), todo
        h.load_matrices()
        out = []
        if a.bf16_activations:
            out = [measure_bf16(torch, h, name, i, B, a.rounds, a.reps) for name, i, _w, _rows, _cols in todo for B in vecs]
            todo = []
        for name, i, (r, c, v), rows, cols in todo:
            W = torch.zeros((rows, cols), dtype=torch.float32, device=dev)
            W.index_put_((torch.from_numpy(r.astype(np.int64)).to(dev), torch.from_numpy(c.astype(np.int64)).to(dev)), torch.from_numpy(v).to(dev), accumulate=True)
            out += [measure(torch, h, name, i, W, B, a.rounds, a.reps) for B in vecs]
            del W
    finally:
        h.close()
    if a.bf16_activations:
        print(f"{'layer':44s} {'B':>4s} {'VL':>2s} {'VB':>2s} {'(s) us':>9s} {'(sb) us':>9s} {'s/sb':>5s} {'spread':>6s} {'(st) us':>9s} {'(stb) us':>9s} {'st/stb':>6s} {'spread':>6s} bits")
        for q in out:
            print(f"{q['name'][:44]:44s} {q['B']:4d} {q['spmm_info']['vl']:2d} {q['spmm_bf16_info']['vb']:2d} {q['spmm_us']:9.1f} {q['spmm_bf16_us']:9.1f} {q['speedup']:5.2f} "
                  f"{q['spread']:6.2f} {q['spmm_t_us']:9.1f} {q['spmm_t_bf16_us']:9.1f} {q['speedup_t']:6.2f} {q['spread_t']:6.2f} {'equal' if q['equal_bits'] else 'DIFFER'}")
        line = json.dumps({"spmm_bf16_bench": out, "rounds": a.rounds, "reps": a.reps, "device": torch.cuda.get_device_name(0)})
        print(line)
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.out).write_text(line + "\n")
        return
    print(f"{'layer':44s} {'B':>3s} {'VL':>2s} {'tiles':>5s} {'(s) us':>9s} {'(s+) us':>9s} {'(l) us':>9s} {'l/s':>5s} {'l/s+':>5s} {'spread':>6s} {'(st) us':>9s} {'(lt) us':>9s} "
          f"{'lt/st':>5s} {'spread':>6s} {'(mm) us':>9s} {'diff':>8s}")
    for q in out:
        si = q["spmm_info"]
        st = f"{q['spmm_t_us']:9.1f}" if q["spmm_t_us"] is not None else f"{'-':>9s}"
        rt = f"{q['speedup_t']:5.2f} {q['spread_t']:6.2f}" if q["speedup_t"] is not None else f"{'-':>5s} {'-':>6s}"
        print(f"{q['name'][:44]:44s} {q['B']:3d} {si['vl']:2d} {si['tiles']:5d} {q['spmm_us']:9.1f} {q['spmm_with_transposes_us']:9.1f} {q['linear_device_us']:9.1f} "
              f"{q['speedup']:5.2f} {q['speedup_with_transposes']:5.2f} {max(q['spread'], q['spread_with_transposes']):6.2f} {st} {q['linear_device_t_us']:9.1f} {rt} "
              f"{q['matmul_us']:9.1f} {q['max_rel_diff']:8.1e}")
    line = json.dumps({"spmm_bench": out, "rounds": a.rounds, "reps": a.reps, "device": torch.cuda.get_device_name(0)})
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
