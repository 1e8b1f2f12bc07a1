"""In-place value updates against re-creation (hispmv_update_values*; not part of bench.py).

On the 20-matrix benchmark set and on the model_test layers (apps/model_test.py), in a context with value updates on:
  * create + load time of the handles, wall clock: in a plain context (what an update replaces: the full COO/CSR -> layout ->
    upload chain) and in the updatable one (the same + the payloads, the map and the first update);
  * host update time (hispmv_update_values: pinned staging, one copy, the kernel, a synchronise), warmed, per round of all handles;
  * device update time (hispmv_update_values_device of every handle back to back on one stream), HIP events over warmed repeats;
  * bytes per round: 4 * map slots + 4 * slots written + 4 * values gathered, GB/s and the fraction of 8 TB/s.
--bf16: the same handles a second time in the same context with bf16 value storage (set_value_updates("any_storage")), timed beside
the fp32 ones in the same run (groups `*_bf16`; an update then reads 4-byte values and map words and writes 2 bytes per slot of a
half slice or a dense W, 4 bytes per 32-bit slot).
Prints one JSON line (and writes it to --out).  Kernel-only times: run it under `rocprofv3 --kernel-trace --stats -- python
tools/update_bench.py` and read the update_values_kernel dispatches from the trace (the `kernels` view of its database).

    python tools/update_bench.py [--reps 50] [--warmup 5] [--bf16] [--out FILE]
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

HBM_PEAK = 8.0e12      # MI355X HBM3E, bytes / s


def group(torch, h, handles, reps, warmup):
    dev = torch.device("cuda", 0)
    infos = [h.value_update_info(i) for i, _ in handles]
    new = [np.random.default_rng(k).random(u["n"], dtype=np.float32) for k, u in enumerate(infos)]
    dnew = [torch.from_numpy(v).to(dev) for v in new]
    torch.cuda.synchronize()
    # host entry: every handle once per round
    for _ in range(warmup):
        for (i, _), v in zip(handles, new):
            h.update_values(i, v)
    t0 = time.perf_counter()
    for _ in range(reps):
        for (i, _), v in zip(handles, new):
            h.update_values(i, v)
    host_ms = (time.perf_counter() - t0) * 1e3 / reps
    # device entry: all handles back to back on one stream, HIP events around `reps` rounds
    s = torch.cuda.Stream(device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        for _ in range(warmup):
            for (i, _), d in zip(handles, dnew):
                h.update_values_device(i, d.data_ptr(), d.numel(), s.cuda_stream)
        e0.record(s)
        for _ in range(reps):
            for (i, _), d in zip(handles, dnew):
                h.update_values_device(i, d.data_ptr(), d.numel(), s.cuda_stream)
        e1.record(s)
    s.synchronize()
    h.synchronize()
    dev_ms = e0.elapsed_time(e1) / reps
    # bytes written: by slot size (a dense handle has no map: its `written` values are the slots of W, 2 or 4 bytes each)
    stores = [h.value_storage_info(i) for i, _ in handles]
    byts = sum(4 * u["map_slots"] + 4 * u["n"] + (2 * s["slots_2byte"] + 4 * s["slots_4byte"]) for u, s in zip(infos, stores))
    return dict(handles=len(handles), values=sum(u["n"] for u in infos), map_slots=sum(u["map_slots"] for u in infos),
                written=sum(u["written"] for u in infos), bytes=byts, device_ms=dev_ms, host_ms=host_ms,
                gbps=byts / (dev_ms * 1e-3) / 1e9, frac_8tbs=byts / (dev_ms * 1e-3) / HBM_PEAK)


def create_all(h, set_mats, layers):
    """-> (set handles, layer handles, seconds for the set, seconds for the layers): create + load, wall clock."""
    t0 = time.perf_counter()
    set_h = [(h.create_sparse_handle_from_csr(m["rp"], m["ci"], m["va"], m["rows"], m["cols"]), m["name"]) for m in set_mats]
    h.load_matrices()
    t_set = time.perf_counter() - t0
    t0 = time.perf_counter()
    lay_h = []
    for k, (kind, W, rows, cols, _b) in enumerate(layers):
        if kind == "dense":
            lay_h.append((h.create_dense_handle(W.reshape(-1), rows, cols), f"layer{k}:dense"))
        else:
            r, c, v = W
            lay_h.append((h.create_sparse_handle(r, c, v, rows, cols), f"layer{k}:sparse"))
    h.load_matrices()
    t_lay = time.perf_counter() - t0
    assert min(i for i, _ in set_h + lay_h) >= 0
    return set_h, lay_h, t_set, t_lay


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bf16", action="store_true", help="also time the same handles with bf16 value storage, in the same run")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import pyhispmv
    from hispmv_amd import matrices as M

    set_mats = [m for m in M.benchmark_set() if "rp" in m]
    layers = M.model_test_layers()
    out = {}
    # the plain context first (it also pays the process's first-use costs), then the updatable one
    h = pyhispmv.FpgaHandle("bench.xclbin", 0, 24, 1, 1, 2, 5, True, False, True)
    h.set_arena_bytes(64 << 30)
    try:
        _, _, p_set, p_lay = create_all(h, set_mats, layers)
    finally:
        h.close()
    h = pyhispmv.FpgaHandle("bench.xclbin", 0, 24, 1, 1, 2, 5, True, False, True)
    h.set_arena_bytes(64 << 30)
    h.set_value_updates("any_storage" if a.bf16 else True)          # (fp32 handles are the same in both states)
    try:
        set_h, lay_h, t_set, t_lay = create_all(h, set_mats, layers)
        if a.bf16:
            h.set_value_storage("bf16")
            set_b, lay_b, b_set, b_lay = create_all(h, set_mats, layers)
            h.set_value_storage("fp32")
            out["set20_bf16"] = dict(group(torch, h, set_b, a.reps, a.warmup), create_load_updatable_s=b_set)
            out["model_test_layers_bf16"] = dict(group(torch, h, lay_b, a.reps, a.warmup), create_load_updatable_s=b_lay)
        out["set20"] = dict(group(torch, h, set_h, a.reps, a.warmup), create_load_plain_s=p_set, create_load_updatable_s=t_set)
        out["model_test_layers"] = dict(group(torch, h, lay_h, a.reps, a.warmup), create_load_plain_s=p_lay, create_load_updatable_s=t_lay)
    finally:
        h.close()
    line = json.dumps({"update_bench": out, "reps": a.reps, "warmup": a.warmup})
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
