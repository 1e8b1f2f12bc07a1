"""bf16 handles on the step kernel (hispmv_set_step_half; not part of bench.py): four routes of the same 20-matrix step.

The stand-ins of the benchmark set (hispmv_amd.matrices.benchmark_set: seeded, nothing read from outside the tree) as ONE
hispmv_spmv_device_batch call per step, issued four ways and timed alternately inside one process:
  fp32 / step    fp32 handles, the step kernel (the headline path)
  fp32 / grids   fp32 handles in a context created under HISPMV_STEP_KERNEL=0
  bf16 / grids   bf16 handles, the switch off: the route such a call takes by default
  bf16 / step    bf16 handles after set_step_half(True): spmv_step_kernel<., HALF = 1> over the half batch layouts
Every route is warmed up; then `--rounds` rounds (>= 9) of `--steps` steps (>= 20) per route, the routes alternating within a round,
every step between two device events on one non-default stream.  A round's figure is the median of its steps; per route the median,
min and max over the rounds are reported, next to the stream bytes of the route (values + metas of the layouts the route reads) and the
library's own account of the call (batch_call_info).  Before anything is timed, every y of bf16 / step must have the bits of bf16 /
grids.  No GPU: the tool fails.  HISPMV_STEP_COST_HALF (the queue cost of a half slice, read by the library) is recorded.

    python tools/step_half_bench.py [--rounds 9] [--steps 20] [--warmup 5] [--out profiles/step_half/routes.json]
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

HW = ("bench.xclbin", 0, 24, 1, 1, 2, 5, True, False, True)
SLICE_BYTES = {"half": 4096, "compact": 6144, "wide": 8192}
ALPHA, BETA = 0.85, -2.06


def stream_bytes(info, storage):
    """Bytes one SpMV streams from the handle's matrix layout (values + metas; headers, x and y left out)."""
    if info["format"] == 1:
        return info["n_slices"] * SLICE_BYTES["wide"]
    compact = info["compact_slices"]
    return compact * SLICE_BYTES["half" if storage["slots_2byte"] > 0 else "compact"] + (info["n_slices"] - compact) * SLICE_BYTES["wide"]


class Route:
    def __init__(self, name, h, idx, batch, ys, half):
        self.name, self.h, self.idx, self.batch, self.ys, self.half = name, h, idx, batch, ys, half
        self.rounds, self.info = [], None

    def select(self):
        """The route's state of the switch, set once before its steps -- outside the timed events."""
        if self.half is not None:
            self.h.set_step_half(self.half)

    def step(self, sptr):
        self.h.spmv_device_batch(self.batch, ALPHA, BETA, sptr)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="profiles/step_half/routes.json")
    a = ap.parse_args()
    if a.rounds < 9 or a.steps < 20:
        sys.exit("step_half_bench: at least 9 rounds of at least 20 steps")
    import torch
    if not torch.cuda.is_available():
        sys.exit("step_half_bench: no GPU")
    import pyhispmv
    from hispmv_amd import matrices as M

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    sptr = stream.cuda_stream
    mats = M.benchmark_set(None, False)

    def context(env):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            h = pyhispmv.FpgaHandle(*HW)                  # (the switches are read when the context is created)
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        h.set_arena_bytes(200 << 30)
        return h

    def create(h, storage):
        h.set_value_storage(storage)
        idx = []
        for m in mats:
            idx.append(h.create_sparse_handle_from_csr(m["rp"], m["ci"], m["va"], m["rows"], m["cols"]) if "rp" in m
                       else h.create_sparse_handle_from_mtx(m["path"], 1))
            assert idx[-1] >= 0, f"{m['name']}: arena full"
        return idx

    os.environ.pop("HISPMV_STEP_HALF", None)              # the switch is flipped through the setter, per route
    os.environ.pop("HISPMV_STEP_KERNEL", None)
    h_step, h_grids = context({}), context({"HISPMV_STEP_KERNEL": "0"})
    try:
        i_fp32, i_bf16 = create(h_step, "fp32"), create(h_step, "bf16")
        i_grids = create(h_grids, "fp32")
        h_step.load_matrices()
        h_grids.load_matrices()
        g = torch.Generator(device="cpu").manual_seed(1234)
        dims = [h_step.matrix_info(i) for i in i_fp32]
        xs = [torch.rand(d["cols"], generator=g, dtype=torch.float32).to(dev) for d in dims]
        bs = [torch.rand(d["rows"], generator=g, dtype=torch.float32).to(dev) for d in dims]

        def route(name, h, idx, half):
            ys = [torch.zeros(d["rows"], dtype=torch.float32, device=dev) for d in dims]
            batch = h.prepare_batch(idx, [x.data_ptr() for x in xs], [b.data_ptr() for b in bs], [y.data_ptr() for y in ys])
            r = Route(name, h, idx, batch, ys, half)
            r.bytes = int(sum(stream_bytes(h.matrix_info(i), h.value_storage_info(i)) for i in idx))
            return r
        routes = [route("fp32/step", h_step, i_fp32, False), route("fp32/grids", h_grids, i_grids, None),
                  route("bf16/grids", h_step, i_bf16, False), route("bf16/step", h_step, i_bf16, True)]
        torch.cuda.synchronize()
        for r in routes:                                  # warm-up of every route; the library's account of the call
            r.select()
            for _ in range(a.warmup):
                r.step(sptr)
            r.info = r.h.batch_call_info()
            torch.cuda.synchronize()
        by = {r.name: r for r in routes}
        assert by["fp32/step"].info["step_kernel"] and by["bf16/step"].info["step_kernel"], {r.name: r.info for r in routes}
        assert not by["fp32/grids"].info["step_kernel"] and not by["bf16/grids"].info["step_kernel"], {r.name: r.info for r in routes}
        # the bits of bf16 / step are those of bf16 / grids (the two routes write their own y vectors)
        for m, ya, yb in zip(mats, by["bf16/step"].ys, by["bf16/grids"].ys):
            assert torch.equal(ya.view(torch.int32), yb.view(torch.int32)), f"{m['name']}: bf16 / step differs from bf16 / grids"
            assert bool(torch.isfinite(ya).all()), m["name"]
        for _ in range(a.rounds):
            for r in routes:
                r.select()
                evs = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
                evs[0].record(stream)
                for k in range(a.steps):
                    r.step(sptr)
                    evs[k + 1].record(stream)
                torch.cuda.synchronize()
                r.rounds.append(float(np.median([evs[k].elapsed_time(evs[k + 1]) for k in range(a.steps)])))
        info = {r.name: [dict(name=m["name"], **{k: r.h.matrix_info(i)[k] for k in ("format", "block_threads", "group_slices", "batch_group_slices", "n_slices", "compact_slices")},
                              slots_2byte=r.h.value_storage_info(i)["slots_2byte"]) for m, i in zip(mats, r.idx)] for r in routes if r.name in ("fp32/step", "bf16/step")}
    finally:
        h_step.close()
        h_grids.close()
    out = dict(step_half_bench=[dict(route=r.name, ms_median=float(np.median(r.rounds)), ms_min=float(min(r.rounds)), ms_max=float(max(r.rounds)),
                                     rounds_ms=r.rounds, stream_bytes=r.bytes, batch_call_info=r.info) for r in routes],
               rounds=a.rounds, steps=a.steps, warmup=a.warmup, matrices=len(mats), bits_bf16_step_equal_grids=True,
               step_cost_half_env=os.environ.get("HISPMV_STEP_COST_HALF"), device=torch.cuda.get_device_name(0), handles=info)
    print(f"{'route':12s} {'median ms':>10s} {'min':>8s} {'max':>8s} {'MB':>8s}  call")
    for q in out["step_half_bench"]:
        print(f"{q['route']:12s} {q['ms_median']:10.4f} {q['ms_min']:8.4f} {q['ms_max']:8.4f} {q['stream_bytes'] / 1e6:8.1f}  {q['batch_call_info']}")
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
