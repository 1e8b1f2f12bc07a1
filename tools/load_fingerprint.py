#!/usr/bin/env python3
"""What hispmv_load_matrices leaves on the device, as one JSON line per case, to compare two builds of the library:

    HISPMV_LIB=<one build>   python tools/load_fingerprint.py > A.jsonl
    HISPMV_LIB=<the other>   python tools/load_fingerprint.py > B.jsonl      # a process of its own
    diff A.jsonl B.jsonl

A case is a small matrix (the builders of tests/step_small_cases.py), the switches it is created under and a variant: plain, updatable
("upd"), bf16 storage ("bf16"), both ("bf16upd", under any_storage) or with a stored transpose ("companion").  Its line holds the
info getters of the loaded handle (matrix_info without prep_seconds) and the SHA-256 of y after run_kernel (alpha = beta = 1),
spmv_device, one spmv_device_batch call together with one_by_one() -- the call that reads a batch layout --, spmv_device after
update_values with a second value vector (updatable cases) and linear_device_t over the stored transpose (companion cases).  Forward
products only: the atomic transposed kernels have no fixed summation order.  Every case asserts the format and the part count its
`expect` names.  No builder here yields column parts with a chain of more than 32 slices, so the merge that cannot apply the
fix-ups itself (no d_fix_of_row) is not among the cases."""
from __future__ import annotations

import hashlib
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import step_small_cases as S  # noqa: E402

HW = ("load_fingerprint.xclbin", 0, 24, 1, 1, 2, 5, True, False, True)
ALPHA, BETA = 0.85, -2.06
HOST, DEVICE = {"HISPMV_LAYOUT": "host"}, {"HISPMV_LAYOUT": "device"}
BATCHED = {"HISPMV_FORMAT": "slices", "HISPMV_BATCH_STREAMS": "2", "HISPMV_BATCH_LAYOUT": "1"}      # tests/test_gpu_parity.py: test_batch_layout_of_short_groups


def empty():
    return S._finish("empty_40x30", 40, 30, [], [], 90, dict(format=0))


def dense(rows=17, cols=33, seed=7):
    rng = np.random.default_rng(seed)
    m = S._finish(f"dense_{rows}x{cols}", rows, cols, [], [], seed, dict(dense=True))
    return dict(m, dense=True, W=rng.random((rows, cols), dtype=np.float32) - np.float32(0.5))


def cases():
    out = [(S.one_by_one(), S.SLICES, ""), (empty(), S.SLICES, ""),
           (S.uniform(40, 30, 200, 5, dict(format=0)), S.SLICES, ""), (S.two_way_band(), S.NOSPLIT, "")]
    for layout in (HOST, DEVICE):           # the three header / stray cases; a batch layout packed on the host and laid out on the device
        big = S.big_band()
        out += [(S.stray_slot_band(), dict(S.SLICES, **layout), ""), (dict(big, expect=dict(big["expect"], batch_layout=True)), dict(BATCHED, **layout), "")]
    out += [(S.stray_split_band(), S.SLICES, ""), (S.column_tiled(), S.COLTILES, ""),
            (S.tile_stream(), S.AUTO, ""), (S.tile_stream_cut_row(), S.AUTO, "")]
    out += [(S.tall(S.tile_stream(), g), dict(S.tall_env(g), HISPMV_TTS_MIN_NNZ="20000"), "") for g in ("tall", "tallgap")]
    out += [(dense(), {}, v) for v in ("", "bf16", "upd", "bf16upd")]
    for v in ("upd", "bf16", "bf16upd", "companion"):
        out += [(S.two_way_band(), S.NOSPLIT, v), (S.stray_slot_band(), S.SLICES, v), (S.tile_stream(), S.AUTO, v)]
    return out


def sha(t):
    return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()


def fingerprint(m, env, variant, torch, pyhispmv):
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(3)
    is_dense = bool(m.get("dense"))
    with S.environment(env):
        h = pyhispmv.FpgaHandle(*HW)
        if "bf16" in variant:
            h.set_value_storage("bf16")
        if "upd" in variant:
            h.set_value_updates("any_storage" if "bf16" in variant else True)
        if variant == "companion":
            h.set_transposable("companion")
        k = h.create_dense_handle(m["W"].flatten(), m["rows"], m["cols"]) if is_dense else h.create_sparse_handle(m["r"], m["c"], m["v"], m["rows"], m["cols"])
        h.set_value_updates(False), h.set_value_storage("fp32"), h.set_transposable(False)
        one = S.one_by_one()
        k1 = h.create_sparse_handle(one["r"], one["c"], one["v"], 1, 1)
        h.load_matrices()
        info = h.matrix_info(k)
        e = m["expect"]
        assert bool(info["is_dense"]) == is_dense and (is_dense or (info["format"] == e["format"] and info["col_tiles"] == e.get("parts", 1))), (m["name"], env, info)
        assert not e.get("batch_layout") or info["batch_group_slices"] > info["group_slices"], (m["name"], env, info)
        line = dict(case=m["name"], env=env, variant=variant, matrix_info={a: b for a, b in info.items() if a != "prep_seconds"},
                    transpose_info=h.transpose_info(k), companion_info=h.companion_info(k), value_update_info=h.value_update_info(k),
                    value_storage_info=h.value_storage_info(k), linear_info=h.linear_info(k, 5), arena_bytes_used=h.arena_bytes_used())
        y = np.zeros(m["rows"], np.float32)
        h.select_matrix(k)
        h.run_kernel(m["x"], m["b"], y, 1.0, 1.0)
        line["run_kernel"] = hashlib.sha256(y.tobytes()).hexdigest()
        x, b, x1, b1 = (torch.from_numpy(a).to(dev) for a in (m["x"], m["b"], one["x"], one["b"]))
        yd, y1 = torch.zeros(m["rows"], device=dev), torch.zeros(1, device=dev)
        h.spmv_device(k, x.data_ptr(), b.data_ptr(), yd.data_ptr(), ALPHA, BETA)
        h.synchronize()
        line["spmv_device"] = sha(yd)
        yd.zero_()
        batch = h.prepare_batch([k, k1], [x.data_ptr(), x1.data_ptr()], [b.data_ptr(), b1.data_ptr()], [yd.data_ptr(), y1.data_ptr()])
        h.spmv_device_batch(batch, ALPHA, BETA)
        h.synchronize()
        line["spmv_device_batch"] = [sha(yd), sha(y1), h.batch_call_info()]
        if "upd" in variant:
            h.update_values(k, rng.random(m["W"].size if is_dense else m["v"].size, dtype=np.float32) - np.float32(0.5))
            yd.zero_()
            h.spmv_device(k, x.data_ptr(), b.data_ptr(), yd.data_ptr(), ALPHA, BETA)
            h.synchronize()
            line["spmv_device_updated"] = sha(yd)
        if variant == "companion":          # two vectors [2, rows] -> [2, cols], one shared bias
            xt = torch.from_numpy(rng.random(2 * m["rows"], dtype=np.float32)).to(dev)
            yt = torch.zeros(2 * m["cols"], device=dev)
            h.linear_device_t(k, xt.data_ptr(), 2, x.data_ptr(), yt.data_ptr(), ALPHA, BETA)
            h.synchronize()
            line["linear_device_t"] = sha(yt)
        h.close()
    return line


def main():
    import torch
    import pyhispmv
    for m, env, variant in cases():
        print(json.dumps(fingerprint(m, env, variant, torch, pyhispmv), sort_keys=True), flush=True)


if __name__ == "__main__":
    main()
