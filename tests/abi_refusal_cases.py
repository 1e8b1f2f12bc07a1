"""The refusals of the device-pointer entries of the C ABI, as (return code, hispmv_last_error text) per case: the case list of
tests/test_gpu_abi_refusals.py and the function that collects it from whatever library hispmv_amd._lib loaded (HISPMV_LIB).

    python tests/abi_refusal_cases.py out.json          # on a GPU: how tests/golden/abi_refusals.json was made

Handle kinds, each at the smallest size that yields the kind: a 40 x 30 slice stream, a 17 x 33 dense handle, the 40 x 30 matrix again
updatable, with a stored transpose and as an updatable dense handle (all under HISPMV_FORMAT=slices), and -- the loader makes no tile
stream below 20 000 entries and 64 K columns -- the tile streams of tests/step_small_cases.py created with transposable off (one of them
updatable) and one whose stored transpose is a tile stream.  A third context holds the small handles before load_matrices.

Every case calls one entry with the arguments of a call that would be accepted -- every pointer a device allocation large enough for
that handle and entry -- but for the one thing the case is about.  A case that is NOT refused (a handle kind the entry accepts) computes
on those buffers; its text is recorded as "".  No product code; not a test module and not a conftest."""
from __future__ import annotations

import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for _p in (ROOT, ROOT / "tests"):
    if str(_p) not in sys.path:
        sys.path.insert(0, str(_p))

import step_small_cases as S  # noqa: E402

HW = ("tests.xclbin", 0, 24, 1, 1, 2, 5, True, False, True)
NV = 3
ENTRIES = ("spmv_device", "spmv_device_t", "linear_device", "linear_device_t", "value_grad_device", "spmm_device", "spmm_device_t",
           "spmm_device_bf16", "spmm_device_t_bf16", "spmm_value_grad_device", "update_values_device")
WIDE = ("spmm_device", "spmm_device_t", "spmm_device_bf16", "spmm_device_t_bf16")


def small():
    return S.uniform(40, 30, 200, 7, {}, name="small")


def transposed(m):
    return dict(m, rows=m["cols"], cols=m["rows"], r=m["c"], c=m["r"])


class Context:
    """One library context with some handles and one set of device buffers every handle's calls fit in."""

    def __init__(self, torch, env, make, load=True):
        import pyhispmv
        from hispmv_amd._lib import lib
        self.lib, self.torch = lib, torch
        with S.environment(env):
            self.h = pyhispmv.FpgaHandle(*HW)
            try:
                self.kinds = make(self.h)          # name -> handle index
                if load:
                    self.h.load_matrices()
            except BaseException:
                self.h.close()
                raise
        self.ctx = self.h._ctx
        dims = [self.h.matrix_info(k) for k in self.kinds.values()]
        n = NV * max(max(i["rows"], i["cols"]) for i in dims) + 64
        zeros = lambda count: torch.zeros(int(count), dtype=torch.float32, device="cuda")          # noqa: E731
        self.x, self.y, self.bias = zeros(n), zeros(n), zeros(n)
        self.n_values = {k: max(self.h.value_update_info(k)["n"], self.h.matrix_info(k)["nnz"]) for k in self.kinds.values()}
        self.values = zeros(max(self.n_values.values()) + 64)
        self.grad = zeros(self.values.numel())
        self.work = zeros(1 << 20)
        torch.cuda.synchronize()

    def close(self):
        self.torch.cuda.synchronize()
        self.h.close()

    def good(self, k):
        """The arguments of an accepted call on handle k, by name; an entry takes the ones it has."""
        return dict(idx=k, x=self.x.data_ptr(), y=self.y.data_ptr(), bias=self.bias.data_ptr(), nv=NV, stride=0, ld_x=NV, ld_y=NV, alpha=1.0, beta=1.0,
                    work=self.work.data_ptr(), work_bytes=4 * self.work.numel(), grad=self.grad.data_ptr(), values=self.values.data_ptr(),
                    n=self.n_values[k])

    def call(self, entry, a):
        """-> [return code, text]: one call, then hispmv_synchronize, which must return OK whatever the call did."""
        p, lib, c = C.c_void_p, self.lib, self.ctx
        if entry in ("spmv_device", "spmv_device_t"):
            rc = getattr(lib, "hispmv_" + entry)(c, a["idx"], p(a["x"]), p(a["bias"]), p(a["y"]), a["alpha"], a["beta"], None)
        elif entry == "linear_device":
            rc = lib.hispmv_linear_device(c, a["idx"], p(a["x"]), a["nv"], p(a["bias"]), p(a["y"]), a["alpha"], a["beta"], None)
        elif entry == "linear_device_t":
            rc = lib.hispmv_linear_device_t(c, a["idx"], p(a["x"]), a["nv"], p(a["bias"]), a["stride"], p(a["y"]), a["alpha"], a["beta"], None)
        elif entry == "value_grad_device":
            rc = lib.hispmv_value_grad_device(c, a["idx"], p(a["y"]), p(a["x"]), a["nv"], p(a["grad"]), a["alpha"], a["beta"], None)
        elif entry in WIDE:
            rc = getattr(lib, "hispmv_" + entry)(c, a["idx"], p(a["x"]), a["nv"], a["ld_x"], p(a["bias"]), a["stride"], p(a["y"]), a["ld_y"], a["alpha"], a["beta"],
                                                 p(a["work"]), a["work_bytes"], None)
        elif entry == "spmm_value_grad_device":
            rc = lib.hispmv_spmm_value_grad_device(c, a["idx"], p(a["y"]), a["ld_y"], p(a["x"]), a["ld_x"], a["nv"], p(a["grad"]), a["alpha"], a["beta"], None)
        elif entry == "update_values_device":
            rc = lib.hispmv_update_values_device(c, a["idx"], p(a["values"]), a["n"], None)
        else:
            raise KeyError(entry)
        text = lib.hispmv_last_error(c).decode() if rc != 0 else ""
        assert lib.hispmv_synchronize(c) == 0, (entry, a, lib.hispmv_last_error(c).decode())
        return [int(rc), text]


def argument_cases(cx, entry, k):
    """name -> arguments: every refusal `entry` has for its arguments, on a handle k that it accepts."""
    g = cx.good(k)
    out = {"idx_minus_1": dict(g, idx=-1), "idx_past_the_end": dict(g, idx=cx.h.num_matrices())}
    if entry == "update_values_device":
        out.update(null_values=dict(g, values=None), wrong_n=dict(g, n=g["n"] + 1))
        return out
    out.update(null_x=dict(g, x=None), null_y=dict(g, y=None), x_is_y=dict(g, y=g["x"]))
    if entry in ("value_grad_device", "spmm_value_grad_device"):
        out.update(null_grad=dict(g, grad=None), grad_is_x=dict(g, grad=g["x"]), grad_is_gy=dict(g, grad=g["y"]))
        del out["x_is_y"]          # (gy and x may be the same vectors)
    else:
        out.update(null_bias=dict(g, bias=None), null_bias_beta_0=dict(g, bias=None, beta=0.0))
    if entry not in ("spmv_device", "spmv_device_t"):
        out.update(num_vecs_0=dict(g, nv=0))
    if entry == "linear_device_t" or entry in WIDE:
        out.update(bad_bias_stride=dict(g, stride=7), shared_bias_in_place=dict(g, bias=g["y"]))
    if entry in WIDE or entry == "spmm_value_grad_device":
        out.update(ld_x_below_num_vecs=dict(g, ld_x=NV - 1), ld_y_below_num_vecs=dict(g, ld_y=NV - 1),
                   misaligned_x=dict(g, x=g["x"] + (1 if "bf16" in entry else 2)), misaligned_y=dict(g, y=g["y"] + (1 if "bf16" in entry else 2)))
    if entry in WIDE:
        info = (cx.h.spmm_bf16_info if "bf16" in entry else cx.h.spmm_info)(k, NV)
        need = info["work_bytes_t" if "_t" in entry else "work_bytes"]
        assert need > 0, info
        out.update(misaligned_work=dict(g, work=g["work"] + 2), misaligned_shared_bias=dict(g, bias=g["bias"] + 2),
                   short_workspace=dict(g, work_bytes=need - 1), exact_workspace=dict(g, work_bytes=need), null_workspace=dict(g, work=None))
    return out


def collect(torch):
    """-> {"<context>/<entry>/<handle kind>/<case>": [return code, text]} in a fixed order."""
    out = {}
    m, mt = small(), transposed(small())
    W = np.arange(17 * 33, dtype=np.float32)

    def small_handles(h):
        k = {}
        k["slices"] = h.create_sparse_handle(m["r"], m["c"], m["v"], m["rows"], m["cols"])
        k["dense"] = h.create_dense_handle(W, 17, 33)
        h.set_transposable("companion")
        k["stored_transpose"] = h.create_sparse_handle(m["r"], m["c"], m["v"], m["rows"], m["cols"])
        h.set_transposable(0)
        h.set_value_updates(True)
        k["updatable"] = h.create_sparse_handle(m["r"], m["c"], m["v"], m["rows"], m["cols"])
        k["updatable_dense"] = h.create_dense_handle(W, 17, 33)
        h.set_value_updates(False)
        return k

    def tile_handles(h):
        t, tc = S.tile_stream(), transposed(S.tile_stream_cut_row())
        k = {}
        k["tile_stream"] = h.create_sparse_handle(t["r"], t["c"], t["v"], t["rows"], t["cols"])
        h.set_value_updates(True)
        k["updatable_tile_stream"] = h.create_sparse_handle(t["r"], t["c"], t["v"], t["rows"], t["cols"])
        h.set_value_updates(False)
        h.set_transposable("companion")
        k["tile_stream_stored_transpose"] = h.create_sparse_handle(tc["r"], tc["c"], tc["v"], tc["rows"], tc["cols"])
        h.set_transposable(0)
        return k

    # handle kind an entry's argument cases run on: one it accepts
    accepted = {e: "slices" for e in ENTRIES}
    accepted.update(spmm_device_t="stored_transpose", spmm_device_t_bf16="stored_transpose", value_grad_device="updatable",
                    spmm_value_grad_device="updatable", update_values_device="updatable")

    cx = Context(torch, S.SLICES, small_handles)
    try:
        assert [cx.h.matrix_info(k)["format"] for k in cx.kinds.values()] == [0, 0, 0, 0, 0]
        assert cx.h.companion_info(cx.kinds["stored_transpose"])["has"] and cx.h.companion_info(cx.kinds["stored_transpose"])["format"] == 0
        for e in ENTRIES:
            for kind, k in cx.kinds.items():          # wrong (and right) handle kinds, accepted arguments otherwise
                out[f"small/{e}/{kind}/accepted_arguments"] = cx.call(e, cx.good(k))
            for name, a in argument_cases(cx, e, cx.kinds[accepted[e]]).items():
                out[f"small/{e}/{accepted[e]}/{name}"] = cx.call(e, a)
        # linear_device_t over the stored transpose takes the same argument checks before it branches
        for name, a in argument_cases(cx, "linear_device_t", cx.kinds["stored_transpose"]).items():
            out[f"small/linear_device_t/stored_transpose/{name}"] = cx.call("linear_device_t", a)
    finally:
        cx.close()

    cx = Context(torch, S.AUTO, tile_handles)
    try:
        assert [cx.h.matrix_info(k)["format"] for k in cx.kinds.values()][:2] == [1, 1]
        assert cx.h.companion_info(cx.kinds["tile_stream_stored_transpose"])["format"] == 1
        for e in ENTRIES:
            for kind, k in cx.kinds.items():
                out[f"tile/{e}/{kind}/accepted_arguments"] = cx.call(e, cx.good(k))
    finally:
        cx.close()

    cx = Context(torch, S.SLICES, small_handles, load=False)
    try:
        for e in ENTRIES:
            for kind, k in cx.kinds.items():
                out[f"not_loaded/{e}/{kind}/accepted_arguments"] = cx.call(e, cx.good(k))
    finally:
        cx.close()
    return out


if __name__ == "__main__":
    import torch
    cases = collect(torch)
    Path(sys.argv[1]).write_text(json.dumps(cases, indent=0, sort_keys=True) + "\n")
    print(f"{len(cases)} cases -> {sys.argv[1]}")
