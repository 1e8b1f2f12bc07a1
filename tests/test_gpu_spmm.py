"""The wide-batch product yt[rows, B] = alpha * A xt[cols, B] + beta * bias on feature-major operands (hispmv_spmm_device;
hispmv_spmm.hip) on loaded slice-stream handles, at the small shapes of tests/step_small_cases.py: every group kind (no window,
compact and wide windows, stray slots, half groups, 256 and 1024 threads) and every multi-part handle (two parts of a stray split,
eight column parts).  Each handle's plan is asserted with check_expect (the context helper of tests/test_gpu_transpose.py).

Batches B in {1, 64, 65, 200, 257}, ld_x = ld_y = B rounded up to 4; once per class ld = B + 3 with xt, yt and the workspace moved by
one float (VL = 1).  Vector v is pool[v % 16] * 2^((v // 16) % 5 - 2): 16 pool vectors per matrix (pool[1] is all zeros, so vector 1
is), scaled by powers of two, which scale every product and sum exactly.  The truth of a pool vector is csr_truth's fp64 accumulation
(oracle.spmv_f64 on the CSR sorted once per matrix) with its magnitude sum; the truth of vector v follows from it exactly.

Gates: (a) per vector bwd_err < TOL = 1e-5 for the four (alpha, beta) pairs, alpha = 0 giving exactly beta * bias.  A sequential fp32
sum in stream order, simulated on the CPU for single_row, single_row_long, big_band, the windowed uniform and xlds_A, stayed <= 1.6e-7,
so the gate has about 60x room.  (b) the zero vector's product is exactly zero for beta = 0.  (c) vectors 0, 63, 64, 199, 256 of the
B = 65, 200 and 257 calls equal bit for bit the B = 1 call on that vector alone.  (d) two identical calls give identical bits.
(e) spmm_info reports the VL and tiles of hispmv_prep_spmm_tiles and launches = tiles * sum over the parts of (1 + 1 if the part has
a cut row).  (f) beta = 0 with a NaN-filled and with a NULL bias gives finite y.  (g) bias_stride = ld_y with d_bias == d_yt
accumulates in place.  (h) spmv_device on the handle gives identical bits before and after the wide calls.  yt starts as NaN inside a
tensor of sentinel words; every word outside [rows, B] -- the pad columns B .. ld - 1 included -- and every word around the workspace
must still be the sentinel.  The pad columns of xt hold NaN."""
import zlib

import numpy as np
import pytest

import step_small_cases as S
from conftest import TOL
from test_gpu_transpose import _PACKS, Ctx
from util import bwd_err

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0x5EA15EA1
ALL_PAIRS = S.PAIRS + S.MORE_PAIRS
BATCHES = (1, 64, 65, 200, 257)
PROBES = (0, 63, 64, 199, 256)
POOL = 16
_TRUTH = {}


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def scale_of(v):
    return np.float32(2.0 ** ((v // POOL) % 5 - 2))


def pool_of(m, n_in):
    rng = np.random.default_rng(zlib.crc32(m.get("pool_key", m["name"]).encode()) + 1)
    p = rng.random((POOL, n_in), dtype=np.float32) - np.float32(0.3)
    p[1] = 0.0
    return p


def batch(pool, B):
    return np.stack([pool[v % POOL] * scale_of(v) for v in range(B)])


def pool_truth(m):
    """Per pool vector (sum_k a_rk x_k, sum_k |a_rk x_k|) in fp64: csr_truth's accumulation, the CSR sorted once per matrix."""
    if m["name"] not in _TRUTH:
        import oracle
        order = np.lexsort((m["c"], m["r"]))
        rp = np.zeros(m["rows"] + 1, np.int64)
        np.add.at(rp, np.asarray(m["r"], np.int64) + 1, 1)
        rp = np.cumsum(rp).astype(np.int32)
        ci, va = np.asarray(m["c"], np.int32)[order], np.asarray(m["v"], np.float32)[order]
        zero = np.zeros(m["rows"], np.float32)
        pool = pool_of(m, m["cols"])
        out = [oracle.spmv_f64(rp, ci, va, pool[p], zero, 1.0, 0.0) for p in range(POOL)]
        _TRUTH[m["name"]] = (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]))
    return _TRUTH[m["name"]]


def truth(m, vecs, bias64, alpha, beta):
    """(y64, mag) [len(vecs), rows] for the vectors `vecs` of the batch; bias64 is [rows] or [len(vecs), rows]."""
    s, a = pool_truth(m)
    sc = np.array([float(scale_of(v)) for v in vecs])[:, None]
    idx = [v % POOL for v in vecs]
    bb = beta * np.asarray(bias64, np.float64)
    return alpha * s[idx] * sc + bb, abs(alpha) * a[idx] * sc + np.abs(bb)


class Wide:
    """The wide calls of one matrix of a Ctx: operands built on the host, framed with sentinels, checked after every call."""

    def __init__(self, cx, k, t=False):
        self.cx, self.k, self.t, self.m = cx, k, t, cx.mats[k]
        self.n_in = self.m["rows"] if t else self.m["cols"]
        self.n_out = self.m["cols"] if t else self.m["rows"]
        self.pool = pool_of(self.m, self.n_in)
        self._xt = {}

    def xt(self, X, ld, shift):
        """xt [n_in, ld] on the device (pad columns NaN), cached per batch of the pool: -> (tensor, pointer)."""
        key = (X.shape[0], ld, shift, bits(X[:, :8]).tobytes())
        if key not in self._xt:
            a = np.full(self.n_in * ld + shift, np.nan, np.float32)
            a[shift:].reshape(self.n_in, ld)[:, :X.shape[0]] = X.T
            self._xt = {key: self.cx.device(a)}               # (one at a time: the largest is 200 MB)
        d = self._xt[key]
        return d, d.data_ptr() + 4 * shift

    def call(self, X, b, alpha, beta, ld=None, shift=0, bias="given", work_bytes=None):
        """One call -> Y [B, n_out] (numpy).  bias: "given" (b = [n_out], shared), "null", "nan" (a NaN-filled shared bias), "in_place"
        (b = [B, n_out]: yt holds it and is passed as the bias with bias_stride = ld)."""
        cx, torch, h, idx = self.cx, self.cx.torch, self.cx.h, self.cx.idx[self.k]
        B = X.shape[0]
        ld = (B + 3) & ~3 if ld is None else ld
        dX, px = self.xt(X, ld, shift)
        n = self.n_out * ld
        Y0 = np.full(n + 2 * GUARD + shift, SENTINEL, np.int32).view(np.float32)
        lo = GUARD + shift
        Y0[lo:lo + n].reshape(self.n_out, ld)[:, :B] = np.asarray(b, np.float32).T if bias == "in_place" else np.nan
        dY = cx.device(Y0)
        py = dY.data_ptr() + 4 * lo
        info = h.spmm_info(idx, B, ld)
        need = info["work_bytes_t" if self.t else "work_bytes"]
        wb = need if work_bytes is None else work_bytes
        dW = cx.device(np.full(need // 4 + 2 * GUARD + shift, SENTINEL, np.int32).view(np.float32))
        pw = dW.data_ptr() + 4 * lo
        dB, pb, stride = None, 0, 0
        if bias == "given":
            dB = cx.device(b)
            pb = dB.data_ptr()
        elif bias == "nan":
            dB = cx.device(np.full(self.n_out, np.nan, np.float32))
            pb = dB.data_ptr()
        elif bias == "in_place":
            pb, stride = py, ld
        torch.cuda.synchronize()
        (h.spmm_device_t if self.t else h.spmm_device)(idx, px, B, pb, py, alpha, beta, ld_x=ld, ld_y=ld, bias_stride=stride, work=pw, work_bytes=wb)
        h.synchronize()
        out = dY.cpu().numpy()
        inside = np.zeros(out.size, bool)
        inside[lo:lo + n].reshape(self.n_out, ld)[:, :B] = True
        assert (out.view(np.int32)[~inside] == SENTINEL).all(), f'{self.m["name"]}: words outside yt[rows, B] were written (B={B}, ld={ld})'
        w = dW.cpu().numpy().view(np.int32)
        assert (w[:lo] == SENTINEL).all() and (w[lo + need // 4:] == SENTINEL).all(), f'{self.m["name"]}: words around the workspace were written'
        return out[lo:lo + n].reshape(self.n_out, ld)[:, :B].T.copy()

    def gate(self, Y, vecs, bias64, alpha, beta, what):
        y64, mag = self.truth(vecs, bias64, alpha, beta)
        assert np.isfinite(Y).all(), (self.m["name"], what)
        err = max(bwd_err(Y[i], y64[i], mag[i]) for i in range(len(vecs)))
        print(f'{self.m["name"]}: {what} alpha={alpha} beta={beta} worst backward error of {len(vecs)} vectors {err:.3e}')
        assert err < TOL, (self.m["name"], what, alpha, beta, err)

    def truth(self, vecs, bias64, alpha, beta):
        assert not self.t
        return truth(self.m, vecs, bias64, alpha, beta)


def expected_launches(cx, k, tiles):
    info = cx.info[k]
    key = (cx.mats[k]["name"], info["format"], info["col_tiles"], info["tile_kind"], info["col_tile_width"], info["col_tile_base"], info["group_slices"])
    cuts = S.cut_rows(info, _PACKS[key])
    assert len(cuts) == info["col_tiles"]
    return tiles * sum(1 + (1 if n > 0 else 0) for n in cuts)


def run_class(cx, k):
    """Every gate of the module docstring on matrix k of the context."""
    from hispmv_amd import prep
    m, h, idx = cx.mats[k], cx.h, cx.idx[k]
    w = Wide(cx, k)
    b = m["b"]
    before = cx.spmv(k, m["x"], b, 0.85, -2.06)
    ones = {}
    for v in PROBES:                                        # the B = 1 call on vector v alone
        ones[v] = w.call(batch(w.pool, v + 1)[v:], b, *S.PAIRS[0])[0]
    for B in BATCHES:
        X = batch(w.pool, B)
        ld = (B + 3) & ~3
        info, tiles = h.spmm_info(idx, B, ld), prep.spmm_tiles(m["cols"], B, ld, 16)
        assert info["accepted"] and (info["vl"], info["tiles"]) == (tiles["vl"], tiles["tiles"]), (m["name"], B, info, tiles)      # (e)
        assert info["launches"] == expected_launches(cx, k, tiles["tiles"]) <= 2 * tiles["tiles"] * cx.info[k]["col_tiles"], (m["name"], B, info)
        for alpha, beta in ALL_PAIRS:
            Y = w.call(X, b, alpha, beta, bias="given" if beta != 0.0 else "null")
            w.gate(Y, range(B), b, alpha, beta, f"B={B}")                                                                         # (a)
            if alpha == 0.0:
                assert all(np.array_equal(bits(Y[v]), bits(np.float32(beta) * b)) for v in range(B)), (m["name"], B)
            if beta == 0.0 and B > 1:
                assert (Y[1] == 0.0).all(), (m["name"], B)                                                                        # (b)
            if (alpha, beta) == S.PAIRS[0]:
                for v in PROBES:
                    if v < B:
                        assert np.array_equal(bits(Y[v]), bits(ones[v])), (m["name"], B, v)                                       # (c)
                if B == 257:
                    again = w.call(X, b, alpha, beta)
                    assert np.array_equal(bits(Y), bits(again)), m["name"]                                                        # (d)
    # ld = B + 3 with every operand moved by one float: VL = 1, four-byte aligned rows
    B = 65
    X = batch(w.pool, B)
    assert prep.spmm_tiles(m["cols"], B, B + 3, 4) == dict(vl=1, tiles=2, last_vecs=1, vl_last=1)
    Y = w.call(X, b, *S.PAIRS[0], ld=B + 3, shift=1)
    w.gate(Y, range(B), b, *S.PAIRS[0], "B=65 ld=68 shifted")
    for v in (0, 63, 64):
        assert np.array_equal(bits(Y[v]), bits(ones[v])), (m["name"], "shifted", v)
    for bias in ("nan", "null"):                                                                                                  # (f)
        Y = w.call(X, b, 1.0, 0.0, bias=bias)
        w.gate(Y, range(B), b, 1.0, 0.0, f"bias {bias}")
    rng = np.random.default_rng(5)
    Bm = rng.random((B, m["rows"]), dtype=np.float32)
    Y = w.call(X, Bm, -1.5, 0.5, bias="in_place")                                                                                  # (g)
    w.gate(Y, range(B), Bm, -1.5, 0.5, "in place")
    after = cx.spmv(k, m["x"], b, 0.85, -2.06)
    assert np.array_equal(bits(before), bits(after)), m["name"]                                                                   # (h)


def test_plans_without_a_window(torch_mod):
    """256 threads, no window: the six plain matrices of case A (nnz = 0 and 1024 among them)."""
    mats = S.case_a()[:6]
    with Ctx(torch_mod, S.SLICES, mats) as cx:
        for k in range(len(mats)):
            assert cx.info[k]["block_threads"] == 256 and cx.info[k]["lds_bytes"] == 0, cx.info[k]
            run_class(cx, k)


@pytest.mark.parametrize("make", [S.one_by_one, S.single_row, S.single_row_long, S.sparse_rows],
                         ids=["one_by_one", "single_row", "single_row_long", "sparse_rows"])
def test_chains_and_fillers(torch_mod, make):
    """The 1 x 1 matrix; one row over some thirty slices (the chain of partial sums); a chain of more than kFixShortMax slices; 50
    live rows among 49 950 fillers."""
    m = make()
    with Ctx(torch_mod, S.SLICES, [m]) as cx:
        assert cx.info[0]["block_threads"] == 256 and cx.info[0]["lds_bytes"] == 0, cx.info[0]
        if m["name"].startswith("single_row"):
            assert cx.h.spmm_info(cx.idx[0], 4)["launches"] == 2, m["name"]
        run_class(cx, 0)


def test_compact_windows_256_threads(torch_mod):
    mats = S.case_a()[6:8]
    with Ctx(torch_mod, S.SLICES, mats) as cx:
        assert all(i["block_threads"] == 256 and i["lds_bytes"] > 0 and i["compact_slices"] == i["n_slices"] for i in cx.info), cx.info
        for k in range(2):
            run_class(cx, k)


def test_wide_groups_with_a_window_and_l2_elements(torch_mod):
    m = S.two_way_band()
    with Ctx(torch_mod, S.NOSPLIT, [m]) as cx:
        assert cx.info[0]["compact_slices"] == 0 and cx.info[0]["lds_bytes"] > 0, cx.info[0]
        run_class(cx, 0)


def test_1024_threads_compact(torch_mod):
    m = S.big_band()
    with Ctx(torch_mod, S.SLICES, [m]) as cx:
        assert cx.info[0]["block_threads"] == 1024 and cx.info[0]["compact_slices"] == cx.info[0]["n_slices"], cx.info[0]
        run_class(cx, 0)


def test_stray_slots(torch_mod):
    m = S.stray_slot_band()
    with Ctx(torch_mod, S.SLICES, [m]) as cx:
        assert cx.info[0]["block_threads"] == 1024 and cx.info[0]["compact_slices"] == cx.info[0]["n_slices"], cx.info[0]
        run_class(cx, 0)


def test_two_parts_of_a_stray_split(torch_mod):
    m = S.stray_split_band()
    with Ctx(torch_mod, S.SLICES, [m]) as cx:
        assert cx.info[0]["tile_kind"] == 3 and cx.info[0]["col_tiles"] == 2, cx.info[0]
        run_class(cx, 0)


def test_eight_column_parts(torch_mod):
    m = S.column_tiled()
    with Ctx(torch_mod, S.COLTILES, [m]) as cx:
        assert cx.info[0]["tile_kind"] == 1 and cx.info[0]["col_tiles"] == 8, cx.info[0]
        assert cx.h.spmm_info(cx.idx[0], 64)["launches"] == 16
        run_class(cx, 0)


@pytest.mark.parametrize("make", [S.big_band, S.stray_slot_band], ids=["big_band", "stray_slot_band"])
def test_half_groups(torch_mod, make):
    m = S.as_bf16(make())
    with Ctx(torch_mod, S.SLICES, [m]) as cx:
        st = cx.h.value_storage_info(cx.idx[0])
        assert st["storage"] == "bf16" and st["slots_2byte"] > 0, st
        run_class(cx, 0)


def test_tile_stream_and_dense_handles_are_refused(torch_mod):
    m, d = S.tile_stream(), S.dense_shapes()[1]
    with Ctx(torch_mod, S.AUTO, [m, d]) as cx:
        assert cx.info[0]["format"] == 1
        for k, match in ((0, "set_transposable"), (1, "dense")):
            info = cx.h.spmm_info(cx.idx[k], 8)
            assert info == dict(accepted=False, accepted_t=False, vl=0, tiles=0, launches=0, work_bytes=0, work_bytes_t=0), info
            t = torch_mod.zeros(8 * (cx.mats[k]["rows"] + cx.mats[k]["cols"]) + 64, dtype=torch_mod.float32, device="cuda")
            with pytest.raises(NotImplementedError, match=match):
                cx.h.spmm_device(cx.idx[k], t.data_ptr(), 8, 0, t.data_ptr() + 32 * cx.mats[k]["cols"], work=t.data_ptr(), work_bytes=0)
            with pytest.raises(NotImplementedError, match="companion"):
                cx.h.spmm_device_t(cx.idx[k], t.data_ptr(), 8, 0, t.data_ptr() + 32 * cx.mats[k]["rows"], work=t.data_ptr(), work_bytes=0)
            if k == 0:
                from hispmv_amd.torch_ops import sparse_linear
                with pytest.raises(NotImplementedError):
                    sparse_linear(cx.h, cx.idx[k], t[:8 * m["cols"]].view(8, m["cols"]), spmm=True)
    with Ctx(torch_mod, S.AUTO, [S.as_slices(m)], transposable=True) as cx:
        assert cx.info[0]["format"] == 0
        w = Wide(cx, 0)
        Y = w.call(batch(w.pool, 65), m["b"], *S.PAIRS[0])
        w.gate(Y, range(65), m["b"], *S.PAIRS[0], "kept a slice stream")


def test_argument_errors_come_before_any_launch(torch_mod):
    """A workspace too small and ld < B are HISPMV_EINVAL (ValueError); yt is untouched."""
    m = S.case_a()[7]
    with Ctx(torch_mod, S.SLICES, [m]) as cx:
        h, idx, B = cx.h, cx.idx[0], 8
        need = h.spmm_info(idx, B)["work_bytes"]
        assert need > 0
        xt = torch_mod.zeros(m["cols"] * B, dtype=torch_mod.float32, device="cuda")
        yt = torch_mod.full((m["rows"] * B,), 7.0, dtype=torch_mod.float32, device="cuda")
        wk = torch_mod.zeros(need // 4, dtype=torch_mod.float32, device="cuda")
        with pytest.raises(ValueError, match="workspace"):
            h.spmm_device(idx, xt.data_ptr(), B, 0, yt.data_ptr(), work=wk.data_ptr(), work_bytes=need - 4)
        with pytest.raises(ValueError, match="workspace"):
            h.spmm_device(idx, xt.data_ptr(), B, 0, yt.data_ptr(), work=0, work_bytes=need)
        with pytest.raises(ValueError, match="at least num_vecs"):
            h.spmm_device(idx, xt.data_ptr(), B, 0, yt.data_ptr(), ld_x=B - 1, work=wk.data_ptr(), work_bytes=need)
        with pytest.raises(ValueError, match="at least num_vecs"):
            h.spmm_device(idx, xt.data_ptr(), B, 0, yt.data_ptr(), ld_y=B - 1, work=wk.data_ptr(), work_bytes=need)
        with pytest.raises(ValueError):
            h.spmm_device(idx, xt.data_ptr(), 0, 0, yt.data_ptr(), ld_x=B, ld_y=B, work=wk.data_ptr(), work_bytes=need)
        with pytest.raises(ValueError):
            h.spmm_device(idx, xt.data_ptr(), B, 0, yt.data_ptr(), beta=1.0, work=wk.data_ptr(), work_bytes=need)          # beta != 0 without a bias
        with pytest.raises(ValueError):
            h.spmm_device(idx, xt.data_ptr(), B, 0, yt.data_ptr(), bias_stride=3, work=wk.data_ptr(), work_bytes=need)
        with pytest.raises(IndexError):
            h.spmm_device(99, xt.data_ptr(), B, 0, yt.data_ptr(), work=wk.data_ptr(), work_bytes=need)
        with pytest.raises(NotImplementedError, match="companion"):
            h.spmm_device_t(idx, yt.data_ptr(), B, 0, xt.data_ptr(), work=wk.data_ptr(), work_bytes=need)
        h.synchronize()
        assert (yt == 7.0).all()


def test_refused_before_load_matrices(torch_mod):
    import pyhispmv
    from step_small_harness import HW
    m = S.case_a()[1]
    h = pyhispmv.FpgaHandle(*HW)
    try:
        i = h.create_sparse_handle(m["r"], m["c"], m["v"], m["rows"], m["cols"])
        d = torch_mod.zeros(4 * (m["rows"] + m["cols"]) + (1 << 16), dtype=torch_mod.float32, device="cuda")
        with pytest.raises(AssertionError, match="before load_matrices"):
            h.spmm_device(i, d.data_ptr(), 4, 0, d.data_ptr() + 16 * m["cols"], work=d.data_ptr() + 16 * (m["rows"] + m["cols"]), work_bytes=1 << 16)
        with pytest.raises(AssertionError, match="before load_matrices"):
            h.spmm_device_t(i, d.data_ptr(), 4, 0, d.data_ptr() + 16 * m["rows"], work=d.data_ptr() + 16 * (m["rows"] + m["cols"]), work_bytes=1 << 16)
        assert not h.spmm_info(i, 4)["accepted"]
        h.load_matrices()
        assert h.spmm_info(i, 4)["accepted"]
    finally:
        h.close()


def test_updated_values_reach_the_wide_product(torch_mod):
    m = S.case_a()[7]
    with Ctx(torch_mod, S.SLICES, [m], updates=True) as cx:
        assert cx.h.value_update_info(cx.idx[0])["updatable"]
        w = Wide(cx, 0)
        X = batch(w.pool, 65)
        alpha, beta = S.PAIRS[0]
        w.gate(w.call(X, m["b"], alpha, beta), range(65), m["b"], alpha, beta, "creation values")
        v2 = (np.random.default_rng(77).random(m["v"].size, dtype=np.float32) - np.float32(0.5)) * np.float32(3.0)
        cx.h.update_values(cx.idx[0], v2)
        new = dict(m, name=m["name"] + "_updated", pool_key=m["name"], v=v2)
        Y = w.call(X, m["b"], alpha, beta)
        y64, mag = truth(new, range(65), m["b"], alpha, beta)
        old64, _ = truth(m, range(65), m["b"], alpha, beta)
        assert max(bwd_err(Y[i], y64[i], mag[i]) for i in range(65)) < TOL
        assert bwd_err(Y[0], old64[0], mag[0]) > 100 * TOL                       # ... and not the truth of the old values


def test_no_free_was_rejected():
    from hispmv_amd._lib import lib
    assert lib.hispmv_free_failures() == 0
