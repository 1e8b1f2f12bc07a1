"""Several vectors on device pointers: hispmv_linear_device (forward), hispmv_linear_device_t (transposed; the NV-vector kernels of
hispmv_transpose.hip) and hispmv_amd.torch_ops.sparse_linear on top of both, at the small shapes of tests/step_small_cases.py and
with the Ctx of tests/test_gpu_transpose.py (every plan is asserted with check_expect there).

Vectors are drawn per matrix and vector index; vector 1 is all zeros, so that a sum landing in a neighbour's accumulator window
shows.  Y is [B, n] inside a larger tensor whose other floats hold a sentinel, and starts as NaN.  The dense cases, the compact
256-thread windows and big_band run every B twice: aligned, and with y, bias and x each shifted by one float.

Transposed gate: per vector the fp64 scatter truth of tests/test_gpu_transpose.py and bwd_err < TOL = 1e-5 -- the per-vector sums are
the terms of the single-vector product, which that module measured at <= 3.4e-7 in any order (about 30x room).  linear_info must
report the width the plan gives and passes by the 4-2-1 rule (dense 8-4-2-1): a per-vector fall-back would pass every numeric gate.
Expected widths: every small plan below keeps 4 windows in the LDS (the widest, stray_slot_band, has 464 + 1024 floats per vector);
the two W-matrices of tests/test_linear_widths_host.py under HISPMV_PLAN_CUS=32 take 2 and 1.
Forward gate: bits of FpgaHandle.linear for alpha = beta = 1, bits of the one-vector call per vector, TOL against csr_truth otherwise."""
import zlib

import numpy as np
import pytest

import step_small_cases as S
from conftest import TOL
from step_small_harness import HW
from test_gpu_transpose import GUARD, SENTINEL, Ctx as TCtx, scatter_sums
from test_linear_widths_host import w_matrix
from util import bwd_err, csr_truth

pytestmark = pytest.mark.gpu

BS_T = (1, 2, 3, 4, 5, 7, 8, 9)
BS_F = (1, 2, 3, 4, 5, 9)
ZERO_VEC = 1
_VECS = {}
_TRUTH_F = {}


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def vec(m, v, n):
    """Vector v of matrix m with n floats (drawn once per (matrix, v, n)); vector ZERO_VEC is all zeros."""
    key = (m["name"], v, n)
    if key not in _VECS:
        rng = np.random.default_rng(zlib.crc32(f'{m["name"]}/{v}'.encode()))
        _VECS[key] = np.zeros(n, np.float32) if v == ZERO_VEC else rng.random(n, dtype=np.float32) - np.float32(0.3)
    return _VECS[key]


def vecs(m, B, n):
    return np.stack([vec(m, v, n) for v in range(B)])


def passes(B, widest, ladder):
    n = 0
    while B > 0:
        B -= next(w for w in ladder if w <= min(B, widest))
        n += 1
    return n


def ladder(m):
    return (8, 4, 2, 1) if m.get("dense") else (4, 2, 1)


class Ctx(TCtx):
    def _run(self, n_out, B, Y0, call, name, shift=0):
        """shift: floats by which y is moved off the 16-byte alignment of its allocation."""
        torch = self.torch
        lo = GUARD + shift
        full = np.full(B * n_out + 2 * GUARD + shift, SENTINEL, np.int32).view(np.float32)
        full[lo:lo + B * n_out] = Y0.reshape(-1)
        dY = self.device(full)
        torch.cuda.synchronize()
        call(dY.data_ptr() + 4 * lo)
        self.h.synchronize()
        out = dY.cpu().numpy()
        guard = np.ones(out.size, bool)
        guard[lo:lo + B * n_out] = False
        assert (out.view(np.int32)[guard] == SENTINEL).all(), f"{name}: floats outside y were written"
        return out[lo:lo + B * n_out].reshape(B, n_out).copy()

    def linear_t(self, k, X, b, alpha, beta, bias="given", stride=0, shift=0):
        """bias: "given" (b is [cols] for stride 0, [B, cols] for stride cols), "null", "nan", "in_place" (y starts as b, [B, cols]).
        shift: floats by which y, bias AND x are each moved off the 16-byte alignment of their allocations (as spmv_t of
        tests/test_gpu_transpose.py moves y and bias)."""
        m, B = self.mats[k], X.shape[0]
        cols = m["cols"]
        pad = np.full(shift, np.nan, np.float32)
        dX = self.device(np.concatenate([pad, X.reshape(-1)]))
        Y0 = np.asarray(b, np.float32) if bias == "in_place" else np.full((B, cols), np.nan, np.float32)
        flat = np.full(B * cols, np.nan, np.float32) if bias in ("nan", "null", "in_place") else np.asarray(b, np.float32).reshape(-1)
        dB = self.device(np.concatenate([pad, flat]))

        def call(py):
            pb = {"given": dB.data_ptr() + 4 * shift, "nan": dB.data_ptr() + 4 * shift, "null": 0, "in_place": py}[bias]
            self.h.linear_device_t(self.idx[k], dX.data_ptr() + 4 * shift, B, pb, py, alpha, beta, bias_stride=stride)
        return self._run(cols, B, Y0, call, m["name"], shift)

    def linear(self, k, X, b, alpha, beta, shift=0):
        """shift: floats by which d_x is moved off its 16-byte alignment."""
        m, B = self.mats[k], X.shape[0]
        dX = self.device(np.concatenate([np.zeros(shift, np.float32), X.reshape(-1)]))
        dB = self.device(b)

        def call(py):
            self.h.linear_device(self.idx[k], dX.data_ptr() + 4 * shift, B, dB.data_ptr() if beta != 0.0 else 0, py, alpha, beta)
        return self._run(m["rows"], B, np.full((B, m["rows"]), np.nan, np.float32), call, m["name"])

    def truth_t(self, k, X, bias, alpha, beta):
        """Per vector (y64, mag); bias is [cols] or [B, cols]."""
        m = self.mats[k]
        out = []
        for v in range(X.shape[0]):
            s, a = scatter_sums(m, X[v], key=(m["name"], v))
            bb = beta * np.asarray(bias if np.ndim(bias) == 1 else bias[v], np.float64)
            out.append((bb + alpha * s, abs(alpha) * a + np.abs(bb)))
        return out

    def gate_t(self, k, B, width, shift=0):
        m = self.mats[k]
        info = self.h.linear_info(self.idx[k], B)
        exp_w = next(w for w in ladder(m) if w <= min(B, width))
        assert info["width_t"] == exp_w and info["passes_t"] == passes(B, width, ladder(m)), (m["name"], B, info)
        parts = 1 if m.get("dense") else sum(1 for _ in range(self.info[k]["col_tiles"]))
        if m.get("dense") or m["r"].size:
            assert info["launches_t"] == 1 + parts * info["passes_t"], (m["name"], B, info)
        X = vecs(m, B, m["rows"])
        b = vec(m, 100, m["cols"])
        worst = 0.0
        for alpha, beta, bias in ((0.85, -2.06, "given"), (1.0, 0.0, "null")):
            Y = self.linear_t(k, X, b, alpha, beta, bias=bias, shift=shift)
            for v, (y64, mag) in enumerate(self.truth_t(k, X, b, alpha, beta)):
                err = bwd_err(Y[v], y64, mag)
                worst = max(worst, err)
                assert np.isfinite(Y[v]).all() and err < TOL, (m["name"], B, v, alpha, beta, shift, err)
            if B > ZERO_VEC and beta == 0.0:
                assert not Y[ZERO_VEC].any(), (m["name"], B, "the zero vector's product is not zero")
        print(f'{m["name"]}: B={B} shift {shift} width {info["width_t"]} passes {info["passes_t"]} worst backward error {worst:.3e}')

    def bias_only(self, k, B, shift=0):
        """alpha = 0, beta = 1: y is the bias bit for bit, shared and per vector; (-1.5, 0.5) with a bias per vector passes the gate."""
        m = self.mats[k]
        X = vecs(m, B, m["rows"])
        b = vec(m, 100, m["cols"])
        Bb = np.stack([vec(m, 100 + v, m["cols"]) for v in range(B)])
        Y = self.linear_t(k, X, b, 0.0, 1.0, shift=shift)
        assert all(np.array_equal(Y[v].view(np.uint32), b.view(np.uint32)) for v in range(B)), m["name"]
        Y = self.linear_t(k, X, Bb, 0.0, 1.0, stride=m["cols"], shift=shift)
        assert np.array_equal(Y.view(np.uint32), Bb.view(np.uint32)), m["name"]
        Y = self.linear_t(k, X, Bb, -1.5, 0.5, stride=m["cols"], shift=shift)
        for v, (y64, mag) in enumerate(self.truth_t(k, X, Bb, -1.5, 0.5)):
            assert bwd_err(Y[v], y64, mag) < TOL, (m["name"], B, v)


def _all_t(cx, width=4, bs=BS_T, shifts=(0,)):
    """shifts: every B runs once per shift (0 = y, bias and x aligned as allocated, 1 = each moved by one float)."""
    for k in range(len(cx.mats)):
        for shift in shifts:
            for B in bs:
                cx.gate_t(k, B, width, shift)
            cx.bias_only(k, 1, shift)
            cx.bias_only(k, 5, shift)


# ---- transposed: matrices ------------------------------------------------------------------------------------------------------------
def test_t_plans_without_a_window(torch_mod):
    a = S.case_a()
    with Ctx(torch_mod, S.SLICES, a[:6] + a[8:]) as cx:
        assert all(i["lds_bytes"] == 0 for i in cx.info)
        _all_t(cx)


def test_t_compact_windows_256_threads(torch_mod):
    with Ctx(torch_mod, S.SLICES, S.case_a()[6:8]) as cx:
        assert all(i["block_threads"] == 256 and i["lds_bytes"] > 0 and i["compact_slices"] == i["n_slices"] for i in cx.info), cx.info
        _all_t(cx, shifts=(0, 1))


def test_t_wide_groups_with_a_window(torch_mod):
    with Ctx(torch_mod, S.NOSPLIT, [S.two_way_band()]) as cx:
        assert cx.info[0]["compact_slices"] == 0 and cx.info[0]["lds_bytes"] > 0
        _all_t(cx)


@pytest.mark.parametrize("make", [S.big_band, S.stray_slot_band, S.stray_split_band], ids=["big_band", "stray_slot_band", "stray_split_band"])
def test_t_1024_threads(torch_mod, make):
    m = make()
    with Ctx(torch_mod, S.SLICES, [m]) as cx:
        assert cx.info[0]["block_threads"] == 1024 and cx.info[0]["col_tiles"] == m["expect"].get("parts", 1), cx.info[0]
        _all_t(cx, shifts=(0, 1) if make is S.big_band else (0,))


def test_t_eight_column_parts(torch_mod):
    with Ctx(torch_mod, S.COLTILES, [S.column_tiled()]) as cx:
        assert cx.info[0]["col_tiles"] == 8
        _all_t(cx)


@pytest.mark.parametrize("make", [S.big_band, S.stray_slot_band], ids=["big_band", "stray_slot_band"])
def test_t_half_groups(torch_mod, make):
    with Ctx(torch_mod, S.SLICES, [S.as_bf16(make())]) as cx:
        st = cx.h.value_storage_info(cx.idx[0])
        assert st["storage"] == "bf16" and st["slots_2byte"] > 0, st
        _all_t(cx)


def _dense_cases():
    rng = np.random.default_rng(62)
    odd = dict(name="dense_odd_1000x1003", dense=True, rows=1000, cols=1003, W=rng.standard_normal((1000, 1003), dtype=np.float32))
    return S.dense_shapes()[:5] + [odd]


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
def test_t_dense_handles(torch_mod, storage):
    """fp32 and bf16 W, every B once with y, bias and x aligned and once with each shifted by one float: with cols % 4 == 0 (64, 520)
    the shifted shared bias takes the prologue's element path with a period; with odd cols (1003, 1001, 4099, 1) the vectors v > 0
    are unaligned either way."""
    mats = _dense_cases()
    if storage == "bf16":
        mats = [S.as_bf16(m) for m in mats]
    with Ctx(torch_mod, S.SLICES, mats) as cx:
        _all_t(cx, width=8, shifts=(0, 1))


@pytest.mark.parametrize("W, width", [(12000, 2), (26000, 1)])
def test_t_wide_windows_take_narrower_passes(torch_mod, W, width):
    """The W-matrices of tests/test_linear_widths_host.py planned for 32 CUs: 2 windows fit the LDS, or only one (the fall-back to the
    single-vector launches)."""
    m = w_matrix(W)
    with Ctx(torch_mod, dict(S.SLICES, HISPMV_PLAN_CUS="32"), [m]) as cx:
        assert cx.info[0]["block_threads"] == 1024 and cx.info[0]["lds_bytes"] > 4 * W, cx.info[0]
        _all_t(cx, width=width, bs=(1, 2, 3, 5))
        assert cx.h.linear_info(cx.idx[0], 5)["width"] == width


# ---- transposed: contracts ------------------------------------------------------------------------------------------------------------
def test_t_contracts(torch_mod):
    a = S.case_a()
    mats = [a[7], a[10], S.dense_shapes()[1]]
    with Ctx(torch_mod, S.SLICES, mats) as cx:
        for k, m in enumerate(mats):
            B = 5
            X = vecs(m, B, m["rows"])
            Bb = np.stack([vec(m, 100 + v, m["cols"]) for v in range(B)])
            before = cx.spmv(k, m["x"], m["b"], 0.85, -2.06) if "x" in m else None
            Y = cx.linear_t(k, X, Bb, -1.5, 0.5, bias="in_place", stride=m["cols"])          # d_bias == d_y, one bias per vector
            for v, (y64, mag) in enumerate(cx.truth_t(k, X, Bb, -1.5, 0.5)):
                assert bwd_err(Y[v], y64, mag) < TOL, (m["name"], v)
            for bias in ("null", "nan"):                                                     # beta = 0: no bias is read
                Y = cx.linear_t(k, X, None, 1.0, 0.0, bias=bias)
                for v, (y64, mag) in enumerate(cx.truth_t(k, X, np.zeros(m["cols"]), 1.0, 0.0)):
                    assert np.isfinite(Y[v]).all() and bwd_err(Y[v], y64, mag) < TOL, (m["name"], bias, v)
            if before is not None:
                after = cx.spmv(k, m["x"], m["b"], 0.85, -2.06)
                assert np.array_equal(before.view(np.uint32), after.view(np.uint32)), m["name"]
            d = cx.device(np.zeros(B * max(m["rows"], m["cols"]) + 64, np.float32))
            p = d.data_ptr()
            for args in ((p, 0, 0, p + 256), (p, B, 0, p), (0, B, 0, p), (p, B, 0, 0)):       # num_vecs < 1, x == y, NULL vectors
                with pytest.raises(ValueError):
                    cx.h.linear_device_t(cx.idx[k], args[0], args[1], args[2], args[3], 1.0, 0.0)
            with pytest.raises(ValueError):
                cx.h.linear_device_t(cx.idx[k], p, 1, 0, p + 4 * m["rows"], 1.0, 1.0)         # beta != 0 without a bias
            with pytest.raises(ValueError, match="bias_stride"):
                cx.h.linear_device_t(cx.idx[k], p, 1, p, p + 4 * m["rows"], 1.0, 1.0, bias_stride=m["cols"] + 1)
            with pytest.raises(ValueError, match="2\\^30"):
                cx.h.linear_device_t(cx.idx[k], p, (1 << 30) // min(m["rows"], m["cols"]) + 1, 0, p + 256, 1.0, 0.0)
            with pytest.raises(ValueError, match="2\\^30"):
                cx.h.linear_device(cx.idx[k], p, (1 << 30) // min(m["rows"], m["cols"]) + 1, 0, p + 256, 1.0, 0.0)
        with pytest.raises(IndexError):
            cx.h.linear_device_t(99, 1, 1, 0, 2, 1.0, 0.0)
        # sparse_rows: x = +Inf on an empty row, in vector 1 only: a zero slot adds nothing, every vector stays finite
        m = mats[1]
        X = vecs(m, 4, m["rows"]).copy()
        empty = int(np.setdiff1d(np.arange(m["rows"]), m["r"])[777])
        b = vec(m, 100, m["cols"])
        ref = cx.truth_t(1, X, b, 0.85, -2.06)
        X[1, empty] = np.inf
        Y = cx.linear_t(1, X, b, 0.85, -2.06)
        for v, (y64, mag) in enumerate(ref):
            assert np.isfinite(Y[v]).all() and bwd_err(Y[v], y64, mag) < TOL, v


def test_t_tile_stream_is_refused(torch_mod):
    m = S.tile_stream()
    with Ctx(torch_mod, S.AUTO, [m]) as cx:
        assert cx.info[0]["format"] == 1
        info = cx.h.linear_info(cx.idx[0], 4)
        assert (info["width_t"], info["passes_t"], info["launches_t"]) == (0, 0, 0) and info["width"] >= 1, info
        with pytest.raises(NotImplementedError, match="set_transposable"):
            cx.linear_t(0, vecs(m, 3, m["rows"]), None, 1.0, 0.0, bias="null")


def test_refused_before_load_matrices(torch_mod):
    import pyhispmv
    m = S.case_a()[1]
    h = pyhispmv.FpgaHandle(*HW)
    try:
        i = h.create_sparse_handle(m["r"], m["c"], m["v"], m["rows"], m["cols"])
        d = torch_mod.zeros(2 * (m["rows"] + m["cols"]), dtype=torch_mod.float32, device="cuda")
        with pytest.raises(AssertionError, match="before load_matrices"):
            h.linear_device_t(i, d.data_ptr(), 2, 0, d.data_ptr() + 8 * m["rows"], 1.0, 0.0)
        with pytest.raises(AssertionError, match="before load_matrices"):
            h.linear_device(i, d.data_ptr(), 2, 0, d.data_ptr() + 8 * m["cols"], 1.0, 0.0)
        assert h.linear_info(i, 4) == dict(width=0, passes=0, width_t=0, passes_t=0, launches_t=0)
    finally:
        h.close()


# ---- forward --------------------------------------------------------------------------------------------------------------------------
def _forward(cx, k, width=None):
    m = cx.mats[k]
    rows, cols, b = m["rows"], m["cols"], m["b"]
    single = {}
    for B in BS_F:
        X = vecs(m, B, cols)
        info = cx.h.linear_info(cx.idx[k], B)
        if width is not None:
            assert info["width"] == next(w for w in ladder(m) if w <= min(B, width)) and info["passes"] == passes(B, width, ladder(m)), (m["name"], B, info)
        Y = cx.linear(k, X, b, 1.0, 1.0)
        host = cx.h.linear(cx.idx[k], X.reshape(-1), b).reshape(B, rows)
        assert np.array_equal(Y.view(np.uint32), host.view(np.uint32)), (m["name"], B, "linear_device != linear")
        for v in range(B):
            if v not in single:
                single[v] = cx.linear(k, X[v:v + 1], b, 1.0, 1.0)[0]
            assert np.array_equal(Y[v].view(np.uint32), single[v].view(np.uint32)), (m["name"], B, v, "differs from its one-vector call")
        for shift in (0, 1) if B in (2, 5) else (0,):
            Y = cx.linear(k, X, b, 0.85, -2.06, shift=shift)
            for v in range(B):
                if m.get("dense"):
                    W64, x64, b64 = m["W"].astype(np.float64), X[v].astype(np.float64), b.astype(np.float64)
                    y64, mag = 0.85 * (W64 @ x64) - 2.06 * b64, 0.85 * (np.abs(W64) @ np.abs(x64)) + np.abs(2.06 * b64)
                else:
                    if (m["name"], v) not in _TRUTH_F:              # (computed once per matrix and vector)
                        _TRUTH_F[(m["name"], v)] = csr_truth(m["r"], m["c"], m["v"], rows, X[v], b, 0.85, -2.06)
                    y64, mag = _TRUTH_F[(m["name"], v)]
                assert bwd_err(Y[v], y64, mag) < TOL, (m["name"], B, v, shift)


_FORWARD_SLICES = dict(no_window=lambda: S.case_a()[4], compact_256=lambda: S.case_a()[7], big_band=S.big_band, stray_slot_band=S.stray_slot_band,
                       stray_split_band=S.stray_split_band, big_band_bf16=lambda: S.as_bf16(S.big_band()))


@pytest.mark.parametrize("which", list(_FORWARD_SLICES))
def test_forward_slice_plans(torch_mod, which):
    with Ctx(torch_mod, S.SLICES, [_FORWARD_SLICES[which]()]) as cx:
        _forward(cx, 0, width=4)


def test_forward_wide_groups_and_column_parts(torch_mod):
    with Ctx(torch_mod, S.NOSPLIT, [S.two_way_band()]) as cx:
        _forward(cx, 0, width=4)
    with Ctx(torch_mod, S.COLTILES, [S.column_tiled()]) as cx:
        _forward(cx, 0, width=4)


def test_forward_tile_stream_and_dense(torch_mod):
    with Ctx(torch_mod, S.AUTO, [S.tile_stream()]) as cx:
        assert cx.info[0]["format"] == 1
        _forward(cx, 0)
    d = S.dense_shapes()
    with Ctx(torch_mod, S.SLICES, [d[1], d[4]]) as cx:
        _forward(cx, 0, width=8)
        _forward(cx, 1, width=8)


# ---- the adjoint identity across the two entries --------------------------------------------------------------------------------------------
def test_adjoint_across_both_entries(torch_mod):
    """|<A X, W> - <X, A^T W>| <= TOL * sum |a_ij x_j w_i|, summed over the B = 4 vectors, both products from the device."""
    m = S.big_band()
    with Ctx(torch_mod, S.SLICES, [m]) as cx:
        X, Wv = vecs(m, 4, m["cols"]), np.stack([vec(m, 50 + v, m["rows"]) for v in range(4)])
        AX = cx.linear(0, X, m["b"], 1.0, 0.0).astype(np.float64)
        AtW = cx.linear_t(0, Wv, None, 1.0, 0.0, bias="null").astype(np.float64)
        X64, W64, v64 = X.astype(np.float64), Wv.astype(np.float64), m["v"].astype(np.float64)
        scale = float(sum(np.sum(np.abs(v64 * X64[v][m["c"]] * W64[v][m["r"]])) for v in range(4)))
        lhs, rhs = float(np.sum(AX * W64)), float(np.sum(X64 * AtW))
        print(f"adjoint: {lhs!r} vs {rhs!r}, |difference| / scale = {abs(lhs - rhs) / scale:.3e}")
        assert abs(lhs - rhs) <= TOL * scale


# ---- sparse_linear --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["big_band", "dense"])
def test_sparse_linear_forward_and_backward(torch_mod, kind):
    """y, x.grad and bias.grad of loss = sum(y * w) against fp64 (the matrix as COO triplets or dense W, in fp64): x.grad = A^T w per
    vector, bias.grad = sum_v w; bias=None, a 1-D x and a non-contiguous x."""
    from hispmv_amd.torch_ops import sparse_linear
    torch = torch_mod
    m = S.big_band() if kind == "big_band" else S.dense_shapes()[1]
    B, rows, cols = 5, m["rows"], m["cols"]

    def products(X64, W64):
        """-> (A X, |A| |X|, A^T W, |A|^T |W|) per vector in fp64"""
        if m.get("dense"):
            A = m["W"].astype(np.float64)
            return X64 @ A.T, np.abs(X64) @ np.abs(A).T, W64 @ A, np.abs(W64) @ np.abs(A)
        v64, r, c = m["v"].astype(np.float64), m["r"], m["c"]
        f = [(np.bincount(r, weights=v64 * x[c], minlength=rows), np.bincount(r, weights=np.abs(v64 * x[c]), minlength=rows)) for x in X64]
        t = [(np.bincount(c, weights=v64 * w[r], minlength=cols), np.bincount(c, weights=np.abs(v64 * w[r]), minlength=cols)) for w in W64]
        return np.stack([a for a, _ in f]), np.stack([a for _, a in f]), np.stack([a for a, _ in t]), np.stack([a for _, a in t])

    with Ctx(torch, S.SLICES, [m]) as cx:
        Xn, Wn, bn = vecs(m, B, cols), np.stack([vec(m, 50 + v, rows) for v in range(B)]), m["b"]
        AX, AXm, AtW, AtWm = products(Xn.astype(np.float64), Wn.astype(np.float64))
        b64 = bn.astype(np.float64)
        w = cx.device(Wn)
        for variant in ("bias", "no_bias", "strided"):
            if variant == "strided":
                wide = torch.zeros((B, 2 * cols), dtype=torch.float32, device=cx.dev)
                wide[:, ::2] = cx.device(Xn)
                x = wide[:, ::2].detach().requires_grad_(True)
                assert not x.is_contiguous()
            else:
                x = cx.device(Xn).requires_grad_(True)
            bias = None if variant == "no_bias" else cx.device(bn).requires_grad_(True)
            y = sparse_linear(cx.h, cx.idx[0], x, bias)
            assert tuple(y.shape) == (B, rows)
            (y * w).sum().backward()
            torch.cuda.synchronize()
            yb = b64 if bias is not None else 0.0
            assert bwd_err(y.detach().cpu().numpy(), AX + yb, AXm + np.abs(yb)) < TOL, variant
            assert tuple(x.grad.shape) == (B, cols) and bwd_err(x.grad.cpu().numpy(), AtW, AtWm) < TOL, variant
            if bias is not None:
                assert bwd_err(bias.grad.cpu().numpy(), Wn.astype(np.float64).sum(0), np.abs(Wn.astype(np.float64)).sum(0)) < TOL, variant
        x1 = cx.device(Xn[0]).requires_grad_(True)
        y1 = sparse_linear(cx.h, cx.idx[0], x1, cx.device(bn))
        assert tuple(y1.shape) == (rows,)
        (y1 * w[0]).sum().backward()
        torch.cuda.synchronize()
        assert bwd_err(y1.detach().cpu().numpy(), AX[0] + b64, AXm[0] + np.abs(b64)) < TOL
        assert tuple(x1.grad.shape) == (cols,) and bwd_err(x1.grad.cpu().numpy(), AtW[0], AtWm[0]) < TOL
        with pytest.raises(TypeError):
            sparse_linear(cx.h, cx.idx[0], cx.device(Xn).double())
        with pytest.raises(ValueError):
            sparse_linear(cx.h, cx.idx[0], torch.from_numpy(Xn))
        with pytest.raises(ValueError):
            sparse_linear(cx.h, cx.idx[0], cx.device(Xn)[:, :-1])
        with pytest.raises(TypeError):
            sparse_linear(cx.h, cx.idx[0], cx.device(Xn), cx.device(bn).double())


def test_no_free_was_rejected():
    from hispmv_amd._lib import lib
    assert lib.hispmv_free_failures() == 0
