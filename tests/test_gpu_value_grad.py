"""The value gradient grad[k] = alpha * sum_v gy[v, row_k] * x[v, col_k] + beta * grad[k] (hispmv_value_grad_device; the kernels of
hispmv_value_grad.hip) and sparse_linear(..., values=v) on top of it, at the small shapes of tests/step_small_cases.py with the Ctx of
tests/test_gpu_transpose.py created with value updates on: every plan kind the slice kernels have (no window, compact and wide windows,
stray slots, 256 and 1024 threads, cut matrices of two and eight parts), a tile stream kept as slices, dense handles.

EXACTNESS: gy and x hold integers in [-3, 3] drawn per (matrix, vector), grad0 integers in [-8, 8], (alpha, beta) one of (1, 0),
(2, -1), (0, 1), (0, 0).  With B <= 9 every partial sum stays below 2 * 81 + 8 < 2^24, so fp32 is exact in any order and grad must equal
the numpy result bit for bit at all n positions.  For beta = 0 grad starts as NaN; it always lies inside a sentinel-filled tensor whose
guards must survive.  RANDOM FLOATS: the per-vector draws of tests/test_gpu_linear_device.py, (alpha, beta) = (0.85, -2.06), gate
|grad - g64| <= TOL * (|alpha| sum_v |gy x| + |beta grad0|): an fp32 sum of B <= 9 products plus two operations is bounded by about
(B + 2) * 2^-24 = 7e-7 of that magnitude, more than 10x below TOL = 1e-5.  A second identical call must give identical bits (plain
stores, one writer per entry).  value_grad_info must report the width the plan gives and the passes of the 4-2-1 rule (dense: all
vectors in one pass): a per-vector fall-back would pass every numeric gate.  The references are computed once per matrix, as prefix
sums over the vectors."""
import zlib

import numpy as np
import pytest

import step_small_cases as S
from conftest import TOL
from step_small_harness import HW
from test_gpu_linear_device import passes, vec, vecs
from test_gpu_transpose import GUARD, SENTINEL, Ctx as TCtx, _dense_cases
from test_linear_widths_host import w_matrix
from test_value_grad_host import shuffled_with_duplicates
from util import bwd_err, csr_truth

pytestmark = pytest.mark.gpu

BS = (1, 2, 3, 4, 5, 9)
PAIRS = ((1.0, 0.0), (2.0, -1.0), (0.0, 1.0), (0.0, 0.0))
_INTS = {}


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def ints(m, tag, v, n, lo=-3, hi=3):
    """n integers in [lo, hi] as float32, drawn once per (matrix, tag, vector)."""
    key = (m["name"], tag, v, n, lo, hi)
    if key not in _INTS:
        rng = np.random.default_rng(zlib.crc32(f'{m["name"]}/{tag}/{v}'.encode()))
        _INTS[key] = rng.integers(lo, hi + 1, n).astype(np.float32)
    return _INTS[key]


def entries(m):
    """(row, column) of every entry of the creation input, in its order: the COO arrays, or W row-major."""
    if m.get("dense"):
        k = np.arange(m["rows"] * m["cols"], dtype=np.int64)
        return k // m["cols"], k % m["cols"]
    return m["r"].astype(np.int64), m["c"].astype(np.int64)


def prefix_refs(cache, m, GY, X, key, magnitudes):
    """{B: (sum_{v < B} gy[v, r] x[v, c], sum_{v < B} |gy x| or None)} in fp64 for every B in BS, computed once per key in `cache` (a
    context's: the sums of a 4.6 M-entry matrix are released with it)."""
    if key not in cache:
        r, c = entries(m)
        s, a, out = np.zeros(r.size), np.zeros(r.size) if magnitudes else None, {}
        for v in range(GY.shape[0]):
            t = GY[v].astype(np.float64)[r] * X[v].astype(np.float64)[c]
            s = s + t
            if magnitudes:
                a = a + np.abs(t)
            if v + 1 in BS:
                out[v + 1] = (s, a)
        cache[key] = out
    return cache[key]


class Ctx(TCtx):
    def __init__(self, torch, env, mats, transposable=None):
        super().__init__(torch, env, mats, transposable=transposable, updates=True)
        self.n, self.refs = [], {}
        for k, m in enumerate(mats):
            u = self.h.value_update_info(self.idx[k])
            assert u["updatable"] and u["n"] == (m["rows"] * m["cols"] if m.get("dense") else m["r"].size), (m["name"], u)
            self.n.append(u["n"])

    def value_grad(self, k, GY, X, grad0, alpha, beta, shift=0):
        """One call on matrix k -> grad (numpy).  grad0 None: grad starts as NaN.  shift: floats by which gy, x and grad are each moved
        off the 16-byte alignment of their allocations.  The guards on both sides of grad must survive."""
        torch, m, n, B = self.torch, self.mats[k], self.n[k], GY.shape[0]
        pad = np.full(shift, np.nan, np.float32)
        dG = self.device(np.concatenate([pad, GY.reshape(-1)]))
        dX = self.device(np.concatenate([pad, X.reshape(-1)]))
        lo = GUARD + shift
        full = np.full(n + 2 * GUARD + shift, SENTINEL, np.int32).view(np.float32)
        full[lo:lo + n] = np.nan if grad0 is None else grad0
        dR = self.device(full)
        torch.cuda.synchronize()
        self.h.value_grad_device(self.idx[k], dG.data_ptr() + 4 * shift, dX.data_ptr() + 4 * shift, B, dR.data_ptr() + 4 * lo, alpha, beta)
        self.h.synchronize()
        out = dR.cpu().numpy()
        guard = np.ones(out.size, bool)
        guard[lo:lo + n] = False
        assert (out.view(np.int32)[guard] == SENTINEL).all(), f'{m["name"]}: floats outside grad were written'
        return out[lo:lo + n].copy()

    def check_info(self, k, B, width=4):
        m = self.mats[k]
        info = self.h.value_grad_info(self.idx[k], B)
        if m.get("dense"):
            assert info == dict(accepted=True, width=B, passes=1, launches=1), (m["name"], B, info)
            return info
        exp_w = next(w for w in (4, 2, 1) if w <= min(B, width))
        n_pass = passes(B, width, (4, 2, 1))
        parts = self.info[k]["col_tiles"]
        assert info["accepted"] and info["width"] == exp_w and info["passes"] == n_pass, (m["name"], B, info)
        assert info["launches"] == (parts * n_pass if self.n[k] > 0 else 0), (m["name"], B, info, parts)
        return info

    def exact(self, k, B, alpha, beta, shift=0):
        m, n = self.mats[k], self.n[k]
        GY = np.stack([ints(m, "gy", v, m["rows"]) for v in range(B)])
        X = np.stack([ints(m, "x", v, m["cols"]) for v in range(B)])
        g0 = ints(m, "grad0", 0, n, -8, 8)
        s, _ = prefix_refs(self.refs, m, np.stack([ints(m, "gy", v, m["rows"]) for v in range(max(BS))]),
                           np.stack([ints(m, "x", v, m["cols"]) for v in range(max(BS))]), (m["name"], "ints"), False)[B]
        # (alpha == 0: gy and x are not read, the result is beta * grad0 -- or +0 -- and not 0 * s, which is -0 where s < 0)
        want = ((alpha * s if alpha != 0.0 else np.zeros(n)) + (beta * g0.astype(np.float64) if beta != 0.0 else 0.0)).astype(np.float32)
        got = self.value_grad(k, GY, X, None if beta == 0.0 else g0, alpha, beta, shift=shift)
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (m["name"], B, alpha, beta, shift, bad.size, bad[:8], got[bad[:8]], want[bad[:8]])

    def floats(self, k, B):
        m, n = self.mats[k], self.n[k]
        alpha, beta = 0.85, -2.06
        full_gy = np.stack([vec(m, 50 + v, m["rows"]) for v in range(max(BS))])
        full_x = vecs(m, max(BS), m["cols"])
        g0 = vec(m, 200, n)
        s, a = prefix_refs(self.refs, m, full_gy, full_x, (m["name"], "floats"), True)[B]
        g64 = alpha * s + beta * g0.astype(np.float64)
        mag = abs(alpha) * a + np.abs(beta * g0.astype(np.float64))
        got = self.value_grad(k, full_gy[:B], full_x[:B], g0, alpha, beta)
        err = np.abs(got.astype(np.float64) - g64)
        print(f'{m["name"]}: B={B} worst |grad - g64| / mag = {bwd_err(got, g64, mag) if n else 0.0:.3e}')
        assert np.isfinite(got).all() and (err <= TOL * mag).all(), (m["name"], B, float((err - TOL * mag).max()))
        again = self.value_grad(k, full_gy[:B], full_x[:B], g0, alpha, beta)
        assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), (m["name"], B, "a second identical call gave other bits")

    def all(self, width=4, bs=BS):
        """Every B: the info, the exact gate for (1, 0) and (2, -1), the random-float gate; B = 5 also alpha = 0 and one shifted run."""
        for k in range(len(self.mats)):
            for B in bs:
                self.check_info(k, B, width)
                for alpha, beta in PAIRS if B == 5 else PAIRS[:2]:
                    self.exact(k, B, alpha, beta)
                self.floats(k, B)
            self.exact(k, 5, 2.0, -1.0, shift=1)


# ---- matrices -----------------------------------------------------------------------------------------------------------------------
def test_plans_without_a_window(torch_mod):
    """256 threads, no window: the plain matrices of case A (nnz = 0 and 1024 among them), the 1 x 1 matrix, one row over some thirty
    slices, 50 live rows among 49 950 fillers.  Every x is gathered through L2."""
    a = S.case_a()
    with Ctx(torch_mod, S.SLICES, a[:6] + a[8:]) as cx:
        assert all(i["lds_bytes"] == 0 and i["block_threads"] == 256 and i["col_tiles"] == 1 and i["tile_kind"] == 0 for i in cx.info), cx.info
        assert cx.n[0] == 0 and cx.n[1] == 1024
        cx.all()


def test_compact_windows_256_threads(torch_mod):
    with Ctx(torch_mod, S.SLICES, S.case_a()[6:8]) as cx:
        assert all(i["block_threads"] == 256 and i["lds_bytes"] > 0 and i["compact_slices"] == i["n_slices"] and i["col_tiles"] == 1 for i in cx.info), cx.info
        cx.all()


def test_wide_groups_with_a_window_and_l2_elements(torch_mod):
    with Ctx(torch_mod, S.NOSPLIT, [S.two_way_band()]) as cx:
        i = cx.info[0]
        assert i["compact_slices"] == 0 and i["lds_bytes"] > 0 and i["block_threads"] == 256 and i["col_tiles"] == 1, i
        cx.all()


def test_1024_threads_compact(torch_mod):
    with Ctx(torch_mod, S.SLICES, [S.big_band()]) as cx:
        i = cx.info[0]
        assert i["block_threads"] == 1024 and i["lds_bytes"] > 0 and i["compact_slices"] == i["n_slices"] and i["col_tiles"] == 1, i
        cx.all()


def test_stray_slots(torch_mod):
    with Ctx(torch_mod, S.SLICES, [S.stray_slot_band()]) as cx:
        i = cx.info[0]
        assert i["block_threads"] == 1024 and i["lds_bytes"] > 0 and i["compact_slices"] == i["n_slices"] and i["col_tiles"] == 1, i
        cx.all()


def test_two_parts_of_a_stray_split(torch_mod):
    with Ctx(torch_mod, S.SLICES, [S.stray_split_band()]) as cx:
        i = cx.info[0]
        assert i["tile_kind"] == 3 and i["col_tiles"] == 2 and i["block_threads"] == 1024, i
        assert cx.h.value_grad_info(cx.idx[0], 9)["launches"] == 2 * 3
        cx.all()


def test_eight_column_parts(torch_mod):
    with Ctx(torch_mod, S.COLTILES, [S.column_tiled()]) as cx:
        i = cx.info[0]
        assert i["tile_kind"] == 1 and i["col_tiles"] == 8 and i["block_threads"] == 256, i
        assert cx.h.value_grad_info(cx.idx[0], 5)["launches"] == 8 * 2
        cx.all()


def test_tile_stream_kept_as_slices(torch_mod):
    with Ctx(torch_mod, S.AUTO, [S.as_slices(S.tile_stream())], transposable=True) as cx:
        assert cx.info[0]["format"] == 0, cx.info[0]
        cx.all()


@pytest.mark.parametrize("W, width", [(12000, 2), (26000, 1)])
def test_wide_windows_take_narrower_passes(torch_mod, W, width):
    """The W-matrices of tests/test_linear_widths_host.py planned for 32 CUs: only 2 windows fit the LDS, or only one, so the FIRST pass
    (the one that takes alpha and beta) runs the 2- or 1-wide window kernel and B = 5 takes 3 or 5 passes."""
    m = w_matrix(W)
    with Ctx(torch_mod, dict(S.SLICES, HISPMV_PLAN_CUS="32"), [m]) as cx:
        assert cx.info[0]["block_threads"] == 1024 and cx.info[0]["lds_bytes"] > 4 * W and cx.info[0]["col_tiles"] == 1, cx.info[0]
        assert cx.h.value_grad_info(cx.idx[0], 5) == dict(accepted=True, width=width, passes=5 // width + 5 % width, launches=5 // width + 5 % width)
        cx.all(width=width, bs=(1, 2, 3, 5))


def test_dense_handles(torch_mod):
    """The first five dense shapes and 1000 x 1003: odd cols put a row of grad at any 4-byte boundary (the element path); 64 and 520
    columns take the 16-byte path when aligned and the element path when shifted."""
    with Ctx(torch_mod, S.SLICES, _dense_cases()) as cx:
        cx.all()


# ---- the order of the input, explicit zeros --------------------------------------------------------------------------------------------
def test_coo_order_duplicates_and_explicit_zeros(torch_mod):
    """A shuffled COO input with 5000 entries entered twice and a tenth of the values exactly 0: every position gets its gradient,
    duplicates get equal gradients, zero-valued entries get non-zero gradients (gy and x are positive here); the forward product still
    multiplies with the values (zeros and all)."""
    m = shuffled_with_duplicates()
    rng = np.random.default_rng(405)
    v = rng.random(m["r"].size, dtype=np.float32) - np.float32(0.5)
    zero = rng.random(v.size) < 0.1
    v[zero] = 0.0
    m = dict(m, v=v, expect=dict(format=0, threads=256, window=True))
    with Ctx(torch_mod, S.SLICES, [m]) as cx:
        B = 5
        GY = np.stack([ints(m, "gy+", u, m["rows"], 1, 3) for u in range(B)])
        X = np.stack([ints(m, "x+", u, m["cols"], 1, 3) for u in range(B)])
        r, c = entries(m)
        want = sum(GY[u].astype(np.float64)[r] * X[u].astype(np.float64)[c] for u in range(B)).astype(np.float32)
        got = cx.value_grad(0, GY, X, None, 1.0, 0.0)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert zero.sum() > 1000 and (got[zero] > 0).all()
        _, inv, cnt = np.unique(r * m["cols"] + c, return_inverse=True, return_counts=True)
        assert (cnt == 2).sum() == 5000
        hi, lo = np.full(cnt.size, -np.inf), np.full(cnt.size, np.inf)
        np.maximum.at(hi, inv, got)
        np.minimum.at(lo, inv, got)
        assert np.array_equal(hi, lo), "duplicated entries got different gradients"
        y = cx.spmv(0, m["x"], m["b"], 0.85, -2.06)
        y64, mag = csr_truth(m["r"], m["c"], m["v"], m["rows"], m["x"], m["b"], 0.85, -2.06)
        assert bwd_err(y, y64, mag) < TOL


def test_csr_order_before_the_per_row_sort(torch_mod):
    """A _from_csr handle whose rows hold their columns in random order: grad comes back in the order of the input col_idx."""
    import pyhispmv
    torch = torch_mod
    m = S.case_a()[4]
    rng = np.random.default_rng(406)
    order = np.lexsort((rng.random(m["r"].size), m["r"]))             # by row, columns shuffled inside a row
    r, c = m["r"][order], m["c"][order]
    assert (np.diff(c)[np.diff(r) == 0] < 0).any()
    rp = np.zeros(m["rows"] + 1, np.int32)
    np.add.at(rp, r.astype(np.int64) + 1, 1)
    rp = np.cumsum(rp).astype(np.int32)
    with S.environment(S.SLICES):
        h = pyhispmv.FpgaHandle(*HW)
    try:
        h.set_value_updates(True)
        i = h.create_sparse_handle_from_csr(rp, c, m["v"][order], m["rows"], m["cols"])
        h.load_matrices()
        n, B = r.size, 3
        assert h.value_update_info(i)["n"] == n
        GY = np.stack([ints(m, "gy", u, m["rows"]) for u in range(B)])
        X = np.stack([ints(m, "x", u, m["cols"]) for u in range(B)])
        want = sum(GY[u].astype(np.float64)[r] * X[u].astype(np.float64)[c] for u in range(B)).astype(np.float32)
        dG, dX = torch.from_numpy(GY).cuda(), torch.from_numpy(X).cuda()
        dR = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        h.value_grad_device(i, dG.data_ptr(), dX.data_ptr(), B, dR.data_ptr())
        h.synchronize()
        assert np.array_equal(dR.cpu().numpy().view(np.uint32), want.view(np.uint32))
    finally:
        h.close()


# ---- contracts ----------------------------------------------------------------------------------------------------------------------------
def test_contracts(torch_mod):
    """beta = 0 overwrites a NaN-filled grad everywhere and alpha = 0 gives beta * grad exactly (both inside Ctx.exact); NULL and
    aliased pointers, num_vecs < 1, a batch of 2^30 floats and a bad index are refused; spmv_device on the handle gives identical bits
    before and after gradient calls."""
    a = S.case_a()
    mats = [a[7], a[10], S.dense_shapes()[1]]
    with Ctx(torch_mod, S.SLICES, mats) as cx:
        for k, m in enumerate(mats):
            before = cx.spmv(k, m["x"], m["b"], 0.85, -2.06)
            for alpha, beta in PAIRS:
                cx.exact(k, 3, alpha, beta)
            after = cx.spmv(k, m["x"], m["b"], 0.85, -2.06)
            assert np.array_equal(before.view(np.uint32), after.view(np.uint32)), m["name"]
            B = 2
            d = cx.device(np.zeros(B * (m["rows"] + m["cols"]) + cx.n[k] + 64, np.float32))
            pg = d.data_ptr()
            px, pr = pg + 4 * B * m["rows"], pg + 4 * B * (m["rows"] + m["cols"])
            cx.h.value_grad_device(cx.idx[k], pg, px, B, pr)                                     # (the layout the refusals below vary)
            cx.h.synchronize()
            for args in ((pg, px, 0, pr), (0, px, B, pr), (pg, 0, B, pr), (pg, px, B, 0), (pg, px, B, pg), (pg, px, B, px)):
                with pytest.raises(ValueError):
                    cx.h.value_grad_device(cx.idx[k], *args)
            with pytest.raises(ValueError, match="2\\^30"):
                cx.h.value_grad_device(cx.idx[k], pg, px, (1 << 30) // min(m["rows"], m["cols"]) + 1, pr)
            with pytest.raises(ValueError):
                cx.h.value_grad_info(cx.idx[k], 0)
        with pytest.raises(IndexError):
            cx.h.value_grad_device(99, 1, 2, 1, 3)
        with pytest.raises(IndexError):
            cx.h.value_grad_info(99, 1)


def test_refused_without_value_updates(torch_mod):
    m = S.case_a()[7]
    with TCtx(torch_mod, S.SLICES, [m, S.dense_shapes()[1]], updates=False) as cx:
        for k, mm in enumerate(cx.mats):
            assert cx.h.value_grad_info(cx.idx[k], 4) == dict(accepted=False, width=0, passes=0, launches=0)
            d = cx.device(np.zeros(mm["rows"] + mm["cols"] + mm["rows"] * mm["cols"], np.float32))
            with pytest.raises(AssertionError, match="set_value_updates"):
                cx.h.value_grad_device(cx.idx[k], d.data_ptr(), d.data_ptr() + 4 * mm["rows"], 1, d.data_ptr() + 4 * (mm["rows"] + mm["cols"]))


def test_tile_stream_is_refused(torch_mod):
    m = S.tile_stream()
    with TCtx(torch_mod, S.AUTO, [m], updates=True) as cx:
        assert cx.info[0]["format"] == 1 and cx.h.value_update_info(cx.idx[0])["updatable"]
        assert cx.h.value_grad_info(cx.idx[0], 4) == dict(accepted=False, width=0, passes=0, launches=0)
        before = cx.spmv(0, m["x"], m["b"], 0.85, -2.06)
        d = cx.device(np.zeros(m["rows"] + m["cols"] + m["r"].size, np.float32))
        with pytest.raises(NotImplementedError, match="set_transposable"):
            cx.h.value_grad_device(cx.idx[0], d.data_ptr(), d.data_ptr() + 4 * m["rows"], 1, d.data_ptr() + 4 * (m["rows"] + m["cols"]))
        after = cx.spmv(0, m["x"], m["b"], 0.85, -2.06)
        assert np.array_equal(before.view(np.uint32), after.view(np.uint32))


def test_refused_before_load_matrices(torch_mod):
    import pyhispmv
    m = S.case_a()[1]
    h = pyhispmv.FpgaHandle(*HW)
    try:
        h.set_value_updates(True)
        i = h.create_sparse_handle(m["r"], m["c"], m["v"], m["rows"], m["cols"])
        d = torch_mod.zeros(m["rows"] + m["cols"] + m["r"].size, dtype=torch_mod.float32, device="cuda")
        with pytest.raises(AssertionError, match="before load_matrices"):
            h.value_grad_device(i, d.data_ptr(), d.data_ptr() + 4 * m["rows"], 1, d.data_ptr() + 4 * (m["rows"] + m["cols"]))
        assert h.value_grad_info(i, 4) == dict(accepted=False, width=0, passes=0, launches=0)
        h.load_matrices()
        assert h.value_grad_info(i, 4) == dict(accepted=True, width=4, passes=1, launches=1)
    finally:
        h.close()


# ---- sparse_linear(values=...) ------------------------------------------------------------------------------------------------------------
def _forward64(m, vals, X64):
    """-> (A X + b, |A| |X| + |b|) per vector in fp64, A built from `vals` in input order (duplicates add)"""
    r, c = entries(m)
    v64 = np.asarray(vals, np.float64)
    b64 = m["b"].astype(np.float64)
    y = np.stack([np.bincount(r, weights=v64 * x[c], minlength=m["rows"]) for x in X64]) + b64
    mag = np.stack([np.bincount(r, weights=np.abs(v64 * x[c]), minlength=m["rows"]) for x in X64]) + np.abs(b64)
    return y, mag


def test_sparse_linear_with_values_on_the_default_stream(torch_mod):
    """The natural loop on torch's default stream, with no synchronisation by the caller between torch's operations and the layer:
    forward, backward, v -= 0.1 * v.grad, forward.  The default stream has the handle 0 (the context's own stream to the library), so
    the layer orders the two itself: both forwards meet the fp64 truth of the values they were given, v.grad meets its gate, and the
    bits of y and v.grad are those of the same loop on a stream of its own (both are plain-store results)."""
    from hispmv_amd.torch_ops import sparse_linear
    torch = torch_mod
    m = S.case_a()[7]
    B = 5
    r, c = entries(m)
    Xn, Wn = vecs(m, B, m["cols"]), np.stack([vec(m, 50 + u, m["rows"]) for u in range(B)])
    vn = m["v"].astype(np.float32) * np.float32(0.5) + np.float32(0.125)
    X64, W64 = Xn.astype(np.float64), Wn.astype(np.float64)

    def loop(cx):
        x, bias, w = cx.device(Xn), cx.device(m["b"]), cx.device(Wn)
        v = (cx.device(vn) * 1.0).requires_grad_(True)                  # (written by a kernel on the current stream just before)
        y = sparse_linear(cx.h, cx.idx[0], x, bias, values=v)
        (y * w).sum().backward()
        with torch.no_grad():
            v2 = v - 0.1 * v.grad
            y2 = sparse_linear(cx.h, cx.idx[0], x, bias, values=v2)
            out = [t.clone() for t in (y, v.grad, v2, y2)]
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in out]

    with Ctx(torch, S.SLICES, [m]) as cx:
        assert torch.cuda.current_stream(cx.dev).cuda_stream == 0
        y, gv, v2, y2 = loop(cx)
        with torch.cuda.stream(torch.cuda.Stream(device=cx.dev)):
            side = loop(cx)
    y64, ymag = _forward64(m, vn, X64)
    assert bwd_err(y, y64, ymag) < TOL
    g64 = sum(W64[u][r] * X64[u][c] for u in range(B))
    gmag = sum(np.abs(W64[u][r] * X64[u][c]) for u in range(B))
    assert (np.abs(gv.astype(np.float64) - g64) <= TOL * gmag).all()
    new64, newmag = _forward64(m, v2, X64)
    assert bwd_err(y2, new64, newmag) < TOL and bwd_err(y2, y64, newmag) > 100 * TOL
    for got, want, name in zip((y, gv, v2, y2), side, ("y", "v.grad", "v2", "y2")):
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name


@pytest.mark.parametrize("kind", ["band_4000x300", "dense"])
def test_sparse_linear_with_values(torch_mod, kind):
    """loss = sum(y * w), y = sparse_linear(h, i, x, bias, values=v): x.grad, bias.grad and v.grad against fp64 numpy (the matrix with
    values v as COO triplets -- duplicates add -- or dense W); one SGD step v2 = v - 0.1 * v.grad, whose forward meets the truth of v2
    and misses the truth of v; values=None gives the bits of linear_device."""
    from hispmv_amd.torch_ops import sparse_linear
    torch = torch_mod
    m = S.case_a()[7] if kind == "band_4000x300" else S.dense_shapes()[1]
    B, rows, cols = 5, m["rows"], m["cols"]
    r, c = entries(m)

    def forward64(vals, X64):
        return _forward64(m, vals, X64)

    # (a stream of its own: torch's default stream has the handle 0, which the library reads as "the context's own stream"; torch's
    # kernels and the library's launches are ordered only when both run on one real stream)
    with Ctx(torch, S.SLICES, [m]) as cx, torch.cuda.stream(torch.cuda.Stream(device=cx.dev)):
        n = cx.n[0]
        Xn, Wn = vecs(m, B, cols), np.stack([vec(m, 50 + u, rows) for u in range(B)])
        vn = (m["W"].reshape(-1) if m.get("dense") else m["v"]).astype(np.float32) * np.float32(0.5) + np.float32(0.125)
        X64, W64 = Xn.astype(np.float64), Wn.astype(np.float64)
        x = cx.device(Xn).requires_grad_(True)
        bias = cx.device(m["b"]).requires_grad_(True)
        v = cx.device(vn).requires_grad_(True)
        w = cx.device(Wn)
        y = sparse_linear(cx.h, cx.idx[0], x, bias, values=v)
        (y * w).sum().backward()
        torch.cuda.synchronize()
        y64, ymag = forward64(vn, X64)
        assert bwd_err(y.detach().cpu().numpy(), y64, ymag) < TOL
        v64 = vn.astype(np.float64)
        gx = np.stack([np.bincount(c, weights=v64 * wv[r], minlength=cols) for wv in W64])
        gxm = np.stack([np.bincount(c, weights=np.abs(v64 * wv[r]), minlength=cols) for wv in W64])
        assert bwd_err(x.grad.cpu().numpy(), gx, gxm) < TOL                                    # the transposed gate of tests/test_gpu_linear_device.py
        assert bwd_err(bias.grad.cpu().numpy(), W64.sum(0), np.abs(W64).sum(0)) < TOL
        gv = sum(W64[u][r] * X64[u][c] for u in range(B))
        gvm = sum(np.abs(W64[u][r] * X64[u][c]) for u in range(B))
        got = v.grad.cpu().numpy()
        assert tuple(v.grad.shape) == (n,) and (np.abs(got.astype(np.float64) - gv) <= TOL * gvm).all()
        # one step
        v2 = (v.detach() - 0.1 * v.grad).requires_grad_(True)
        with torch.no_grad():
            y2 = sparse_linear(cx.h, cx.idx[0], x.detach(), bias.detach(), values=v2.detach())
        torch.cuda.synchronize()
        new64, newmag = forward64(v2.detach().cpu().numpy(), X64)
        assert bwd_err(y2.cpu().numpy(), new64, newmag) < TOL
        assert bwd_err(y2.cpu().numpy(), y64, newmag) > 100 * TOL                              # ... and not the truth of v
        # values=None: the handle's values (v2 now), the bits of linear_device
        y3 = sparse_linear(cx.h, cx.idx[0], x.detach(), bias.detach())
        ref = torch.empty_like(y3)
        torch.cuda.synchronize()
        cx.h.linear_device(cx.idx[0], x.data_ptr(), B, bias.data_ptr(), ref.data_ptr(), 1.0, 1.0)
        cx.h.synchronize()
        torch.cuda.synchronize()
        assert torch.equal(y3, ref) and torch.equal(y3, y2)
        # values that need no gradient: nothing is saved, backward still gives x.grad
        x4 = cx.device(Xn).requires_grad_(True)
        y4 = sparse_linear(cx.h, cx.idx[0], x4, None, values=v2.detach())
        (y4 * w).sum().backward()
        torch.cuda.synchronize()
        assert x4.grad is not None and v2.grad is None
        with pytest.raises(TypeError):
            sparse_linear(cx.h, cx.idx[0], x.detach(), values=v2.detach().double())
        with pytest.raises(ValueError):
            sparse_linear(cx.h, cx.idx[0], x.detach(), values=v2.detach()[:-1])
        with pytest.raises(ValueError):
            sparse_linear(cx.h, cx.idx[0], x.detach(), values=v2.detach().cpu())
    with TCtx(torch, S.SLICES, [m], updates=False) as cx:
        with pytest.raises(ValueError, match="set_value_updates"):
            sparse_linear(cx.h, cx.idx[0], cx.device(Xn), values=cx.device(vn))


def test_no_free_was_rejected():
    from hispmv_amd._lib import lib
    assert lib.hispmv_free_failures() == 0
