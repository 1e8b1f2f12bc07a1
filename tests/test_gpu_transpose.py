"""The transposed product y[cols] = alpha * A^T x[rows] + beta * bias[cols] (hispmv_spmv_device_t; hispmv_transpose.hip) on loaded
handles, at the small shapes of tests/step_small_cases.py: every plan kind the slice kernels have (no window, compact and wide
windows, stray slots, half groups, 256 and 1024 threads, cut matrices of two and eight parts), dense handles in fp32 and bf16, and
the tile stream, which has no transposed kernel.  Each handle's plan is asserted with check_expect under the environment
tests/test_gpu_step_small.py uses for the same input.

Truth is the fp64 scatter  y64 = beta * b + alpha * sum v * x[r] at c,  mag = |alpha| * sum |v * x[r]| + |beta * b|;  the gate is
bwd_err(y, y64, mag) < TOL = 1e-5.  The sums arrive through float atomics in no fixed order: on the CPU a float32 sum of the same
terms in three random orders stayed within 3.4e-7 on every sparse input below (columns of up to 309 entries), so the gate leaves
about 30x room.  x (length rows) and bias (length cols) are drawn here, seeded per matrix.  y starts as NaN inside a larger tensor
whose other floats hold a sentinel that must survive the call."""
import zlib

import numpy as np
import pytest

import step_small_cases as S
from conftest import TOL
from step_small_harness import HW, SHARED
from util import bwd_err, csr_truth

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0x5EA15EA1
ALL_PAIRS = S.PAIRS + S.MORE_PAIRS
_SUMS = {}
_PACKS = {}          # the host packer's parts per (matrix, plan), for check_expect


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def vectors(m):
    rng = np.random.default_rng(zlib.crc32(m["name"].encode()))
    return rng.random(m["rows"], dtype=np.float32) - np.float32(0.3), rng.random(m["cols"], dtype=np.float32)


def scatter_sums(m, x, key=None):
    """(sum v * x[r], sum |v * x[r]|) per column in fp64; cached per matrix when `key` is given (the reference is computed once)."""
    if key is not None and key in _SUMS:
        return _SUMS[key]
    x64 = np.asarray(x, np.float64)
    if m.get("dense"):
        W64 = m["W"].astype(np.float64)
        out = (W64.T @ x64, np.abs(W64).T @ np.abs(x64))
    else:
        t = m["v"].astype(np.float64) * x64[m["r"]]
        out = (np.bincount(m["c"], weights=t, minlength=m["cols"]), np.bincount(m["c"], weights=np.abs(t), minlength=m["cols"]))
    if key is not None:
        _SUMS[key] = out
    return out


def truth(m, x, b, alpha, beta, key=None):
    s, a = scatter_sums(m, x, key)
    bb = beta * np.asarray(b, np.float64)
    return bb + alpha * s, abs(alpha) * a + np.abs(bb)


class Ctx:
    """One context created under the case's switches, the matrices created (each under its own storage / updates / transposable
    switches), loaded, and their plans checked against the expectations of tests/step_small_cases.py."""

    def __init__(self, torch, env, mats, transposable=None, updates=False):
        import pyhispmv
        self.torch, self.env, self.mats = torch, dict(SHARED, **env), mats
        self.dev = torch.device("cuda", 0)
        with S.environment(self.env):
            self.h = pyhispmv.FpgaHandle(*HW)
        try:
            with S.environment(self.env):
                if transposable is not None:
                    self.h.set_transposable(transposable)
                self.h.set_value_updates(updates)
                self.idx = []
                for m in mats:
                    self.h.set_value_storage(m.get("storage", "fp32"))
                    if m.get("dense"):
                        self.idx.append(self.h.create_dense_handle(m["W"].flatten(), m["rows"], m["cols"]))
                    else:
                        self.idx.append(self.h.create_sparse_handle(m["r"], m["c"], m["v"], m["rows"], m["cols"]))
                    assert self.idx[-1] >= 0
                self.h.load_matrices()
            self.info = [self.h.matrix_info(i) for i in self.idx]
            for m, info in zip(mats, self.info):
                if m.get("dense"):
                    continue
                key = (m["name"], info["format"], info["col_tiles"], info["tile_kind"], info["col_tile_width"], info["col_tile_base"], info["group_slices"])
                if key not in _PACKS:
                    _PACKS[key] = S.packed(m, info)
                S.check_expect(m, info, _PACKS[key])
        except BaseException:
            self.h.close()
            raise

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.torch.cuda.synchronize()
        self.h.close()

    def device(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(self.dev)

    def spmv_t(self, k, x, b, alpha, beta, bias="given", shift=0):
        """One transposed call on matrix k -> y (numpy).  bias: "given", "null" (pointer 0), "nan" (a NaN-filled buffer), "in_place"
        (y holds the bias and is passed as both).  shift: floats by which y and bias are moved off the 16-byte alignment."""
        torch, m = self.torch, self.mats[k]
        cols = m["cols"]
        Y0 = np.full(cols + 2 * GUARD + shift, SENTINEL, np.int32).view(np.float32)
        lo = GUARD + shift
        Y0[lo:lo + cols] = np.asarray(b, np.float32) if bias == "in_place" else np.nan
        dY = self.device(Y0)
        dX = self.device(x)
        B = np.full(cols + shift, np.nan, np.float32)
        if bias == "given":
            B[shift:] = b
        dB = self.device(B)
        py = dY.data_ptr() + 4 * lo
        pb = {"given": dB.data_ptr() + 4 * shift, "nan": dB.data_ptr() + 4 * shift, "null": 0, "in_place": py}[bias]
        torch.cuda.synchronize()
        self.h.spmv_device_t(self.idx[k], dX.data_ptr(), pb, py, alpha, beta)
        self.h.synchronize()
        out = dY.cpu().numpy()
        guard = np.ones(out.size, bool)
        guard[lo:lo + cols] = False
        assert (out.view(np.int32)[guard] == SENTINEL).all(), f'{m["name"]}: floats outside y were written'
        return out[lo:lo + cols].copy()

    def spmv(self, k, x, b, alpha, beta):
        torch, m = self.torch, self.mats[k]
        dX, dB = self.device(x), self.device(b)
        dY = self.device(np.full(m["rows"], np.nan, np.float32))
        torch.cuda.synchronize()
        self.h.spmv_device(self.idx[k], dX.data_ptr(), dB.data_ptr() if beta != 0.0 else 0, dY.data_ptr(), alpha, beta)
        self.h.synchronize()
        return dY.cpu().numpy()

    def gate(self, k, pairs=ALL_PAIRS, shift=0):
        """Every (alpha, beta) pair on matrix k against the fp64 scatter; beta = 0 passes no bias; alpha = 0, beta = 1 must give the bias bit for bit."""
        m = self.mats[k]
        x, b = vectors(m)
        errs = []
        for alpha, beta in pairs:
            y = self.spmv_t(k, x, b, alpha, beta, bias="given" if beta != 0.0 else "null", shift=shift)
            y64, mag = truth(m, x, b, alpha, beta, key=m["name"])
            err = bwd_err(y, y64, mag)
            print(f'{m["name"]}: alpha={alpha} beta={beta} backward error {err:.3e}')
            assert np.isfinite(y).all() and err < TOL, (m["name"], alpha, beta, err)
            if alpha == 0.0 and beta == 1.0:
                assert np.array_equal(y.view(np.uint32), b.view(np.uint32)), m["name"]
            errs.append(err)
        return errs


def _all(cx, **kw):
    for k in range(len(cx.mats)):
        info = cx.h.transpose_info(cx.idx[k])
        assert info["transposable"] and info["launches"] >= 2, (cx.mats[k]["name"], info)
        cx.gate(k, **kw)


def test_plans_without_a_window(torch_mod):
    """256 threads, no window: the six plain matrices of case A (nnz = 0 and 1024 among them), the 1 x 1 matrix, one row over some
    thirty slices, 50 live rows among 49 950 fillers.  Every element adds to y directly."""
    a = S.case_a()
    mats = a[:6] + a[8:]
    with Ctx(torch_mod, S.SLICES, mats) as cx:
        _all(cx)
        for k, m in enumerate(mats):
            info, ti = cx.info[k], cx.h.transpose_info(cx.idx[k])
            if info["lds_bytes"] == 0:
                assert ti["direct_elems"] == info["n_elems"] and ti["atomic_bytes"] == 4 * info["n_elems"], (m["name"], ti, info)


def test_compact_windows_256_threads(torch_mod):
    """Window, 256 threads, compact: the windowed uniform matrix and band_4000x300.  Only flushes add to y."""
    mats = S.case_a()[6:8]
    with Ctx(torch_mod, S.SLICES, mats) as cx:
        assert all(i["block_threads"] == 256 and i["lds_bytes"] > 0 and i["compact_slices"] == i["n_slices"] for i in cx.info), cx.info
        _all(cx)
        for k in range(2):
            ti = cx.h.transpose_info(cx.idx[k])
            assert ti["direct_elems"] == 0 and ti["atomic_bytes"] > 0 and ti["launches"] == 2, ti


def test_wide_groups_with_a_window_and_l2_elements(torch_mod):
    m = S.two_way_band()
    with Ctx(torch_mod, S.NOSPLIT, [m]) as cx:
        assert cx.info[0]["compact_slices"] == 0 and cx.info[0]["lds_bytes"] > 0
        ti = cx.h.transpose_info(cx.idx[0])
        assert 0 < ti["direct_elems"] < m["r"].size // 20, ti                    # about 1 % of the entries were re-drawn
        _all(cx)


def test_1024_threads_compact_and_the_handle_stays_as_it_was(torch_mod):
    """big_band: the 1024-thread compact plan.  Two identical calls both pass the gate (equality is not required); spmv_device on
    the same handle gives identical bits before and after the transposed calls; the adjoint identity
    |<A x, w> - <x, A^T w>| <= TOL * sum |a_ij x_j w_i| with both products from the device."""
    m = S.big_band()
    with Ctx(torch_mod, S.SLICES, [m]) as cx:
        w, b = vectors(m)                      # w: rows floats, the transposed product's input
        before = cx.spmv(0, m["x"], m["b"], 0.85, -2.06)
        first = cx.gate(0)
        second = cx.gate(0, pairs=S.PAIRS)
        assert len(first) == 4 and len(second) == 2
        after = cx.spmv(0, m["x"], m["b"], 0.85, -2.06)
        assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
        Ax = cx.spmv(0, m["x"], m["b"], 1.0, 0.0).astype(np.float64)
        Atw = cx.spmv_t(0, w, b, 1.0, 0.0, bias="null").astype(np.float64)
        x64, w64 = m["x"].astype(np.float64), w.astype(np.float64)
        scale = float(np.sum(np.abs(m["v"].astype(np.float64) * x64[m["c"]] * w64[m["r"]])))
        lhs, rhs = float(Ax @ w64), float(x64 @ Atw)
        print(f"adjoint: <Ax,w> = {lhs!r}, <x,A^T w> = {rhs!r}, |difference| / scale = {abs(lhs - rhs) / scale:.3e}")
        assert abs(lhs - rhs) <= TOL * scale


def test_stray_slots(torch_mod):
    m = S.stray_slot_band()
    with Ctx(torch_mod, S.SLICES, [m]) as cx:
        assert cx.info[0]["block_threads"] == 1024 and cx.info[0]["compact_slices"] == cx.info[0]["n_slices"], cx.info[0]
        ti = cx.h.transpose_info(cx.idx[0])
        assert ti["direct_elems"] == 0, ti
        _all(cx)


def test_two_parts_of_a_stray_split(torch_mod):
    m = S.stray_split_band()
    with Ctx(torch_mod, S.SLICES, [m]) as cx:
        assert cx.info[0]["tile_kind"] == 3 and cx.info[0]["col_tiles"] == 2
        assert cx.h.transpose_info(cx.idx[0])["launches"] == 3
        _all(cx)


def test_eight_column_parts(torch_mod):
    m = S.column_tiled()
    with Ctx(torch_mod, S.COLTILES, [m]) as cx:
        assert cx.info[0]["tile_kind"] == 1 and cx.info[0]["col_tiles"] == 8
        assert cx.h.transpose_info(cx.idx[0])["launches"] == 9
        _all(cx)


@pytest.mark.parametrize("make", [S.big_band, S.stray_slot_band], ids=["big_band", "stray_slot_band"])
def test_half_groups(torch_mod, make):
    m = S.as_bf16(make())
    with Ctx(torch_mod, S.SLICES, [m]) as cx:
        st = cx.h.value_storage_info(cx.idx[0])
        assert st["storage"] == "bf16" and st["slots_2byte"] > 0, st
        _all(cx)


def _dense_cases():
    rng = np.random.default_rng(62)
    odd = dict(name="dense_odd_1000x1003", dense=True, rows=1000, cols=1003, W=rng.standard_normal((1000, 1003), dtype=np.float32))
    return S.dense_shapes()[:5] + [odd]


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
def test_dense_handles(torch_mod, storage):
    """The first five dense shapes and 1000 x 1003 (odd cols: rows of W start at any 4-byte -- bf16: 2-byte -- boundary; 63 row
    blocks add into y), y and bias once 16-byte aligned and once shifted by one float."""
    mats = _dense_cases()
    if storage == "bf16":
        mats = [S.as_bf16(m) for m in mats]
    with Ctx(torch_mod, S.SLICES, mats) as cx:
        for k, m in enumerate(mats):
            ti = cx.h.transpose_info(cx.idx[k])
            assert ti["transposable"] and ti["launches"] == 2 and ti["direct_elems"] == 0, ti
            assert (ti["atomic_bytes"] > 0) == (m["rows"] > 16), (m["name"], ti)
            cx.gate(k)
            cx.gate(k, pairs=S.PAIRS[:1], shift=1)


def test_tile_stream_is_refused_until_created_transposable(torch_mod):
    m = S.tile_stream()
    x, b = vectors(m)
    with Ctx(torch_mod, S.AUTO, [m]) as cx:
        assert cx.info[0]["format"] == 1
        assert cx.h.transpose_info(cx.idx[0]) == dict(transposable=False, launches=0, atomic_bytes=0, direct_elems=0)
        before = cx.spmv(0, m["x"], m["b"], 0.85, -2.06)
        with pytest.raises(NotImplementedError, match="set_transposable"):
            cx.spmv_t(0, x, b, 1.0, 0.0, bias="null")
        after = cx.spmv(0, m["x"], m["b"], 0.85, -2.06)
        assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
        y64, mag = csr_truth(m["r"], m["c"], m["v"], m["rows"], m["x"], m["b"], 0.85, -2.06)
        assert bwd_err(after, y64, mag) < TOL
    with Ctx(torch_mod, S.AUTO, [S.as_slices(m)], transposable=True) as cx:
        assert cx.info[0]["format"] == 0
        _all(cx)


def test_contracts(torch_mod):
    """beta = 0: a NULL bias is accepted, a NaN-filled bias buffer is not read, the NaN-filled y is overwritten everywhere;
    d_bias == d_y in place; d_x == d_y, NULL vectors and a bad index are refused; on sparse_rows, x = +Inf on one empty row gives a
    finite y within TOL of the run with 0 there (a zero slot adds nothing)."""
    a = S.case_a()
    mats = [a[7], a[10], S.dense_shapes()[1]]
    with Ctx(torch_mod, S.SLICES, mats) as cx:
        for k, m in enumerate(mats):
            x, b = vectors(m)
            y64, mag = truth(m, x, b, 1.0, 0.0, key=m["name"])
            for bias in ("null", "nan"):
                y = cx.spmv_t(k, x, b, 1.0, 0.0, bias=bias)
                assert np.isfinite(y).all() and bwd_err(y, y64, mag) < TOL, (m["name"], bias)
            y64, mag = truth(m, x, b, -1.5, 0.5, key=m["name"])
            y = cx.spmv_t(k, x, b, -1.5, 0.5, bias="in_place")
            assert bwd_err(y, y64, mag) < TOL, m["name"]
            d = cx.device(np.zeros(max(m["rows"], m["cols"]), np.float32))
            with pytest.raises(ValueError):
                cx.h.spmv_device_t(cx.idx[k], d.data_ptr(), 0, d.data_ptr(), 1.0, 0.0)
            with pytest.raises(ValueError):
                cx.h.spmv_device_t(cx.idx[k], d.data_ptr(), 0, 0, 1.0, 0.0)
            with pytest.raises(ValueError):
                cx.h.spmv_device_t(cx.idx[k], d.data_ptr(), 0, d.data_ptr() + 4 * 4096, 1.0, 1.0)      # beta != 0 without a bias
        with pytest.raises(IndexError):
            cx.h.spmv_device_t(99, 1, 0, 2, 1.0, 0.0)
        m = mats[1]
        x, b = vectors(m)
        empty = int(np.setdiff1d(np.arange(m["rows"]), m["r"])[777])
        x0, xi = x.copy(), x.copy()
        x0[empty], xi[empty] = 0.0, np.inf
        y0 = cx.spmv_t(1, x0, b, 0.85, -2.06)
        yi = cx.spmv_t(1, xi, b, 0.85, -2.06)
        y64, mag = truth(m, x0, b, 0.85, -2.06)
        assert np.isfinite(yi).all() and bwd_err(yi, y64, mag) < TOL and bwd_err(y0, y64, mag) < TOL


def test_refused_before_load_matrices(torch_mod):
    """HISPMV_ESTATE for a handle that is created but not loaded (an AssertionError in Python); transpose_info reports zeros for it."""
    import pyhispmv
    m = S.case_a()[1]
    h = pyhispmv.FpgaHandle(*HW)
    try:
        i = h.create_sparse_handle(m["r"], m["c"], m["v"], m["rows"], m["cols"])
        d = torch_mod.zeros(m["rows"] + m["cols"], dtype=torch_mod.float32, device="cuda")
        with pytest.raises(AssertionError, match="before load_matrices"):
            h.spmv_device_t(i, d.data_ptr(), 0, d.data_ptr() + 4 * m["rows"], 1.0, 0.0)
        assert h.transpose_info(i) == dict(transposable=False, launches=0, atomic_bytes=0, direct_elems=0)
        h.load_matrices()
        assert h.transpose_info(i)["transposable"]
    finally:
        h.close()


def test_updated_values_reach_the_transposed_product(torch_mod):
    m = S.case_a()[7]
    with Ctx(torch_mod, S.SLICES, [m], updates=True) as cx:
        assert cx.h.value_update_info(cx.idx[0])["updatable"]
        x, b = vectors(m)
        cx.gate(0, pairs=S.PAIRS[:1])
        v2 = (np.random.default_rng(77).random(m["v"].size, dtype=np.float32) - np.float32(0.5)) * np.float32(3.0)
        cx.h.update_values(cx.idx[0], v2)
        new = dict(m, v=v2)
        alpha, beta = S.PAIRS[0]
        y = cx.spmv_t(0, x, b, alpha, beta)
        y64, mag = truth(new, x, b, alpha, beta)
        old64, _ = truth(m, x, b, alpha, beta, key=m["name"])
        assert bwd_err(y, y64, mag) < TOL
        assert bwd_err(y, old64, mag) > 100 * TOL                       # ... and not the truth of the old values


def test_no_free_was_rejected():
    from hispmv_amd._lib import lib
    assert lib.hispmv_free_failures() == 0
