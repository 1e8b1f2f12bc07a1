"""The wide-batch product with bf16 activations (hispmv_spmm_device_bf16; hispmv_spmm.hip) on loaded slice-stream handles, at the
small shapes of tests/step_small_cases.py, one matrix per code path: no window (256 threads, the nnz = 0 matrix as well), a long chain
(fix-up launch), a compact 256-thread window, wide groups, 1024 threads, stray slots, the two parts of a stray split and eight column
parts (the fp32 tile accumulator), half groups; and, since those 1024-thread matrices are too wide for more than VB 2, the same plans
squeezed into 8000 columns (test_wide_lanes_at_1024_threads: VB 4 and 8 in the window bodies and in the tile accumulator).

Batches B in {1, 65, 130, 257, 513}, ld = B rounded up to 8: VB 1, 2, 4, 8 and 8 with a second tile of one vector; every tile's last
lanes are masked.  The vectors are the pool of tests/test_gpu_spmm.py rounded once to bf16 by CPU torch (the powers of two that scale
them keep them bf16).  The pad columns of xt hold bf16 NaN; yt starts as bf16 NaN inside a tensor of 16-bit sentinel words.

THE ORACLE IS THE FP32 ENTRY.  spmm_device runs on the widened operands with the same (alpha, beta) and the fp32 bias (for a matrix
bias: the widened bf16 matrix), its yt is rounded to bf16 by CPU torch, and the new entry's yt must equal that BIT FOR BIT: (a) for
every vector, the four (alpha, beta) pairs and every class.  Both entries add the same fp32 products in stream order and finish a row
with the same expression, so no tolerance is involved.  The fp32 call itself passes Wide.gate against the fp64 truth of the rounded
pool (bwd_err < TOL), so the oracle is known to have run on the right data.
(b) alpha = 0 gives exactly bf16(beta * bias); beta = 0 with a NaN-filled and with a NULL bias gives finite yt; the zero vector gives +0.
(c) vectors 0, 64, 129, 256, 512 of the larger calls equal the B = 1 call on that vector bit for bit.  (d) two identical calls give
identical bits.  (e) once per class ld = B + 3 with every operand moved by one element (xt, yt: 2 bytes; the fp32 workspace and bias:
4 bytes): spmm_bf16_tiles reports VB 1 and the bits are those of the aligned call.  (f) bias_stride = ld_y with d_bias == d_yt lands
in place and equals the oracle called the same way on the widened matrix.  (g) every word outside yt[rows, B], pad columns included,
and every word around the spmm_bf16_info bytes of the workspace still holds the sentinel; spmm_bf16_info gives the VB and tiles of
the host rule and launches = tiles * sum over the parts of (1 + 1 if the part has a cut row).  (h) spmv_device and spmm_device give
identical bits before and after the bf16 calls.  (i) refusals and argument errors come before any launch."""
import numpy as np
import pytest

import step_small_cases as S
from test_gpu_spmm import ALL_PAIRS, GUARD, Wide, batch, bits, expected_launches, pool_of
from test_gpu_transpose import Ctx

pytestmark = pytest.mark.gpu

SENTINEL16 = 0x5EA1
NAN16 = 0x7FC0
WORK_SENTINEL = 0x5EA15EA1
BATCHES = (1, 65, 130, 257, 513)
PROBES = (0, 64, 129, 256, 512)
_TRUTH = {}


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def to_bf16(torch, a):
    """fp32 -> the bf16 bits (uint16), rounded by CPU torch"""
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16)
    return t.view(torch.int16).numpy().view(np.uint16).copy()


def widen(a16):
    return (np.ascontiguousarray(a16, np.uint16).astype(np.uint32) << 16).view(np.float32)


def ld8(B):
    return (B + 7) & ~7


class Oracle(Wide):
    """The fp32 entry on the pool rounded to bf16: Wide with the rounded pool and its fp64 truth."""

    def __init__(self, cx, k, t=False):
        super().__init__(cx, k, t)
        self.pool = widen(to_bf16(cx.torch, self.pool))

    def truth(self, vecs, bias64, alpha, beta):
        import oracle
        from test_gpu_spmm import POOL, scale_of
        m = self.m
        if m["name"] not in _TRUTH:
            order = np.lexsort((m["c"], m["r"]))
            rp = np.zeros(m["rows"] + 1, np.int64)
            np.add.at(rp, np.asarray(m["r"], np.int64) + 1, 1)
            rp = np.cumsum(rp).astype(np.int32)
            ci, va = np.asarray(m["c"], np.int32)[order], np.asarray(m["v"], np.float32)[order]
            zero = np.zeros(m["rows"], np.float32)
            out = [oracle.spmv_f64(rp, ci, va, self.pool[p], zero, 1.0, 0.0) for p in range(POOL)]
            _TRUTH[m["name"]] = (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]))
        s, a = _TRUTH[m["name"]]
        sc = np.array([float(scale_of(v)) for v in vecs])[:, None]
        idx = [v % POOL for v in vecs]
        bb = beta * np.asarray(bias64, np.float64)
        return alpha * s[idx] * sc + bb, abs(alpha) * a[idx] * sc + np.abs(bb)


class WideBf16:
    """The bf16 calls of one matrix of a Ctx: operands built on the host as 16-bit words, framed with sentinels, checked after every call."""

    def __init__(self, cx, k, t=False):
        self.cx, self.k, self.t, self.m = cx, k, t, cx.mats[k]
        self.n_in = self.m["rows"] if t else self.m["cols"]
        self.n_out = self.m["cols"] if t else self.m["rows"]
        self._xt = {}

    def words(self, a16):
        return self.cx.torch.from_numpy(np.ascontiguousarray(a16, np.uint16).view(np.int16)).to(self.cx.dev)

    def xt(self, X16, ld, shift):
        key = (X16.shape[0], ld, shift, X16[:, :8].tobytes())
        if key not in self._xt:
            a = np.full(self.n_in * ld + shift, NAN16, np.uint16)
            a[shift:].reshape(self.n_in, ld)[:, :X16.shape[0]] = X16.T
            self._xt = {key: self.words(a)}
        d = self._xt[key]
        return d, d.data_ptr() + 2 * shift

    def call(self, X16, b, alpha, beta, ld=None, shift=0, bias="given", work_bytes=None):
        """One call -> Y16 [B, n_out] (uint16).  bias: "given" (b = fp32 [n_out], shared), "null", "nan" (a NaN-filled shared bias),
        "in_place" (b = uint16 [B, n_out]: yt holds it and is passed as the bias with bias_stride = ld).  shift: xt and yt are moved by
        that many 2-byte elements, the fp32 workspace and shared bias by as many floats."""
        cx, torch, h, idx = self.cx, self.cx.torch, self.cx.h, self.cx.idx[self.k]
        B = X16.shape[0]
        ld = ld8(B) if ld is None else ld
        dX, px = self.xt(X16, ld, shift)
        n = self.n_out * ld
        Y0 = np.full(n + 2 * GUARD + shift, SENTINEL16, np.uint16)
        lo = GUARD + shift
        Y0[lo:lo + n].reshape(self.n_out, ld)[:, :B] = np.asarray(b, np.uint16).T if bias == "in_place" else NAN16
        dY = self.words(Y0)
        py = dY.data_ptr() + 2 * lo
        info = h.spmm_bf16_info(idx, B, ld)
        need = info["work_bytes_t" if self.t else "work_bytes"]
        wb = need if work_bytes is None else work_bytes
        dW = torch.from_numpy(np.full(need // 4 + 2 * GUARD + shift, WORK_SENTINEL, np.int32)).to(cx.dev)
        pw = dW.data_ptr() + 4 * lo
        dB, pb, stride = None, 0, 0
        if bias in ("given", "nan"):
            host = np.full(self.n_out + shift, np.nan, np.float32)
            if bias == "given":
                host[shift:] = b
            dB = cx.device(host)
            pb = dB.data_ptr() + 4 * shift
        elif bias == "in_place":
            pb, stride = py, ld
        torch.cuda.synchronize()
        (h.spmm_device_t_bf16 if self.t else h.spmm_device_bf16)(idx, px, B, pb, py, alpha, beta, ld_x=ld, ld_y=ld, bias_stride=stride, work=pw, work_bytes=wb)
        h.synchronize()
        out = dY.cpu().numpy().view(np.uint16)
        inside = np.zeros(out.size, bool)
        inside[lo:lo + n].reshape(self.n_out, ld)[:, :B] = True
        assert (out[~inside] == SENTINEL16).all(), f'{self.m["name"]}: words outside yt[rows, B] were written (B={B}, ld={ld})'        # (g)
        w = dW.cpu().numpy()
        assert (w[:lo] == WORK_SENTINEL).all() and (w[lo + need // 4:] == WORK_SENTINEL).all(), f'{self.m["name"]}: words around the workspace were written'
        return out[lo:lo + n].reshape(self.n_out, ld)[:, :B].T.copy()


def finite16(Y16):
    return ((Y16 & 0x7F80) != 0x7F80).all()


def run_class(cx, k):
    """Every gate of the module docstring on matrix k of the context."""
    from hispmv_amd import prep
    torch = cx.torch
    m, h, idx = cx.mats[k], cx.h, cx.idx[k]
    o, w = Oracle(cx, k), WideBf16(cx, k)
    b = m["b"]
    name = m["name"]
    spmv_before = cx.spmv(k, m["x"], b, 0.85, -2.06)
    spmm_before = o.call(batch(o.pool, 65), b, *S.PAIRS[0])

    def operands(B):
        X = batch(o.pool, B)                       # fp32 [B, cols] holding bf16 values: the oracle's input ...
        X16 = to_bf16(torch, X)                    # ... and the same values as 16-bit words
        assert np.array_equal(bits(widen(X16)), bits(X)), name
        return X, X16

    ones = {}
    for v in PROBES:                                            # the B = 1 call on vector v alone
        ones[v] = w.call(operands(v + 1)[1][v:], b, *S.PAIRS[0])[0]
    aligned65 = None
    for B in BATCHES:
        X, X16 = operands(B)
        ld = ld8(B)
        info, tiles = h.spmm_bf16_info(idx, B, ld), prep.spmm_bf16_tiles(m["cols"], B, ld, 16)
        assert info["accepted"] and (info["vb"], info["tiles"]) == (tiles["vb"], tiles["tiles"]), (name, B, info, tiles)                     # (g)
        if m["cols"] <= 8192:          # (wider matrices are capped by the rule's bound on a tile of xt: 20 000 columns at VB 2, 200 000 at VB 1)
            assert tiles["vb"] == {1: 1, 65: 2, 130: 4, 257: 8, 513: 8}[B] and tiles["tiles"] == (2 if B == 513 else 1), (name, B, tiles)
        assert info["launches"] == expected_launches(cx, k, tiles["tiles"]), (name, B, info)
        parts = cx.info[k]["col_tiles"]
        if parts <= 1:          # one part: the partials alone; more: the fp32 tile accumulator [rows, 64 * VB] behind them
            assert info["work_bytes"] % (2 * 64 * tiles["vb"] * 4) == 0, (name, B, info)
        else:
            assert info["work_bytes"] > m["rows"] * 64 * tiles["vb"] * 4, (name, B, info)
        for alpha, beta in ALL_PAIRS:
            kind = "given" if beta != 0.0 else "null"
            ref = o.call(X, b, alpha, beta, bias=kind)
            o.gate(ref, range(B), b, alpha, beta, f"fp32 oracle B={B}")
            Y = w.call(X16, b, alpha, beta, bias=kind)
            assert np.array_equal(Y, to_bf16(torch, ref)), (name, B, alpha, beta, int((Y != to_bf16(torch, ref)).sum()))                     # (a)
            if alpha == 0.0:
                assert all(np.array_equal(Y[v], to_bf16(torch, np.float32(beta) * b)) for v in range(B)), (name, B)                         # (b)
            if beta == 0.0 and B > 1:
                assert (Y[1] == 0).all(), (name, B)                                                                                          # (b): +0
            if (alpha, beta) == S.PAIRS[0]:
                for v in PROBES:
                    if v < B:
                        assert np.array_equal(Y[v], ones[v]), (name, B, v)                                                                   # (c)
                if B == 65:
                    aligned65 = Y
                if B == 513:
                    assert np.array_equal(Y, w.call(X16, b, alpha, beta)), name                                                              # (d)
    # (e) ld = B + 3 with every operand moved by one element: VB = 1, two-byte aligned rows
    B = 65
    X, X16 = operands(B)
    assert prep.spmm_bf16_tiles(m["cols"], B, B + 3, 2) == dict(vb=1, tiles=2, last_vecs=1, vb_last=1)
    Y = w.call(X16, b, *S.PAIRS[0], ld=B + 3, shift=1)
    assert np.array_equal(Y, aligned65), (name, "shifted")
    for kind in ("nan", "null"):                                                                                                             # (b)
        Y = w.call(X16, b, 1.0, 0.0, bias=kind)
        assert finite16(Y) and np.array_equal(Y, to_bf16(torch, o.call(X, b, 1.0, 0.0, bias=kind))), (name, kind)
    rng = np.random.default_rng(5)
    Bm16 = to_bf16(torch, rng.random((B, m["rows"]), dtype=np.float32))
    ref = o.call(X, widen(Bm16), -1.5, 0.5, bias="in_place")
    o.gate(ref, range(B), widen(Bm16), -1.5, 0.5, "fp32 oracle in place")
    Y = w.call(X16, Bm16, -1.5, 0.5, bias="in_place")                                                                                         # (f)
    assert np.array_equal(Y, to_bf16(torch, ref)), (name, "in place")
    assert np.array_equal(bits(spmv_before), bits(cx.spmv(k, m["x"], b, 0.85, -2.06))), name                                                 # (h)
    assert np.array_equal(bits(spmm_before), bits(o.call(batch(o.pool, 65), b, *S.PAIRS[0]))), name


def test_plans_without_a_window(torch_mod):
    """256 threads, no window: the nnz = 0 matrix and a four-group one of case A."""
    mats = [S.case_a()[0], S.case_a()[4]]
    with Ctx(torch_mod, S.SLICES, mats) as cx:
        for k in range(len(mats)):
            assert cx.info[k]["block_threads"] == 256 and cx.info[k]["lds_bytes"] == 0, cx.info[k]
            run_class(cx, k)


def test_long_chain(torch_mod):
    m = S.single_row_long()
    with Ctx(torch_mod, S.SLICES, [m]) as cx:
        assert cx.info[0]["block_threads"] == 256 and cx.info[0]["lds_bytes"] == 0, cx.info[0]
        assert cx.h.spmm_bf16_info(cx.idx[0], 8)["launches"] == 2
        run_class(cx, 0)


def test_compact_window_256_threads(torch_mod):
    m = S.case_a()[7]
    with Ctx(torch_mod, S.SLICES, [m]) as cx:
        i = cx.info[0]
        assert i["block_threads"] == 256 and i["lds_bytes"] > 0 and i["compact_slices"] == i["n_slices"], i
        run_class(cx, 0)


def test_wide_groups_with_a_window(torch_mod):
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
        assert cx.h.spmm_bf16_info(cx.idx[0], 64)["launches"] == 16
        run_class(cx, 0)


def test_half_groups(torch_mod):
    m = S.as_bf16(S.big_band())
    with Ctx(torch_mod, S.SLICES, [m]) as cx:
        st = cx.h.value_storage_info(cx.idx[0])
        assert st["storage"] == "bf16" and st["slots_2byte"] > 0, st
        run_class(cx, 0)


@pytest.mark.parametrize("kind", ["compact", "stray_slots", "stray_slots_bf16", "stray_split"])
def test_wide_lanes_at_1024_threads(torch_mod, kind):
    """The 1024-thread matrices above have 20 000 columns and more, where the tile rule leaves VB 2: the bodies with the least registers
    to spare would run VB 4 and 8 in no test, and the fp32 tile accumulator only at VB 1 and 2.  The bands of
    tests/test_gpu_spmm_value_grad.py squeezed into 8000 columns keep their plans (1024 threads, compact groups, stray slots in every
    slice of the second, half groups with bf16 values; with 2 % of the entries redrawn the first becomes the two parts of a stray
    split) and take VB 2, 4, 8 at B = 65, 130, 257 (run_class asserts it)."""
    from test_gpu_spmm_value_grad import short_band
    if kind == "compact":
        m = short_band(20000, 8000, 200, 231)
    elif kind == "stray_split":
        m = short_band(20000, 8000, 200, 241, redraw=0.02)
        m = dict(m, expect=dict(format=0, tile_kind=3, parts=2))
    else:
        m = short_band(22000, 8000, 210, 244, redraw=0.02)
    if kind.endswith("bf16"):
        m = S.as_bf16(m)
    with Ctx(torch_mod, S.SLICES, [m]) as cx:
        i = cx.info[0]
        assert i["block_threads"] == 1024 and m["cols"] <= 8192 and i["col_tiles"] == (2 if kind == "stray_split" else 1), i
        if kind != "stray_split":
            assert i["compact_slices"] == i["n_slices"], i
        if kind.startswith("stray_slots"):
            with S.environment(S.SLICES):
                stray, compact, n_slices = S.stray_layout(m)
            assert stray == compact == n_slices > 0, (stray, compact, n_slices)
        if kind.endswith("bf16"):
            assert cx.h.value_storage_info(cx.idx[0])["slots_2byte"] > 0
        run_class(cx, 0)


def test_tile_stream_and_dense_handles_are_refused(torch_mod):
    m, d = S.tile_stream(), S.dense_shapes()[1]
    with Ctx(torch_mod, S.AUTO, [m, d]) as cx:
        assert cx.info[0]["format"] == 1
        for k, match in ((0, "set_transposable"), (1, "dense")):
            info = cx.h.spmm_bf16_info(cx.idx[k], 8)
            assert info == dict(accepted=False, accepted_t=False, vb=0, tiles=0, launches=0, work_bytes=0, work_bytes_t=0), info
            t = torch_mod.zeros(8 * (cx.mats[k]["rows"] + cx.mats[k]["cols"]) + 64, dtype=torch_mod.int16, device="cuda")
            with pytest.raises(NotImplementedError, match=match):
                cx.h.spmm_device_bf16(cx.idx[k], t.data_ptr(), 8, 0, t.data_ptr() + 16 * cx.mats[k]["cols"], work=t.data_ptr(), work_bytes=0)
            with pytest.raises(NotImplementedError, match="companion"):
                cx.h.spmm_device_t_bf16(cx.idx[k], t.data_ptr(), 8, 0, t.data_ptr() + 16 * cx.mats[k]["rows"], work=t.data_ptr(), work_bytes=0)


def test_argument_errors_come_before_any_launch(torch_mod):
    """A workspace too small and ld < B are HISPMV_EINVAL (ValueError); yt is untouched."""
    m = S.case_a()[7]
    with Ctx(torch_mod, S.SLICES, [m]) as cx:
        h, idx, B = cx.h, cx.idx[0], 8
        need = h.spmm_bf16_info(idx, B)["work_bytes"]
        assert need > 0
        xt = torch_mod.zeros(m["cols"] * B, dtype=torch_mod.int16, device="cuda")
        yt = torch_mod.full((m["rows"] * B,), 7, dtype=torch_mod.int16, device="cuda")
        wk = torch_mod.zeros(need // 4, dtype=torch_mod.float32, device="cuda")
        with pytest.raises(ValueError, match="workspace"):
            h.spmm_device_bf16(idx, xt.data_ptr(), B, 0, yt.data_ptr(), work=wk.data_ptr(), work_bytes=need - 4)
        with pytest.raises(ValueError, match="workspace"):
            h.spmm_device_bf16(idx, xt.data_ptr(), B, 0, yt.data_ptr(), work=0, work_bytes=need)
        with pytest.raises(ValueError, match="at least num_vecs"):
            h.spmm_device_bf16(idx, xt.data_ptr(), B, 0, yt.data_ptr(), ld_x=B - 1, work=wk.data_ptr(), work_bytes=need)
        with pytest.raises(ValueError, match="at least num_vecs"):
            h.spmm_device_bf16(idx, xt.data_ptr(), B, 0, yt.data_ptr(), ld_y=B - 1, work=wk.data_ptr(), work_bytes=need)
        with pytest.raises(ValueError):
            h.spmm_device_bf16(idx, xt.data_ptr(), 0, 0, yt.data_ptr(), ld_x=B, ld_y=B, work=wk.data_ptr(), work_bytes=need)
        with pytest.raises(ValueError):
            h.spmm_device_bf16(idx, xt.data_ptr(), B, 0, yt.data_ptr(), beta=1.0, work=wk.data_ptr(), work_bytes=need)          # beta != 0 without a bias
        with pytest.raises(ValueError):
            h.spmm_device_bf16(idx, xt.data_ptr(), B, 0, yt.data_ptr(), bias_stride=3, work=wk.data_ptr(), work_bytes=need)
        with pytest.raises(ValueError, match="aligned"):
            h.spmm_device_bf16(idx, xt.data_ptr() + 1, B, 0, yt.data_ptr(), work=wk.data_ptr(), work_bytes=need)
        with pytest.raises(ValueError, match="aligned"):
            h.spmm_device_bf16(idx, xt.data_ptr(), B, 0, yt.data_ptr(), work=wk.data_ptr() + 2, work_bytes=need)
        with pytest.raises(IndexError):
            h.spmm_device_bf16(99, xt.data_ptr(), B, 0, yt.data_ptr(), work=wk.data_ptr(), work_bytes=need)
        with pytest.raises(NotImplementedError, match="companion"):
            h.spmm_device_t_bf16(idx, yt.data_ptr(), B, 0, xt.data_ptr(), work=wk.data_ptr(), work_bytes=need)
        h.synchronize()
        assert (yt == 7).all()


def test_refused_before_load_matrices(torch_mod):
    import pyhispmv
    from step_small_harness import HW
    m = S.case_a()[1]
    h = pyhispmv.FpgaHandle(*HW)
    try:
        i = h.create_sparse_handle(m["r"], m["c"], m["v"], m["rows"], m["cols"])
        d = torch_mod.zeros(4 * (m["rows"] + m["cols"]) + (1 << 16), dtype=torch_mod.float32, device="cuda")
        with pytest.raises(AssertionError, match="before load_matrices"):
            h.spmm_device_bf16(i, d.data_ptr(), 4, 0, d.data_ptr() + 16 * m["cols"], work=d.data_ptr() + 16 * (m["rows"] + m["cols"]), work_bytes=1 << 16)
        with pytest.raises(AssertionError, match="before load_matrices"):
            h.spmm_device_t_bf16(i, d.data_ptr(), 4, 0, d.data_ptr() + 16 * m["rows"], work=d.data_ptr() + 16 * (m["rows"] + m["cols"]), work_bytes=1 << 16)
        assert not h.spmm_bf16_info(i, 4)["accepted"]
        h.load_matrices()
        assert h.spmm_bf16_info(i, 4)["accepted"]
    finally:
        h.close()


def test_no_free_was_rejected():
    from hispmv_amd._lib import lib
    assert lib.hispmv_free_failures() == 0
