"""The transposed product on TILE-STREAM handles (hispmv_tts_transpose.hip): hispmv_spmv_device_t, hispmv_linear_device_t and the
backward pass of sparse_linear on handles created under set_transposable("keep_format"), at the small shapes of
tests/tts_transpose_cases.py (one and two blocks per tile, rows cut by chunk boundaries, fillers, carry tiles found through `fix`, the
small geometry, pass widths 4, 2 and 1).  tests/test_tts_transpose_host.py checks on the host that the cases reach those paths.

Every test creates its handles in state "keep_format" and asserts matrix_info.format == 1 and transpose_info["transposable"]: on a
library without the tile-stream kernels "keep_format" is not a state of the switch, so these tests fail there.

Truth and gate are those of tests/test_gpu_transpose.py: the fp64 scatter y64 = beta * b + alpha * sum v * x[r] at c, mag = |alpha| *
sum |v * x[r]| + |beta * b|, bwd_err(y, y64, mag) < TOL = 1e-5.  The sums arrive through float atomics in no fixed order: on the CPU a
float32 sum of the same terms in three random orders stayed within 2.2e-7 on every case (columns of at most 57 entries), so the gate
leaves about 45x room.  y starts as NaN inside a larger tensor whose other floats hold a sentinel that must survive the call."""
import numpy as np
import pytest

import step_small_cases as S
from conftest import TOL
from step_small_harness import HW
from test_gpu_linear_device import Ctx as LCtx, passes, vec, vecs
from test_gpu_transpose import ALL_PAIRS, Ctx as TCtx, scatter_sums, truth, vectors
from tts_transpose_cases import CASES, case
from util import bwd_err

pytestmark = pytest.mark.gpu

KEEP = "keep_format"


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def accepted(cx, k=0):
    """The handle is a tile stream that the transposed entries accept: what the whole module is about."""
    m, info, ti = cx.mats[k], cx.info[k], cx.h.transpose_info(cx.idx[k])
    assert info["format"] == 1 and info["col_tiles"] == 1, (m["name"], info)
    assert ti["transposable"], (m["name"], ti)
    # the prologue + one launch; one float atomic per stored word that is neither filler nor padding (an upper bound)
    assert ti == dict(transposable=True, launches=2, atomic_bytes=4 * m["r"].size, direct_elems=m["r"].size), (m["name"], ti)
    return info


@pytest.mark.parametrize("name", list(CASES))
def test_parity(torch_mod, name):
    """Every (alpha, beta) pair against the fp64 scatter: beta = 0 passes no bias and must overwrite the NaN-filled y, alpha = 0 and
    beta = 1 gives the bias bit for bit; then d_bias == d_y in place."""
    m, env, _, _ = case(name)
    with TCtx(torch_mod, env, [m], transposable=KEEP) as cx:
        info = accepted(cx)
        assert info["group_slices"] == (13 if name == "small_band" else 28), info
        errs = cx.gate(0, pairs=ALL_PAIRS)
        assert len(errs) == 4
        x, b = vectors(m)
        y = cx.spmv_t(0, x, b, -1.5, 0.5, bias="in_place")
        y64, mag = truth(m, x, b, -1.5, 0.5, key=m["name"])
        assert bwd_err(y, y64, mag) < TOL, name
        y = cx.spmv_t(0, x, b, 1.0, 0.0, bias="nan")                   # beta = 0: a NaN-filled bias buffer is not read
        y64, mag = truth(m, x, b, 1.0, 0.0, key=m["name"])
        assert np.isfinite(y).all() and bwd_err(y, y64, mag) < TOL, name


def test_zero_slots_add_nothing(torch_mod):
    """tts_cut_row: x = +Inf on an empty row (its fillers are zero-valued words) gives a finite y within TOL of the run with 0 there;
    the same with one explicit zero entry of the input in that row."""
    m, env, _, _ = case("tts_cut_row")
    empty = int(np.setdiff1d(np.arange(m["rows"]), m["r"])[77])
    m0 = dict(m, name="tts_cut_row_zero", r=np.append(m["r"], np.int32(empty)), c=np.append(m["c"], np.int32(5)), v=np.append(m["v"], np.float32(0.0)))
    with TCtx(torch_mod, env, [m, m0], transposable=KEEP) as cx:
        for k, mk in enumerate((m, m0)):
            assert cx.info[k]["format"] == 1 and cx.h.transpose_info(cx.idx[k])["transposable"], (mk["name"], cx.info[k])
            x, b = vectors(m)
            x0, xi = x.copy(), x.copy()
            x0[empty], xi[empty] = 0.0, np.inf
            y0 = cx.spmv_t(k, x0, b, 0.85, -2.06)
            yi = cx.spmv_t(k, xi, b, 0.85, -2.06)
            y64, mag = truth(mk, x0, b, 0.85, -2.06)
            assert np.isfinite(yi).all() and bwd_err(yi, y64, mag) < TOL and bwd_err(y0, y64, mag) < TOL, mk["name"]


def test_the_handle_stays_as_it_was(torch_mod):
    """The bits of a forward spmv before and after transposed calls are equal -- on tts_cut_row, whose forward product goes through
    carry[] and the fix-up launch, which the transposed kernel must not touch."""
    m, env, _, _ = case("tts_cut_row")
    with TCtx(torch_mod, env, [m], transposable=KEEP) as cx:
        accepted(cx)
        assert cx.info[0]["n_split_rows"] > 0
        before = cx.spmv(0, m["x"], m["b"], 0.85, -2.06)
        cx.gate(0, pairs=S.PAIRS)
        X = vecs(m, 3, m["rows"])
        dX, dY = cx.device(X), cx.device(np.zeros((3, m["cols"]), np.float32))
        cx.h.linear_device_t(cx.idx[0], dX.data_ptr(), 3, 0, dY.data_ptr(), 1.0, 0.0)
        cx.h.synchronize()
        after = cx.spmv(0, m["x"], m["b"], 0.85, -2.06)
        assert np.array_equal(before.view(np.uint32), after.view(np.uint32))


def test_bf16_tile_stream(torch_mod):
    m = S.as_bf16(S.tile_stream())
    with TCtx(torch_mod, S.AUTO, [m], transposable=KEEP) as cx:
        accepted(cx)
        assert cx.h.value_storage_info(cx.idx[0])["storage"] == "bf16"
        cx.gate(0)


def test_updated_values_reach_the_transposed_product(torch_mod):
    m, env, _, _ = case("tile_stream")
    with TCtx(torch_mod, env, [m], transposable=KEEP, updates=True) as cx:
        accepted(cx)
        assert cx.h.value_update_info(cx.idx[0])["updatable"]
        x, b = vectors(m)
        cx.gate(0, pairs=S.PAIRS[:1])
        v2 = (np.random.default_rng(78).random(m["v"].size, dtype=np.float32) - np.float32(0.5)) * np.float32(3.0)
        cx.h.update_values(cx.idx[0], v2)
        alpha, beta = S.PAIRS[0]
        y = cx.spmv_t(0, x, b, alpha, beta)
        y64, mag = truth(dict(m, v=v2), x, b, alpha, beta)
        old64, _ = truth(m, x, b, alpha, beta, key=m["name"])
        assert bwd_err(y, y64, mag) < TOL
        assert bwd_err(y, old64, mag) > 100 * TOL                       # ... and not the truth of the old values


def _gate_vectors(cx, B, width):
    """linear_device_t for B vectors on matrix 0: the widths, passes and launches linear_info reports, then every vector within TOL
    with a shared bias, without a bias, with a bias per vector and in place.  The references are computed per vector and dropped (x
    of the two-block cases has 5 M columns)."""
    m = cx.mats[0]
    info = cx.h.linear_info(cx.idx[0], B)
    n_pass = passes(B, width, (4, 2, 1))
    assert info["width_t"] == next(w for w in (4, 2, 1) if w <= min(B, width)), (m["name"], B, info)
    assert info["passes_t"] == n_pass and info["launches_t"] == 1 + n_pass, (m["name"], B, info)
    X = vecs(m, B, m["rows"])
    b = vec(m, 100, m["cols"])
    sums = [scatter_sums(m, X[v]) for v in range(B)]

    def check(Y, bias, alpha, beta, what):
        for v, (s, a) in enumerate(sums):
            bb = beta * np.asarray(bias if np.ndim(bias) == 1 else bias[v], np.float64)
            err = bwd_err(Y[v], bb + alpha * s, abs(alpha) * a + np.abs(bb))
            assert np.isfinite(Y[v]).all() and err < TOL, (m["name"], B, v, what, err)

    check(cx.linear_t(0, X, b, 0.85, -2.06), b, 0.85, -2.06, "shared bias")
    check(cx.linear_t(0, X, b, 1.0, 0.0, bias="null"), b, 1.0, 0.0, "no bias")
    Bb = np.stack([b * np.float32(v + 1) for v in range(B)])
    check(cx.linear_t(0, X, Bb, -1.5, 0.5, stride=m["cols"]), Bb, -1.5, 0.5, "a bias per vector")
    check(cx.linear_t(0, X, Bb, -1.5, 0.5, bias="in_place", stride=m["cols"]), Bb, -1.5, 0.5, "in place")
    Y = cx.linear_t(0, X, Bb, 0.0, 1.0, stride=m["cols"])
    assert np.array_equal(Y.view(np.uint32), Bb.view(np.uint32)), (m["name"], B, "alpha = 0 must give the bias bit for bit")


@pytest.mark.parametrize("name,bs", [("xlds_A", (1, 3, 5, 7)), ("two_blocks_3000", (3, 5)), ("two_blocks_20000", (3,)), ("small_band", (7,))])
def test_multi_vector(torch_mod, name, bs):
    """1, 3, 5 and 7 vectors at width 4 (7 = a 4-, a 2- and a 1-wide pass); 3 (a 2-wide and a 1-wide pass) and 5 vectors at width 2;
    3 vectors at width 1 (three launches of the one-vector kernel); 7 vectors in the small geometry."""
    m, env, _, width = case(name)
    with LCtx(torch_mod, env, [m], transposable=KEEP) as cx:
        accepted(cx)
        for B in bs:
            _gate_vectors(cx, B, width)


def test_sparse_linear_backward(torch_mod):
    """x.grad of loss = sum(y * w), y = sparse_linear(h, i, x, bias) on xlds_A against A^T w per vector in fp64."""
    from hispmv_amd.torch_ops import sparse_linear
    torch = torch_mod
    m, env, _, _ = case("xlds_A")
    B, rows, cols = 5, m["rows"], m["cols"]
    with LCtx(torch, env, [m], transposable=KEEP) as cx:
        accepted(cx)
        Xn, Wn = vecs(m, B, cols), np.stack([vec(m, 50 + v, rows) for v in range(B)])
        x = cx.device(Xn).requires_grad_(True)
        bias = cx.device(m["b"]).requires_grad_(True)
        y = sparse_linear(cx.h, cx.idx[0], x, bias)
        (y * cx.device(Wn)).sum().backward()
        torch.cuda.synchronize()
        cx.h.synchronize()
        g = x.grad.cpu().numpy()
        assert tuple(g.shape) == (B, cols)
        for v in range(B):
            s, a = scatter_sums(m, Wn[v])
            assert bwd_err(g[v], s, a) < TOL, v
        v64, X64 = m["v"].astype(np.float64), Xn.astype(np.float64)
        for v in range(B):
            t = v64 * X64[v][m["c"]]
            y64 = np.bincount(m["r"], weights=t, minlength=rows) + m["b"].astype(np.float64)
            mag = np.bincount(m["r"], weights=np.abs(t), minlength=rows) + np.abs(m["b"].astype(np.float64))
            assert bwd_err(y[v].detach().cpu().numpy(), y64, mag) < TOL, v


def test_refusals(torch_mod):
    """In ONE context: a tile stream created in state 0 is refused as before, with both remedies in the message; its twin created in
    state 2 is accepted and takes the same device bytes.  The tall geometry stays refused in state 2, with its name in the message.
    An unknown state raises."""
    import pyhispmv
    m = S.tile_stream()
    x, b = vectors(m)
    with S.environment(S.AUTO):
        h = pyhispmv.FpgaHandle(*HW)
    try:
        with S.environment(S.AUTO):
            i0 = h.create_sparse_handle(m["r"], m["c"], m["v"], m["rows"], m["cols"])
            h.set_transposable(KEEP)
            i2 = h.create_sparse_handle(m["r"], m["c"], m["v"], m["rows"], m["cols"])
            h.set_transposable(2)
            h.set_transposable(0)
            for bad in (3, -1, "slices"):
                with pytest.raises(ValueError):
                    h.set_transposable(bad)
            h.load_matrices()
        a, c = h.matrix_info(i0), h.matrix_info(i2)
        assert a["format"] == 1 and c["format"] == 1 and a["device_bytes"] == c["device_bytes"], (a, c)
        assert h.transpose_info(i0) == dict(transposable=False, launches=0, atomic_bytes=0, direct_elems=0)
        assert h.transpose_info(i2)["transposable"]
        assert h.linear_info(i0, 4)["width_t"] == 0 and h.linear_info(i2, 4)["width_t"] == 1
        d = torch_mod.zeros(4 * (m["rows"] + m["cols"]), dtype=torch_mod.float32, device="cuda")
        px, py = d.data_ptr(), d.data_ptr() + 16 * m["rows"]
        for call in (lambda: h.spmv_device_t(i0, px, 0, py, 1.0, 0.0), lambda: h.linear_device_t(i0, px, 2, 0, py, 1.0, 0.0)):
            with pytest.raises(NotImplementedError, match=r"set_transposable\(True\).*keep_format"):
                call()
        h.spmv_device_t(i2, px, 0, py, 1.0, 0.0)
        h.synchronize()
    finally:
        h.close()
    t = S.tall(S.tile_stream_cut_row(), "tall")             # (120 K entries: under HISPMV_FORMAT=tts fewer than 64 K stay a slice stream)
    x, b = vectors(t)
    with TCtx(torch_mod, S.tall_env("tall"), [t], transposable=KEEP) as cx:
        assert cx.info[0]["format"] == 1 and cx.info[0]["col_tiles"] == 2
        assert cx.h.transpose_info(cx.idx[0]) == dict(transposable=False, launches=0, atomic_bytes=0, direct_elems=0)
        with pytest.raises(NotImplementedError, match="tall geometry"):
            cx.spmv_t(0, x, b, 1.0, 0.0, bias="null")


def test_no_free_was_rejected():
    from hispmv_amd._lib import lib
    assert lib.hispmv_free_failures() == 0
