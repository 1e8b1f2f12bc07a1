"""The value gradient grad[k] = alpha * sum_v gy[v, row_k] * x[v, col_k] + beta * grad[k] on TILE-STREAM handles
(hispmv_value_grad_device through hispmv_tts_transpose.hip) and sparse_linear(..., values=v) on top of it: updatable handles created
under set_transposable("keep_format"), the first five cases of tests/tts_transpose_cases.py (the small geometry cannot be updatable).
Every test asserts matrix_info.format == 1 and value_grad_info["accepted"]: on a library without the tile-stream kernels
"keep_format" is not a state of the switch, so these tests fail there.

EXACTNESS, the integer scheme of tests/test_gpu_value_grad.py: gy and x hold integers in [-3, 3] drawn per (matrix, vector), grad0
integers in [-8, 8], (alpha, beta) one of (1, 0), (0.5, 1), (0, 1).  With at most 7 vectors every partial sum stays below
7 * 9 + 8 < 2^24 and 0.5 * s is exact, so fp32 is exact in any order and grad must equal the numpy result BIT FOR BIT at every entry of
the creation input -- duplicates (each with its own, equal gradient; the uniform cases draw some) and explicit zeros (appended here:
the kernel goes by the map, not by the values) included.  For beta = 0 grad starts as NaN and must be overwritten everywhere; it lies
inside a sentinel-filled tensor whose guards must survive.  A second identical call must give identical bits."""
import numpy as np
import pytest

from test_gpu_linear_device import passes
from test_gpu_value_grad import Ctx as VCtx, ints
from tts_transpose_cases import UPDATABLE, case

pytestmark = pytest.mark.gpu

KEEP = "keep_format"
BS = (1, 2, 5, 7)
PAIRS = ((1.0, 0.0), (0.5, 1.0), (0.0, 1.0))


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def with_explicit_zeros(m):
    """The matrix with 16 explicit zeros appended to its input: 8 at positions that hold no other entry, 8 duplicating an entry."""
    rng = np.random.default_rng(9)
    r = np.concatenate([rng.integers(0, m["rows"], 8), m["r"][:8]]).astype(np.int32)
    c = np.concatenate([rng.integers(0, m["cols"], 8), m["c"][:8]]).astype(np.int32)
    return dict(m, name=m["name"] + "_zeros", r=np.append(m["r"], r), c=np.append(m["c"], c), v=np.append(m["v"], np.zeros(16, np.float32)))


@pytest.mark.parametrize("name", UPDATABLE)
def test_bit_equal_to_numpy(torch_mod, name):
    m, env, _, width = case(name)
    m = with_explicit_zeros(m)
    with VCtx(torch_mod, env, [m], transposable=KEEP) as cx:
        assert cx.info[0]["format"] == 1 and cx.info[0]["col_tiles"] == 1, cx.info[0]
        assert cx.h.transpose_info(cx.idx[0])["transposable"]
        n = cx.n[0]
        assert n == m["r"].size
        key = np.stack([m["r"], m["c"]], 1)
        assert np.unique(key, axis=0).shape[0] < n                       # the input holds duplicates
        r, c = m["r"].astype(np.int64), m["c"].astype(np.int64)
        GY = np.stack([ints(m, "gy", v, m["rows"]) for v in range(max(BS))])
        X = np.stack([ints(m, "x", v, m["cols"]) for v in range(max(BS))])
        g0 = ints(m, "grad0", 0, n, -8, 8)
        s = np.zeros(n)
        sums = {}
        for v in range(max(BS)):
            s = s + GY[v].astype(np.float64)[r] * X[v].astype(np.float64)[c]
            sums[v + 1] = s
        for B in BS:
            info = cx.h.value_grad_info(cx.idx[0], B)
            n_pass = passes(B, width, (4, 2, 1))
            assert info == dict(accepted=True, width=next(w for w in (4, 2, 1) if w <= min(B, width)), passes=n_pass, launches=n_pass), (name, B, info)
            for alpha, beta in PAIRS:
                # (alpha == 0: gy and x are not read, the result is beta * grad0 and not 0 * s, which is -0 where s < 0)
                want = ((alpha * sums[B] if alpha != 0.0 else np.zeros(n)) + (beta * g0.astype(np.float64) if beta != 0.0 else 0.0)).astype(np.float32)
                got = cx.value_grad(0, GY[:B], X[:B], None if beta == 0.0 else g0, alpha, beta)       # beta = 0: grad starts as NaN
                bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
                assert bad.size == 0, (name, B, alpha, beta, bad.size, bad[:8], got[bad[:8]], want[bad[:8]])
        first = cx.value_grad(0, GY[:5], X[:5], g0, 0.5, 1.0)
        second = cx.value_grad(0, GY[:5], X[:5], g0, 0.5, 1.0)
        assert np.array_equal(first.view(np.uint32), second.view(np.uint32)), (name, "a second identical call gave other bits")


def test_refused_without_updates_or_in_state_0(torch_mod):
    """The order of the refusals: not updatable -> AssertionError (HISPMV_ESTATE) even on an accepted tile stream; an updatable tile
    stream created in state 0 -> NotImplementedError naming both remedies."""
    import pyhispmv
    import step_small_cases as S
    from step_small_harness import HW
    m = S.tile_stream()
    with S.environment(S.AUTO):
        h = pyhispmv.FpgaHandle(*HW)
    try:
        with S.environment(S.AUTO):
            h.set_transposable(KEEP)
            plain = h.create_sparse_handle(m["r"], m["c"], m["v"], m["rows"], m["cols"])
            h.set_transposable(False)
            h.set_value_updates(True)
            state0 = h.create_sparse_handle(m["r"], m["c"], m["v"], m["rows"], m["cols"])
            h.load_matrices()
        assert h.matrix_info(plain)["format"] == 1 and h.matrix_info(state0)["format"] == 1
        assert h.value_grad_info(plain, 4) == dict(accepted=False, width=0, passes=0, launches=0)
        assert h.value_grad_info(state0, 4) == dict(accepted=False, width=0, passes=0, launches=0)
        d = torch_mod.zeros(m["rows"] + m["cols"] + m["r"].size, dtype=torch_mod.float32, device="cuda")
        pg, px, pr = d.data_ptr(), d.data_ptr() + 4 * m["rows"], d.data_ptr() + 4 * (m["rows"] + m["cols"])
        with pytest.raises(AssertionError, match="set_value_updates"):
            h.value_grad_device(plain, pg, px, 1, pr)
        with pytest.raises(NotImplementedError, match=r"set_transposable\(True\).*keep_format"):
            h.value_grad_device(state0, pg, px, 1, pr)
    finally:
        h.close()


def test_three_training_steps_reduce_the_loss(torch_mod):
    """loss(v) = 1/2 sum_b |A(v) x_b - t_b|^2 on xlds_A, t = A(v*) x: three steps v -= lr * v.grad through sparse_linear(..., values=v)
    reduce it every time.  The Hessian in v is block diagonal per row, its largest eigenvalue at most sum_b sum_{k in the row} x_b[c_k]^2
    <= B * (entries of the fullest row) * max x^2 =: L, and a step of 1 / L cannot increase a quadratic loss."""
    from hispmv_amd.torch_ops import sparse_linear
    torch = torch_mod
    m, env, _, _ = case("xlds_A")
    B = 4
    with VCtx(torch, env, [m], transposable=KEEP) as cx:
        assert cx.info[0]["format"] == 1 and cx.h.value_grad_info(cx.idx[0], B)["accepted"]
        rng = np.random.default_rng(11)
        X = rng.random((B, m["cols"]), dtype=np.float32) - np.float32(0.3)
        lr = 1.0 / (B * np.bincount(m["r"]).max() * float((X * X).max()))
        x = cx.device(X)
        target_values = cx.device(m["v"])
        with torch.no_grad():
            t = sparse_linear(cx.h, cx.idx[0], x, None, values=target_values).clone()
        v = cx.device(m["v"] + np.float32(0.25) * (rng.random(m["v"].size, dtype=np.float32) - np.float32(0.5))).requires_grad_(True)
        losses = []
        for _ in range(4):
            y = sparse_linear(cx.h, cx.idx[0], x, None, values=v)
            loss = 0.5 * ((y - t) ** 2).sum()
            losses.append(float(loss.detach()))
            loss.backward()
            with torch.no_grad():
                v -= lr * v.grad
                v.grad = None
            torch.cuda.synchronize()
        print("losses", losses)
        assert losses[0] > 0 and all(b < a for a, b in zip(losses, losses[1:])), losses


def test_no_free_was_rejected():
    from hispmv_amd._lib import lib
    assert lib.hispmv_free_failures() == 0
