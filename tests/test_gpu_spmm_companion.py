"""The transposed wide-batch product (hispmv_spmm_device_t) and sparse_linear(..., spmm=True).

spmm_device_t runs the launches of spmm_device over the stored transpose of a handle created under set_transposable("companion").
P is such a handle, R a handle made from the swapped COO in the same context.  Gates on big_band (1024 threads, compact) and the
windowed uniform matrix (256 threads, compact): every vector of spmm_device_t on P against the fp64 scatter truth of
tests/test_gpu_transpose.py (bwd_err < TOL), bit-equal to spmm_device on R, and bit-stable across two runs; a handle without a
companion raises NotImplementedError.  sparse_linear(spmm=True): forward close to spmm=False within TOL * mag, grad_x and grad_bias
finite and within TOL of the fp64 truth, two backward passes bit-equal, and spmm=False still gives the bits of linear_device."""
import numpy as np
import pytest

import step_small_cases as S
from conftest import TOL
from test_gpu_spmm import Wide, batch, bits, scale_of, POOL
from test_gpu_transpose import Ctx, scatter_sums
from util import bwd_err

pytestmark = pytest.mark.gpu

B = 65


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def swapped(m):
    return dict(m, name=m["name"] + "_T", pool_key=m["name"] + "_rows", rows=m["cols"], cols=m["rows"], r=m["c"], c=m["r"],
                x=np.resize(m["x"], m["rows"]).astype(np.float32), b=np.resize(m["b"], m["cols"]).astype(np.float32), expect=dict(format=0))


class Pair(Ctx):
    """P = mats[0] (created under "companion") and R = mats[1] (the swapped COO, created with the switch off), loaded in one context."""

    def __init__(self, torch, m, updates=False):
        import pyhispmv
        from step_small_harness import HW, SHARED
        self.torch, self.env = torch, dict(SHARED, **S.SLICES)
        self.mats = [dict(m, pool_key=m["name"] + "_rows"), swapped(m)]
        self.dev = torch.device("cuda", 0)
        with S.environment(self.env):
            self.h = h = pyhispmv.FpgaHandle(*HW)
            try:
                h.set_value_updates(updates)
                h.set_transposable("companion")
                p = h.create_sparse_handle(m["r"], m["c"], m["v"], m["rows"], m["cols"])
                h.set_transposable(0)
                r = h.create_sparse_handle(m["c"], m["r"], m["v"], m["cols"], m["rows"])
                self.idx = [p, r]
                h.load_matrices()
                self.info = [h.matrix_info(i) for i in self.idx]
            except BaseException:
                h.close()
                raise


def scatter_truth(m, pool, vecs, bias64, alpha, beta):
    """fp64 truth of A^T x for vectors `vecs` of the batch made from `pool` [POOL, rows]: scatter_sums per pool vector, scaled exactly."""
    sums = {p: scatter_sums(m, pool[p]) for p in sorted({v % POOL for v in vecs})}
    bb = beta * np.asarray(bias64, np.float64)
    y64 = np.stack([alpha * sums[v % POOL][0] * float(scale_of(v)) for v in vecs]) + bb
    mag = np.stack([abs(alpha) * sums[v % POOL][1] * float(scale_of(v)) for v in vecs]) + np.abs(bb)
    return y64, mag


@pytest.mark.parametrize("make", [S.big_band, lambda: S.case_a()[6]], ids=["big_band", "windowed_uniform"])
def test_transposed_wide_product_over_the_stored_transpose(torch_mod, make):
    m = make()
    with Pair(torch_mod, m) as cx:
        ci = cx.h.companion_info(cx.idx[0])
        assert ci["has"] and ci["format"] == 0, ci
        assert cx.info[0]["format"] == 0 and cx.info[1]["format"] == 0
        info = cx.h.spmm_info(cx.idx[0], B, 68)
        assert info["accepted"] and info["accepted_t"] and info["work_bytes_t"] > 0, info
        assert not cx.h.spmm_info(cx.idx[1], B, 68)["accepted_t"]
        wt, wr = Wide(cx, 0, t=True), Wide(cx, 1)
        assert np.array_equal(wt.pool, wr.pool)                   # the same batch of [B, rows] vectors for both routes
        X = batch(wt.pool, B)
        bias = np.resize(m["b"], m["cols"]).astype(np.float32)
        for alpha, beta in S.PAIRS:
            kind = "given" if beta != 0.0 else "null"
            Yt = wt.call(X, bias, alpha, beta, bias=kind)
            y64, mag = scatter_truth(m, wt.pool, range(B), bias, alpha, beta)
            err = max(bwd_err(Yt[i], y64[i], mag[i]) for i in range(B))
            print(f'{m["name"]}: spmm_device_t alpha={alpha} beta={beta} worst backward error {err:.3e}')
            assert np.isfinite(Yt).all() and err < TOL, (m["name"], alpha, beta, err)
            Yr = wr.call(X, bias, alpha, beta, bias=kind)
            assert np.array_equal(bits(Yt), bits(Yr)), (m["name"], alpha, beta)
            assert np.array_equal(bits(Yt), bits(wt.call(X, bias, alpha, beta, bias=kind))), (m["name"], alpha, beta)
        d = torch_mod.zeros(4 * (m["rows"] + m["cols"]) + (1 << 20), dtype=torch_mod.float32, device="cuda")
        with pytest.raises(NotImplementedError, match="companion"):            # R has no stored transpose
            cx.h.spmm_device_t(cx.idx[1], d.data_ptr(), 4, 0, d.data_ptr() + 16 * m["cols"], work=d.data_ptr() + 16 * (m["rows"] + m["cols"]), work_bytes=4 << 20)


@pytest.mark.parametrize("B", [65, 200])
def test_sparse_linear_through_the_wide_entries(torch_mod, B):
    """On torch's default stream and inside a stream of its own.  x [B, cols] and grad_y [B, rows] are drawn here.  sparse_linear pads
    the leading dimension to a multiple of 4, so B = 65 runs the VL = 2 kernels (one tile of 65 in 128 lanes' worth) and B = 200 VL = 4."""
    from hispmv_amd import prep
    from hispmv_amd.torch_ops import sparse_linear
    torch = torch_mod
    m = S.case_a()[6]
    rng = np.random.default_rng(11)
    X = rng.random((B, m["cols"]), dtype=np.float32) - np.float32(0.3)
    G = rng.random((B, m["rows"]), dtype=np.float32) - np.float32(0.5)
    X[1] = 0.0
    with Pair(torch_mod, m) as cx:
        h, P = cx.h, cx.idx[0]
        ld = (B + 3) & ~3
        assert h.spmm_info(P, B, ld)["vl"] == prep.spmm_tiles(m["cols"], B, ld, 16)["vl"] == (2 if B == 65 else 4)
        bias = cx.device(m["b"]).requires_grad_(True)
        g = cx.device(G)
        # fp64 truths: forward per vector, grad_x = A^T g per vector, grad_bias = sum of g
        t = m["v"].astype(np.float64)
        y64 = np.stack([np.bincount(m["r"], weights=t * X[v].astype(np.float64)[m["c"]], minlength=m["rows"]) for v in range(B)]) + m["b"].astype(np.float64)
        ymag = np.stack([np.bincount(m["r"], weights=np.abs(t * X[v].astype(np.float64)[m["c"]]), minlength=m["rows"]) for v in range(B)]) + np.abs(m["b"].astype(np.float64))
        gx64 = np.stack([np.bincount(m["c"], weights=t * G[v].astype(np.float64)[m["r"]], minlength=m["cols"]) for v in range(B)])
        gxmag = np.stack([np.bincount(m["c"], weights=np.abs(t * G[v].astype(np.float64)[m["r"]]), minlength=m["cols"]) for v in range(B)])

        def passes(spmm):
            x = cx.device(X).requires_grad_(True)
            bias.grad = None
            y = sparse_linear(h, P, x, bias, spmm=spmm)
            y.backward(g)
            torch.cuda.synchronize()
            h.synchronize()
            return y.detach().cpu().numpy(), x.grad.cpu().numpy(), bias.grad.cpu().numpy()

        for scope in ("default stream", "own stream"):
            stream = torch.cuda.Stream() if scope == "own stream" else None
            with torch.cuda.stream(stream):
                y0, gx0, gb0 = passes(False)
                y1, gx1, gb1 = passes(True)
                y2, gx2, gb2 = passes(True)
            assert y1.shape == (B, m["rows"]) and gx1.shape == (B, m["cols"])
            assert np.isfinite(y1).all() and np.isfinite(gx1).all() and np.isfinite(gb1).all(), scope
            assert (np.abs(y1.astype(np.float64) - y0) <= TOL * ymag).all(), scope                      # forward close to spmm=False within TOL * mag
            assert max(bwd_err(y1[v], y64[v], ymag[v]) for v in range(B)) < TOL, scope
            assert max(bwd_err(gx1[v], gx64[v], gxmag[v]) for v in range(B)) < TOL, scope
            assert bwd_err(gb1, G.astype(np.float64).sum(0), np.abs(G.astype(np.float64)).sum(0)) < TOL, scope
            assert np.array_equal(bits(y1), bits(y2)) and np.array_equal(bits(gx1), bits(gx2)) and np.array_equal(bits(gb1), bits(gb2)), scope
            assert (y1[1] == m["b"]).all(), scope                                                      # the zero vector: exactly the bias
            # spmm=False is what it was: the bits of linear_device
            dx, dy = cx.device(X), cx.device(np.full((B, m["rows"]), np.nan, np.float32))
            torch.cuda.synchronize()
            h.linear_device(P, dx.data_ptr(), B, bias.data_ptr(), dy.data_ptr(), 1.0, 1.0)
            h.synchronize()
            assert np.array_equal(bits(y0), bits(dy.cpu().numpy())), scope

        # a handle without a companion: forward through spmm_device, grad_x falls back to linear_device_t (atomics: gated, not compared)
        R = cx.idx[1]
        xr = cx.device(G).requires_grad_(True)                      # R is the swapped matrix: [B, rows of m] -> [B, cols of m]
        yr = sparse_linear(h, R, xr, None, spmm=True)
        yr.backward(cx.device(X))
        torch.cuda.synchronize()
        h.synchronize()
        assert max(bwd_err(yr.detach().cpu().numpy()[v], gx64[v], gxmag[v]) for v in range(B)) < TOL
        assert max(bwd_err(xr.grad.cpu().numpy()[v], y64[v] - m["b"].astype(np.float64), ymag[v] - np.abs(m["b"].astype(np.float64))) for v in range(B)) < TOL


def test_sparse_linear_spmm_with_values(torch_mod):
    """values=: the update pass and value_grad_device stay as they are; grad_values equals the spmm=False route bit for bit."""
    from hispmv_amd.torch_ops import sparse_linear
    torch = torch_mod
    m = S.case_a()[6]
    rng = np.random.default_rng(12)
    X = rng.random((B, m["cols"]), dtype=np.float32) - np.float32(0.3)
    G = rng.random((B, m["rows"]), dtype=np.float32) - np.float32(0.5)
    with Pair(torch_mod, m, updates=True) as cx:
        h, P = cx.h, cx.idx[0]
        out = {}
        with torch.cuda.stream(torch.cuda.Stream()):
            for spmm in (False, True):
                x = cx.device(X).requires_grad_(True)
                v = cx.device(m["v"] * np.float32(2.0)).requires_grad_(True)
                y = sparse_linear(h, P, x, None, values=v, spmm=spmm)
                y.backward(cx.device(G))
                torch.cuda.synchronize()
                out[spmm] = (y.detach().cpu().numpy(), x.grad.cpu().numpy(), v.grad.cpu().numpy())
        assert np.array_equal(bits(out[False][2]), bits(out[True][2]))
        t = 2.0 * m["v"].astype(np.float64)
        for v in (0, 1, B - 1):
            y64 = np.bincount(m["r"], weights=t * X[v].astype(np.float64)[m["c"]], minlength=m["rows"])
            mag = np.bincount(m["r"], weights=np.abs(t * X[v].astype(np.float64)[m["c"]]), minlength=m["rows"])
            assert bwd_err(out[True][0][v], y64, mag) < TOL
            gx64 = np.bincount(m["c"], weights=t * G[v].astype(np.float64)[m["r"]], minlength=m["cols"])
            gmag = np.bincount(m["c"], weights=np.abs(t * G[v].astype(np.float64)[m["r"]]), minlength=m["cols"])
            assert bwd_err(out[True][1][v], gx64, gmag) < TOL
