"""The transposed wide-batch product with bf16 activations (hispmv_spmm_device_t_bf16) and sparse_linear(..., spmm=True) on a bfloat16 x.

Handles are created under set_transposable("companion") (Pair of tests/test_gpu_spmm_companion.py) on a rectangular windowed matrix
(256 threads, compact) and on big_band (1024 threads).  spmm_device_t_bf16 must equal bf16(spmm_device_t on the widened operands) bit for
bit, for B = 65 (VB 2) and B = 513 (VB 8 and a second tile of one vector; VB 2 on big_band, whose 20 000 columns cap the lanes), with a
shared fp32 bias and without one.

sparse_linear(spmm=True) with a bf16 x: y is bf16 and torch.equal to sparse_linear(x.float(), spmm=True).to(bfloat16); x.grad is bf16 and
equals the fp32 route's grad_x on the widened bf16 grad_y, rounded; bias.grad equals grad_y.float().sum(0); with `values` on an updatable
handle (fp32 storage, and bf16 storage under "any_storage") values.grad equals bit for bit what the fp32-activation call returns for
the widened inputs, with and without wide_grad; on a handle without a companion grad_x is the narrowed linear_device_t result (float
atomics: compared within TOL of the fp32 route's magnitudes, not bit for bit); a bf16 x with spmm=False raises TypeError."""
import numpy as np
import pytest

import step_small_cases as S
from conftest import TOL
from test_gpu_spmm import Wide, batch
from test_gpu_spmm_bf16 import WideBf16, to_bf16, widen
from test_gpu_spmm_companion import Pair
from test_gpu_transpose import Ctx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def rectangular():
    """the windowed uniform matrix of case A: 3000 x 2500, 256 threads, compact"""
    return S.case_a()[6]


@pytest.mark.parametrize("make", [rectangular, S.big_band], ids=["windowed_uniform", "big_band"])
def test_transposed_product_equals_the_rounded_fp32_entry(torch_mod, make):
    from hispmv_amd import prep
    m = make()
    with Pair(torch_mod, m) as cx:
        ci = cx.h.companion_info(cx.idx[0])
        assert ci["has"] and ci["format"] == 0, ci
        o, w = Wide(cx, 0, t=True), WideBf16(cx, 0, t=True)
        pool = widen(to_bf16(torch_mod, o.pool))
        bias = np.resize(m["b"], m["cols"]).astype(np.float32)
        for B in (65, 513):
            info = cx.h.spmm_bf16_info(cx.idx[0], B, (B + 7) & ~7)
            assert info["accepted"] and info["accepted_t"] and info["work_bytes_t"] > 0, info
            assert info["vb"] == prep.spmm_bf16_tiles(m["cols"], B, (B + 7) & ~7)["vb"] == (2 if B == 65 or m["cols"] > 16384 else 8), info
            assert not cx.h.spmm_bf16_info(cx.idx[1], B, (B + 7) & ~7)["accepted_t"]
            X = batch(pool, B)
            X16 = to_bf16(torch_mod, X)
            for alpha, beta in S.PAIRS:
                kind = "given" if beta != 0.0 else "null"
                ref = o.call(X, bias, alpha, beta, bias=kind)
                assert np.isfinite(ref).all() and np.abs(ref).max() > 0
                Y = w.call(X16, bias, alpha, beta, bias=kind)
                assert np.array_equal(Y, to_bf16(torch_mod, ref)), (m["name"], B, alpha, beta)
        d = torch_mod.zeros(4 * (m["rows"] + m["cols"]) + (1 << 20), dtype=torch_mod.float32, device="cuda")
        with pytest.raises(NotImplementedError, match="companion"):            # R has no stored transpose
            cx.h.spmm_device_t_bf16(cx.idx[1], d.data_ptr(), 4, 0, d.data_ptr() + 16 * m["cols"], work=d.data_ptr() + 16 * (m["rows"] + m["cols"]), work_bytes=4 << 20)


@pytest.mark.parametrize("B", [65, 300])
def test_sparse_linear_with_bf16_activations(torch_mod, B):
    """On torch's default stream and inside a stream of its own.  B = 65: ld 72, VB 2; B = 300: ld 304, VB 8."""
    from hispmv_amd.torch_ops import sparse_linear
    torch = torch_mod
    m = rectangular()
    rng = np.random.default_rng(21)
    X = rng.random((B, m["cols"]), dtype=np.float32) - np.float32(0.3)
    G = rng.random((B, m["rows"]), dtype=np.float32) - np.float32(0.5)
    X[1] = 0.0
    with Pair(torch_mod, m) as cx:
        h, P, R = cx.h, cx.idx[0], cx.idx[1]
        assert h.spmm_bf16_info(P, B, (B + 7) & ~7)["vb"] == (2 if B == 65 else 8)
        x16 = cx.device(X).to(torch.bfloat16)
        g16 = cx.device(G).to(torch.bfloat16)
        bias = cx.device(m["b"]).requires_grad_(True)

        def passes(x0, g0):
            x = x0.clone().requires_grad_(True)
            bias.grad = None
            y = sparse_linear(h, P, x, bias, spmm=True)
            y.backward(g0)
            torch.cuda.synchronize()
            h.synchronize()
            return y.detach(), x.grad, bias.grad.clone()

        for scope in ("default stream", "own stream"):
            stream = torch.cuda.Stream() if scope == "own stream" else None
            with torch.cuda.stream(stream):
                y32, gx32, gb32 = passes(x16.float(), g16.float())
                y, gx, gb = passes(x16, g16)
                torch.cuda.synchronize()
            assert y.dtype == torch.bfloat16 and y.shape == (B, m["rows"]) and gx.dtype == torch.bfloat16 and gx.shape == (B, m["cols"]), scope
            assert torch.equal(y, y32.to(torch.bfloat16)), scope
            assert torch.equal(gx, gx32.to(torch.bfloat16)), scope
            assert gb.dtype == torch.float32 and torch.equal(gb, g16.float().sum(0)) and torch.equal(gb, gb32), scope
            assert torch.equal(y[1].float(), bias.detach().to(torch.bfloat16).float()), scope          # the zero vector: exactly bf16(bias)

        # a handle without a companion: grad_x is linear_device_t on the widened grad_y, narrowed by torch
        xr = g16.clone().requires_grad_(True)                       # R is the swapped matrix: [B, rows of m] -> [B, cols of m]
        yr = sparse_linear(h, R, xr, None, spmm=True)
        yr.backward(x16)
        xf = g16.float().requires_grad_(True)
        yf = sparse_linear(h, R, xf, None, spmm=True)
        yf.backward(x16.float())
        torch.cuda.synchronize()
        h.synchronize()
        assert yr.dtype == torch.bfloat16 and torch.equal(yr.detach(), yf.detach().to(torch.bfloat16))
        assert xr.grad.dtype == torch.bfloat16 and torch.isfinite(xr.grad).all()
        # two sums of the same fp32 products in two orders (float atomics), each rounded to bf16 (2^-8 relative)
        mag = np.stack([np.bincount(m["r"], weights=np.abs(m["v"].astype(np.float64) * x16[v].float().cpu().numpy().astype(np.float64)[m["c"]]),
                                    minlength=m["rows"]) for v in (0, 1, B - 1)])
        diff = (xr.grad.float() - xf.grad).abs().cpu().numpy()[[0, 1, B - 1]]
        assert (diff <= 2 * TOL * mag + 2.0 ** -8 * np.abs(xf.grad.cpu().numpy()[[0, 1, B - 1]])).all()

        for bad in (x16, x16[0]):
            with pytest.raises(TypeError, match="float32"):
                sparse_linear(h, P, bad, bias, spmm=False)
        with pytest.raises(TypeError):
            sparse_linear(h, P, x16.double(), bias, spmm=True)


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
def test_value_gradient_keeps_the_bits_of_the_fp32_route(torch_mod, storage):
    """values= on an updatable handle: y, grad_x as above; values.grad bit for bit that of the fp32-activation call on the widened
    inputs, through value_grad_device (wide_grad=False) and through spmm_value_grad_device (wide_grad=True)."""
    from hispmv_amd.torch_ops import sparse_linear
    torch = torch_mod
    m = rectangular()
    if storage == "bf16":
        m = S.as_bf16(m)
    B = 65
    rng = np.random.default_rng(22)
    X = rng.random((B, m["cols"]), dtype=np.float32) - np.float32(0.3)
    G = rng.random((B, m["rows"]), dtype=np.float32) - np.float32(0.5)
    with Ctx(torch_mod, S.SLICES, [m], transposable="companion", updates="any_storage" if storage == "bf16" else True) as cx:
        h, P = cx.h, cx.idx[0]
        assert h.companion_info(P)["has"] and h.spmm_bf16_info(P, B, 72)["accepted_t"]
        assert h.value_storage_info(P)["storage"] == storage
        x16, g16 = cx.device(X).to(torch.bfloat16), cx.device(G).to(torch.bfloat16)
        with torch.cuda.stream(torch.cuda.Stream()):
            for wide in (False, True):
                out = {}
                for half in (False, True):
                    x = (x16 if half else x16.float()).clone().requires_grad_(True)
                    v = cx.device(m["v"] * np.float32(2.0)).requires_grad_(True)
                    y = sparse_linear(h, P, x, None, values=v, spmm=True, wide_grad=wide)
                    y.backward(g16 if half else g16.float())
                    torch.cuda.synchronize()
                    out[half] = (y.detach(), x.grad, v.grad)
                assert out[True][2].dtype == torch.float32 and torch.isfinite(out[True][2]).all() and out[True][2].abs().max() > 0
                assert torch.equal(out[True][2], out[False][2]), (storage, wide)
                assert out[True][0].dtype == torch.bfloat16 and torch.equal(out[True][0], out[False][0].to(torch.bfloat16)), (storage, wide)
                assert out[True][1].dtype == torch.bfloat16 and torch.equal(out[True][1], out[False][1].to(torch.bfloat16)), (storage, wide)
