"""The wide-batch value gradient with bf16 activations without a device: the order model of tests/spmm_grad_bf16_cases.py against a
float64 brute force and a closed form, the two C entries' refusals that need no context, the methods' signatures, and the argument
checks of sparse_linear(..., wide_grad="bf16"), which come before any device use.

THE BOUND of the model against float64.  Write u = 2^-24.  A product of the model is rounded once; it then passes through at most VB
sequential adds, 6 adds of the lane tree, the multiplication by alpha and the add of beta * grad (grad0 itself through the
multiplication by beta and that add), and for every later tile the add that accumulates it: k = 1 + VB + 6 + 2 + (tiles - 1) roundings
at most, so |model - g64| <= gamma_k * (|alpha| sum |gy x| + |beta grad0|) with gamma_k = k u / (1 - k u) (Higham, Accuracy and
Stability of Numerical Algorithms, lemma 3.1).  The operands are random float32 in [-0.5, 0.5): no overflow, and the test asserts that
no product is subnormal."""
import ctypes as C
import inspect

import numpy as np
import pytest

import spmm_grad_bf16_cases as M


def gamma(k):
    u = 2.0 ** -24
    return k * u / (1 - k * u)


@pytest.mark.parametrize("B, tiles", [(1, [(0, 1, 1)]), (65, [(0, 65, 2)]), (130, [(0, 130, 4)]), (257, [(0, 256, 4), (256, 1, 1)]),
                                      (258, [(0, 258, 8)]), (513, [(0, 512, 8), (512, 1, 1)]), (65, [(0, 64, 1), (64, 1, 1)])])
def test_model_against_float64(B, tiles):
    rng = np.random.default_rng(B)
    n = 300
    gy = rng.random((n, B), dtype=np.float32) - np.float32(0.5)
    x = rng.random((n, B), dtype=np.float32) - np.float32(0.5)
    g0 = rng.random(n, dtype=np.float32) - np.float32(0.5)
    prod = gy.astype(np.float64) * x.astype(np.float64)
    assert (np.abs(prod[prod != 0]) > 2.0 ** -126).all()
    for alpha, beta in ((1.0, 0.0), (0.85, -2.06)):
        got = M.model(gy, x, tiles, alpha, beta, g0 if beta else None)
        a32, b32 = float(np.float32(alpha)), float(np.float32(beta))
        g64 = a32 * prod.sum(1) + b32 * g0.astype(np.float64)
        mag = abs(a32) * np.abs(prod).sum(1) + np.abs(b32 * g0.astype(np.float64))
        k = 1 + max(t[2] for t in tiles) + 6 + 2 + (len(tiles) - 1)
        err = np.abs(got.astype(np.float64) - g64)
        print(f"B={B} tiles={len(tiles)} worst err / (gamma_{k} mag) = {float((err / (gamma(k) * mag)).max()):.3f}")
        assert got.dtype == np.float32 and (err <= gamma(k) * mag).all()


def test_model_closed_form_of_64_equal_products():
    """VB = 1, 64 vectors with the same product p: every level of the tree doubles exactly, so the sum is 64 * fl(p)."""
    gy = np.full((3, 64), np.float32(0.1))
    x = np.full((3, 64), np.float32(0.3))
    p = np.float32(0.1) * np.float32(0.3)
    got = M.model(gy, x, [(0, 64, 1)], 1.0, 0.0)
    assert got.view(np.uint32).tolist() == [np.float32(64 * p).view(np.uint32)] * 3
    # one vector fewer: lane 63 adds +0, and the tree is 32 p + (16 p + (8 p + (4 p + (2 p + (p + 0))))), every power-of-two multiple exact
    got = M.model(gy[:, :63], x[:, :63], [(0, 63, 1)], 1.0, 0.0)
    two = np.float32(2.0)
    tree = two ** 5 * p + (two ** 4 * p + (two ** 3 * p + (two ** 2 * p + (two * p + p))))
    assert tree.dtype == np.float32 and got.view(np.uint32).tolist() == [tree.view(np.uint32)] * 3


def test_model_masks_products_past_the_batch_and_orders_a_lane_ascending():
    """A lane of VB 4 with 2 live vectors: the pad products are +0 whatever the operands hold; and (a + b) + c differs from a + (b + c)
    for a = 1, b = 2^-24, c = 2^-24 in float32, which pins the ascending order inside a lane."""
    gy = np.array([[1.0, 2.0 ** -24, 2.0 ** -24]], np.float32)
    x = np.ones((1, 3), np.float32)
    up = M.model(gy, x, [(0, 3, 4)], 1.0, 0.0)
    down = M.model(gy[:, ::-1].copy(), x, [(0, 3, 4)], 1.0, 0.0)
    assert up[0] == np.float32(1.0) and down[0] == np.float32(1.0) + np.float32(2.0 ** -23)
    bits = M.to_bf16_bits(np.array([1.0, -2.5, np.inf, np.nan], np.float32))
    assert bits[:3].tolist() == [0x3F80, 0xC020, 0x7F80] and (bits[3] & 0x7FC0) == 0x7FC0
    assert M.widen(bits[:2]).tolist() == [1.0, -2.5]


def test_tile_list_follows_the_host_rule():
    from hispmv_amd import prep
    assert M.tile_list(prep.spmm_bf16_tiles(4000, 513, 520, 16)) == [(0, 512, 8), (512, 1, 1)]
    assert M.tile_list(prep.spmm_bf16_tiles(4000, 257, 260, 16)) == [(0, 256, 4), (256, 1, 1)]
    assert M.tile_list(prep.spmm_bf16_tiles(4000, 65, 72, 2)) == [(0, 64, 1), (64, 1, 1)]
    assert M.tile_list(prep.spmm_bf16_tiles(4000, 65, 72, 4)) == [(0, 65, 2)]
    # B = 65, 130, 257 at ld = 68, 132, 260: the bf16 rule and the fp32 rule give the same lane width and tiles up to 8192 columns
    for B, ld in ((65, 68), (130, 132), (257, 260)):
        for cols in (1, 4000, 8192):
            assert M.tile_list(prep.spmm_bf16_tiles(cols, B, ld, 16)) == M.tile_list(prep.spmm_tiles(cols, B, ld, 16), key="vl"), (B, ld, cols)


def test_null_context_is_refused():
    from hispmv_amd import _lib
    lib = _lib.lib
    out = (C.c_int64 * 4)()
    assert lib.hispmv_spmm_value_grad_device_bf16(None, 0, None, 1, None, 1, 1, None, 1.0, 0.0, None) == _lib.HISPMV_EINVAL
    assert lib.hispmv_spmm_value_grad_bf16_info(None, 0, 1, 1, out) == _lib.HISPMV_EINVAL


def test_info_refuses_a_leading_dimension_below_the_batch():
    """(a context needs a device: the same check on a real context is in tests/test_gpu_spmm_value_grad_bf16.py)"""
    from hispmv_amd import _lib
    out = (C.c_int64 * 4)(7, 7, 7, 7)
    assert _lib.lib.hispmv_spmm_value_grad_bf16_info(None, 0, 8, 7, out) == _lib.HISPMV_EINVAL
    assert _lib.lib.hispmv_spmm_value_grad_bf16_info(None, 0, 8, 8, None) == _lib.HISPMV_EINVAL
    assert list(out) == [7, 7, 7, 7]
    assert _lib.SIGNATURES["hispmv_spmm_value_grad_device_bf16"] == _lib.SIGNATURES["hispmv_spmm_value_grad_device"]
    assert _lib.SIGNATURES["hispmv_spmm_value_grad_bf16_info"] == _lib.SIGNATURES["hispmv_spmm_value_grad_info"]


def test_methods_and_defaults():
    from hispmv_amd.fpga_handle import FpgaHandle
    p = inspect.signature(FpgaHandle.spmm_value_grad_device_bf16).parameters
    assert list(p) == ["self", "matrix_idx", "d_gyt", "d_xt", "num_vecs", "d_grad", "alpha", "beta", "ld_gy", "ld_x", "stream"]
    assert (p["alpha"].default, p["beta"].default, p["ld_gy"].default, p["ld_x"].default, p["stream"].default) == (1.0, 0.0, None, None, 0)
    assert list(p) == list(inspect.signature(FpgaHandle.spmm_value_grad_device).parameters)
    q = inspect.signature(FpgaHandle.spmm_value_grad_bf16_info).parameters
    assert list(q) == ["self", "matrix_idx", "num_vecs", "ld"] and q["ld"].default is None


def test_wide_grad_keeps_its_default_and_checks_its_state_before_any_device_use():
    """The handle is None: a check that touched it would raise AttributeError, not ValueError."""
    import torch
    from hispmv_amd.torch_ops import sparse_linear
    p = inspect.signature(sparse_linear).parameters
    assert p["wide_grad"].default is False and list(p)[-2:] == ["spmm", "wide_grad"]
    x32, x16, v = torch.zeros(2, 4), torch.zeros(2, 4, dtype=torch.bfloat16), torch.zeros(3)
    with pytest.raises(ValueError, match="bfloat16"):
        sparse_linear(None, 0, x32, None, values=v, spmm=True, wide_grad="bf16")
    with pytest.raises(ValueError, match="spmm=True"):
        sparse_linear(None, 0, x16, None, values=v, wide_grad="bf16")
    with pytest.raises(ValueError, match="values"):
        sparse_linear(None, 0, x16, None, spmm=True, wide_grad="bf16")
    for state in ("fp16", "BF16", 2, None, 1.0):
        with pytest.raises(ValueError, match="False, True"):
            sparse_linear(None, 0, x16, None, values=v, spmm=True, wide_grad=state)
