"""The value gradient on updatable bf16 handles (hispmv_value_grad_device, HALF decode of the slice kernel) on the MI355X.

The gradient does not read the values, and plan, pass widths and map of a bf16 handle are those of the fp32 handle of the same input:
grad of the bf16 handle equals grad of the fp32 updatable handle BIT FOR BIT, for 1, 3 and 7 vectors (passes of 4, 2 and 1), with
alpha = 0.5, beta = 0.25 on a pre-filled grad and with beta = 0 on a NaN-filled one.  gy and x hold small integers, so every product
and sum is exact in fp32 and both must also equal the numpy reference exactly.  Then one forward and backward pass of
torch_ops.sparse_linear(..., values=v) with v as the fp32 master copy."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HW = ("tests.xclbin", 0, 24, 1, 1, 2, 5, True, False, True)
TOL = 1e-5          # the gate tests/test_gpu_linear_device.py puts on the atomic (transposed) path, as a backward error
NVS = (1, 3, 7)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def R(v):
    import torch
    return torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def make_handle(storage="fp32", updates=False, transposable=False):
    import pyhispmv
    h = pyhispmv.FpgaHandle(*HW)
    h.set_arena_bytes(64 << 30)
    h.set_value_storage(storage)
    h.set_value_updates(updates)
    h.set_transposable(transposable)
    return h


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def _band(rows, per_row, half, seed=3):
    rng = np.random.default_rng(seed)
    r = np.repeat(np.arange(rows, dtype=np.int64), per_row)
    c = np.clip(r + rng.integers(-half, half + 1, size=r.size), 0, rows - 1)
    return r.astype(np.int32), c.astype(np.int32)


def _strays(share, rows=300000):
    r, c = _band(rows, 16, 1500)
    far = np.random.default_rng(5).random(c.size) < share
    return r, np.where(far, np.random.default_rng(6).integers(0, rows, c.size), c).astype(np.int32)


def _shuffled_with_duplicates(r, c, seed=1):
    rng = np.random.default_rng(seed)
    dup = rng.integers(0, r.size, r.size // 50)
    r, c = np.concatenate([r, r[dup]]), np.concatenate([c, c[dup]])
    p = rng.permutation(r.size)
    return r[p], c[p]


# name -> (env, transposable state, matrix, check on matrix_info, half groups expected): the builders of tests/test_gpu_value_storage.py
CASES = {
    "slices_compact": ({}, False, lambda: _band(200000, 12, 400), lambda i: i["format"] == 0 and i["col_tiles"] == 1 and i["compact_slices"] > 0, True),
    "stray_slots": ({}, False, lambda: _strays(0.03), lambda i: i["tile_kind"] == 0 and i["compact_slices"] == i["n_slices"], True),
    "stray_split": ({"HISPMV_STRAY_SLOTS": "0"}, False, lambda: _strays(0.03), lambda i: i["tile_kind"] == 3, True),
    "column_tiles": ({"HISPMV_FORMAT": "slices", "HISPMV_BAND_TILES": "0", "HISPMV_COL_TILE_BYTES": "65536"}, False, lambda: _band(100000, 8, 45000),
                     lambda i: i["tile_kind"] == 1 and i["col_tiles"] >= 2, False),
    "plan_global": ({"HISPMV_FORMAT": "slices", "HISPMV_PLAN": "global"}, False, lambda: _band(200000, 12, 400), lambda i: i["format"] == 0, False),
    "tile_stream_keep_format": ({"HISPMV_FORMAT": "tts"}, "keep_format", lambda: _band(100000, 8, 45000), lambda i: i["format"] == 1, False),
}


def _grads(torch, h, idx, n, GY, X, prefill):
    """-> {(nv, variant): grad} for nv in NVS: alpha = 0.5, beta = 0.25 on `prefill`; alpha = 1, beta = 0 on NaN."""
    dev = torch.device("cuda", 0)
    dgy, dx = torch.from_numpy(GY).to(dev), torch.from_numpy(X).to(dev)
    out = {}
    for nv in NVS:
        for variant, (alpha, beta) in (("axpby", (0.5, 0.25)), ("overwrite", (1.0, 0.0))):
            g = torch.from_numpy(prefill).to(dev) if variant == "axpby" else torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            h.value_grad_device(idx, dgy.data_ptr(), dx.data_ptr(), nv, g.data_ptr(), alpha, beta)
            h.synchronize()
            out[(nv, variant)] = g.cpu().numpy()
    return out


def _check_against_fp32(torch, h, i_bf16, i_fp32, er, ec, rows, cols, what):
    """er, ec: row and column of every entry of the creation input, in its order."""
    n = er.size
    rng = np.random.default_rng(41)
    GY = rng.integers(-3, 4, (max(NVS), rows)).astype(np.float32)
    X = rng.integers(-3, 4, (max(NVS), cols)).astype(np.float32)
    prefill = rng.integers(-8, 9, n).astype(np.float32)
    for nv in NVS:
        assert h.value_grad_info(i_bf16, nv) == h.value_grad_info(i_fp32, nv) and h.value_grad_info(i_bf16, nv)["accepted"], (what, nv)
    got, want = _grads(torch, h, i_bf16, n, GY, X, prefill), _grads(torch, h, i_fp32, n, GY, X, prefill)
    for nv in NVS:
        s = np.zeros(n, np.float32)
        for v in range(nv):
            s += GY[v][er] * X[v][ec]                    # small integers: exact
        for variant, ref in (("axpby", np.float32(0.5) * s + np.float32(0.25) * prefill), ("overwrite", s)):
            g, w = got[(nv, variant)], want[(nv, variant)]
            assert np.all(np.isfinite(g)), (what, nv, variant)
            assert same_bits(g, w), f"{what}: grad of the bf16 handle differs from the fp32 handle's ({nv} vectors, {variant})"
            assert np.array_equal(g, ref), (what, nv, variant)


@pytest.mark.parametrize("case", sorted(CASES))
def test_grad_of_a_bf16_handle_has_the_bits_of_the_fp32_handle(torch_mod, monkeypatch, case):
    env, transposable, make, check, half = CASES[case]
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    r, c = _shuffled_with_duplicates(*make())
    rows = cols = int(max(r.max(), c.max())) + 1
    v = np.random.default_rng(17).random(r.size, dtype=np.float32) - np.float32(0.5)
    h = make_handle("fp32", "any_storage", transposable)
    try:
        f = h.create_sparse_handle(r, c, v, rows, cols)
        h.set_value_storage("bf16")
        a = h.create_sparse_handle(r, c, v, rows, cols)
        assert min(f, a) >= 0
        h.load_matrices()
        ia, i_f = h.matrix_info(a), h.matrix_info(f)
        assert check(ia), (case, ia)
        for k in ("format", "tile_kind", "col_tiles", "n_slices", "compact_slices", "block_threads", "group_slices", "lds_bytes"):
            assert ia[k] == i_f[k], (k, ia[k], i_f[k])
        assert (h.value_storage_info(a)["slots_2byte"] > 0) == (ia["compact_slices"] > 0) == half and h.value_storage_info(f)["slots_2byte"] == 0
        assert h.value_update_info(a) == h.value_update_info(f)
        print(case, ia, {nv: h.value_grad_info(a, nv) for nv in NVS})
        _check_against_fp32(torch_mod, h, a, f, r, c, rows, cols, case)
    finally:
        h.close()
    from hispmv_amd._lib import lib
    assert lib.hispmv_free_failures() == 0


def test_grad_of_a_dense_bf16_handle(torch_mod):
    rows, cols = 1000, 1003
    W = np.random.default_rng(5).random(rows * cols, dtype=np.float32) - np.float32(0.5)
    h = make_handle("fp32", "any_storage")
    try:
        f = h.create_dense_handle(W, rows, cols)
        h.set_value_storage("bf16")
        a = h.create_dense_handle(W, rows, cols)
        h.load_matrices()
        er, ec = np.divmod(np.arange(rows * cols), cols)
        _check_against_fp32(torch_mod, h, a, f, er, ec, rows, cols, "dense")
    finally:
        h.close()
    from hispmv_amd._lib import lib
    assert lib.hispmv_free_failures() == 0


def test_bf16_handle_with_updates_off_is_refused(torch_mod):
    torch = torch_mod
    r, c = _band(20000, 12, 400)
    v = np.random.default_rng(1).random(r.size, dtype=np.float32)
    h = make_handle("bf16", False)
    try:
        a = h.create_sparse_handle(r, c, v, 20000, 20000)
        d = h.create_dense_handle(v[:64 * 48], 64, 48)
        h.load_matrices()
        dev = torch.device("cuda", 0)
        gy, x, g = torch.ones(20000, device=dev), torch.ones(20000, device=dev), torch.zeros(r.size, device=dev)
        for idx in (a, d):
            assert not h.value_grad_info(idx, 1)["accepted"]
            with pytest.raises(AssertionError, match="value updates"):
                h.value_grad_device(idx, gy.data_ptr(), x.data_ptr(), 1, g.data_ptr())
    finally:
        h.close()


def test_sparse_linear_with_values_on_a_bf16_handle(torch_mod):
    """v is the fp32 master copy: y and grad_x come from R(v), v.grad is value_grad_device's result (straight-through)."""
    torch = torch_mod
    from hispmv_amd.torch_ops import sparse_linear
    r, c = _shuffled_with_duplicates(*_band(50000, 12, 400))
    rows = cols = 50000
    rng = np.random.default_rng(7)
    v0 = rng.random(r.size, dtype=np.float32) - np.float32(0.5)
    v1 = rng.random(r.size, dtype=np.float32) * np.float32(2.0) - np.float32(1.0)
    B = 3
    dev = torch.device("cuda", 0)
    xn = rng.random((B, cols), dtype=np.float32) - np.float32(0.5)
    wn = rng.random((B, rows), dtype=np.float32) - np.float32(0.5)
    bn = rng.random(rows, dtype=np.float32)
    hu, hp = make_handle("bf16", "any_storage", True), make_handle("bf16", False, True)
    try:
        u = hu.create_sparse_handle(r, c, v0, rows, cols)
        p = hp.create_sparse_handle(r, c, v1, rows, cols)
        hu.load_matrices()
        hp.load_matrices()
        assert hu.value_storage_info(u)["slots_2byte"] > 0
        x = torch.from_numpy(xn).to(dev).requires_grad_(True)
        v = torch.from_numpy(v1).to(dev).requires_grad_(True)
        bias, w = torch.from_numpy(bn).to(dev), torch.from_numpy(wn).to(dev)
        y = sparse_linear(hu, u, x, bias, values=v)
        (y * w).sum().backward()
        torch.cuda.synchronize()
        # forward: the fresh bf16 handle of v1
        y_ref = torch.full((B, rows), float("nan"), dtype=torch.float32, device=dev)
        gx_ref = torch.full((B, cols), float("nan"), dtype=torch.float32, device=dev)
        hp.linear_device(p, x.data_ptr(), B, bias.data_ptr(), y_ref.data_ptr(), 1.0, 1.0)
        hp.linear_device_t(p, w.data_ptr(), B, 0, gx_ref.data_ptr(), 1.0, 0.0)
        hp.synchronize()
        assert same_bits(y.detach().cpu().numpy(), y_ref.cpu().numpy())
        # v.grad: the entry's own result, which does not depend on the values
        g_ref = torch.full((r.size,), float("nan"), dtype=torch.float32, device=dev)
        hu.value_grad_device(u, w.data_ptr(), x.data_ptr(), B, g_ref.data_ptr(), 1.0, 0.0)
        hu.synchronize()
        assert tuple(v.grad.shape) == (r.size,) and np.all(np.isfinite(v.grad.cpu().numpy()))
        assert same_bits(v.grad.cpu().numpy(), g_ref.cpu().numpy())
        # grad_x = R(v1)^T w through float atomics: the backward-error gate of the transposed path, against the fresh handle
        rv = R(v1).astype(np.float64)
        gx, ref = x.grad.cpu().numpy(), gx_ref.cpu().numpy()
        for k in range(B):
            mag = np.zeros(cols, np.float64)
            np.add.at(mag, c, np.abs(rv) * np.abs(wn[k].astype(np.float64)[r]))
            t64 = np.zeros(cols, np.float64)
            np.add.at(t64, c, rv * wn[k].astype(np.float64)[r])
            mag = np.maximum(mag, np.finfo(np.float64).tiny)
            assert np.max(np.abs(ref[k] - t64) / mag) < TOL and np.max(np.abs(gx[k] - t64) / mag) < TOL
            assert np.max(np.abs(gx[k].astype(np.float64) - ref[k]) / mag) < TOL
    finally:
        hu.close()
        hp.close()
    from hispmv_amd._lib import lib
    assert lib.hispmv_free_failures() == 0
