"""The block-Jacobi preconditioner without a device: the layout rule on both sides of the ABI, the entries' refusal without a context,
and the numpy model of tests/block_jacobi_model.py itself -- is its inversion an inversion, does it flag what it must, and does the
preconditioner buy the iterations the case table records?"""
import ctypes as C

import numpy as np
import pytest

import block_jacobi_model as bj
import krylov_model as km
from hispmv_amd import _lib, prep

f32 = np.float32


@pytest.mark.parametrize("bs", bj.SIZES)
@pytest.mark.parametrize("n", (1, 3, 4, 5, 1023, 1024, 1025, 4099))
def test_layout_rule_is_the_same_on_both_sides_of_the_abi(n, bs):
    got = prep.block_jacobi(n, bs)
    assert got == bj.layout(n, bs)
    assert got["n_blocks"] == -(-n // bs) and got["block_floats"] == bs * bs
    assert got["flags_offset"] % 16 == 0 and got["pre_bytes"] % 16 == 0
    assert got["flags_offset"] >= got["n_blocks"] * bs * bs * 4 and got["pre_bytes"] >= got["flags_offset"] + 4 * got["n_blocks"]


def test_layout_rule_refuses_bad_arguments():
    for n, bs in ((-1, 8), (10, 5), (10, 0), (10, 64), (1 << 31, 4)):
        with pytest.raises(ValueError):
            prep.block_jacobi(n, bs)
    assert prep.block_jacobi(0, 8)["n_blocks"] == 0


def test_every_device_entry_returns_einval_without_a_context():
    lib = _lib.lib
    out = (C.c_int64 * 8)()
    res = _lib.KrylovResult()
    assert lib.hispmv_block_jacobi_info(None, 0, 8, out) == _lib.HISPMV_EINVAL
    assert lib.hispmv_block_jacobi_extract_device(None, 0, 8, None, 0, None) == _lib.HISPMV_EINVAL
    assert lib.hispmv_block_invert_device(None, None, 1, 8, None) == _lib.HISPMV_EINVAL
    assert lib.hispmv_block_jacobi_setup_device(None, 0, 8, None, 0, None) == _lib.HISPMV_EINVAL
    assert lib.hispmv_block_jacobi_status(None, None, 8, 8, None, out) == _lib.HISPMV_EINVAL
    assert lib.hispmv_block_jacobi_apply_device(None, None, 8, 8, None, None, None) == _lib.HISPMV_EINVAL
    assert lib.hispmv_cg_bj_device(None, 0, None, None, None, 8, 1e-6, 10, 1, None, 0, None, C.byref(res)) == _lib.HISPMV_EINVAL
    assert lib.hispmv_gmres_bj_device(None, 0, None, None, None, 8, 10, 1e-6, 10, 1, None, 0, None, C.byref(res)) == _lib.HISPMV_EINVAL


@pytest.mark.parametrize("bs", bj.SIZES)
def test_model_inverse_against_fp64(bs):
    """Gauss-Jordan with partial pivoting in float32 on well-conditioned blocks (a random matrix of unit-variance rows plus 2 I, no
    growth to speak of): the error of the computed inverse is a small multiple of bs * cond * u, u = 2^-24 -- the bound of an
    inverse computed through LU with partial pivoting (Higham, Accuracy and Stability, 14.3) with the constant taken as 8."""
    rng = np.random.default_rng(bs)
    blocks = (rng.standard_normal((20, bs, bs)) / np.sqrt(bs) + 2 * np.eye(bs)).astype(f32)
    inv, flags = bj.invert(blocks)
    assert not flags.any()
    for b, x in zip(blocks, inv):
        b64 = b.astype(np.float64)
        ref = np.linalg.inv(b64)
        cond = np.linalg.cond(b64)
        err = np.linalg.norm(x.astype(np.float64) - ref, 2) / np.linalg.norm(ref, 2)
        assert cond < 100
        assert err <= 8 * bs * cond * 2.0 ** -24, (bs, err, cond)


@pytest.mark.parametrize("bs", bj.SIZES)
def test_model_flags_and_exact_cases(bs):
    rng = np.random.default_rng(100 + bs)
    eye = np.eye(bs, dtype=f32)
    for kind in bj.BAD_KINDS:          # a zero block, two equal rows, a NaN, an Inf: the identity, flagged
        x, flag = bj.invert_block(bj.block_of(kind, bs, rng))
        assert flag == 1 and np.array_equal(x, eye), kind
    for kind in ("dominant", "pivoting", "tie"):
        blk = bj.block_of(kind, bs, rng)
        x, flag = bj.invert_block(blk)
        assert flag == 0 and np.isfinite(x).all(), kind
        assert np.abs(x.astype(np.float64) @ blk.astype(np.float64) - eye).max() < 1e-3, kind
    good = bj.block_of("dominant", bs, rng)
    perm = bj.block_of("permutation", bs, rng)
    x, flag = bj.invert_block(perm)
    assert flag == 0 and np.array_equal(x, perm.T)
    # padding: the inverse of a padded block is the inverse of its present part, padded the same way
    part = good[:bs - 1, :bs - 1]
    padded = eye.copy()
    padded[:bs - 1, :bs - 1] = part
    x, flag = bj.invert_block(padded)
    assert flag == 0 and np.array_equal(x[bs - 1], eye[bs - 1]) and np.array_equal(x[:, bs - 1], eye[:, bs - 1])


def test_model_extraction_pads_and_sums():
    import scipy.sparse as sp
    A = km.tridiag(5)
    blocks = bj.extract(A, 4)
    assert blocks.shape == (2, 4, 4)
    assert np.array_equal(blocks[0], A.toarray()[:4, :4])
    want = np.eye(4, dtype=f32)
    want[0, 0] = 2.5
    assert np.array_equal(blocks[1], want)
    twice = sp.coo_matrix((np.concatenate([A.data, A.data]), (np.concatenate([A.row, A.row]), np.concatenate([A.col, A.col]))), shape=A.shape)
    assert np.array_equal(bj.extract(twice, 4)[0], 2 * A.toarray()[:4, :4])


def test_model_multiply_is_the_inverse_times_r():
    rng = np.random.default_rng(3)
    for bs in bj.SIZES:
        for n in (1, bs - 1, bs, bs + 1, 5 * bs + 3):
            nb = -(-n // bs)
            inv = rng.standard_normal((nb, bs, bs)).astype(f32)
            r = rng.standard_normal(n).astype(f32)
            z = bj.BlockInverse(inv, n) * r
            assert z.dtype == f32 and z.shape == (n,)
            rp = np.zeros(nb * bs)
            rp[:n] = r
            ref = np.einsum("kij,kj->ki", inv.astype(np.float64), rp.reshape(nb, bs)).reshape(-1)[:n]
            mag = np.einsum("kij,kj->ki", np.abs(inv).astype(np.float64), np.abs(rp).reshape(nb, bs)).reshape(-1)[:n]
            assert (np.abs(z - ref) <= bs * 2.0 ** -24 * mag + 1e-30).all()


@pytest.mark.parametrize("name", sorted(bj.CASES))
def test_iteration_counts(name):
    """The model with scipy products: the block solve converges in at most `ratio` of the iterations of the minv solve, and both
    counts and the attained true residual are the ones the table records."""
    case = bj.CASES[name]
    A = case["make"]()
    xm, im, _, b = bj.run_model(case, "minv", A=A)
    xb, ib, _, _ = bj.run_model(case, "blocks", A=A)
    res = km.true_relres(A, xb, b)
    print(f"{name}: minv {im}, blocks {ib}, true relative residual {res:.3e}, recorded {case['attained']:.3e}")
    assert im["status"] == "CONVERGED" and ib["status"] == "CONVERGED"
    assert ib["iterations"] <= case["ratio"] * im["iterations"], (ib, im)
    assert (im["iterations"], ib["iterations"]) == (case["minv_iterations"], case["iterations"])
    assert res <= 1.05 * case["attained"]


def test_zero_block_system_is_what_it_says():
    A = bj.zero_block_system()
    dense = A.toarray()
    assert not (dense[8:16, 8:16] != 0).any() and not np.array_equal(dense, dense.T)
    assert np.linalg.cond(dense.astype(np.float64)) < 100
    m = bj.setup(A, 8)
    assert m.flags.tolist() == [0, 1, 0, 0, 0, 0, 0, 0]
