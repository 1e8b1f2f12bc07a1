"""The Krylov layer's host side, no device: the rule of the dot product's partials on both sides of the ABI, the argument errors of
the new entries, and the numpy model of tests/krylov_model.py on the case tables with scipy products -- the check that the inputs of
the GPU tests are fair (every case converges well inside its iteration budget; an all-zero matrix is a breakdown that leaves x alone)."""
import ctypes as C
import math

import numpy as np
import pytest

import krylov_model as km


def test_groups_rule_on_both_sides_of_the_abi():
    from hispmv_amd import _lib, prep
    out = C.c_int64(-7)
    boundaries = [1024 * k + d for k in (1, 2, 1023, 1024, 1025, 4096) for d in (-1, 0, 1)] + [2 ** 31 - 1, 2 ** 31, 2 ** 40]
    for n in list(range(0, 5001)) + boundaries:
        assert _lib.lib.hispmv_prep_krylov_groups(n, C.byref(out)) == _lib.HISPMV_OK
        assert out.value == prep.krylov_groups(n) == km.groups(n) == min(-(-n // 1024), 1024), n
    assert prep.krylov_groups(0) == 0 and prep.krylov_groups(1) == 1 and prep.krylov_groups(1024 * 1024 + 1) == 1024
    assert _lib.lib.hispmv_prep_krylov_groups(-1, C.byref(out)) == _lib.HISPMV_EINVAL
    assert _lib.lib.hispmv_prep_krylov_groups(5, None) == _lib.HISPMV_EINVAL
    with pytest.raises(ValueError):
        prep.krylov_groups(-1)


def test_argument_errors_without_a_context():
    from hispmv_amd import _lib
    lib = _lib.lib
    res = _lib.KrylovResult()
    out = (C.c_int64 * 8)()
    assert lib.hispmv_krylov_info(None, 0, 0, out) == _lib.HISPMV_EINVAL
    assert lib.hispmv_dot_device(None, 4, None, None, None, None, 0, None) == _lib.HISPMV_EINVAL
    assert lib.hispmv_cg_device(None, 0, None, None, None, 1e-6, 10, 1, None, 0, None, C.byref(res)) == _lib.HISPMV_EINVAL
    assert lib.hispmv_bicgstab_device(None, 0, None, None, 1e-6, 10, 1, None, 0, None, C.byref(res)) == _lib.HISPMV_EINVAL
    assert lib.hispmv_cgls_device(None, 0, None, None, 1e-6, 10, 1, None, 0, None, C.byref(res)) == _lib.HISPMV_EINVAL
    assert lib.hispmv_krylov_status(None, None, None, C.byref(res)) == _lib.HISPMV_EINVAL


def test_dot_model_is_within_the_bound_of_any_order():
    rng = np.random.default_rng(7)
    for n in km.DOT_SIZES[:-1]:
        a, b = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
        exact = (a.astype(np.float64) * b.astype(np.float64)).tolist()
        bound = (n - 1) * 2.0 ** -53 * math.fsum(abs(t) for t in exact)
        assert abs(float(km.dot(a, b)) - math.fsum(exact)) <= bound, n
    assert km.dot(np.zeros(0, np.float32), np.zeros(0, np.float32)) == 0.0


@pytest.mark.parametrize("name", sorted(km.CASES))
def test_model_converges_within_half_the_budget(name):
    case = km.CASES[name]
    x, r, info, A, b = km.run_model(case)
    res = km.residual_of(case, A, x, b)
    print(f"{name}: {info}, true relative residual {res:.3e} (recorded {case['attained']:.3e})")
    assert info["status"] == "CONVERGED" and 0 < info["iterations"] <= case["max_iters"] // 2, info
    assert info["relres"] <= case["rtol"]
    # the recorded figure is what the tests' bounds are made from: it must be this model's, to two digits
    assert 0.9 * case["attained"] <= res <= 1.1 * case["attained"], (res, case["attained"])


def test_rescaled_laplacian_needs_its_preconditioner():
    case = dict(km.CASES["pcg_rescaled_laplacian_48"], precond=False, max_iters=5000)
    _, _, info, _, _ = km.run_model(case)
    assert info["status"] == "MAX_ITERS", info


def test_all_zero_values_are_a_breakdown_that_leaves_x_alone():
    A = km.zero_pattern(300)
    b, x0 = km.rhs(300), km.rhs(300, seed=2)
    prod, prod_t = km.scipy_products(A)
    for x, r, info in (km.cg(prod, b, x0, None, 1e-6, 5), km.bicgstab(prod, b, x0, 1e-6, 5), km.cgls(prod, prod_t, b, x0, 1e-6, 5)):
        assert info["status"] == "BREAKDOWN" and info["iterations"] == 0, info
        assert np.array_equal(x.view(np.uint32), x0.view(np.uint32))
    x, r, info = km.cg(prod, np.zeros(300, np.float32), x0, None, 1e-6, 5)
    assert info["status"] == "CONVERGED" and info["iterations"] == 0 and not x.any()
