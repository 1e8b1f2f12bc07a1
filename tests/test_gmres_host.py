"""Restarted GMRES without a device: the workspace rule (hispmv_prep_gmres against prep.gmres and the layout include/hispmv.h describes),
the refusals that need no context, and the numpy model of tests/gmres_model.py with scipy products -- does the arithmetic the header
writes down converge in float32, where BiCGSTAB does not, and in the inner iterations scipy's fp64 GMRES takes?"""
import ctypes as C

import numpy as np
import pytest

import gmres_model as gm
import krylov_model as km
from hispmv_amd import _lib, prep

f32 = np.float32


def _raw(n, restart, with_minv):
    out = (C.c_int64 * 8)()
    rc = _lib.lib.hispmv_prep_gmres(n, restart, with_minv, out)
    return rc, [int(v) for v in out]


@pytest.mark.parametrize("n", [0, 1, 3, 1023, 1024, 1025, 4099, 1024 * 1024 + 1029, 5 * 1024 * 1024])
@pytest.mark.parametrize("restart", [1, 5, 30, 64])
@pytest.mark.parametrize("with_minv", [0, 1])
def test_prep_gmres_is_the_rule_of_the_header(n, restart, with_minv):
    rc, out = _raw(n, restart, with_minv)
    assert rc == _lib.HISPMV_OK
    p = prep.gmres(n, restart, bool(with_minv))
    keys = ("work_bytes", "v_offset", "stride", "groups", "dot_tile", "launches_per_iteration", "launches_per_cycle", "basis_vectors")
    assert [p[k] for k in keys] == out
    stride, groups = (n + 3) // 4 * 4, prep.krylov_groups(n)
    assert (p["stride"], p["groups"], p["basis_vectors"]) == (stride, groups, restart + 1)
    assert (p["launches_per_iteration"], p["launches_per_cycle"]) == (4, 3) and 1 <= p["dot_tile"] <= 65
    # the regions in order: two scalar blocks and the scratch double (512 bytes), c s g_fin g_res h1 h (66 doubles each), R (64 x 64),
    # three single partial arrays and two of 65 sums, the basis, z -- each 16-byte aligned, none overlapping the next
    gp = max(groups + groups % 2, 2)
    regions = [512] + [66 * 8] * 6 + [64 * 64 * 8] + [gp * 8] * 3 + [65 * gp * 8] * 2
    v_offset = sum(regions)
    assert all(r % 16 == 0 for r in regions) and p["v_offset"] == v_offset and v_offset % 16 == 0 and (4 * stride) % 16 == 0
    assert p["work_bytes"] == v_offset + 4 * stride * (restart + 1 + with_minv)
    assert 8 * gp >= 8 * groups


def test_prep_gmres_refuses():
    for n, restart in ((10, 0), (10, 65), (-1, 30), (10, -3)):
        assert _raw(n, restart, 0)[0] == _lib.HISPMV_EINVAL
        with pytest.raises(ValueError):
            prep.gmres(n, restart)
    assert _lib.lib.hispmv_prep_gmres(10, 30, 0, None) == _lib.HISPMV_EINVAL
    assert _lib.HISPMV_GMRES_MAX_RESTART == gm.MAX_RESTART == 64


def test_device_entries_refuse_a_missing_context():
    out = (C.c_int64 * 8)()
    res = _lib.KrylovResult()
    assert _lib.lib.hispmv_gmres_info(None, 0, 30, 0, out) == _lib.HISPMV_EINVAL
    assert _lib.lib.hispmv_dot_basis_device(None, 4, 1, None, 4, None, None, None, 0, None) == _lib.HISPMV_EINVAL
    assert _lib.lib.hispmv_gmres_device(None, 0, None, None, None, 30, 1e-6, 10, 8, None, 0, None, C.byref(res)) == _lib.HISPMV_EINVAL


# ---- the model with scipy products ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(gm.CASES))
def test_model_converges_and_reproduces_the_table(name):
    case = gm.CASES[name]
    x, V, info, A, b = gm.run_model(case)
    res = km.true_relres(A, x, b)
    print(f"{name}: {info}, true relative residual {res:.4e}, recorded {case['attained']:.3e}")
    assert info["status"] == "CONVERGED" and info["iterations"] == case["iterations"] <= case["max_iters"], info
    assert info["relres"] <= case["rtol"]
    assert abs(res - case["attained"]) <= 0.01 * case["attained"], (res, case["attained"])
    cycles = -(-case["max_iters"] // case["restart"])
    assert info["products"] == cycles + case["max_iters"]          # the products run on after the freeze and are ignored
    assert V.shape[0] == min(case["restart"], case["max_iters"] - (cycles - 1) * case["restart"]) + 1


def test_model_takes_the_inner_iterations_of_scipys_fp64_gmres_where_bicgstab_stalls():
    import scipy.sparse.linalg as sla
    case = gm.CASES["convdiff_48_pe1000"]
    A = case["make"]()
    b = km.rhs(A.shape[0])
    A64 = A.tocsr().astype(np.float64)
    for restart, want in ((10, 127), (30, 156)):
        x, V, info, _, _ = gm.run_model(case, A=A, restart=restart)
        count = [0]

        def tick(_):
            count[0] += 1
        xs, flag = sla.gmres(A64, b.astype(np.float64), rtol=case["rtol"], atol=0.0, restart=restart, maxiter=100, callback=tick, callback_type="pr_norm")
        print(f"restart {restart}: model {info}, scipy {count[0]} inner iterations")
        assert flag == 0 and info["status"] == "CONVERGED"
        assert info["iterations"] == count[0] == want
    prod, _ = km.scipy_products(A)
    _, _, binfo = km.bicgstab(prod, b, np.zeros(len(b), f32), case["rtol"], 600)
    print(f"BiCGSTAB: {binfo}")
    assert binfo["status"] == "MAX_ITERS" and binfo["iterations"] == 600


def test_model_edge_cases():
    A = km.zero_pattern(300)
    prod, _ = km.scipy_products(A)
    b, x0 = km.rhs(300), km.rhs(300, seed=2)
    x, V, info = gm.gmres(prod, b, x0, None, 1e-6, 5, 3)
    assert info["status"] == "BREAKDOWN" and info["iterations"] == 0 and np.array_equal(x, x0), info
    x, V, info = gm.gmres(prod, np.zeros(300, f32), x0, None, 1e-6, 5, 3)
    assert info["status"] == "CONVERGED" and info["iterations"] == 0 and not x.any(), info
    import scipy.sparse as sp
    D = sp.diags([np.full(300, 3.0, f32)], [0], format="coo", dtype=f32)          # v_0 is an eigenvector: hn = 0, the lucky breakdown
    prod, _ = km.scipy_products(D)
    x, V, info = gm.gmres(prod, b, np.zeros(300, f32), None, 1e-6, 5, 3)
    assert info["status"] == "CONVERGED" and info["iterations"] == 1 and km.true_relres(D, x, b) < 1e-6, info
    bad = b.copy()
    bad[7] = np.nan
    x, V, info = gm.gmres(km.scipy_products(km.band(300))[0], bad, x0, None, 1e-6, 5, 3)
    assert info["status"] == "BREAKDOWN" and info["iterations"] == 0 and np.array_equal(x, x0), info
