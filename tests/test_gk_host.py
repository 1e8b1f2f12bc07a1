"""Thick-restart Golub-Kahan without a device: the workspace rule (hispmv_prep_gk against the layout include/hispmv.h describes), the
small SVD of the library (hispmv_prep_bsvd: one-sided Jacobi, the order, the residual estimates, the converged count) against
numpy.linalg.svd, and the numpy model of tests/gk_model.py with scipy products -- does the arithmetic the header writes down find the
singular values in float32, in the products the first prototype took, with the library's Jacobi and with numpy's SVD alike?"""
import ctypes as C
import functools

import numpy as np
import pytest

import gk_model as gm
import lanczos_model as lm
from hispmv_amd import _lib, prep

f32 = np.float32
f64 = np.float64


# ---- the workspace rule --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 5), (5000, 3), (4099, 5000), (0, 0), (1024, 1025)])
@pytest.mark.parametrize("ncv", [2, 20, 64])
def test_prep_gk_is_the_rule_of_the_header(shape, ncv):
    rows, cols = shape
    p = prep.gk(rows, cols, ncv)
    sv, su = (cols + 3) // 4 * 4, (rows + 3) // 4 * 4
    assert (p["v_stride"], p["u_stride"]) == (sv, su)
    # the partials are sized by the larger of the two grids, whichever side it belongs to
    groups = max(prep.krylov_groups(rows), prep.krylov_groups(cols))
    gp = max(groups + groups % 2, 2)
    # the regions in order: three scalar blocks in 512 bytes, g1 and g (66 doubles each), Gc (64 columns of 66 doubles), the alphas and
    # the betas (66 doubles each), Yt (64 x 65 floats), two single partial arrays and two of 65 sums, V (ncv + 1 vectors), U (ncv)
    regions = [512, 66 * 8, 66 * 8, 64 * 66 * 8, 66 * 8, 66 * 8, 64 * 65 * 4, gp * 8, gp * 8, 65 * gp * 8, 65 * gp * 8, 4 * sv * (ncv + 1), 4 * su * ncv]
    assert all(r % 16 == 0 for r in regions)
    offsets = np.cumsum([0] + regions)
    assert p["gc_offset"] == offsets[3] and p["yt_offset"] == offsets[6] and p["part_offset"] == offsets[7]
    assert p["v_offset"] == offsets[11] and p["u_offset"] == offsets[12] and p["work_bytes"] == offsets[13]
    assert p["v_offset"] - p["part_offset"] == 132 * gp * 8
    assert all(p[key] % 16 == 0 for key in ("gc_offset", "yt_offset", "part_offset", "v_offset", "u_offset", "work_bytes"))
    assert 512 < p["gc_offset"] < p["yt_offset"] < p["part_offset"] < p["v_offset"] <= p["u_offset"] <= p["work_bytes"]


def test_prep_gk_refuses():
    out = (C.c_int64 * 8)()
    for rows, cols, ncv in ((10, 10, 1), (10, 10, 65), (-1, 10, 20), (10, -1, 20), (10, 10, 0), (10, 10, -3)):
        assert _lib.lib.hispmv_prep_gk(rows, cols, ncv, out) == _lib.HISPMV_EINVAL
        with pytest.raises(ValueError):
            prep.gk(rows, cols, ncv)
    assert _lib.lib.hispmv_prep_gk(10, 10, 20, None) == _lib.HISPMV_EINVAL
    assert _lib.HISPMV_GK_MAX_NCV == gm.MAX_NCV == 64


def test_device_entries_refuse_a_missing_context():
    out = (C.c_int64 * 8)()
    res = _lib.EigshResult()
    assert _lib.lib.hispmv_gk_info(None, 0, 20, out) == _lib.HISPMV_EINVAL
    assert _lib.lib.hispmv_gk_steps_device(None, 0, 2, 0, 1, 1, None, None, 0, None) == _lib.HISPMV_EINVAL
    assert _lib.lib.hispmv_gk_status(None, None, None, out) == _lib.HISPMV_EINVAL
    assert _lib.lib.hispmv_svds_device(None, 0, 1, 2, 1e-5, 10, None, 1, None, 4, None, 4, None, None, None, 0, None, C.byref(res)) == _lib.HISPMV_EINVAL


# ---- the small SVD ---------------------------------------------------------------------------------------------------------------------
def _upper_arrow(m, rng, cols=None):
    """what a look sees after a restart: kept values on the diagonal, the arrow column, then the upper part the device computed"""
    cols = m if cols is None else cols
    keep = m // 2
    B = np.zeros((m, cols))
    B[np.arange(keep), np.arange(keep)] = np.sort(rng.uniform(1.0, 60.0, keep))[::-1]
    for j in range(keep, cols):
        B[:min(j, m), j] = rng.standard_normal(min(j, m)) * (1e-2 if j == keep else 1e-6)
        if j < m:
            B[j, j] = rng.uniform(1.0, 60.0)
        if 0 < j <= m:
            B[j - 1, j] = rng.standard_normal()
    return B


def _bsvd_cases():
    rng = np.random.default_rng(64)
    cases = {f"arrow_{m}": _upper_arrow(m, rng) for m in (1, 2, 3, 20, 64)}
    cases["wide_20x21"] = _upper_arrow(20, rng, 21)
    cases["wide_1x2"] = _upper_arrow(1, rng, 2)
    zero_row = _upper_arrow(12, rng)
    zero_row[5, :] = 0.0
    cases["zero_row"] = zero_row
    cases["all_zero"] = np.zeros((3, 4))
    g = np.triu(rng.standard_normal((24, 24))) * 1e-3
    g[np.arange(24), np.arange(24)] = np.logspace(0, 6.5, 24)[::-1]
    cases["graded_over_1e6"] = g
    return cases


BSVD_CASES = _bsvd_cases()


@pytest.mark.parametrize("name", sorted(BSVD_CASES))
def test_prep_bsvd_against_numpy(name):
    B = BSVD_CASES[name]
    m, cols = B.shape
    beta, tol = 0.37, 1e-5
    r = prep.bsvd(B, 3, beta, tol)
    ref = gm.bsvd_numpy(B, 3, beta, tol)
    s, P, Q = r["s"], r["Pt"].T, r["Qt"].T
    s0 = max(ref["s"][0], 1e-300)
    print(f"{name}: {r['sweeps']} sweeps, values off by {np.abs(s - ref['s']).max() / s0:.2e} s_0, "
          f"|B - P S Q^T| {np.abs(B - (P * s) @ Q.T).max() / s0:.2e} s_0, |P^T P - I| {np.abs(P.T @ P - np.eye(m)).max():.2e}, "
          f"|Q^T Q - I| {np.abs(Q.T @ Q - np.eye(m)).max():.2e}")
    assert s.shape == (m,) and P.shape == (m, m) and Q.shape == (cols, m) and r["sweeps"] < 64
    assert np.all(np.diff(s) <= 0) and np.all(s >= 0)
    assert np.abs(s - ref["s"]).max() <= 1e-13 * s0
    assert np.linalg.norm(B - (P * s) @ Q.T) <= 1e-13 * s0
    assert np.abs(P.T @ P - np.eye(m)).max() <= 1e-13 and np.abs(Q.T @ Q - np.eye(m)).max() <= 1e-13
    assert np.array_equal(r["res"], beta * np.abs(r["Pt"][:, m - 1]))
    assert r["converged"] == int((r["res"][:min(3, m)] <= tol * s[0]).sum())
    if name == "zero_row":
        assert s[-1] == 0.0 and s[-2] > 0.0
    if name == "all_zero":
        assert not s.any()


def test_prep_bsvd_refuses_bad_shapes():
    dp = C.POINTER(C.c_double)
    buf = np.zeros(66 * 66)
    p = buf.ctypes.data_as(dp)
    counts = (C.c_int64 * 2)()

    def call(B=p, ld=4, rb=3, cb=4, k=1, beta=0.0, tol=1e-5, out=p):
        return _lib.lib.hispmv_prep_bsvd(B, ld, rb, cb, k, beta, tol, out, out, out, out, counts)
    assert call() == _lib.HISPMV_OK
    for kw in (dict(rb=0), dict(rb=65, cb=65, ld=66), dict(cb=2), dict(cb=5, ld=5), dict(ld=3), dict(k=0), dict(tol=-1.0), dict(tol=float("nan")),
               dict(beta=-1.0), dict(beta=float("nan")), dict(B=None), dict(out=None)):
        assert call(**kw) == _lib.HISPMV_EINVAL, kw
    for shape in ((0, 0), (3, 2), (3, 5), (65, 65)):
        with pytest.raises(ValueError):
            prep.bsvd(np.zeros(shape), 1, 0.0, 1e-5)
    with pytest.raises(ValueError):
        prep.bsvd(np.zeros(3), 1, 0.0, 1e-5)


# ---- the model on the case table -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model_run(name, numpy_svd=False):
    return gm.run_model(gm.CASES[name], bsvd=gm.bsvd_numpy if numpy_svd else None)


@pytest.mark.parametrize("name", sorted(gm.CASES))
def test_model_on_the_case_table(name):
    case = gm.CASES[name]
    s, u, vt, info, A = model_run(name)
    res, err = gm.accuracy(A, s, u, vt, info["status"]) if info["found"] else (0.0, 0.0)
    print(f"{name}: {info['status']}, found {info['found']}, {info['products']} products (prototype {case['prototype']}), {info['cycles']} cycles, "
          f"true residual {res:.3e}, singular-value error {err:.3e}, recorded {case['attained']}")
    assert (info["status"], info["found"]) == (case["status"], case["found"]), info
    assert info["products"] <= 2 * case["prototype"], info
    assert res <= 2 * case["attained"][0] and err <= 2 * case["attained"][1], (res, err, case["attained"])
    assert len(s) == info["found"] and u.shape == (info["found"], A.shape[0]) and vt.shape == (info["found"], A.shape[1])
    assert np.all(np.diff(s) <= 0)
    if info["found"]:
        assert np.abs(u.astype(f64) @ u.astype(f64).T - np.eye(len(s))).max() <= 1e-4
        assert np.abs(vt.astype(f64) @ vt.astype(f64).T - np.eye(len(s))).max() <= 1e-4


@pytest.mark.parametrize("name", sorted(gm.CASES))
def test_model_ends_the_same_way_with_numpy_svd(name):
    case = gm.CASES[name]
    info = model_run(name, True)[3]
    assert (info["status"], info["found"]) == (case["status"], case["found"]), info
    assert info["products"] <= 2 * case["prototype"], info


@pytest.mark.parametrize("kind", sorted(gm.KIND_CASES))
def test_model_on_the_handle_kinds(kind):
    """The figures tests/test_gpu_gk.py holds the handle kinds to: the model with scipy products on the matrix each kind holds."""
    case = gm.KIND_CASES[kind]
    s, u, vt, info, A = gm.run_model(case)
    res, err = gm.accuracy(A, s, u, vt, info["status"])
    print(f"{kind}: {info['status']}, {info['products']} products, {info['cycles']} cycles, true residual {res:.3e}, singular-value error {err:.3e}, "
          f"recorded {case['attained']}")
    assert (info["status"], info["found"]) == ("CONVERGED", 4), info
    assert res <= case["attained"][0] and err <= case["attained"][1], (res, err, case["attained"])
    assert res >= 0.5 * case["attained"][0] or case["attained"][0] == gm.FLOOR, "the recorded figure has drifted from what the model attains"


def test_where_the_tiny_cases_freeze():
    """The rows whose point is where the state freezes: the step, the side and the products."""
    import krylov_model as km
    want = {"graded_1x1": (1, False, 2), "graded_1x5": (1, True, 3), "graded_5x1": (1, False, 2), "graded_2x3": (2, True, 5), "graded_3x2": (2, False, 4),
            "graded_63x64": (63, True, 127), "graded_64x63": (63, False, 126), "rank3_k2": (3, True, 7), "zero_40x30": (0, True, 1)}
    for name, (m, closed, products) in want.items():
        case = gm.CASES[name]
        A = case["make"]()
        prod, prod_t = km.scipy_products(A)
        rows, cols = A.shape
        ncv = case["ncv"]
        V, U, st = np.zeros((ncv + 1, cols), f32), np.zeros((ncv, rows), f32), gm.Run()
        gm.open_run(gm.start(cols), V, st)
        gm.steps(prod, prod_t, V, U, 0, ncv, st)
        assert st.status() == {"steps": m, "invariant": True, "closed_u": closed, "breakdown": False, "products": products}, (name, st.status())


def test_breakdown_of_the_model():
    import krylov_model as km
    A = gm.graded(30, 20)
    prod, prod_t = km.scipy_products(A)
    for v0 in (np.zeros(20, f32), np.full(20, np.nan, f32)):
        s, u, vt, info = gm.svds(prod, prod_t, prep.bsvd, v0, 2, 8, gm.TOL, 1000, 30)
        assert info["status"] == "BREAKDOWN" and info["found"] == 0 and len(s) == 0 and u.shape == (0, 30) and vt.shape == (0, 20)


# ---- the arrow column ------------------------------------------------------------------------------------------------------------------
def test_arrow_column_comes_out_of_the_u_side_dots():
    """After one restart of graded(255, 300) the U-side coefficients of step keep are beta * P[m - 1][i]."""
    import krylov_model as km
    A = gm.graded(255, 300)
    prod, prod_t = km.scipy_products(A)
    ncv, k = 20, 4
    V, U, st = np.zeros((ncv + 1, 300), f32), np.zeros((ncv, 255), f32), gm.Run()
    gm.open_run(gm.start(300), V, st)
    gm.steps(prod, prod_t, V, U, 0, ncv, st)
    assert st.steps == ncv and not st.frozen and st.products == 2 * ncv
    B = np.zeros((64, 65), f64)
    gm.fill_b(B, st, 0, ncv, False)
    r = prep.bsvd(B[:ncv, :ncv], k, st.betas[ncv - 1], gm.TOL)
    keep = lm.keep_of(k, ncv)
    assert keep == 12
    new_u, new_v, last = lm.rotate(U[:ncv], r["Pt"][:keep].astype(f32)), lm.rotate(V[:ncv], r["Qt"][:keep].astype(f32)), V[ncv].copy()
    U[:keep], V[:keep], V[keep] = new_u, new_v, last
    gm.steps(prod, prod_t, V, U, keep, keep + 1, st)
    arrow = st.Gc[keep, :keep]
    want = st.betas[ncv - 1] * r["Pt"][:keep, ncv - 1]
    print(f"arrow column off by {np.abs(arrow - want).max() / r['s'][0]:.2e} s_0")
    assert np.abs(arrow - want).max() <= 1e-5 * r["s"][0]
