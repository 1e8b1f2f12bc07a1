"""A numpy restatement of restarted GMRES(m) as include/hispmv.h writes it down ("Restarted GMRES(m) on loaded handles"): krylov_model's
fixed-order fp64 dot product, CGS2 with float32 vector arithmetic (one rounding per operation), fp64 Givens rotations and back
substitution, scalars rounded once to float32, and the freeze rules.  The products come from a callback, as in krylov_model: scipy's on
the CPU, spmv_device's own results on the GPU.  Also the systems and the case table of the GMRES tests."""
import math

import numpy as np

import krylov_model as km

f32 = np.float32
f64 = np.float64
MAX_RESTART = 64


def gmres(prod, b, x0, minv, rtol, max_iters, restart):
    """prod(x, bias, alpha, beta) -> float32 alpha * A x + beta * bias.  Returns (x, V, info): V the basis slots 0 .. m of the last
    cycle as the workspace holds them (m = its columns), info as krylov_model's."""
    with np.errstate(all="ignore"):
        st = km._State()
        n = len(b)
        x = np.array(x0, f32)
        tol2 = f64(rtol) * f64(rtol)
        st.bb = b2 = km.dot(b, b)
        if b2 == 0.0:
            st.done = True
            x[:] = 0
        elif km._bad(st.bb):
            st.brk = True
        V = np.zeros((restart + 1, n), f32)
        z = np.zeros(n, f32)
        c, s = np.zeros(MAX_RESTART, f64), np.zeros(MAX_RESTART, f64)
        g_fin, g_res = np.zeros(MAX_RESTART, f64), np.zeros(MAX_RESTART + 1, f64)
        R = np.zeros((MAX_RESTART, MAX_RESTART), f64)
        cols = 0

        def mv(*a):
            st.products += 1
            return prod(*a)

        def step(j):
            """the four vector kernels behind the product of inner step j; returns the completed columns"""
            w = V[j + 1]
            h1 = np.array([km.dot(V[i], w) for i in range(j + 1)], f64)
            if not np.all(np.isfinite(h1)):
                st.brk = True
                return cols
            for i in range(j + 1):
                t = f32(h1[i]) * V[i]
                w = w - t
            V[j + 1] = w
            h2 = np.array([km.dot(V[i], w) for i in range(j + 1)], f64)
            if not np.all(np.isfinite(h2)):
                st.brk = True
                return cols
            for i in range(j + 1):
                t = f32(h2[i]) * V[i]
                w = w - t
            V[j + 1] = w
            h = h1 + h2
            ww = km.dot(w, w)
            if not math.isfinite(ww):
                st.brk = True
                return cols
            hn = np.sqrt(ww)
            for i in range(j):
                t = c[i] * h[i] + s[i] * h[i + 1]
                h[i + 1] = c[i] * h[i + 1] - s[i] * h[i]
                h[i] = t
            d = np.sqrt(h[j] * h[j] + hn * hn)
            if km._bad(d):
                st.brk = True
                return cols
            c[j], s[j] = h[j] / d, hn / d
            R[:j, j] = h[:j]
            R[j, j] = d
            g_fin[j] = c[j] * g_res[j]
            g_res[j + 1] = -(s[j] * g_res[j])
            st.iters += 1
            st.rr = g_res[j + 1] * g_res[j + 1]
            if st.rr <= tol2 * st.bb:
                st.done = True
            else:
                V[j + 1] = f32(f64(1.0) / hn) * w
                if minv is not None:
                    z[:] = minv * V[j + 1]
            return j + 1

        it, m = 0, 0
        while it < max_iters:
            m = min(restart, max_iters - it)
            V[0] = mv(x, b, -1.0, 1.0)
            rr = km.dot(V[0], V[0])
            if not st.frozen:
                st.rr = rr
                if not math.isfinite(rr):
                    st.brk = True
                elif rr <= tol2 * st.bb:
                    st.done = True
                else:
                    beta = np.sqrt(rr)
                    V[0] = f32(f64(1.0) / beta) * V[0]
                    g_res[0] = beta
                    cols = 0
                    if minv is not None:
                        z[:] = minv * V[0]
            for j in range(m):
                V[j + 1] = mv(z if minv is not None else V[j], None, 1.0, 0.0)
                if not st.frozen:
                    cols = step(j)
                it += 1
            if cols > 0:          # the close: acts once, also for a solve that froze inside the cycle
                y = np.zeros(cols, f64)
                for i in range(cols - 1, -1, -1):
                    acc = g_fin[i]
                    for k in range(i + 1, cols):
                        acc = acc - R[i, k] * y[k]
                    y[i] = acc / R[i, i]
                u = f32(y[0]) * V[0]
                for i in range(1, cols):
                    t = f32(y[i]) * V[i]
                    u = u + t
                x = x + (minv * u if minv is not None else u)
                cols = 0
        return x, V[:m + 1].copy(), st.info()


# ---- the systems -------------------------------------------------------------------------------------------------------------------
def convdiff(m, pe):
    """Convection-diffusion on an m x m grid, central differences: kron(I, T1) + kron(T2, I), h = 1 / (m + 1),
    T1 = tridiag(-(1 + pe h / 2), 2, -(1 - pe h / 2)), T2 = tridiag(-1, 2, -1); strongly non-normal for a large Peclet number pe."""
    import scipy.sparse as sp
    h = 1.0 / (m + 1)
    t1 = sp.diags([np.full(m - 1, -(1 + pe * h / 2)), np.full(m, 2.0), np.full(m - 1, -(1 - pe * h / 2))], [-1, 0, 1])
    t2 = sp.diags([-np.ones(m - 1), 2 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1])
    return (sp.kron(sp.identity(m), t1) + sp.kron(t2, sp.identity(m))).astype(f32).tocoo()


# Convergence cases: the system, restart, rtol, the budget of inner iterations, and what the model reaches with scipy products on the
# CPU: its inner iterations and `attained`, the fp64 true relative residual; a test's bound is twice that.  precond: minv = 1 / diag.
CASES = {
    "band_4099": dict(make=lambda: km.band(4099), restart=30, rtol=1e-6, max_iters=100, precond=False, iterations=11, attained=8.34e-7),
    "band_1025_r5": dict(make=lambda: km.band(1025), restart=5, rtol=1e-6, max_iters=100, precond=False, iterations=11, attained=7.70e-7),
    "tridiag_4099_minv": dict(make=lambda: km.tridiag(4099, lo=-1.3, d=2.5, up=-0.7), restart=20, rtol=1e-6, max_iters=100, precond=True, iterations=30,
                              attained=8.09e-7),
    "convdiff_48_pe1000": dict(make=lambda: convdiff(48, 1000), restart=10, rtol=1e-5, max_iters=200, precond=False, iterations=127, attained=9.86e-6),
    "convdiff_40_pe30": dict(make=lambda: convdiff(40, 30), restart=30, rtol=1e-5, max_iters=200, precond=False, iterations=123, attained=9.13e-6),
}


def run_model(case, A=None, products=None, **over):
    """The model on a case with the given product callbacks (default: scipy's): (x, V, info, A, b); over: restart, rtol, max_iters."""
    A = case["make"]() if A is None else A
    b = km.rhs(A.shape[0])
    prod, _ = km.scipy_products(A) if products is None else products
    minv = (1.0 / A.tocsr().diagonal()).astype(f32) if case["precond"] else None
    p = {k: over.get(k, case[k]) for k in ("rtol", "max_iters", "restart")}
    x, V, info = gmres(prod, b, np.zeros(A.shape[1], f32), minv, p["rtol"], p["max_iters"], p["restart"])
    return x, V, info, A, b
