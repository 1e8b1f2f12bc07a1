"""A numpy restatement of the Krylov layer (include/hispmv.h, "Krylov solvers on loaded handles"): the fixed-order fp64 dot product and the
three loops with float32 vector arithmetic, one rounding per operation, and fp64 scalars rounded once to float32.  The products come
from a callback, so the same model runs against scipy on the CPU (are the inputs fair?) and against spmv_device's own results on the
GPU (does the layer compute what it says, bit for bit?).  Also the systems and case tables of the Krylov tests."""
import math

import numpy as np

f32 = np.float32


# ---- the dot product ---------------------------------------------------------------------------------------------------------------
def groups(n: int) -> int:
    return min((n + 1023) // 1024, 1024)


def _tree(v):
    """v[..., 256] -> v[..., 0] by v[t] += v[t + h], h = 128, 64, ... 1"""
    h = 128
    while h >= 1:
        v = v[..., :h] + v[..., h:2 * h]
        h //= 2
    return v[..., 0]


def _sum4(s):
    """s[..., 4] -> (((+0 + s0) + s1) + s2) + s3"""
    acc = np.zeros(s.shape[:-1], np.float64)
    for j in range(4):
        acc = acc + s[..., j]
    return acc


def dot_partials(a, b):
    n = len(a)
    chunks, g = (n + 1023) // 1024, groups(n)
    prod = np.zeros(chunks * 1024, np.float64)
    prod[:n] = a.astype(np.float64) * b.astype(np.float64)          # exact
    s = _sum4(prod.reshape(chunks, 256, 4))
    acc = np.zeros((g, 256), np.float64)
    for k in range(0, chunks, max(g, 1)):          # workgroup w adds chunks w, w + g, ... ascending
        part = s[k:k + g]
        acc[:len(part)] = acc[:len(part)] + part
    return _tree(acc)


def sum_partials(p):
    u = np.zeros(1024, np.float64)
    u[:len(p)] = p
    return np.float64(_tree(_sum4(u.reshape(256, 4))))


def dot(a, b):
    a = np.ascontiguousarray(a, f32)
    b = np.ascontiguousarray(b, f32)
    if len(a) == 0:
        return np.float64(0.0)
    return sum_partials(dot_partials(a, b))


def _bad(d) -> bool:
    return not (d != 0.0 and math.isfinite(d))


# ---- the loops ---------------------------------------------------------------------------------------------------------------------
class _State:
    def __init__(self):
        self.done = self.brk = False
        self.iters = 0
        self.rr = np.float64(0.0)
        self.rho = np.float64(0.0)
        self.bb = np.float64(0.0)
        self.products = 0

    @property
    def frozen(self):
        return self.done or self.brk

    def info(self):
        relres = math.sqrt(self.rr / self.bb) if self.bb > 0 else 0.0
        return {"status": "BREAKDOWN" if self.brk else "CONVERGED" if self.done else "MAX_ITERS", "iterations": self.iters, "relres": relres,
                "products": self.products}


def cg(prod, b, x0, minv, rtol, max_iters):
    """prod(x, bias, alpha, beta) -> float32 alpha * A x + beta * bias.  Returns (x, r, info)."""
    with np.errstate(all="ignore"):
        st = _State()
        x = np.array(x0, f32)
        tol2 = np.float64(rtol) * np.float64(rtol)
        st.bb = b2 = dot(b, b)
        if b2 == 0.0:
            st.done = True
            x[:] = 0
        elif _bad(st.bb):
            st.brk = True

        def mv(*a):
            st.products += 1
            return prod(*a)
        r = mv(x0, b, -1.0, 1.0)
        z = minv * r if minv is not None else r
        p = z.copy()
        rr_new = dot(r, r)
        rho_new = dot(r, z) if minv is not None else rr_new
        for it in range(max_iters):
            q = mv(p, None, 1.0, 0.0)
            if it == 0 and not st.frozen:
                st.rr, st.rho = rr_new, rho_new
                st.done = bool(st.rr <= tol2 * st.bb)
            pq = dot(p, q)
            if not st.frozen:
                if _bad(pq) or not math.isfinite(st.rho):
                    st.brk = True
                else:
                    a32 = f32(st.rho / pq)
                    x = x + a32 * p
                    r = r - a32 * q
                    st.iters += 1
                    z = minv * r if minv is not None else r
                    rr_new = dot(r, r)
                    rho_new = dot(r, z) if minv is not None else rr_new
            if not st.frozen:
                st.rr = rr_new
                if st.rr <= tol2 * st.bb:
                    st.done, st.rho = True, rho_new
                elif _bad(st.rho) or not math.isfinite(rho_new):
                    st.brk = True
                else:
                    b32 = f32(rho_new / st.rho)
                    st.rho = rho_new
                    p = z + b32 * p
        return x, r, st.info()


def bicgstab(prod, b, x0, rtol, max_iters):
    with np.errstate(all="ignore"):
        st = _State()
        x = np.array(x0, f32)
        tol2 = np.float64(rtol) * np.float64(rtol)
        st.bb = b2 = dot(b, b)
        if b2 == 0.0:
            st.done = True
            x[:] = 0
        elif _bad(st.bb):
            st.brk = True

        def mv(*a):
            st.products += 1
            return prod(*a)
        r = mv(x0, b, -1.0, 1.0)
        rhat, p = r.copy(), r.copy()
        rr_new = rho_new = dot(r, r)
        alpha = omega = np.float64(1.0)
        a32 = w32 = f32(1.0)
        ss = np.float64(0.0)
        for it in range(max_iters):
            v = mv(p, None, 1.0, 0.0)
            if it == 0 and not st.frozen:
                st.rr = st.rho = rr_new
                st.done = bool(st.rr <= tol2 * st.bb)
            den = dot(rhat, v)
            if not st.frozen:
                if _bad(den) or _bad(st.rho):
                    st.brk = True
                else:
                    alpha = st.rho / den
                    a32 = f32(alpha)
                    r = r - a32 * v          # s
                    ss = dot(r, r)
            t = mv(r, None, 1.0, 0.0)
            ts, tt = dot(t, r), dot(t, t)
            if not st.frozen:
                if ss <= tol2 * st.bb:
                    x = x + a32 * p
                    st.rr, st.done = ss, True
                    st.iters += 1
                elif _bad(tt) or _bad(ts / tt):
                    st.brk = True
                else:
                    omega = ts / tt
                    w32 = f32(omega)
                    x = x + a32 * p
                    x = x + w32 * r
                    r = r - w32 * t
                    st.iters += 1
                    rr_new, rho_new = dot(r, r), dot(rhat, r)
            if not st.frozen:
                st.rr = rr_new
                beta = (rho_new / st.rho) * (alpha / omega)
                if st.rr <= tol2 * st.bb:
                    st.done, st.rho = True, rho_new
                elif not math.isfinite(beta):
                    st.brk = True
                else:
                    st.rho = rho_new
                    p = r + f32(beta) * (p - w32 * v)
        return x, r, st.info()


def cgls(prod, prod_t, b, x0, rtol, max_iters):
    """prod_t(x) -> float32 A^T x.  The residual of the stopping rule is s = A^T r; returns (x, r, info)."""
    with np.errstate(all="ignore"):
        st = _State()
        x = np.array(x0, f32)
        tol2 = np.float64(rtol) * np.float64(rtol)
        b2 = dot(b, b)

        def mv(*a):
            st.products += 1
            return prod(*a)

        def mvt(v):
            st.products += 1
            return prod_t(v)
        s = mvt(b)
        st.bb = dot(s, s)
        if b2 == 0.0:
            st.done = True
            x[:] = 0
        elif _bad(st.bb) or not math.isfinite(b2):
            st.brk = True
        r = mv(x0, b, -1.0, 1.0)
        s = mvt(r)
        p = s.copy()
        g_new = dot(s, s)
        for it in range(max_iters):
            q = mv(p, None, 1.0, 0.0)
            if it == 0 and not st.frozen:
                st.rr = st.rho = g_new
                st.done = bool(st.rr <= tol2 * st.bb)
            den = dot(q, q)
            if not st.frozen:
                if _bad(den) or not math.isfinite(st.rho):
                    st.brk = True
                else:
                    a32 = f32(st.rho / den)
                    x = x + a32 * p
                    r = r - a32 * q
                    st.iters += 1
            s = mvt(r)
            g_new = dot(s, s)
            if not st.frozen:
                st.rr = g_new
                if st.rr <= tol2 * st.bb:
                    st.done, st.rho = True, g_new
                elif _bad(st.rho) or not math.isfinite(g_new):
                    st.brk = True
                else:
                    b32 = f32(g_new / st.rho)
                    st.rho = g_new
                    p = s + b32 * p
        return x, r, st.info()


def scipy_products(A):
    """The callbacks over a scipy matrix: float32 data, float32 results (scipy sums in float32, in its own order)."""
    A = A.tocsr().astype(f32)
    At = A.T.tocsr()

    def prod(x, bias, alpha, beta):
        y = f32(alpha) * (A @ np.asarray(x, f32))
        return (y + f32(beta) * bias).astype(f32) if bias is not None and beta != 0 else y.astype(f32)

    def prod_t(x):
        return (At @ np.asarray(x, f32)).astype(f32)
    return prod, prod_t


# ---- the systems -------------------------------------------------------------------------------------------------------------------
DOT_SIZES = (1, 2, 3, 63, 64, 65, 255, 1023, 1024, 1025, 4099, 1024 * 1024 + 1029)          # the last: workgroups 0 and 1 take a second chunk
TRIDIAG_SIZES = (1, 2, 3, 63, 64, 65, 255, 1023, 1024, 1025, 4099)


def tridiag(n, lo=-1.0, d=2.5, up=-1.0):
    import scipy.sparse as sp
    return sp.diags([np.full(max(n - 1, 0), lo, f32), np.full(n, d, f32), np.full(max(n - 1, 0), up, f32)], [-1, 0, 1], shape=(n, n), format="coo", dtype=f32)


def arrow(n=5000):
    """Symmetric positive definite: a dense first row and column (the row is 5000 elements, cut by five slices of 1024) on a diagonal."""
    import scipy.sparse as sp
    u = (0.01 * (1.0 + (np.arange(1, n) % 7) / 7.0)).astype(f32)
    i = np.arange(1, n)
    rows = np.concatenate([[0], np.zeros(n - 1, np.int64), i, i])
    cols = np.concatenate([[0], i, np.zeros(n - 1, np.int64), i])
    vals = np.concatenate([[f32(5.0)], u, u, np.full(n - 1, 2.5, f32)]).astype(f32)
    return sp.coo_matrix((vals, (rows, cols)), shape=(n, n))


def laplacian(m=48):
    import scipy.sparse as sp
    t = sp.diags([-np.ones(m - 1), 2 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1])
    return (sp.kron(sp.identity(m), t) + sp.kron(t, sp.identity(m))).astype(f32).tocoo()


def rescaled_laplacian(m=48, seed=5):
    import scipy.sparse as sp
    d = (10.0 ** np.random.default_rng(seed).uniform(-2, 2, m * m)).astype(f32)
    return (sp.diags(d) @ laplacian(m) @ sp.diags(d)).astype(f32).tocoo()


def band(n, seed=3):
    """Non-symmetric, diagonally dominant: five diagonals with random off-diagonal entries."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    offs = [o for o in (-3, -1, 1, 2) if abs(o) < n]
    diags = [rng.uniform(-1, 1, n - abs(o)).astype(f32) for o in offs]
    return sp.diags(diags + [np.full(n, 4.5, f32)], offs + [0], shape=(n, n), format="coo", dtype=f32)


def least_squares(rows=300, cols=200, seed=11):
    import scipy.sparse as sp
    A = sp.random(rows, cols, density=0.05, random_state=np.random.default_rng(seed), dtype=np.float64).astype(f32)
    return (A + sp.eye(rows, cols, dtype=f32)).astype(f32).tocoo()


def zero_pattern(n=300):
    A = tridiag(n)
    A.data[:] = 0
    return A


def rhs(n, seed=1):
    return np.random.default_rng(seed).uniform(-1, 1, n).astype(f32)


def true_relres(A, x, b):
    A64 = A.tocsr().astype(np.float64)
    b64 = b.astype(np.float64)
    return float(np.linalg.norm(b64 - A64 @ x.astype(np.float64)) / np.linalg.norm(b64))


def normal_relres(A, x, b):
    A64 = A.tocsr().astype(np.float64)
    b64 = b.astype(np.float64)
    return float(np.linalg.norm(A64.T @ (b64 - A64 @ x.astype(np.float64))) / np.linalg.norm(A64.T @ b64))


# Convergence cases: the solver, the system, rtol, max_iters, and `attained`: the fp64 true relative residual (CGLS: of the normal
# equations) the model reaches with scipy products on the CPU; a test's bound is twice that.  precond: minv = 1 / diag.
# bound None: convergence only (the rescaled Laplacian's recursive and true residuals part by 1e-3 in the model itself).
CASES = {
    "cg_tridiag_4099": dict(solver="cg", make=lambda: tridiag(4099), rtol=1e-6, max_iters=100, precond=False, attained=7.3e-7),
    "cg_laplacian_48": dict(solver="cg", make=lambda: laplacian(48), rtol=1e-5, max_iters=400, precond=False, attained=1.02e-5),
    "cg_arrow_5000": dict(solver="cg", make=lambda: arrow(5000), rtol=1e-6, max_iters=100, precond=False, attained=6.5e-8),
    "pcg_arrow_5000": dict(solver="cg", make=lambda: arrow(5000), rtol=1e-6, max_iters=100, precond=True, attained=6.0e-8),
    "pcg_rescaled_laplacian_48": dict(solver="cg", make=lambda: rescaled_laplacian(48), rtol=1e-5, max_iters=600, precond=True, attained=2.1e-3, bound=False),
    "bicgstab_band_4099": dict(solver="bicgstab", make=lambda: band(4099), rtol=1e-6, max_iters=100, precond=False, attained=3.3e-7),
    "cgls_300x200": dict(solver="cgls", make=lambda: least_squares(300, 200), rtol=1e-5, max_iters=400, precond=False, attained=9.7e-6),
}


def run_model(case, A=None, products=None):
    """The model on a case with the given product callbacks (default: scipy's): (x, r, info, A, b)."""
    A = case["make"]() if A is None else A
    b = rhs(A.shape[0])
    prod, prod_t = scipy_products(A) if products is None else products
    x0 = np.zeros(A.shape[1], f32)
    minv = (1.0 / A.tocsr().diagonal()).astype(f32) if case["precond"] else None
    if case["solver"] == "cg":
        x, r, info = cg(prod, b, x0, minv, case["rtol"], case["max_iters"])
    elif case["solver"] == "bicgstab":
        x, r, info = bicgstab(prod, b, x0, case["rtol"], case["max_iters"])
    else:
        x, r, info = cgls(prod, prod_t, b, x0, case["rtol"], case["max_iters"])
    return x, r, info, A, b


def residual_of(case, A, x, b):
    return normal_relres(A, x, b) if case["solver"] == "cgls" else true_relres(A, x, b)
