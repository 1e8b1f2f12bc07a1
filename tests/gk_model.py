"""A numpy restatement of thick-restart Golub-Kahan bidiagonalisation as include/hispmv.h writes it down ("Golub-Kahan / svds"):
krylov_model's fixed-order fp64 dot product, CGS2 on both sides with float32 vector arithmetic (one rounding per operation), fp64
scalars rounded once to float32, the closed-space rule of the U side and the invariant rule of the V side, the host look, the restart
and the finish.  The products come from callbacks, as in krylov_model: scipy's on the CPU, spmv_device's and spmv_device_t's own results
on the GPU.  The small SVD is a callback too: the tests pass prep.bsvd, the library's own host code, so lockstep never depends on
restating Jacobi here; bsvd_numpy is the independent check of that code.  Also the matrices and the case table of the svds tests."""
import math

import numpy as np

import krylov_model as km
import lanczos_model as lm

f32 = np.float32
f64 = np.float64
MAX_NCV = 64
GC_LD = 66
TINY2 = lm.TINY2


class Run:
    """The scalar block, Gc, the alphas and the betas of a run."""

    def __init__(self):
        self.brk = self.inv = self.closed = False
        self.steps = self.products = 0
        self.Gc = np.zeros((MAX_NCV, GC_LD), f64)
        self.alphas = np.zeros(GC_LD, f64)
        self.betas = np.zeros(GC_LD, f64)

    @property
    def frozen(self):
        return self.brk or self.inv

    def status(self):
        return {"steps": self.steps, "invariant": self.inv, "closed_u": self.closed, "breakdown": self.brk, "products": self.products}


def open_run(v0, V, st):
    """Lanczos's open on V slot 0"""
    lm.open_run(v0, V, st)


def _cgs2(W, cnt, w, st):
    """Two passes of classical Gram-Schmidt of w against W[:cnt]: (w, g1 + g2), or None after a breakdown (w's slot then holds what
    the kernel that broke down left)."""
    g = np.zeros(cnt, f64)
    for _ in range(2):
        gp = np.array([km.dot(W[i], w) for i in range(cnt)], f64)
        if not np.all(np.isfinite(gp)):
            st.brk = True
            return w, None
        for i in range(cnt):
            t = f32(gp[i]) * W[i]
            w = w - t
        g = g + gp if _ else gp
    return w, g


def _closes(ww, g):
    gsq = f64(0.0)
    for gi in g:
        sq = gi * gi
        gsq = gsq + sq
    return bool(ww <= TINY2 * (ww + gsq))


def steps(prod, prod_t, V, U, j0, j1, st):
    """Steps j0 .. j1 - 1 on the bases V [>= j1 + 1, cols] and U [>= j1, rows] in place.  prod(x, bias, alpha, beta) and prod_t(x) as in
    krylov_model; the products of a frozen run still land in their slots and are ignored."""
    with np.errstate(all="ignore"):
        for j in range(j0, j1):
            # the U side
            U[j] = prod(V[j], None, 1.0, 0.0)
            if not st.frozen:
                u, g = _cgs2(U, j, U[j].copy(), st)
                U[j] = u
                if g is not None:
                    uu = km.dot(u, u)
                    if not math.isfinite(uu):
                        st.brk = True
                    else:
                        st.Gc[j, :j] = g
                        if _closes(uu, g):
                            st.products += 1
                            st.steps = j
                            st.inv = st.closed = True
                        else:
                            alpha = np.sqrt(uu)
                            st.alphas[j] = alpha
                            U[j] = f32(f64(1.0) / alpha) * u
            # the V side
            V[j + 1] = prod_t(U[j])
            if st.frozen:
                continue
            w, h = _cgs2(V, j + 1, V[j + 1].copy(), st)
            V[j + 1] = w
            if h is None:
                continue
            ww = km.dot(w, w)
            if not math.isfinite(ww):
                st.brk = True
                continue
            beta = np.sqrt(ww)
            st.products += 2
            st.steps = j + 1
            st.betas[j] = beta
            if _closes(ww, h):
                st.inv = True
                continue
            V[j + 1] = f32(f64(1.0) / beta) * w


def fill_b(B, st, j0, m, closed):
    """The columns of this cycle into B [64, 65]: B[i][j] = Gc[j][i], B[j][j] = alpha_j; after closed_u also the column m of B'"""
    for j in range(j0, m + 1 if closed else m):
        B[:min(j, m), j] = st.Gc[j, :min(j, m)]
        if j < m:
            B[j, j] = st.alphas[j]


def svds(prod, prod_t, bsvd, v0, k, ncv, tol, max_products, rows):
    """The driver: (s [found] float64, u [found, rows] float32, vt [found, cols] float32, info).  bsvd(B, k, beta, tol) -> prep.bsvd's
    dict."""
    cols = len(v0)
    V, U = np.zeros((ncv + 1, cols), f32), np.zeros((ncv, rows), f32)
    st = Run()
    open_run(np.asarray(v0, f32), V, st)
    B = np.zeros((MAX_NCV, MAX_NCV + 1), f64)
    j0 = cycles = 0
    none = (np.zeros(0, f64), np.zeros((0, rows), f32), np.zeros((0, cols), f32))
    while True:
        steps(prod, prod_t, V, U, j0, ncv, st)
        cycles += 1
        info = {"status": "BREAKDOWN", "found": 0, "products": st.products, "cycles": cycles, "residuals": np.zeros(0, f64), "scale": 0.0}
        m = st.steps
        if st.brk or (m == 0 and not st.closed):
            return none + (info,)
        if m == 0:
            info["status"] = "INVARIANT"
            return none + (info,)
        mc = m + 1 if st.closed else m
        fill_b(B, st, j0, m, st.closed)
        r = bsvd(B[:m, :mc].copy(), k, 0.0 if st.closed else st.betas[m - 1], tol)
        found = min(k, m)
        info["scale"] = float(r["s"][0])
        status = None
        if r["converged"] == found and m >= k:
            status = "CONVERGED"
        elif st.inv:
            status = "INVARIANT"
        elif st.products >= max_products:
            status = "MAX_ITERS"
        if status is not None:
            info.update(status=status, found=found, residuals=r["res"][:found].copy())
            return r["s"][:found].copy(), lm.rotate(U[:m], r["Pt"][:found].astype(f32)), lm.rotate(V[:mc], r["Qt"][:found].astype(f32)), info
        keep = lm.keep_of(k, ncv)
        new_u, new_v, last = lm.rotate(U[:m], r["Pt"][:keep].astype(f32)), lm.rotate(V[:m], r["Qt"][:keep].astype(f32)), V[m].copy()
        U[:keep] = new_u
        V[:keep] = new_v
        V[keep] = last
        B[:] = 0
        B[np.arange(keep), np.arange(keep)] = r["s"][:keep]
        j0 = keep


def bsvd_numpy(B, k, beta, tol):
    """prep.bsvd by numpy.linalg.svd: the same order, residual estimates and converged count from an independent SVD"""
    B = np.asarray(B, f64)
    m = B.shape[0]
    P, s, Qt = np.linalg.svd(B, full_matrices=False)
    res = beta * np.abs(P[m - 1, :])
    return {"s": s, "Pt": P.T.copy(), "Qt": Qt.copy(), "res": res, "converged": int((res[:min(k, m)] <= tol * s[0]).sum()), "sweeps": 0}


# ---- the matrices ------------------------------------------------------------------------------------------------------------------
def graded(R, C):
    """A[i][i] = linspace(1, 2, p)[i] ** 6 with p = min(R, C), -0.1 above and 0.05 below the diagonal, float32"""
    import scipy.sparse as sp
    p = min(R, C)
    d = (np.linspace(1.0, 2.0, p) ** 6).astype(f32)
    i = np.arange(p)
    up, lo = i[i + 1 < C], i[i + 1 < R]
    r = np.concatenate([i, up, lo + 1])
    c = np.concatenate([i, up + 1, lo])
    v = np.concatenate([d, np.full(len(up), -0.1, f32), np.full(len(lo), 0.05, f32)]).astype(f32)
    return sp.coo_matrix((v, (r, c)), shape=(R, C))


def rank3(R=200, C=150):
    """L @ R of standard normal factors, float32, every entry stored"""
    import scipy.sparse as sp
    rng = np.random.default_rng(5)
    L, Rm = rng.standard_normal((R, 3)), rng.standard_normal((3, C))
    return sp.coo_matrix((L @ Rm).astype(f32))


def zero_pattern(R=40, C=30):
    """every entry stored, every value an explicit zero"""
    import scipy.sparse as sp
    r, c = np.divmod(np.arange(R * C), C)
    return sp.coo_matrix((np.zeros(R * C, f32), (r, c)), shape=(R, C))


def tile_stream_rectangular(R=20000, C=24000, nnz=35000, seed=78):
    """scattered entries plus a graded diagonal, rectangular: a tile stream under HISPMV_FORMAT=tts"""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    r, c = rng.integers(0, R, nnz), rng.integers(0, C, nnz)
    v = rng.uniform(-0.05, 0.05, nnz).astype(f32)
    S = sp.coo_matrix((v, (r, c)), shape=(R, C)).tocsr()
    return (S + graded(R, C).tocsr()).astype(f32).tocoo()


def dense_rectangular(R=96, C=64, seed=97):
    M = np.random.default_rng(seed).standard_normal((R, C)) / np.sqrt(2.0 * R)
    M[np.arange(C), np.arange(C)] += np.linspace(0.0, 3.0, C)
    return M.astype(f32)


def start(n, seed=1):
    return lm.start(n, seed)


def accuracy(A, s, u, vt, status):
    """(fp64 true residual, singular-value error), both relative to sigma_max: max_i of |A v_i - s_i u_i| and |A^T u_i - s_i v_i|, and
    max_i |s_i - ref_i| against the reference values -- for an INVARIANT run against the nearest one.  The reference: the fp64 SVD of the
    dense matrix up to 1300 on the longer side, above that scipy's svds at tol 1e-12 for two values more than the run returned."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    if max(A.shape) <= 1300:
        A64 = A.astype(f64) if isinstance(A, np.ndarray) else sp.csr_matrix(A).astype(f64).toarray()
        ref = np.linalg.svd(A64, compute_uv=False)
    else:
        A64 = sp.csr_matrix(A).astype(f64)
        ref = np.sort(spl.svds(A64, k=len(s) + 2, tol=1e-12, return_singular_vectors=False, v0=np.ones(min(A.shape))))[::-1]
    scale = ref[0] if ref[0] > 0 else 1.0
    res = err = 0.0
    for i, (si, ui, vi) in enumerate(zip(s, np.asarray(u, f64), np.asarray(vt, f64))):
        res = max(res, float(np.linalg.norm(A64 @ vi - si * ui)), float(np.linalg.norm(A64.T @ ui - si * vi)))
        err = max(err, float(np.abs(ref - si).min()) if status == "INVARIANT" else float(abs(ref[i] - si)))
    return res / scale, err / scale


# The cases: the matrix, k, ncv (tol 1e-5 throughout), the status and `found` the run ends with, `prototype` = the products a plain
# numpy version of the algorithm (fp32 vectors, fp64 dots, CGS2, numpy.linalg.svd) took with the same start vector when the solver was
# designed (a run above twice that means something is wrong), and what THIS model reaches with scipy products
# and prep.bsvd on the CPU: `attained` = (fp64 true residual, singular-value error), both relative to sigma_max; a test's bound is twice
# that.  An attained figure below 1e-7 is recorded as 1e-7: that is one float32 rounding of a vector.
# graded(1, 1), graded(1, 5) and graded(5, 1) at k = 1 freeze after 2, 3 and 2 products with one triplet, m = 1 >= k and residual
# estimates of zero.  One might expect INVARIANT there, as eigsh reports for a 1 x 1 matrix at k = 2; but the STOP rule -- eigsh's:
# CONVERGED when the first min(k, m) pairs are converged and m >= k, and only ELSE invariant -- calls that CONVERGED, as it does for
# graded(2, 3) and graded(3, 2), which freeze the same way at m = k = 2.  k cannot exceed min(rows, cols) = 1 on these shapes, so no
# run on them has m < k.  Where and on which side they freeze is pinned in tests/test_gk_host.py.
TOL = 1e-5
FLOOR = 1e-7


def _case(make, k, ncv, status, found, prototype, attained, gpu=True):
    return dict(make=make, k=k, ncv=ncv, status=status, found=found, prototype=prototype, attained=attained, gpu=gpu)


CASES = {
    "graded_1x1": _case(lambda: graded(1, 1), 1, 2, "CONVERGED", 1, 2, (FLOOR, FLOOR)),
    "graded_1x5": _case(lambda: graded(1, 5), 1, 2, "CONVERGED", 1, 3, (FLOOR, FLOOR)),
    "graded_5x1": _case(lambda: graded(5, 1), 1, 2, "CONVERGED", 1, 2, (FLOOR, FLOOR)),
    "graded_2x3": _case(lambda: graded(2, 3), 2, 64, "CONVERGED", 2, 5, (FLOOR, FLOOR)),
    "graded_3x2": _case(lambda: graded(3, 2), 2, 64, "CONVERGED", 2, 4, (1.50e-7, FLOOR)),
    "graded_63x64": _case(lambda: graded(63, 64), 2, 64, "CONVERGED", 2, 127, (1.16e-7, FLOOR)),
    "graded_64x63": _case(lambda: graded(64, 63), 2, 64, "CONVERGED", 2, 126, (2.39e-7, FLOOR)),
    "graded_65x65": _case(lambda: graded(65, 65), 2, 64, "CONVERGED", 2, 128, (2.41e-7, FLOOR)),
    "graded_255x300": _case(lambda: graded(255, 300), 4, 20, "CONVERGED", 4, 104, (1.84e-7, FLOOR)),
    "graded_300x255": _case(lambda: graded(300, 255), 4, 20, "CONVERGED", 4, 104, (3.29e-7, FLOOR)),
    "graded_1025x700": _case(lambda: graded(1025, 700), 4, 20, "CONVERGED", 4, 152, (4.24e-7, FLOOR)),
    "graded_1025x700_ncv2": _case(lambda: graded(1025, 700), 1, 2, "CONVERGED", 1, 992, (9.94e-6, 2.73e-7)),
    "graded_4099x5000": _case(lambda: graded(4099, 5000), 8, 64, "CONVERGED", 8, 408, (1.47e-6, FLOOR)),
    "graded_5000x4099": _case(lambda: graded(5000, 4099), 8, 24, "CONVERGED", 8, 432, (6.80e-6, 1.37e-7), gpu=False),
    "rank3_k2": _case(rank3, 2, 12, "CONVERGED", 2, 7, (1.31e-6, FLOOR)),
    "rank3_k5": _case(rank3, 5, 12, "INVARIANT", 3, 7, (2.99e-6, FLOOR)),
    "zero_40x30": _case(zero_pattern, 2, 8, "INVARIANT", 0, 1, (FLOOR, FLOOR)),
}
GPU_CASES = [name for name, case in CASES.items() if case["gpu"]]


# The handle kinds of tests/test_gpu_gk.py (k = 4, ncv = 20): the matrix whose singular values the handle has -- for bf16 storage the
# values rounded to bfloat16 -- and what this model attains on it with scipy products and prep.bsvd on the CPU, recorded as above;
# tests/test_gk_host.py runs the model on each and holds it to these figures, tests/test_gpu_gk.py holds the device to twice them.
def bf16_graded(R=1025, C=700):
    import scipy.sparse as sp
    import step_small_cases as S
    A = graded(R, C)
    return sp.coo_matrix((S.bf16_exact(A.data.astype(f32)), (A.row, A.col)), shape=A.shape)


KIND_CASES = {
    "slices_atomic": dict(make=lambda: graded(1025, 700), k=4, ncv=20, attained=(4.24e-7, FLOOR)),
    "tile_stream": dict(make=tile_stream_rectangular, k=4, ncv=20, attained=(6.64e-6, 1.54e-7)),
    "dense_96x64": dict(make=dense_rectangular, k=4, ncv=20, attained=(1.93e-7, FLOOR)),
    "bf16_storage": dict(make=bf16_graded, k=4, ncv=20, attained=(5.78e-6, FLOOR)),
}


def run_model(case, A=None, products=None, bsvd=None):
    """The model on a case with the given product callbacks (default: scipy's) and small SVD (default: prep.bsvd)."""
    from hispmv_amd import prep
    A = case["make"]() if A is None else A
    if isinstance(A, np.ndarray):
        import scipy.sparse as sp
        A = sp.coo_matrix(A)
    prod, prod_t = km.scipy_products(A) if products is None else products
    rows, cols = A.shape
    s, u, vt, info = svds(prod, prod_t, prep.bsvd if bsvd is None else bsvd, start(cols), case["k"], case["ncv"], TOL, max(20 * max(rows, cols), 2000), rows)
    return s, u, vt, info, A
