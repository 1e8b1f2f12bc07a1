"""A numpy restatement of thick-restart Lanczos as include/hispmv.h writes it down ("Lanczos / eigsh"): krylov_model's fixed-order fp64
dot product, CGS2 with float32 vector arithmetic (one rounding per operation), fp64 scalars rounded once to float32, the invariant
subspace rule, the host look, the restart and the finish.  The products come from a callback, as in krylov_model: scipy's on the CPU,
spmv_device's own results on the GPU.  The Ritz step is a callback too: the tests pass prep.ritz, the library's own host code, so
lockstep never depends on restating Jacobi here; ritz_numpy is the independent check of that code.  Also the matrices and the case
table of the Lanczos tests."""
import math

import numpy as np

import krylov_model as km

f32 = np.float32
f64 = np.float64
MAX_NCV = 64
HC_LD = 66
TINY2 = f64(2.0) ** -24          # tiny = 2^-12


class Run:
    """The scalar block, Hc and the betas of a run."""

    def __init__(self):
        self.brk = self.inv = False
        self.steps = self.products = 0
        self.Hc = np.zeros((MAX_NCV, HC_LD), f64)
        self.betas = np.zeros(HC_LD, f64)

    @property
    def frozen(self):
        return self.brk or self.inv

    def status(self):
        return {"steps": self.steps, "invariant": self.inv, "breakdown": self.brk, "products": self.products}


def open_run(v0, V, st):
    """slot 0 = v0; (v0, v0) zero or not finite: breakdown; else V_0 = f32(1 / sqrt) * v0"""
    with np.errstate(all="ignore"):
        V[0] = v0
        vv = km.dot(v0, v0)
        if km._bad(vv):
            st.brk = True
        else:
            V[0] = f32(f64(1.0) / np.sqrt(vv)) * v0


def steps(prod, V, j0, j1, st):
    """Steps j0 .. j1 - 1 on the basis V [>= j1 + 1, n] in place.  prod(x, bias, alpha, beta) as in krylov_model; the products of a
    frozen run still land in their slots and are ignored."""
    with np.errstate(all="ignore"):
        for j in range(j0, j1):
            V[j + 1] = prod(V[j], None, 1.0, 0.0)
            if st.frozen:
                continue
            w = V[j + 1].copy()
            h1 = np.array([km.dot(V[i], w) for i in range(j + 1)], f64)
            if not np.all(np.isfinite(h1)):
                st.brk = True
                continue
            for i in range(j + 1):
                t = f32(h1[i]) * V[i]
                w = w - t
            V[j + 1] = w
            h2 = np.array([km.dot(V[i], w) for i in range(j + 1)], f64)
            if not np.all(np.isfinite(h2)):
                st.brk = True
                continue
            for i in range(j + 1):
                t = f32(h2[i]) * V[i]
                w = w - t
            V[j + 1] = w
            h = h1 + h2
            ww = km.dot(w, w)
            if not math.isfinite(ww):
                st.brk = True
                continue
            beta = np.sqrt(ww)
            hsq = f64(0.0)
            for i in range(j + 1):
                sq = h[i] * h[i]
                hsq = hsq + sq
            st.products += 1
            st.steps = j + 1
            st.Hc[j, :j + 1] = h
            st.betas[j] = beta
            if ww <= TINY2 * (ww + hsq):
                st.inv = True
                continue
            V[j + 1] = f32(f64(1.0) / beta) * w


def invariance_ratio(st, j):
    """sqrt(ww / (ww + sum h^2)) of step j: what the rule compares with tiny"""
    ww = st.betas[j] ** 2
    tot = ww + float(np.sum(st.Hc[j, :j + 1] ** 2))
    return math.sqrt(ww / tot) if tot > 0 else 0.0


def rotate(V, Yt):
    """out[c] = sum_i Yt[c, i] * V[i]: float32, the product rounded, then added, i ascending from 0.0f"""
    V = np.asarray(V, f32)
    Yt = np.asarray(Yt, f32)
    out = np.zeros((Yt.shape[0], V.shape[1]), f32)
    for c in range(Yt.shape[0]):
        acc = np.zeros(V.shape[1], f32)
        for i in range(Yt.shape[1]):
            p = Yt[c, i] * V[i]
            acc = acc + p
        out[c] = acc
    return out


def mirror(H, st, j0, m):
    for j in range(j0, m):
        H[:j + 1, j] = st.Hc[j, :j + 1]
        H[j, :j + 1] = st.Hc[j, :j + 1]


def keep_of(k, ncv):
    return min(k + (ncv - k) // 2, ncv - 1)


def eigsh(prod, ritz, v0, k, ncv, which, tol, max_products, trace=None):
    """The driver: (vals [found] float64, vecs [found, n] float32, info).  ritz(H, k, which, beta, tol) -> prep.ritz's dict.
    trace: a list that takes the invariance ratio of every step."""
    n = len(v0)
    V = np.zeros((ncv + 1, n), f32)
    st = Run()
    open_run(np.asarray(v0, f32), V, st)
    H = np.zeros((MAX_NCV, MAX_NCV), f64)
    j0 = cycles = 0
    while True:
        steps(prod, V, j0, ncv, st)
        cycles += 1
        info = {"status": "BREAKDOWN", "found": 0, "products": st.products, "cycles": cycles, "residuals": np.zeros(0, f64), "scale": 0.0}
        if st.brk:
            return np.zeros(0, f64), np.zeros((0, n), f32), info
        m = st.steps
        if trace is not None:
            trace.extend((j, invariance_ratio(st, j), st.inv and j == m - 1) for j in range(j0, m))
        mirror(H, st, j0, m)
        r = ritz(H[:m, :m].copy(), k, which, st.betas[m - 1], tol)
        found = min(k, m)
        info["scale"] = float(np.abs(r["theta"]).max())
        status = None
        if r["converged"] == found and m >= k:
            status = "CONVERGED"
        elif st.inv:
            status = "INVARIANT"
        elif st.products >= max_products:
            status = "MAX_ITERS"
        if status is not None:
            info.update(status=status, found=found, residuals=r["res"][:found].copy())
            return r["theta"][:found].copy(), rotate(V[:m], r["Yt"][:found].astype(f32)), info
        keep = keep_of(k, ncv)
        new = rotate(V[:m], r["Yt"][:keep].astype(f32))
        last = V[m].copy()
        V[:keep] = new
        V[keep] = last
        H[:] = 0
        H[np.arange(keep), np.arange(keep)] = r["theta"][:keep]
        j0 = keep


def order_of(theta, which):
    key = {"LA": -theta, "SA": theta, "LM": -np.abs(theta)}[which]
    return np.argsort(key, kind="stable")


def ritz_numpy(H, k, which, beta, tol):
    """prep.ritz by numpy.linalg.eigh: the same order, residual estimates and converged count from an independent eigensolver"""
    H = np.asarray(H, f64)
    m = H.shape[0]
    theta, Y = np.linalg.eigh((np.triu(H) + np.triu(H, 1).T))
    o = order_of(theta, which)
    theta, Yt = theta[o], Y[:, o].T.copy()
    res = beta * np.abs(Yt[:, m - 1])
    scale = np.abs(theta).max()
    return {"theta": theta, "Yt": Yt, "res": res, "converged": int((res[:min(k, m)] <= tol * scale).sum()), "sweeps": 0}


# ---- the matrices ------------------------------------------------------------------------------------------------------------------
def ramp(n, shift=0.0):
    """diag(linspace(1, 2, n) ** 6 + shift) + tridiag(-0.1, 0, -0.1) in float32: both ends of the spectrum are well separated"""
    import scipy.sparse as sp
    d = (np.linspace(1.0, 2.0, n) ** 6 + shift).astype(f32)
    off = np.full(max(n - 1, 0), -0.1, f32)
    return sp.diags([off, d, off], [-1, 0, 1], shape=(n, n), format="coo", dtype=f32)


def tile_stream_symmetric(n=20000, nnz=35000, seed=78):
    """S + S^T of scattered entries plus a graded diagonal: a tile stream under HISPMV_FORMAT=tts"""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    r, c = rng.integers(0, n, nnz), rng.integers(0, n, nnz)
    v = rng.uniform(-0.05, 0.05, nnz).astype(f32)
    S = sp.coo_matrix((v, (r, c)), shape=(n, n)).tocsr()
    d = (np.linspace(1.0, 2.0, n) ** 6).astype(f32)
    return (S + S.T + sp.diags(d)).astype(f32).tocoo()


def dense_symmetric(n=96, seed=97):
    M = np.random.default_rng(seed).standard_normal((n, n))
    return ((M + M.T) / np.sqrt(2.0 * n) + np.diag(np.linspace(0.0, 3.0, n))).astype(f32)


def start(n, seed=1):
    return np.random.default_rng(seed).standard_normal(n).astype(f32)


def reference_values(A, k, which):
    """The reference spectrum: (the values in the order of `which`, every value known): eigvalsh of the dense fp64 matrix for
    n <= 1200, otherwise scipy's eigsh at tol 1e-12 from both ends."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    n = A.shape[0]
    if n <= 1200:
        full = np.linalg.eigvalsh(A.astype(f64) if isinstance(A, np.ndarray) else A.toarray().astype(f64))
        return full[order_of(full, which)], full
    A64 = sp.csr_matrix(A).astype(f64)
    kk = min(max(k, 1) + 1, n - 2)
    ends = [spl.eigsh(A64, k=kk, which=w, tol=1e-12, return_eigenvectors=False, v0=np.ones(n)) for w in ("LA", "SA")]
    both = np.concatenate(ends)
    cand = both if which == "LM" else ends[0] if which == "LA" else ends[1]
    return cand[order_of(cand, which)], both


def accuracy(A, vals, vecs, k, which, status):
    """(fp64 true residual, eigenvalue error), both relative to max |reference|: max_i |A x_i - theta_i x_i| / |x_i|, and
    max_i |theta_i - ref_i| against the ordered reference -- for an INVARIANT run against the nearest reference value: such a run
    returns eigenvalues, but not necessarily the first ones."""
    import scipy.sparse as sp
    ordered, every = reference_values(A, k, which)
    scale = np.abs(every).max()
    A64 = A.astype(f64) if isinstance(A, np.ndarray) else sp.csr_matrix(A).astype(f64)
    res = err = 0.0
    for i, (t, x) in enumerate(zip(vals, np.asarray(vecs, f64))):
        res = max(res, float(np.linalg.norm(A64 @ x - t * x) / np.linalg.norm(x)))
        err = max(err, float(np.abs(every - t).min()) if status == "INVARIANT" else float(abs(ordered[i] - t)))
    return res / scale, err / scale


# The cases: the matrix, k, ncv, which (tol 1e-5 throughout), the status and `found` the run ends with, `prototype` = the products of
# the algorithm's first numpy prototype (a run above twice that means something is wrong; the shifted ramp had none, its count is this
# model's), and what the model reaches with scipy
# products and prep.ritz on the CPU: `attained` = (fp64 true residual, eigenvalue error), both relative to the spectral radius; a
# test's bound is twice that.  An attained figure below 1e-7 is recorded as 1e-7: that is one float32 rounding of a vector.
TOL = 1e-5
FLOOR = 1e-7


def _case(make, k, ncv, which, status, found, prototype, attained):
    return dict(make=make, k=k, ncv=ncv, which=which, status=status, found=found, prototype=prototype, attained=attained)


CASES = {}
for _w in ("LA", "SA"):
    CASES[f"tridiag_1_{_w}"] = _case(lambda: km.tridiag(1), 2, 64, _w, "INVARIANT", 1, 1, (FLOOR, FLOOR))
    for _n in (2, 3, 63, 64):
        CASES[f"tridiag_{_n}_{_w}"] = _case(lambda n=_n: km.tridiag(n), 2, 64, _w, "CONVERGED", 2, _n, (1.53e-7, FLOOR))
    CASES[f"tridiag_65_{_w}"] = _case(lambda: km.tridiag(65), 2, 64, _w, "CONVERGED", 2, 95, (1.90e-7, FLOOR))
CASES.update({
    "ramp_255_LA": _case(lambda: ramp(255), 4, 20, "LA", "CONVERGED", 4, 60, (4.70e-7, FLOOR)),
    "ramp_255_SA": _case(lambda: ramp(255), 4, 20, "SA", "CONVERGED", 4, 292, (6.73e-6, FLOOR)),
    "ramp_1025_LA": _case(lambda: ramp(1025), 4, 20, "LA", "CONVERGED", 4, 124, (6.64e-6, FLOOR)),
    "ramp_1025_ncv2": _case(lambda: ramp(1025), 1, 2, "LA", "CONVERGED", 1, 848, (9.93e-6, FLOOR)),
    "ramp_4099_k8": _case(lambda: ramp(4099), 8, 64, "LA", "CONVERGED", 8, 288, (6.80e-6, FLOOR)),
    "ramp_4099_k31": _case(lambda: ramp(4099), 31, 64, "LA", "CONVERGED", 31, 472, (7.52e-6, FLOOR)),
    "arrow_5000_k2": _case(lambda: km.arrow(5000), 2, 12, "LA", "CONVERGED", 2, 3, (3.84e-6, 1.42e-6)),
    "arrow_5000_k4": _case(lambda: km.arrow(5000), 4, 12, "LA", "INVARIANT", 3, 3, (3.84e-6, 1.42e-6)),
    "ramp_255_shifted_LM": _case(lambda: ramp(255, shift=-20.0), 4, 20, "LM", "CONVERGED", 4, 68, (6.62e-7, FLOOR)),
})
GPU_CASES = [name for name in CASES if name != "ramp_4099_k31"]


def run_model(case, A=None, products=None, ritz=None, trace=None):
    """The model on a case with the given product callback (default: scipy's) and Ritz step (default: prep.ritz)."""
    from hispmv_amd import prep
    A = case["make"]() if A is None else A
    prod = km.scipy_products(A)[0] if products is None else products
    n = A.shape[0]
    vals, vecs, info = eigsh(prod, prep.ritz if ritz is None else ritz, start(n), case["k"], case["ncv"], case["which"], TOL, max(10 * n, 1000), trace)
    return vals, vecs, info, A
