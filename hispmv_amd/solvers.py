"""Krylov solvers on loaded handles, for torch tensors: ``cg``, ``bicgstab`` and ``cgls`` over FpgaHandle.cg_device /
bicgstab_device / cgls_device (include/hispmv.h: hispmv_cg_device ...).  The products are the launches of spmv_device / spmv_device_t;
everything between two products runs in the library's fused vector kernels with every scalar on the device, and the host looks at the
residual every ``check_every`` iterations only.  There is no torch fallback: the loops exist in the library or not at all.

Streams: the launches go to torch's current stream by its handle.  Inside ``with torch.cuda.stream(torch.cuda.Stream()):`` everything
-- the torch kernels that made b, x0 and minv, the solve, whatever reads x afterwards -- is ordered on one real stream and nothing
waits.  torch's DEFAULT stream has the handle 0, which the library reads as "the context's own stream" (include/hispmv.h: the stream
rule), a stream that is not ordered with torch's kernels on the default stream.  There the solvers order the two themselves: they wait
on the host for the default stream before the first launch (b, x0, minv and the copy of x0 were written there), and a call with
``check_every > 0`` waits for the context's stream before it returns, so the x it returns is ready for torch.  A ``check_every = 0``
call on the default stream returns with the solve in flight on the context's stream: x must not be read, and b and minv not
overwritten, before ``handle.krylov_status(info["work"].data_ptr(), 0)`` or ``handle.synchronize()`` has returned.

Several right-hand sides: ``cg_multi`` and ``bicgstab_multi`` solve the columns of B [n, m] as m independent solves that share their
launches (FpgaHandle.cg_multi_device / bicgstab_multi_device over spmm_device's products); same streams, same rule.

Restarted GMRES: ``gmres`` (FpgaHandle.gmres_device) for square non-symmetric systems, one product per inner iteration.

Block-Jacobi: ``block_jacobi(handle, idx, block_size)`` builds the inverted diagonal blocks of a loaded square handle on the device
(FpgaHandle.block_jacobi_setup_device) and returns an object ``cg`` and ``gmres`` take as ``precond=`` in place of ``minv``; same
streams, same rule.

Eigenvalues: ``eigsh`` (FpgaHandle.eigsh_device) for a few extreme eigenpairs of a symmetric handle by thick-restart Lanczos; its
driver looks at the device once per cycle, so it always returns with its result ready.

Singular values: ``svds`` (FpgaHandle.svds_device) for the k largest singular values of a handle of any shape, with their vectors, by
thick-restart Golub-Kahan bidiagonalisation over spmv_device and spmv_device_t; ``spectral_norm`` is its k = 1.  Same streams as
``eigsh``."""
from __future__ import annotations

import torch


def _vector(t, name: str, n: int):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 1 and t.is_contiguous()):
        raise TypeError(f"{name} must be a contiguous 1-D float32 CUDA tensor")
    if t.numel() != n:
        raise ValueError(f"{name} holds {t.numel()} elements, the handle needs {n}")
    return t


def workspace(handle, idx: int, solver: str, device) -> torch.Tensor:
    """A workspace tensor for `solver` on handle `idx` (krylov_info's work_bytes; torch allocations are 16-byte aligned)."""
    info = handle.krylov_info(idx, solver)
    if not info["accepted"]:
        return torch.empty(0, dtype=torch.uint8, device=device)          # the entry itself says why it refuses
    return torch.empty(info["work_bytes"], dtype=torch.uint8, device=device)


def _launch(handle, device, check_every: int, call):
    """call(stream) on torch's current stream under the stream rule of the module docstring: on the default stream wait for torch
    before the first launch and, where the call itself looks at the result (check_every > 0), for the context's stream behind it."""
    current = torch.cuda.current_stream(device)
    stream = current.cuda_stream
    if stream == 0:          # torch's default stream: the library launches on the context's own stream (module docstring)
        current.synchronize()
    info = call(stream)
    if stream == 0 and check_every > 0:
        handle.synchronize()
    return info


class BlockJacobi:
    """The block-Jacobi preconditioner of handle `idx`: the buffer tensor (``buffer``: the inverted diagonal blocks, then their flags;
    prep.block_jacobi's layout) with ``block_size`` and ``n``.  Made by `block_jacobi`; pass it to `cg` / `gmres` as ``precond=``."""

    def __init__(self, handle, idx: int, block_size: int, device):
        info = handle.block_jacobi_info(idx, block_size)          # a bad block_size or index raises here
        self.handle, self.idx, self.block_size = handle, idx, int(block_size)
        self.n = handle.matrix_info(idx)["rows"]
        # (a handle the setup refuses gets an empty buffer: the entry itself says why it refuses)
        self.buffer = torch.empty(info["pre_bytes"] if info["accepted"] else 0, dtype=torch.uint8, device=device)
        self.refresh()

    def refresh(self) -> "BlockJacobi":
        """A setup again on torch's current stream: after update_values_device the blocks of the new values."""
        _launch(self.handle, self.buffer.device, 1,
                lambda stream: self.handle.block_jacobi_setup_device(self.idx, self.block_size, self.buffer.data_ptr(), self.buffer.numel(), stream))
        return self

    def singular_blocks(self) -> int:
        """Blocks that could not be inverted and were replaced by the identity (waits for the setup)."""
        return _launch(self.handle, self.buffer.device, 0,
                       lambda stream: self.handle.block_jacobi_status(self.buffer.data_ptr(), self.n, self.block_size, stream))

    def apply(self, r):
        """z = M^-1 r as a new tensor, on torch's current stream."""
        r = _vector(r, "r", self.n)
        z = torch.empty_like(r)
        _launch(self.handle, r.device, 1,
                lambda stream: self.handle.block_jacobi_apply_device(self.buffer.data_ptr(), self.n, self.block_size, r.data_ptr(), z.data_ptr(), stream))
        return z


def block_jacobi(handle, idx: int, block_size: int = 8, device=None) -> BlockJacobi:
    """Sets up a block-Jacobi preconditioner for the loaded square handle `idx` on torch's current stream: the diagonal blocks of
    block_size (4, 8, 16 or 32) are extracted from the loaded matrix and inverted on the device; a block that cannot be inverted is
    replaced by the identity (`singular_blocks()` counts them).  Returns the object `cg` and `gmres` take as ``precond=``; after
    update_values_device call its `refresh()`.  A tile-stream handle raises NotImplementedError, a handle that is not square ValueError."""
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return BlockJacobi(handle, idx, block_size, device)


def _precond(precond, minv, n: int):
    if precond is None:
        return None
    if minv is not None:
        raise ValueError("give minv or precond, not both")
    if not isinstance(precond, BlockJacobi):
        raise TypeError("precond must be the object solvers.block_jacobi returns")
    if precond.n != n:
        raise ValueError(f"precond was set up for {precond.n} unknowns, the handle has {n}")
    return precond


def _solve(solver: str, handle, idx: int, b, x0, minv, rtol: float, max_iters, check_every: int, work, precond=None):
    m = handle.matrix_info(idx)
    precond = _precond(precond, minv, m["rows"])
    b = _vector(b, "b", m["rows"])
    x = torch.zeros(m["cols"], dtype=torch.float32, device=b.device) if x0 is None else _vector(x0, "x0", m["cols"]).clone()
    if minv is not None:
        minv = _vector(minv, "minv", m["rows"])
    if max_iters is None:
        max_iters = 2 * max(m["rows"], m["cols"])
    if work is None:
        work = workspace(handle, idx, solver, b.device)

    def call(stream):
        kw = dict(rtol=rtol, max_iters=max_iters, check_every=check_every, work=work.data_ptr(), work_bytes=work.numel() * work.element_size(), stream=stream)
        if solver == "cg" and precond is not None:
            return handle.cg_bj_device(idx, b.data_ptr(), x.data_ptr(), precond.buffer.data_ptr(), precond.block_size, **kw)
        if solver == "cg":
            return handle.cg_device(idx, b.data_ptr(), x.data_ptr(), 0 if minv is None else minv.data_ptr(), **kw)
        if solver == "bicgstab":
            return handle.bicgstab_device(idx, b.data_ptr(), x.data_ptr(), **kw)
        return handle.cgls_device(idx, b.data_ptr(), x.data_ptr(), **kw)
    info = _launch(handle, b.device, check_every, call)
    info["work"] = work          # check_every = 0: handle.krylov_status(info["work"].data_ptr(), stream) reads the outcome
    return x, info


def cg(handle, idx: int, b, x0=None, *, minv=None, rtol: float = 1e-6, max_iters=None, check_every: int = 8, work=None, precond=None):
    """Solves A x = b for the symmetric positive definite handle `idx` by (diagonally preconditioned) CG on torch's current stream.
    b, x0 and minv (the inverse diagonal, optional) are float32 CUDA vectors; returns (x, info) with info = {"status", "iterations",
    "relres", "products", "work"}.  max_iters defaults to twice the dimension; check_every = 0 enqueues exactly max_iters iterations
    and returns without waiting (status "IN_FLIGHT").  precond: the object of `block_jacobi` in place of minv (both: ValueError)."""
    return _solve("cg", handle, idx, b, x0, minv, rtol, max_iters, check_every, work, precond)


def bicgstab(handle, idx: int, b, x0=None, *, rtol: float = 1e-6, max_iters=None, check_every: int = 8, work=None):
    """Solves A x = b for a square, non-symmetric handle by BiCGSTAB (forward products only); arguments and result as `cg`."""
    return _solve("bicgstab", handle, idx, b, x0, None, rtol, max_iters, check_every, work)


def cgls(handle, idx: int, b, x0=None, *, rtol: float = 1e-6, max_iters=None, check_every: int = 8, work=None):
    """min ||b - A x|| for a handle of any shape by CGLS, stopping on ||A^T r|| <= rtol ||A^T b||; the handle must be one spmv_device_t
    accepts (create it under set_transposable(...)); arguments and result as `cg`."""
    return _solve("cgls", handle, idx, b, x0, None, rtol, max_iters, check_every, work)


def workspace_gmres(handle, idx: int, restart: int, with_minv: bool, device) -> torch.Tensor:
    """A workspace tensor for GMRES(restart) on handle `idx` (gmres_info's work_bytes)."""
    info = handle.gmres_info(idx, restart, with_minv)
    return torch.empty(info["work_bytes"] if info["accepted"] else 0, dtype=torch.uint8, device=device)


def gmres(handle, idx: int, b, x0=None, *, minv=None, restart: int = 30, rtol: float = 1e-6, max_iters=None, check_every: int = 8, work=None,
          precond=None):
    """Solves A x = b for a square, non-symmetric handle by restarted GMRES(restart) on torch's current stream: one product per inner
    iteration, the basis orthogonalised by two passes of classical Gram-Schmidt in the library's fused kernels.  minv is an optional
    inverse diagonal used as a right preconditioner; max_iters counts inner iterations (default twice the dimension); result and
    streams as `cg`.  precond: the object of `block_jacobi` in place of minv (both: ValueError)."""
    m = handle.matrix_info(idx)
    precond = _precond(precond, minv, m["rows"])
    b = _vector(b, "b", m["rows"])
    x = torch.zeros(m["cols"], dtype=torch.float32, device=b.device) if x0 is None else _vector(x0, "x0", m["cols"]).clone()
    if minv is not None:
        minv = _vector(minv, "minv", m["rows"])
    if max_iters is None:
        max_iters = 2 * max(m["rows"], m["cols"])
    if work is None:
        work = workspace_gmres(handle, idx, restart, minv is not None or precond is not None, b.device)

    def call(stream):
        if precond is not None:
            return handle.gmres_bj_device(idx, b.data_ptr(), x.data_ptr(), precond.buffer.data_ptr(), precond.block_size, restart=restart, rtol=rtol,
                                          max_iters=max_iters, check_every=check_every, work=work.data_ptr(),
                                          work_bytes=work.numel() * work.element_size(), stream=stream)
        return handle.gmres_device(idx, b.data_ptr(), x.data_ptr(), 0 if minv is None else minv.data_ptr(), restart=restart, rtol=rtol,
                                   max_iters=max_iters, check_every=check_every, work=work.data_ptr(),
                                   work_bytes=work.numel() * work.element_size(), stream=stream)
    info = _launch(handle, b.device, check_every, call)
    info["work"] = work          # check_every = 0: handle.krylov_status(info["work"].data_ptr(), stream) reads the outcome
    return x, info


# ---- eigenvalues -------------------------------------------------------------------------------------------------------------------
def _workspace(info: dict, device) -> torch.Tensor:
    """The workspace tensor an *_info dict asks for; empty for a handle the solver refuses, whose call then says why."""
    return torch.empty(info["work_bytes"] if info["accepted"] else 0, dtype=torch.uint8, device=device)


def _start(v0, n: int, seed: int, k, ncv):
    """(v0, k, ncv) of eigsh and svds with their defaults: v0 = torch.randn from a CPU generator seeded with `seed`, moved to the
    current device; ncv = min(max(2k + 1, 20), 64)."""
    if v0 is None:
        gen = torch.Generator(device="cpu").manual_seed(int(seed))
        v0 = torch.randn(n, generator=gen, dtype=torch.float32).to(torch.device("cuda", torch.cuda.current_device()))
    v0 = _vector(v0, "v0", n)
    k = int(k)
    return v0, k, min(max(2 * k + 1, 20), 64) if ncv is None else ncv


def workspace_eigsh(handle, idx: int, ncv: int, device) -> torch.Tensor:
    """A workspace tensor for a Lanczos run with ncv basis vectors on handle `idx` (lanczos_info's work_bytes)."""
    return _workspace(handle.lanczos_info(idx, ncv), device)


def eigsh(handle, idx: int, k: int = 6, *, which: str = "LA", ncv=None, tol: float = 1e-5, max_products=None, v0=None, seed: int = 0, work=None):
    """The k algebraically largest ("LA"), smallest ("SA") or largest-magnitude ("LM") eigenvalues of the SYMMETRIC handle `idx` and
    their eigenvectors, by thick-restart Lanczos on torch's current stream (FpgaHandle.eigsh_device; the caller owes the symmetry).
    Returns (vals, vecs, info): vals a float64 numpy array [found], vecs a float32 CUDA tensor [n, found] (a transposed view of the
    library's rows), info = {"status", "found", "products", "cycles", "residuals", "work"}; status is "CONVERGED", "MAX_ITERS",
    "INVARIANT" (the Krylov space closed before k pairs converged: found may be below k) or "BREAKDOWN" (found 0).  ncv defaults to
    min(max(2k + 1, 20), 64), max_products to max(10 n, 1000) capped at 2^30, v0 to torch.randn from a generator seeded with `seed`
    (v0 is not written).  The driver looks at the device once per cycle, so the call waits for its result on any stream."""
    m = handle.matrix_info(idx)
    n = m["rows"]
    v0, k, ncv = _start(v0, n, seed, k, ncv)
    if max_products is None:
        max_products = min(max(10 * n, 1000), 1 << 30)
    if work is None:
        work = workspace_eigsh(handle, idx, ncv, v0.device)
    stride = (n + 3) // 4 * 4
    rows = torch.zeros(max(k, 1), stride, dtype=torch.float32, device=v0.device)
    info = _launch(handle, v0.device, 1, lambda stream: handle.eigsh_device(
        idx, k, v0.data_ptr(), rows.data_ptr(), stride, ncv=ncv, which=which, tol=tol, max_products=max_products, work=work.data_ptr(),
        work_bytes=work.numel() * work.element_size(), stream=stream))
    vals = info.pop("vals")
    info.pop("scale")
    info["work"] = work
    return vals, rows[:info["found"], :n].t(), info


# ---- singular values ---------------------------------------------------------------------------------------------------------------
def workspace_svds(handle, idx: int, ncv: int, device) -> torch.Tensor:
    """A workspace tensor for a Golub-Kahan run with ncv basis vectors on handle `idx` (gk_info's work_bytes)."""
    return _workspace(handle.gk_info(idx, ncv), device)


def svds(handle, idx: int, k: int = 6, *, ncv=None, tol: float = 1e-5, max_products=None, v0=None, seed: int = 0, work=None,
         return_vectors: bool = True):
    """The k largest singular values of handle `idx`, of any shape rows x cols, with their singular vectors, by thick-restart
    Golub-Kahan bidiagonalisation on torch's current stream (FpgaHandle.svds_device); the handle must be one spmv_device_t accepts.
    Returns (s, u, vt, info): s a float64 numpy array [found], descending; u a float32 CUDA tensor [rows, found] and vt [found, cols]
    (views of the library's rows; None with return_vectors=False, which skips the two finishing rotations); info = {"status", "found",
    "products", "cycles", "residuals", "scale", "work"}; status as `eigsh`'s.  products counts forward and transposed products together.
    ncv defaults to min(max(2k + 1, 20), 64), max_products to max(20 max(rows, cols), 2000) capped at 2^30, v0 (cols elements, not
    written) to torch.randn from a generator seeded with `seed`.  The call waits for its result on any stream."""
    m = handle.matrix_info(idx)
    rows, cols = m["rows"], m["cols"]
    v0, k, ncv = _start(v0, cols, seed, k, ncv)
    if max_products is None:
        max_products = min(max(20 * max(rows, cols), 2000), 1 << 30)
    if work is None:
        work = workspace_svds(handle, idx, ncv, v0.device)
    ld_u, ld_v = (rows + 3) // 4 * 4, (cols + 3) // 4 * 4
    u = torch.zeros(max(k, 1), ld_u, dtype=torch.float32, device=v0.device) if return_vectors else None
    v = torch.zeros(max(k, 1), ld_v, dtype=torch.float32, device=v0.device) if return_vectors else None
    info = _launch(handle, v0.device, 1, lambda stream: handle.svds_device(
        idx, k, v0.data_ptr(), u.data_ptr() if return_vectors else 0, ld_u, v.data_ptr() if return_vectors else 0, ld_v, ncv=ncv, tol=tol,
        max_products=max_products, work=work.data_ptr(), work_bytes=work.numel() * work.element_size(), stream=stream, vectors=return_vectors))
    s = info.pop("s")
    info["work"] = work
    if not return_vectors:
        return s, None, None, info
    return s, u[:info["found"], :rows].t(), v[:info["found"], :cols], info


def spectral_norm(handle, idx: int, tol: float = 1e-4) -> float:
    """The largest singular value of handle `idx`: svds(k=1) without the vectors.  A run that finds nothing (the all-zero matrix) gives 0."""
    s = svds(handle, idx, 1, tol=tol, return_vectors=False)[0]
    return float(s[0]) if len(s) else 0.0


# ---- several right-hand sides -------------------------------------------------------------------------------------------------------
def _columns(t, name: str, n: int, m=None):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2):
        raise TypeError(f"{name} must be a 2-D float32 CUDA tensor [n, m]")
    if t.shape[0] != n or t.shape[1] < 1 or (m is not None and t.shape[1] != m):
        raise ValueError(f"{name} is {tuple(t.shape)}, the handle needs [{n}, {'m >= 1' if m is None else m}]")
    if t.shape[0] > 1 and (t.stride(1) != 1 or t.stride(0) < t.shape[1]):
        raise ValueError(f"{name} must be row-major: stride(1) == 1 and stride(0) >= m (a narrowed view of a wider tensor is fine)")
    return t


def workspace_multi(handle, idx: int, solver: str, num_vecs: int, device) -> torch.Tensor:
    """A workspace tensor for `solver` with num_vecs right-hand sides on handle `idx` (krylov_multi_info's work_bytes)."""
    info = handle.krylov_multi_info(idx, solver, num_vecs)
    return torch.empty(info["work_bytes"] if info["accepted"] else 0, dtype=torch.uint8, device=device)


def _solve_multi(solver: str, handle, idx: int, B, X0, minv, rtol: float, max_iters, check_every: int, work):
    import numpy as np
    mi = handle.matrix_info(idx)
    n = mi["rows"]
    B = _columns(B, "B", n)
    m = B.shape[1]
    X = torch.zeros(mi["cols"], m, dtype=torch.float32, device=B.device) if X0 is None else _columns(X0, "X0", mi["cols"], m).contiguous().clone()
    if minv is not None:
        minv = _vector(minv, "minv", n)
    if max_iters is None:
        max_iters = 2 * max(mi["rows"], mi["cols"])
    if work is None:
        work = workspace_multi(handle, idx, solver, m, B.device)
    ld_b = B.stride(0) if n > 1 else m

    def call(stream):
        kw = dict(ld_b=ld_b, ld_x=m, rtol=rtol, max_iters=max_iters, check_every=check_every, work=work.data_ptr(),
                  work_bytes=work.numel() * work.element_size(), stream=stream)
        if solver == "cg":
            return handle.cg_multi_device(idx, B.data_ptr(), X.data_ptr(), m, 0 if minv is None else minv.data_ptr(), **kw)
        return handle.bicgstab_multi_device(idx, B.data_ptr(), X.data_ptr(), m, **kw)
    res = _launch(handle, B.device, check_every, call)
    info = {"status": [r["status"] for r in res], "iterations": np.array([r["iterations"] for r in res], np.int32),
            "relres": np.array([r["relres"] for r in res], np.float64), "products": res[0]["products"],
            "work": work}          # check_every = 0: handle.krylov_multi_status(info["work"].data_ptr(), m, stream) reads the outcome
    return X, info


def cg_multi(handle, idx: int, B, X0=None, *, minv=None, rtol: float = 1e-6, max_iters=None, check_every: int = 8, work=None):
    """Solves A x_v = b_v for the m columns of B [n, m] by m independent (diagonally preconditioned) CG solves that share their
    launches, on torch's current stream (FpgaHandle.cg_multi_device): column v is bit for bit what `cg` computes over spmm_device's
    products, with its own iteration count, stopping and breakdown.  B is a float32 CUDA tensor with stride(1) == 1 and stride(0) >= m
    (a narrowed view of a wider tensor is allowed); X0 [n, m] the initial guesses; minv ONE inverse diagonal for all columns.  Returns
    (X, info), X contiguous [n, m], info = {"status": list, "iterations": int array, "relres": float array, "products", "work"}.
    Streams as in the module docstring; a check_every = 0 call is read with handle.krylov_multi_status(info["work"].data_ptr(), m, stream)."""
    return _solve_multi("cg", handle, idx, B, X0, minv, rtol, max_iters, check_every, work)


def bicgstab_multi(handle, idx: int, B, X0=None, *, rtol: float = 1e-6, max_iters=None, check_every: int = 8, work=None):
    """m independent BiCGSTAB solves for a square, non-symmetric handle that share their launches; arguments and result as `cg_multi`."""
    return _solve_multi("bicgstab", handle, idx, B, X0, None, rtol, max_iters, check_every, work)
