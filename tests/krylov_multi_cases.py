"""The right-hand sides the multi-right-hand-side Krylov tests share (tests/test_krylov_multi_host.py, tests/test_gpu_krylov_multi.py):
six columns on km.tridiag(4099) that stop at different iterations -- so a batch of them has columns frozen while others go on -- and
two that never iterate."""
import numpy as np

import krylov_model as km

f32 = np.float32
N = 4099
RTOL, MAX_ITERS = 1e-6, 150
NAMES = ("rhs1", "e0", "A1", "sin", "zero", "nan")


def columns(n=N):
    """[n, 6] float32: rhs(seed 1), e0, A * 1, sin(pi i / n), zero, rhs(seed 3) with one NaN -- slowest first among the four that
    iterate."""
    A = km.tridiag(n).tocsr().astype(f32)
    e0 = np.zeros(n, f32)
    e0[0] = 1
    bad = km.rhs(n, seed=3)
    bad[n // 2] = np.nan
    cols = [km.rhs(n, seed=1), e0, (A @ np.ones(n, f32)).astype(f32), np.sin(np.pi * np.arange(n) / n).astype(f32), np.zeros(n, f32), bad]
    return np.ascontiguousarray(np.stack(cols, axis=1), f32)


def run_models(prod, B, x0=None, solver="cg", minv=None, rtol=RTOL, max_iters=MAX_ITERS):
    """The single-vector model on every column of B with the product callback `prod`: a list of (x, r, info)."""
    out = []
    for v in range(B.shape[1]):
        b = np.ascontiguousarray(B[:, v])
        x = np.zeros(B.shape[0], f32) if x0 is None else np.ascontiguousarray(x0[:, v])
        out.append(km.cg(prod, b, x, minv, rtol, max_iters) if solver == "cg" else km.bicgstab(prod, b, x, rtol, max_iters))
    return out
