"""Solves a generated symmetric positive definite system with CG and a generated least-squares problem with CGLS on loaded handles
(hispmv_amd.solvers), and prints iterations and residuals next to the fp64 residuals computed on the host.  --rhs M also solves the
SPD system for M right-hand sides in one call (solvers.cg_multi) and prints iterations and the true residual of every column.
--gmres also solves a convection-diffusion system on the same grid (Peclet number 1000, strongly non-normal) with restarted GMRES
(solvers.gmres, --restart M) and with BiCGSTAB under the same budget of products, and prints both outcomes.
--block-jacobi BS also sets up a block-Jacobi preconditioner of block size BS (4, 8, 16, 32; solvers.block_jacobi) for the SPD system
and for the convection-diffusion system and prints the iterations of CG and of GMRES without a preconditioner, with the inverse
diagonal and with the blocks.
--eigsh K also computes K extreme eigenvalues (--which LA, SA or LM) of the grid's Laplacian plus a graded diagonal, which keeps its
eigenvalues simple, with thick-restart Lanczos (solvers.eigsh) and prints the values, the fp64 true residuals and the products.
--svds K also computes the K largest singular values of the least-squares matrix with thick-restart Golub-Kahan (solvers.svds) and
prints the values, the fp64 true residuals |A v - s u| and |A^T u - s v|, and the products; the condition number CGLS then meets is
not among them: that needs the smallest singular value, which svds does not compute.

    python examples/solve_check.py [--grid 64] [--rtol 1e-6] [--rhs M] [--gmres [--restart 10]] [--block-jacobi BS] [--eigsh K [--which SA]] [--svds K]
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def laplacian_coo(m):
    """The 5-point Laplacian of an m x m grid as COO triplets."""
    k = np.arange(m * m)
    i, j = k // m, k % m
    r, c, v = [k], [k], [np.full(m * m, 4.0)]
    for ok, off in ((i > 0, -m), (i < m - 1, m), (j > 0, -1), (j < m - 1, 1)):
        r.append(k[ok]); c.append(k[ok] + off); v.append(np.full(int(ok.sum()), -1.0))
    return np.concatenate(r), np.concatenate(c), np.concatenate(v).astype(np.float32)


def convdiff_coo(m, pe=1000.0):
    """Convection-diffusion on an m x m grid by central differences, convection along the fast index, as COO triplets."""
    k = np.arange(m * m)
    i, j = k // m, k % m
    a = pe / (m + 1) / 2
    r, c, v = [k], [k], [np.full(m * m, 4.0)]
    for ok, off, val in ((i > 0, -m, -1.0), (i < m - 1, m, -1.0), (j > 0, -1, -(1 + a)), (j < m - 1, 1, -(1 - a))):
        r.append(k[ok]); c.append(k[ok] + off); v.append(np.full(int(ok.sum()), val))
    return np.concatenate(r), np.concatenate(c), np.concatenate(v).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--rtol", type=float, default=1e-6)
    ap.add_argument("--rhs", type=int, default=0, help="also solve the SPD system for this many right-hand sides in one call")
    ap.add_argument("--gmres", action="store_true", help="also solve a convection-diffusion system with restarted GMRES and with BiCGSTAB")
    ap.add_argument("--restart", type=int, default=10, help="basis vectors of a GMRES cycle, 1 .. 64")
    ap.add_argument("--block-jacobi", type=int, default=0, metavar="BS", help="also solve with a block-Jacobi preconditioner of this block size (4, 8, 16, 32)")
    ap.add_argument("--eigsh", type=int, default=0, metavar="K", help="also compute this many extreme eigenvalues of a symmetric system")
    ap.add_argument("--which", default="LA", choices=("LA", "SA", "LM"), help="which end of the spectrum --eigsh takes")
    ap.add_argument("--svds", type=int, default=0, metavar="K", help="also compute this many of the largest singular values of the least-squares matrix")
    args = ap.parse_args()
    import torch
    import pyhispmv
    from hispmv_amd import solvers

    rng = np.random.default_rng(0)
    n = args.grid * args.grid
    r, c, v = laplacian_coo(args.grid)
    rows, cols, nnz = 3000, 1200, 40000
    lr, lc = rng.integers(0, rows, nnz), rng.integers(0, cols, nnz)
    lv = rng.uniform(-1, 1, nnz).astype(np.float32)

    h = pyhispmv.FpgaHandle("solve.xclbin", 0, 24, 1, 1, 2, 5, True, False, True)
    spd = h.create_sparse_handle(r, c, v, n, n)
    h.set_transposable("companion")          # CGLS multiplies by A^T: a stored transpose keeps that product free of atomics
    ls = h.create_sparse_handle(lr, lc, lv, rows, cols)
    if args.rhs > 0:
        h.set_transposable(True)             # the multi solves run over spmm_device, which takes slice streams: keep that format
        spd_wide = h.create_sparse_handle(r, c, v, n, n)
    if args.gmres:
        gr, gc, gv = convdiff_coo(args.grid)
        cd = h.create_sparse_handle(gr, gc, gv, n, n)
    if args.block_jacobi:
        h.set_transposable(True)             # the extraction walks slice streams: keep that format
        bj_spd = h.create_sparse_handle(r, c, v, n, n)
        gr, gc, gv = convdiff_coo(args.grid)
        bj_cd = h.create_sparse_handle(gr, gc, gv, n, n)
    if args.eigsh:          # a graded diagonal on the Laplacian: the plain grid operator has multiple eigenvalues, of which single-vector
        er = np.concatenate([r, np.arange(n)])          # Lanczos finds one copy each
        ec = np.concatenate([c, np.arange(n)])
        ev = np.concatenate([v, np.linspace(0.0, 4.0, n).astype(np.float32)])
        eig = h.create_sparse_handle(er, ec, ev, n, n)
    h.load_matrices()

    dev = torch.device("cuda", 0)
    b = rng.uniform(-1, 1, n).astype(np.float32)
    x, info = solvers.cg(h, spd, torch.from_numpy(b).to(dev), rtol=args.rtol)
    x64 = x.cpu().numpy().astype(np.float64)
    Ax = np.bincount(r, weights=v.astype(np.float64) * x64[c], minlength=n)
    true = np.linalg.norm(b - Ax) / np.linalg.norm(b)
    print(f"CG    {n} x {n}: {info['status']}, {info['iterations']} iterations, {info['products']} products, "
          f"recursive residual {info['relres']:.3e}, true {true:.3e}")
    assert info["status"] == "CONVERGED" and true < 100 * args.rtol

    if args.rhs > 0:          # smoother columns stop earlier; each column has its own count and is frozen while the others go on
        t = (np.arange(n) + 0.5) / n
        B = np.stack([np.sin(np.pi * (j + 1) * t) if j % 2 else rng.uniform(-1, 1, n) for j in range(args.rhs)], axis=1).astype(np.float32)
        X, info = solvers.cg_multi(h, spd_wide, torch.from_numpy(B).to(dev), rtol=args.rtol)
        X64 = X.cpu().numpy().astype(np.float64)
        print(f"CG    {n} x {n}, {args.rhs} right-hand sides in one call: {info['products']} products")
        for j in range(args.rhs):
            Ax = np.bincount(r, weights=v.astype(np.float64) * X64[c, j], minlength=n)
            true = np.linalg.norm(B[:, j] - Ax) / np.linalg.norm(B[:, j])
            print(f"  column {j:3d}: {info['status'][j]}, {info['iterations'][j]} iterations, recursive residual {info['relres'][j]:.3e}, true {true:.3e}")
            assert info["status"][j] == "CONVERGED"          # (a smooth column's true fp32 residual stalls near cond(A) * 2^-24, above the recursive one)

    if args.gmres:          # one product per inner iteration and a residual that cannot grow inside a cycle, against two products per
        b = rng.uniform(-1, 1, n).astype(np.float32)          # iteration and no such promise
        tb = torch.from_numpy(b).to(dev)
        budget = 20 * args.grid
        for name, (x, info) in (("GMRES", solvers.gmres(h, cd, tb, restart=args.restart, rtol=10 * args.rtol, max_iters=budget)),
                                ("BiCGSTAB", solvers.bicgstab(h, cd, tb, rtol=10 * args.rtol, max_iters=budget // 2))):
            x64 = x.cpu().numpy().astype(np.float64)
            true = np.linalg.norm(b - np.bincount(gr, weights=gv.astype(np.float64) * x64[gc], minlength=n)) / np.linalg.norm(b)
            print(f"{name:8s} {n} x {n}, convection-diffusion: {info['status']}, {info['iterations']} iterations, {info['products']} products, "
                  f"recursive residual {info['relres']:.3e}, true {true:.3e}")
            assert name != "GMRES" or (info["status"] == "CONVERGED" and true < 1000 * args.rtol)

    if args.block_jacobi:          # the blocks follow the fast index of the grid: a block inverts bs coupled unknowns of a grid line at once
        b = rng.uniform(-1, 1, n).astype(np.float32)
        tb = torch.from_numpy(b).to(dev)
        for name, idx, (cr, cc, cv), solve, kw in (("CG", bj_spd, (r, c, v), solvers.cg, dict(rtol=args.rtol)),
                                                   ("GMRES", bj_cd, (gr, gc, gv), solvers.gmres, dict(restart=args.restart, rtol=10 * args.rtol, max_iters=20 * args.grid))):
            pre = solvers.block_jacobi(h, idx, args.block_jacobi)
            minv = torch.full((n,), 0.25, dtype=torch.float32, device=dev)          # both systems have 4 on the diagonal
            print(f"{name} {n} x {n}, block-Jacobi {pre.block_size}: {pre.singular_blocks()} blocks could not be inverted")
            for label, more in (("no preconditioner", {}), ("minv = 1 / diag", dict(minv=minv)), (f"blocks of {pre.block_size}", dict(precond=pre))):
                x, info = solve(h, idx, tb, **kw, **more)
                x64 = x.cpu().numpy().astype(np.float64)
                true = np.linalg.norm(b - np.bincount(cr, weights=cv.astype(np.float64) * x64[cc], minlength=n)) / np.linalg.norm(b)
                print(f"  {label:20s} {info['status']}, {info['iterations']} iterations, recursive residual {info['relres']:.3e}, true {true:.3e}")
            assert info["status"] == "CONVERGED"

    if args.eigsh:
        vals, vecs, info = solvers.eigsh(h, eig, args.eigsh, which=args.which)
        X = vecs.cpu().numpy().astype(np.float64)
        print(f"eigsh {n} x {n}, k = {args.eigsh}, {args.which}: {info['status']}, {info['found']} pairs, {info['products']} products, {info['cycles']} cycles")
        for j in range(info["found"]):
            Ax = np.bincount(er, weights=ev.astype(np.float64) * X[ec, j], minlength=n)
            true = np.linalg.norm(Ax - vals[j] * X[:, j]) / np.linalg.norm(X[:, j])
            print(f"  value {j}: {vals[j]:.9g}, residual estimate {info['residuals'][j]:.3e}, true {true:.3e}")
        assert info["status"] == "CONVERGED"

    if args.svds:          # the stored transpose of `ls` gives both products a fixed order: the run repeats bit for bit
        s, u, vt, info = solvers.svds(h, ls, args.svds)
        U, Vt = u.cpu().numpy().astype(np.float64), vt.cpu().numpy().astype(np.float64)
        print(f"svds  {rows} x {cols}, k = {args.svds}: {info['status']}, {info['found']} triplets, {info['products']} products, {info['cycles']} cycles")
        for j in range(info["found"]):
            Av = np.bincount(lr, weights=lv.astype(np.float64) * Vt[j, lc], minlength=rows)
            Atu = np.bincount(lc, weights=lv.astype(np.float64) * U[lr, j], minlength=cols)
            print(f"  value {j}: {s[j]:.9g}, residual estimate {info['residuals'][j]:.3e}, true |A v - s u| {np.linalg.norm(Av - s[j] * U[:, j]):.3e}, "
                  f"|A^T u - s v| {np.linalg.norm(Atu - s[j] * Vt[j]):.3e}")
        assert info["status"] == "CONVERGED"

    b = rng.uniform(-1, 1, rows).astype(np.float32)
    x, info = solvers.cgls(h, ls, torch.from_numpy(b).to(dev), rtol=args.rtol)
    x64 = x.cpu().numpy().astype(np.float64)
    res = b - np.bincount(lr, weights=lv.astype(np.float64) * x64[lc], minlength=rows)
    atr = np.bincount(lc, weights=lv.astype(np.float64) * res[lr], minlength=cols)
    atb = np.bincount(lc, weights=lv.astype(np.float64) * b.astype(np.float64)[lr], minlength=cols)
    true = np.linalg.norm(atr) / np.linalg.norm(atb)
    print(f"CGLS  {rows} x {cols}: {info['status']}, {info['iterations']} iterations, {info['products']} products, "
          f"|A^T r| / |A^T b| recursive {info['relres']:.3e}, true {true:.3e}, |r| / |b| {np.linalg.norm(res) / np.linalg.norm(b):.3f}")
    assert info["status"] == "CONVERGED" and true < 100 * args.rtol
    h.close()
    print("solve_check ok")


if __name__ == "__main__":
    main()
