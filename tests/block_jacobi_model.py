"""A numpy restatement of the block-Jacobi preconditioner as include/hispmv.h writes it down ("Block-Jacobi preconditioner for CG and
GMRES"): the padded extraction of the diagonal blocks from a scipy matrix, the in-place Gauss-Jordan inversion with partial pivoting
in float32 with its flags, and the multiply z = M^-1 r in float32 with the products added one at a time.  `BlockInverse` multiplies
like an inverse diagonal (``minv * vector``), so krylov_model.cg and gmres_model.gmres run with it unchanged.  Also the multi-dof
system and the case table of the block-Jacobi tests."""
import numpy as np

import gmres_model as gm
import krylov_model as km

f32 = np.float32
SIZES = (4, 8, 16, 32)


def layout(n, bs):
    """{"n_blocks", "pre_bytes", "flags_offset", "block_floats"}: the rule of hispmv_prep_block_jacobi, restated."""
    nb = -(-n // bs)
    off = (nb * bs * bs * 4 + 15) // 16 * 16
    return {"n_blocks": nb, "pre_bytes": (off + nb * 4 + 15) // 16 * 16, "flags_offset": off, "block_floats": bs * bs}


# ---- extraction --------------------------------------------------------------------------------------------------------------------
def extract(A, bs):
    """[n_blocks, bs, bs] float32: the diagonal blocks of A (scipy sparse, or a dense ndarray), duplicates of a COO input summed in
    float32, the last block padded with ones on the diagonal of its absent rows."""
    n = A.shape[0]
    assert A.shape[0] == A.shape[1]
    nb = -(-n // bs)
    out = np.zeros((nb, bs, bs), f32)
    if isinstance(A, np.ndarray):
        r, c = np.nonzero(np.ones_like(A, bool))
        v = np.asarray(A, f32)[r, c]
    else:
        A = A.tocoo()
        r, c, v = A.row.astype(np.int64), A.col.astype(np.int64), A.data.astype(f32)
    keep = (r // bs) == (c // bs)
    np.add.at(out, (r[keep] // bs, r[keep] % bs, c[keep] % bs), v[keep])          # (float32 adds; up to two per position are order-free)
    for i in range(n, nb * bs):
        out[nb - 1, i % bs, i % bs] = 1
    return out


# ---- inversion ---------------------------------------------------------------------------------------------------------------------
def _absbits(x):
    return int(np.asarray(x, f32).view(np.uint32)) & 0x7FFFFFFF


def invert_block(block):
    """(inverse, flag) of one bs x bs float32 block by the rule of include/hispmv.h; flag 1: the identity."""
    a = np.array(block, f32)
    bs = a.shape[0]
    eye = np.eye(bs, dtype=f32)
    used = np.zeros(bs, bool)
    sigma = np.zeros(bs, np.int64)
    with np.errstate(all="ignore"):
        for k in range(bs):
            best, p = -1, -1
            for i in range(bs):          # the largest magnitude by its bits (a NaN counts above Inf), the lowest row on ties
                if not used[i] and _absbits(a[i, k]) > best:
                    best, p = _absbits(a[i, k]), i
            if best == 0 or best >= 0x7F800000:
                return eye, 1
            inv = f32(1.0) / a[p, k]
            w = a[p] * inv
            w[k] = inv
            f = a[:, k].copy()
            a[:, k] = 0
            t = f[:, None] * w[None, :]          # rounded to float32, then subtracted
            rest = a - t
            rest[p] = w
            a = rest
            used[p] = True
            sigma[k] = p
        out = np.zeros_like(a)
        for k in range(bs):
            out[k, sigma] = a[sigma[k]]
    if not np.isfinite(out).all():
        return eye, 1
    return out, 0


def invert(blocks):
    """([n_blocks, bs, bs] inverses, [n_blocks] int32 flags)"""
    inv = np.empty_like(blocks)
    flags = np.zeros(len(blocks), np.int32)
    for k, b in enumerate(blocks):
        inv[k], flags[k] = invert_block(b)
    return inv, flags


def invert_many(blocks):
    """`invert` with every step taken on all blocks at once, for the tens of thousands of blocks of a large system: the same float32
    operations in the same order per block, so the same bits (tests/test_block_jacobi_plans_host.py compares the two).  A block found
    BAD goes on being computed with and is replaced at the end."""
    a = np.array(blocks, f32)
    nb, bs = a.shape[0], a.shape[1]
    if nb == 0:
        return a, np.zeros(0, np.int32)
    b = np.arange(nb)
    used = np.zeros((nb, bs), bool)
    sigma = np.zeros((nb, bs), np.int64)
    bad = np.zeros(nb, bool)
    with np.errstate(all="ignore"):
        for k in range(bs):
            key = (np.ascontiguousarray(a[:, :, k]).view(np.uint32) & 0x7FFFFFFF).astype(np.int64)
            key[used] = -1
            p = key.argmax(axis=1)          # the first of the largest: the lowest row on ties
            best = key[b, p]
            bad |= (best == 0) | (best >= 0x7F800000)
            inv = f32(1.0) / a[b, p, k]
            w = a[b, p, :] * inv[:, None]
            w[:, k] = inv
            f = a[:, :, k].copy()
            a[:, :, k] = 0
            t = f[:, :, None] * w[:, None, :]          # rounded to float32, then subtracted
            a = a - t
            a[b, p, :] = w
            used[b, p] = True
            sigma[:, k] = p
        rows = np.take_along_axis(a, sigma[:, :, None], axis=1)          # rows[., k, j] = a[., sigma[k], j]
        out = np.zeros_like(a)
        np.put_along_axis(out, np.broadcast_to(sigma[:, None, :], a.shape), rows, axis=2)          # out[., k, sigma[j]] = rows[., k, j]
    bad |= ~np.isfinite(out).all(axis=(1, 2))
    out[bad] = np.eye(bs, dtype=f32)
    return out, bad.astype(np.int32)


# ---- the multiply --------------------------------------------------------------------------------------------------------------------
class BlockInverse:
    """M^-1 over the inverted blocks [n_blocks, bs, bs] for n unknowns: ``self * r`` is the multiply of include/hispmv.h."""

    def __init__(self, inv, n, flags=None):
        self.inv, self.n, self.bs = np.asarray(inv, f32), n, inv.shape[1]
        self.flags = flags

    def __mul__(self, r):
        nb, bs = len(self.inv), self.bs
        rp = np.zeros(nb * bs, f32)
        rp[:self.n] = np.asarray(r, f32)
        rp = rp.reshape(nb, bs)
        z = np.zeros((nb, bs), f32)
        with np.errstate(all="ignore"):
            for k in range(bs):          # from +0, the rounded products one at a time, k ascending
                p = self.inv[:, :, k] * rp[:, k:k + 1]
                z = z + p
        return z.reshape(-1)[:self.n].copy()

    __rmul__ = __mul__


def setup(A, bs):
    """The model's preconditioner of A: extraction, inversion, BlockInverse."""
    inv, flags = invert(extract(A, bs))
    return BlockInverse(inv, A.shape[0], flags)


def buffer_bytes(inv, flags):
    """The device buffer that holds these blocks and flags, as uint8."""
    nb, bs = inv.shape[0], inv.shape[1]
    l = layout(nb * bs, bs)
    buf = np.zeros(l["pre_bytes"], np.uint8)
    buf[:nb * bs * bs * 4] = np.ascontiguousarray(inv, f32).view(np.uint8).reshape(-1)
    buf[l["flags_offset"]:l["flags_offset"] + 4 * nb] = np.ascontiguousarray(flags, np.int32).view(np.uint8)
    return buf


# ---- the systems -----------------------------------------------------------------------------------------------------------------------
def multidof(m, bs, seed=7, eps=0.3):
    """m nodes of bs unknowns each: a symmetric positive definite block per node with eigenvalues over three decades in a random
    basis, coupled weakly to the neighbouring nodes.  Scalar Jacobi does nothing for it; the blocks are the whole difficulty."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    blocks = []
    for _ in range(m):
        q, _r = np.linalg.qr(rng.standard_normal((bs, bs)))
        ev = 10.0 ** rng.uniform(0, 3, bs)
        blocks.append(q @ np.diag(ev) @ q.T)
    t = sp.diags([-np.ones(m - 1), np.zeros(m), -np.ones(m - 1)], [-1, 0, 1])
    return (sp.block_diag(blocks) + eps * sp.kron(t, sp.identity(bs))).astype(f32).tocoo()


KINDS = ("dominant", "pivoting", "permutation", "tie", "zero", "twin", "nan", "inf")
BAD_KINDS = ("zero", "twin", "nan", "inf")


def block_of(kind, bs, rng):
    """One bs x bs float32 block of the kind the inversion tests name:
    dominant     random, diagonally dominant
    pivoting     a dominant block with its rows permuted and a zero on the diagonal: no pivot lies where it is needed
    permutation  a permutation matrix: every operation is exact, the inverse is the transpose
    tie          column 0 holds its largest magnitude twice, with opposite signs: the lowest row is the pivot
    zero         all zeros
    twin         two equal rows.  Float32 elimination finds an exact zero pivot only where its arithmetic is exact, so the two rows
                 are the pivot candidates of column 0 with the power of two 16 there and small integers elsewhere: the lower one is
                 the pivot (a tie), the multiples are exact and the other row becomes exactly zero
    nan, inf     a dominant block with one such entry"""
    good = (rng.standard_normal((bs, bs)) + bs * np.eye(bs)).astype(f32)
    if kind == "dominant":
        return good
    if kind == "pivoting":
        b = good[np.roll(np.arange(bs), 1)]
        b[0, 0] = 0
        return b
    if kind == "permutation":
        return np.eye(bs, dtype=f32)[rng.permutation(bs)]
    if kind == "tie":
        good[3, 0] = -good[0, 0]
        return good
    if kind == "zero":
        return np.zeros((bs, bs), f32)
    if kind == "twin":
        b = rng.integers(-3, 4, (bs, bs)).astype(f32) + 8 * np.eye(bs, dtype=f32)
        b[1] = rng.integers(-7, 8, bs)
        b[1, 0] = 16
        b[bs - 1] = b[1]
        return b
    if kind == "nan":
        good[2, 1] = np.nan
        return good
    if kind == "inf":
        good[0, 3] = np.inf
        return good
    raise ValueError(kind)


def zero_block_system(n=64, bs=8):
    """Non-symmetric, non-singular as a whole, its SECOND diagonal block exactly zero: the rows of that block are coupled to the next
    block's columns and the next block's rows to its columns instead, everything else is a dominant band."""
    import scipy.sparse as sp
    A = km.band(n).tolil()
    lo, hi = bs, 2 * bs
    A[lo:hi, lo:hi] = 0
    for i in range(lo, hi):          # rows of the zero block keep a strong entry outside it, columns likewise: a permutation-like coupling
        A[i, i + bs] = 4.5
        A[i + bs, i] = 4.5
        A[i + bs, i + bs] = 0.5
    return sp.coo_matrix(A).astype(f32)


# Convergence cases: the system, the solver, block size, rtol, budget, and what the MODEL reaches with scipy products on the CPU: its
# iterations with minv = 1 / diag and with the blocks, and `attained`, the fp64 true relative residual of the block solve; a device
# test's bound is twice that.  `ratio`: the block solve takes at most that fraction of the minv solve's iterations.
CASES = {
    "cg_multidof_130x8": dict(solver="cg", make=lambda: multidof(130, 8), bs=8, rtol=1e-6, max_iters=600, restart=None, ratio=0.1,
                              minv_iterations=262, iterations=7, attained=4.29e-6),
    "gmres_convdiff_48_pe1000": dict(solver="gmres", make=lambda: gm.convdiff(48, 1000), bs=16, rtol=1e-5, max_iters=400, restart=10, ratio=1.0 / 3.0,
                                     minv_iterations=127, iterations=20, attained=6.17e-6),
}


def run_model(case, precond, A=None, products=None):
    """The model on a case with `precond` ("blocks", "minv" or None) and the given product callbacks (default: scipy's):
    (x, info, A, b)."""
    A = case["make"]() if A is None else A
    b = km.rhs(A.shape[0])
    prod, _ = km.scipy_products(A) if products is None else products
    x0 = np.zeros(A.shape[0], f32)
    m = setup(A, case["bs"]) if precond == "blocks" else (1.0 / A.tocsr().diagonal()).astype(f32) if precond == "minv" else None
    if case["solver"] == "cg":
        x, _r, info = km.cg(prod, b, x0, m, case["rtol"], case["max_iters"])
    else:
        x, _V, info = gm.gmres(prod, b, x0, m, case["rtol"], case["max_iters"], case["restart"])
    return x, info, A, b
