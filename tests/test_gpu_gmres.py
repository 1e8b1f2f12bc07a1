"""Restarted GMRES(m) on the device (include/hispmv.h: hispmv_dot_basis_device, hispmv_gmres_device, hispmv_gmres_info) against the
numpy model of tests/gmres_model.py.

  dot_basis   every value bit-equal to the model's dot product of that pair, for every k around the tile, ld and alignment
  lockstep    status, iterations, relres, products, x and the basis of the last cycle bit for bit the model's, the model driven by the
              products spmv_device itself returns
  convergence CONVERGED, the fp64 true residual under twice what the model attains on the CPU (gm.CASES), iterations the model's
  freeze      the same x bits, iterations and relres for every check_every; a second status read gives the same answer
  breakdown   all-zero values, a NaN in b: BREAKDOWN, x bit-equal to the last applied iterate
  refusals    before any launch, x untouched
"""
import numpy as np
import pytest
import scipy.sparse as sp

import gmres_model as gm
import krylov_model as km
import step_small_cases as S
from hispmv_amd import prep
from step_small_harness import HW, SHARED

pytestmark = pytest.mark.gpu

f32 = np.float32
TILE = prep.gmres(1024, 30)["dot_tile"]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


class Ctx:
    """One context with the given matrices (scipy COO, or a dense ndarray) loaded: the pattern of test_gpu_krylov.py."""

    def __init__(self, torch, mats, env=S.SLICES, storage="fp32"):
        import pyhispmv
        self.torch, self.mats = torch, mats
        self.dev = torch.device("cuda", 0)
        with S.environment(dict(SHARED, **env)):
            self.h = pyhispmv.FpgaHandle(*HW)
            try:
                self.h.set_value_storage(storage)
                self.idx = []
                for A in mats:
                    if isinstance(A, np.ndarray):
                        self.idx.append(self.h.create_dense_handle(A.flatten(), *A.shape))
                    else:
                        A = A.tocoo()
                        self.idx.append(self.h.create_sparse_handle(A.row, A.col, A.data.astype(f32), *A.shape))
                    assert self.idx[-1] >= 0
                self.h.load_matrices()
            except BaseException:
                self.h.close()
                raise

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.torch.cuda.synchronize()
        self.h.close()

    def device(self, a, shift=0):
        """a on the device, `shift` floats off the 16-byte alignment of its allocation"""
        t = self.torch.empty(len(a) + shift + 4, dtype=self.torch.float32, device=self.dev)
        t[shift:shift + len(a)] = self.torch.from_numpy(np.ascontiguousarray(a, f32))
        return t[shift:shift + len(a)]

    def products(self, k):
        """The model's callback over the library's own products on matrix k."""
        rows = self.mats[k].shape[0]

        def prod(x, bias, alpha, beta):
            dx = self.device(x)
            db = self.device(bias) if bias is not None else None
            dy = self.device(np.full(rows, np.nan, f32))
            self.torch.cuda.synchronize()          # the context's stream does not wait for torch's
            self.h.spmv_device(self.idx[k], dx.data_ptr(), db.data_ptr() if db is not None else 0, dy.data_ptr(), alpha, beta)
            self.h.synchronize()
            return dy.cpu().numpy()
        return prod, None

    def solve(self, k, b, x0, minv=None, restart=30, rtol=1e-6, max_iters=10, check_every=0, shift=0, stream=0, twice=False):
        """One solve -> (x, V, info), V the restart + 1 basis slots of the workspace; check_every = 0 reads the outcome with
        krylov_status (twice: and reads it again)."""
        torch = self.torch
        n = len(b)
        gi = self.h.gmres_info(self.idx[k], restart, minv is not None)
        assert gi["accepted"] and gi["n"] == n and gi["stride"] == (n + 3) // 4 * 4 and gi["products_per_iteration"] == 1, gi
        assert gi["work_bytes"] == prep.gmres(n, restart, minv is not None)["work_bytes"]
        work = torch.zeros(gi["work_bytes"], dtype=torch.uint8, device=self.dev)
        db, dx = self.device(b, shift), self.device(x0, shift)
        dm = self.device(minv, shift) if minv is not None else None
        torch.cuda.synchronize()
        info = self.h.gmres_device(self.idx[k], db.data_ptr(), dx.data_ptr(), dm.data_ptr() if dm is not None else 0, restart=restart, rtol=rtol,
                                   max_iters=max_iters, check_every=check_every, work=work.data_ptr(), work_bytes=gi["work_bytes"], stream=stream)
        if check_every == 0:
            assert info["status"] == "IN_FLIGHT" and info["products"] == -(-max_iters // restart) + max_iters, info
            info = self.h.krylov_status(work.data_ptr(), stream)
            if twice:
                assert self.h.krylov_status(work.data_ptr(), stream) == info
        torch.cuda.synchronize()
        V = work[gi["v_offset"]:gi["v_offset"] + 4 * gi["stride"] * (restart + 1)].cpu().numpy().view(f32).reshape(restart + 1, gi["stride"])
        return dx.cpu().numpy(), V[:, :n], info


# ---- dot_basis_device --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dot_ctx(torch_mod):
    with Ctx(torch_mod, [km.tridiag(8)]) as cx:
        yield cx


KS = sorted({1, 2, TILE - 1, TILE, TILE + 1, 64, 65} - {0})


@pytest.mark.parametrize("n", (1, 3, 64, 255, 1023, 1024, 1025, 4099, 1024 * 1024 + 1029))
def test_dot_basis_device(torch_mod, dot_ctx, n):
    torch, cx = torch_mod, dot_ctx
    rng = np.random.default_rng(n)
    V = rng.standard_normal((65, n), dtype=f32)
    w = rng.standard_normal(n, dtype=f32)
    want = np.array([km.dot(V[i], w) for i in range(65)], np.float64)          # once per n: a value does not depend on k, ld or alignment
    stride, groups = (n + 3) // 4 * 4, km.groups(n)
    work = torch.zeros(8 * 65 * groups + 32, dtype=torch.uint8, device=cx.dev)
    out = torch.empty(65, dtype=torch.float64, device=cx.dev)
    # (ld, floats V and w are off the 16-byte alignment); ld = stride + 1: the vectors take turns at being 16-byte aligned
    layouts = ((stride, 0, 0), (stride + 1, 1, 0), (stride + 4, 0, 1), (stride, 1, 1))
    for ld, sv, sw in layouts[:2] if n > 1 << 20 else layouts:
        host = np.full(65 * ld, np.nan, f32)          # the pads between two vectors are never read
        for i in range(65):
            host[i * ld:i * ld + n] = V[i]
        dV, dw = cx.device(host, sv), cx.device(w, sw)
        for k in KS:
            out.fill_(float("nan"))
            torch.cuda.synchronize()
            cx.h.dot_basis_device(n, k, dV.data_ptr(), dw.data_ptr(), out.data_ptr(), work.data_ptr(), 8 * k * groups, ld_v=ld)
            cx.h.synchronize()
            got = out.cpu().numpy()
            assert np.array_equal(got[:k].view(np.uint64), want[:k].view(np.uint64)), (n, k, ld, sv, sw, got[:k], want[:k])
            assert np.isnan(got[k:]).all()
    args = (dV.data_ptr(), dw.data_ptr(), out.data_ptr())
    with pytest.raises(ValueError):
        cx.h.dot_basis_device(n, 3, *args, work.data_ptr(), 8 * 3 * groups - 8, ld_v=stride)
    with pytest.raises(ValueError):
        cx.h.dot_basis_device(n, 3, *args, work.data_ptr() + 8, work.numel() - 8, ld_v=stride)
    with pytest.raises(ValueError):
        cx.h.dot_basis_device(n, 66, *args, work.data_ptr(), work.numel() + (1 << 20), ld_v=stride)
    with pytest.raises(ValueError):
        cx.h.dot_basis_device(n, 0, *args, work.data_ptr(), work.numel(), ld_v=stride)


# ---- lockstep ------------------------------------------------------------------------------------------------------------------------
# (max_iters, restart, floats by which b, x and minv are off the 16-byte alignment): one column; two cycles of one column; a short last
# cycle; three cycles, the last of one column; one open cycle; a pass over more basis vectors than one tile of the multi-dot kernel
RUNS = ((1, 1, 0), (2, 1, 1), (3, 2, 0), (7, 3, 1), (7, 30, 0), (TILE + 2, 64, 0))


def lockstep(cx, k, precond, seed=1):
    n = cx.mats[k].shape[0]
    rng = np.random.default_rng(seed + n)
    b = rng.uniform(-1, 1, n).astype(f32)
    x0 = rng.uniform(-1, 1, n).astype(f32)
    minv = rng.uniform(0.3, 0.5, n).astype(f32) if precond else None
    prod, _ = cx.products(k)
    for iters, restart, shift in RUNS:
        x, V, info = cx.solve(k, b, x0, minv, restart=restart, rtol=1e-6, max_iters=iters, check_every=0, shift=shift)
        mx, mV, minfo = gm.gmres(prod, b, x0, minv, 1e-6, iters, restart)
        tag = (precond, n, iters, restart, shift)
        assert info["status"] == minfo["status"] and info["iterations"] == minfo["iterations"] and info["products"] == minfo["products"], (tag, info, minfo)
        assert info["relres"] == minfo["relres"] or (np.isnan(info["relres"]) and np.isnan(minfo["relres"])), (tag, info, minfo)
        assert np.array_equal(bits(x), bits(mx)), (tag, "x", int((bits(x) != bits(mx)).sum()))
        for i in range(len(mV)):
            assert np.array_equal(bits(V[i]), bits(mV[i])), (tag, "basis vector", i, int((bits(V[i]) != bits(mV[i])).sum()))


@pytest.fixture(scope="module")
def lock_ctx(torch_mod):
    with Ctx(torch_mod, [km.band(n) for n in km.TRIDIAG_SIZES] + [km.arrow(5000)]) as cx:
        yield cx


@pytest.mark.parametrize("precond", [False, True], ids=["plain", "minv"])
@pytest.mark.parametrize("k", range(len(km.TRIDIAG_SIZES)), ids=[str(n) for n in km.TRIDIAG_SIZES])
def test_lockstep_band(lock_ctx, k, precond):
    lockstep(lock_ctx, k, precond)


@pytest.mark.parametrize("precond", [False, True], ids=["plain", "minv"])
def test_lockstep_arrow_whose_first_row_is_cut_by_five_slices(lock_ctx, precond):
    k = len(km.TRIDIAG_SIZES)
    assert lock_ctx.h.matrix_info(lock_ctx.idx[k])["n_split_rows"] >= 1
    lockstep(lock_ctx, k, precond)


# ---- convergence -----------------------------------------------------------------------------------------------------------------------
def converge(cx, k, case, A_true=None):
    """The case on matrix k: CONVERGED within the budget, the fp64 true residual under twice the recorded one, iterations the lockstep
    model's."""
    A = cx.mats[k] if A_true is None else A_true
    n = A.shape[0]
    b, x0 = km.rhs(n), np.zeros(n, f32)
    diag = A.diagonal() if isinstance(A, np.ndarray) else A.tocsr().diagonal()
    minv = (1.0 / diag).astype(f32) if case["precond"] else None
    x, V, info = cx.solve(k, b, x0, minv, restart=case["restart"], rtol=case["rtol"], max_iters=case["max_iters"], check_every=8)
    mx, mV, minfo = gm.gmres(cx.products(k)[0], b, x0, minv, case["rtol"], case["max_iters"], case["restart"])
    res = km.true_relres(sp.coo_matrix(A), x, b)
    print(f"{info}, model {minfo}, true relative residual {res:.3e}, recorded on the CPU {case['attained']:.3e}")
    assert info["status"] == "CONVERGED" and info["iterations"] <= case["max_iters"], info
    assert info["iterations"] == minfo["iterations"] and info["relres"] == minfo["relres"], (info, minfo)
    assert np.array_equal(bits(x), bits(mx))
    assert info["relres"] <= case["rtol"]
    assert res <= 2 * case["attained"], (res, case["attained"])
    return info


@pytest.mark.parametrize("name", sorted(gm.CASES))
def test_convergence(torch_mod, name):
    case = gm.CASES[name]
    with Ctx(torch_mod, [case["make"]()]) as cx:
        info = converge(cx, 0, case)
        if name == "convdiff_48_pe1000":          # where BiCGSTAB ends MAX_ITERS at 600 (test_gmres_host.py)
            assert info["iterations"] <= 200


# Handle kinds, built like the KINDS of test_gpu_krylov.py.  attained: the model with scipy products on the CPU, as in gm.CASES.
def _tile_stream_system():
    """20 000 x 20 000, 70 000 scattered entries and a dominant diagonal: a tile stream under HISPMV_FORMAT=tts, not symmetric."""
    rng = np.random.default_rng(77)
    n, nnz = 20000, 70000
    r, c = rng.integers(0, n, nnz), rng.integers(0, n, nnz)
    v = rng.uniform(-0.5, 0.5, nnz).astype(f32)
    i = np.arange(n)
    return sp.coo_matrix((np.concatenate([v, np.full(n, 4.0, f32)]), (np.concatenate([r, i]), np.concatenate([c, i]))), shape=(n, n))


def _dense_nonsymmetric(n=96):
    M = np.random.default_rng(96).standard_normal((n, n))
    return (M / np.sqrt(n) * 0.5 + 2.0 * np.eye(n)).astype(f32)


def _bf16_system(n=1025):
    return km.tridiag(n, lo=-1.37, d=2.53, up=-0.77)


def _stray_split_system():
    m = S.stray_split_band()
    n = m["rows"]
    i = np.arange(n)
    return sp.coo_matrix((np.concatenate([m["v"], np.full(n, 60.0, f32)]), (np.concatenate([m["r"], i]), np.concatenate([m["c"], i]))), shape=(n, n))


ATT_TILE, ATT_DENSE, ATT_BF16, ATT_STRAY = 7.97e-7, 6.82e-7, 7.26e-7, 4.02e-7
KINDS = {
    "tile_stream": dict(make=_tile_stream_system, env=S.TTS, restart=30, rtol=1e-6, max_iters=60, precond=False, attained=ATT_TILE),
    "dense_96": dict(make=_dense_nonsymmetric, env=S.SLICES, restart=20, rtol=1e-6, max_iters=100, precond=False, attained=ATT_DENSE),
    "bf16_storage": dict(make=_bf16_system, env=S.SLICES, restart=30, rtol=1e-6, max_iters=100, precond=True, storage="bf16", attained=ATT_BF16),
    "stray_split": dict(make=_stray_split_system, env=S.SLICES, restart=10, rtol=1e-6, max_iters=60, precond=False, attained=ATT_STRAY),
}


def kind_system(kind):
    """(what the handle is created from, the system it then holds: bf16 storage holds the rounded values)"""
    A = KINDS[kind]["make"]()
    if kind != "bf16_storage":
        return A, A
    return A, sp.coo_matrix((S.bf16_exact(A.data.astype(f32)), (A.row, A.col)), shape=A.shape)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_handle_kinds(torch_mod, kind):
    case = KINDS[kind]
    A, A_true = kind_system(kind)
    with Ctx(torch_mod, [A], env=case["env"], storage=case.get("storage", "fp32")) as cx:
        info = cx.h.matrix_info(cx.idx[0])
        if kind == "tile_stream":
            assert info["format"] == 1, info
        elif kind == "dense_96":
            assert info["is_dense"] and not np.array_equal(A, A.T), info
        elif kind == "bf16_storage":
            assert cx.h.value_storage_info(cx.idx[0])["storage"] == "bf16" and (A_true.data != A.data).any()
        else:
            assert info["tile_kind"] == 3 and info["col_tiles"] == 2, info
        converge(cx, 0, case, A_true=A_true)


# ---- freeze, breakdown, refusals -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", ["converges_inside_a_cycle", "max_iters_in_a_short_last_cycle"])
def test_freeze_gives_the_same_answer_for_every_check_every(torch_mod, run):
    A = km.band(4099)
    b, x0 = km.rhs(4099), np.zeros(4099, f32)
    restart, rtol, max_iters = (5, 1e-6, 150) if run == "converges_inside_a_cycle" else (3, 0.0, 7)
    with Ctx(torch_mod, [A]) as cx:
        runs = [cx.solve(0, b, x0, restart=restart, rtol=rtol, max_iters=max_iters, check_every=ce, twice=True) for ce in (1, 7, 10 ** 6, 0)]
        x, V, info = runs[0]
        if run == "converges_inside_a_cycle":          # 11 = 5 + 5 + 1: the first column of the third cycle
            assert info["status"] == "CONVERGED" and info["iterations"] == 11, info
            assert info["products"] == 3 + 11          # check_every = 1 stops at once
            assert km.true_relres(A, x, b) < 10 * rtol
        else:                                         # cycles of 3, 3 and 1 columns
            assert info["status"] == "MAX_ITERS" and info["iterations"] == 7, info
            assert info["relres"] < 1.0 and km.true_relres(A, x, b) < 1.0          # x0 = 0 starts at 1, and GMRES's residual never grows
        assert runs[3][2]["products"] == -(-max_iters // restart) + max_iters          # check_every = 0 enqueues them all
        for xo, Vo, io in runs[1:]:
            assert np.array_equal(bits(xo), bits(x))
            assert (io["status"], io["iterations"], io["relres"]) == (info["status"], info["iterations"], info["relres"]), (io, info)


def test_breakdown_leaves_the_last_applied_iterate(torch_mod):
    b, x0 = km.rhs(300), km.rhs(300, seed=2)
    nan_b = b.copy()
    nan_b[7] = np.nan
    with Ctx(torch_mod, [km.zero_pattern(300), km.band(300)]) as cx:
        for k, rhs in ((0, b), (1, nan_b)):          # all-zero values: d = 0 in the first column; a NaN in b: (b, b) is not finite
            for ce in (0, 1):
                x, V, info = cx.solve(k, rhs, x0, restart=3, max_iters=5, check_every=ce)
                assert info["status"] == "BREAKDOWN" and info["iterations"] == 0, (k, ce, info)
                assert np.array_equal(bits(x), bits(x0)) and np.isfinite(x).all(), (k, ce)
        for ce in (0, 1):          # b == 0: x = 0, converged, no iteration -- and no product where the host looks
            x, V, info = cx.solve(1, np.zeros(300, f32), x0, restart=3, max_iters=5, check_every=ce)
            assert info["status"] == "CONVERGED" and info["iterations"] == 0 and not x.any(), info
            assert info["products"] == (7 if ce == 0 else 0)
        # an Inf among the values met in the second cycle: the first cycle's three columns stay applied
        prod, _ = cx.products(1)
        big = b.copy()
        big[5] = f32(3e38)
        x, V, info = cx.solve(1, big, x0, restart=3, max_iters=9, check_every=0)
        mx, mV, minfo = gm.gmres(prod, big, x0, None, 1e-6, 9, 3)
        assert (info["status"], info["iterations"]) == (minfo["status"], minfo["iterations"]), (info, minfo)
        assert np.array_equal(bits(x), bits(mx))


def test_refusals_come_before_any_launch(torch_mod):
    torch = torch_mod
    tall = km.least_squares(300, 200)
    b300 = km.rhs(300)
    with Ctx(torch, [tall, km.band(300)]) as cx:
        assert not cx.h.gmres_info(cx.idx[0], 30)["accepted"]
        with pytest.raises(ValueError):
            cx.h.gmres_info(cx.idx[1], 0)
        with pytest.raises(ValueError):
            cx.h.gmres_info(cx.idx[1], 65)
        with pytest.raises(IndexError):
            cx.h.gmres_info(99, 30)
        need = cx.h.gmres_info(cx.idx[1], 64, True)["work_bytes"]
        work = torch.zeros(need + 64, dtype=torch.uint8, device=cx.dev)
        db, dx = cx.device(b300), cx.device(b300)
        with pytest.raises(ValueError, match="square"):
            cx.h.gmres_device(cx.idx[0], db.data_ptr(), dx.data_ptr(), work=work.data_ptr(), work_bytes=work.numel())
        need = cx.h.gmres_info(cx.idx[1], 30)["work_bytes"]
        assert need < cx.h.gmres_info(cx.idx[1], 30, True)["work_bytes"] < cx.h.gmres_info(cx.idx[1], 31, True)["work_bytes"]
        ok = dict(work=work.data_ptr(), work_bytes=need)
        for kw in (dict(ok, restart=0), dict(ok, restart=65), dict(work=work.data_ptr(), work_bytes=need - 1), dict(work=0, work_bytes=need),
                   dict(work=work.data_ptr() + 4, work_bytes=need), dict(ok, d_minv=db.data_ptr()), dict(ok, rtol=-1.0), dict(ok, max_iters=0),
                   dict(ok, check_every=-1)):          # d_minv: the preconditioned solve needs one vector more
            with pytest.raises(ValueError):
                cx.h.gmres_device(cx.idx[1], db.data_ptr(), dx.data_ptr(), **kw)
        with pytest.raises(IndexError):
            cx.h.gmres_device(99, db.data_ptr(), dx.data_ptr(), **ok)
        torch.cuda.synchronize()
        assert np.array_equal(bits(dx.cpu().numpy()), bits(b300))


def test_refused_before_load_matrices(torch_mod):
    import pyhispmv
    A = km.band(64)
    h = pyhispmv.FpgaHandle(*HW)
    try:
        i = h.create_sparse_handle(A.row, A.col, A.data, 64, 64)
        d = torch_mod.zeros(1 << 20, dtype=torch_mod.float32, device="cuda")
        assert not h.gmres_info(i, 30)["accepted"]
        with pytest.raises(AssertionError, match="before load_matrices"):
            h.gmres_device(i, d.data_ptr(), d.data_ptr() + 1024, work=d.data_ptr() + 4096, work_bytes=(4 << 20) - 4096)
    finally:
        h.close()


# ---- hispmv_amd.solvers.gmres ------------------------------------------------------------------------------------------------------------
def test_torch_front_end_on_a_side_stream_and_on_the_default_stream(torch_mod):
    """The answer of the device entry by another door: on a side stream everything is ordered there; on torch's default stream (the
    handle 0, which the library reads as the context's own stream) solvers.gmres orders the two itself, also for operands still queued
    behind a long kernel, for check_every > 0 and for check_every = 0 (x ready after krylov_status on stream 0)."""
    from hispmv_amd import solvers
    torch = torch_mod
    case = gm.CASES["tridiag_4099_minv"]
    A = case["make"]()
    n = A.shape[0]
    bn, x0n = km.rhs(n), km.rhs(n, seed=4)
    minvn = (1.0 / A.tocsr().diagonal()).astype(f32)
    kw = dict(restart=case["restart"], rtol=case["rtol"], max_iters=case["max_iters"])
    with Ctx(torch, [A]) as cx:
        want, _, winfo = cx.solve(0, bn, x0n, minvn, check_every=8, **kw)
        assert winfo["status"] == "CONVERGED"
        tb, tx, tm = (torch.from_numpy(a).to(cx.dev) for a in (bn, x0n, minvn))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            x, info = solvers.gmres(cx.h, cx.idx[0], tb, tx, minv=tm, **kw)
        side.synchronize()
        assert (info["status"], info["iterations"], info["relres"]) == (winfo["status"], winfo["iterations"], winfo["relres"]), (info, winfo)
        assert np.array_equal(bits(x.cpu().numpy()), bits(want))
        assert torch.cuda.current_stream().cuda_stream == 0
        long = torch.ones(1 << 26, dtype=torch.float32, device=cx.dev)
        for check_every in (8, 0):
            torch.cuda.synchronize()
            for _ in range(4):          # some milliseconds of work on the default stream, and the operands queued behind it
                long = long.sin()
            b, x0, minv = tb * 2.0 - tb, tx + 0.0, tm * 1.0
            x, info = solvers.gmres(cx.h, cx.idx[0], b, x0, minv=minv, check_every=check_every, **kw)
            if check_every == 0:
                assert info["status"] == "IN_FLIGHT"
                info = cx.h.krylov_status(info["work"].data_ptr(), 0)
            assert (info["status"], info["iterations"], info["relres"]) == (winfo["status"], winfo["iterations"], winfo["relres"]), (check_every, info, winfo)
            assert np.array_equal(bits(x.cpu().numpy()), bits(want)), check_every
            assert np.array_equal(bits(x0.cpu().numpy()), bits(x0n))          # the caller's x0 is not written
        with pytest.raises(TypeError):
            solvers.gmres(cx.h, cx.idx[0], tb.double())
        with pytest.raises(ValueError):
            solvers.gmres(cx.h, cx.idx[0], tb[:-1].contiguous())
