"""The Krylov layer on the device (include/hispmv.h: hispmv_dot_device, hispmv_cg_device, hispmv_bicgstab_device, hispmv_cgls_device,
hispmv_krylov_status) against the numpy model of tests/krylov_model.py.

  dot         bit-equal to the model's order, within the bound of any order of the exact sum, the same on every stream and call
  lockstep    x and the workspace's r after K iterations (check_every = 0) bit for bit the model's, the model driven by the products
              spmv_device / spmv_device_t themselves return -- so the layer adds nothing to the products but what the header says
  convergence CONVERGED, the fp64 true residual under twice what the model attains on the CPU (the table), iterations the model's
  freeze      the same x bits, iterations and relres for every check_every
  breakdown   an all-zero matrix: BREAKDOWN, x bit-equal to x0
  refusals    before any launch, x untouched
"""
import math

import numpy as np
import pytest
import scipy.sparse as sp

import krylov_model as km
import step_small_cases as S
from step_small_harness import HW, SHARED

pytestmark = pytest.mark.gpu

f32 = np.float32


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


class Ctx:
    """One context with the given matrices (scipy COO, or a dense ndarray) loaded."""

    def __init__(self, torch, mats, env=S.SLICES, transposable=None, storage="fp32"):
        import pyhispmv
        self.torch, self.mats = torch, mats
        self.dev = torch.device("cuda", 0)
        with S.environment(dict(SHARED, **env)):
            self.h = pyhispmv.FpgaHandle(*HW)
            try:
                if transposable is not None:
                    self.h.set_transposable(transposable)
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
        """The model's callbacks over the library's own products on matrix k."""
        rows, cols = self.mats[k].shape

        def prod(x, bias, alpha, beta):
            dx = self.device(x)
            db = self.device(bias) if bias is not None else None
            dy = self.device(np.full(rows, np.nan, f32))
            self.torch.cuda.synchronize()          # the context's stream does not wait for torch's
            self.h.spmv_device(self.idx[k], dx.data_ptr(), db.data_ptr() if db is not None else 0, dy.data_ptr(), alpha, beta)
            self.h.synchronize()
            return dy.cpu().numpy()

        def prod_t(x):
            dx = self.device(x)
            dy = self.device(np.full(cols, np.nan, f32))
            self.torch.cuda.synchronize()
            self.h.spmv_device_t(self.idx[k], dx.data_ptr(), 0, dy.data_ptr(), 1.0, 0.0)
            self.h.synchronize()
            return dy.cpu().numpy()
        return prod, prod_t

    def solve(self, k, solver, b, x0, minv=None, rtol=1e-6, max_iters=10, check_every=0, shift=0, stream=0):
        """One solve -> (x, r, info); check_every = 0 reads the outcome with krylov_status."""
        torch = self.torch
        ki = self.h.krylov_info(self.idx[k], solver)
        assert ki["accepted"] and ki["x_len"] == len(x0) and ki["b_len"] == len(b), ki
        work = torch.zeros(ki["work_bytes"], dtype=torch.uint8, device=self.dev)
        db, dx = self.device(b, shift), self.device(x0, shift)
        dm = self.device(minv, shift) if minv is not None else None
        torch.cuda.synchronize()
        kw = dict(rtol=rtol, max_iters=max_iters, check_every=check_every, work=work.data_ptr(), work_bytes=ki["work_bytes"], stream=stream)
        if solver == "cg":
            info = self.h.cg_device(self.idx[k], db.data_ptr(), dx.data_ptr(), dm.data_ptr() if dm is not None else 0, **kw)
        elif solver == "bicgstab":
            info = self.h.bicgstab_device(self.idx[k], db.data_ptr(), dx.data_ptr(), **kw)
        else:
            info = self.h.cgls_device(self.idx[k], db.data_ptr(), dx.data_ptr(), **kw)
        if check_every == 0:
            assert info["status"] == "IN_FLIGHT", info
            info = self.h.krylov_status(work.data_ptr(), stream)
        torch.cuda.synchronize()
        r = work[ki["r_offset"]:ki["r_offset"] + 4 * len(b)].cpu().numpy().view(f32)
        return dx.cpu().numpy(), r, info


def model(cx, k, solver, b, x0, minv, rtol, max_iters):
    prod, prod_t = cx.products(k)
    if solver == "cg":
        return km.cg(prod, b, x0, minv, rtol, max_iters)
    if solver == "bicgstab":
        return km.bicgstab(prod, b, x0, rtol, max_iters)
    return km.cgls(prod, prod_t, b, x0, rtol, max_iters)


# ---- dot_device ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dot_ctx(torch_mod):
    with Ctx(torch_mod, [km.tridiag(8)]) as cx:
        yield cx


@pytest.mark.parametrize("n", km.DOT_SIZES)
def test_dot_device(torch_mod, dot_ctx, n):
    torch, cx = torch_mod, dot_ctx
    rng = np.random.default_rng(n)
    a, b = rng.standard_normal(n).astype(f32), rng.standard_normal(n).astype(f32)
    exact = (a.astype(np.float64) * b.astype(np.float64)).tolist()
    want = float(km.dot(a, b))
    bound = (n - 1) * 2.0 ** -53 * math.fsum(abs(t) for t in exact)
    assert abs(want - math.fsum(exact)) <= bound
    work = torch.zeros(8 * 1024, dtype=torch.uint8, device=cx.dev)
    out = torch.full((4,), float("nan"), dtype=torch.float64, device=cx.dev)
    side = torch.cuda.Stream()
    got = []
    for sa, sb in ((0, 0), (1, 0), (0, 1), (1, 1)):          # operands 0 or 4 bytes off the 16-byte alignment
        da, db = cx.device(a, sa), cx.device(b, sb)
        torch.cuda.synchronize()
        for j, stream in enumerate((0, 0, side.cuda_stream)):          # the context's stream, again, a torch stream
            cx.h.dot_device(n, da.data_ptr(), db.data_ptr(), out.data_ptr() + 8 * j, work.data_ptr(), work.numel(), stream)
            cx.h.synchronize()
            side.synchronize()
        got.append(out[:3].cpu().numpy().copy())
    got = np.concatenate(got)
    print(f"n={n}: device {got[0]!r}, model {want!r}, fsum {math.fsum(exact)!r}, bound {bound:.3e}")
    assert (got.view(np.uint64) == np.float64(want).view(np.uint64)).all(), (got, want)
    assert abs(float(got[0]) - math.fsum(exact)) <= bound
    with pytest.raises(ValueError):
        cx.h.dot_device(n, da.data_ptr(), db.data_ptr(), out.data_ptr(), work.data_ptr(), 8 * km.groups(n) - 8, 0)
    with pytest.raises(ValueError):
        cx.h.dot_device(n, da.data_ptr(), db.data_ptr(), out.data_ptr(), work.data_ptr() + 4, work.numel() - 4, 0)


# ---- lockstep --------------------------------------------------------------------------------------------------------------------------
RUNS = ((1, 0), (2, 1), (7, 0), (7, 1))          # (iterations, floats by which b, x and minv are off the 16-byte alignment)


def lockstep(cx, k, solver, precond=False, seed=1):
    rows, cols = cx.mats[k].shape
    rng = np.random.default_rng(seed + rows)
    b = rng.uniform(-1, 1, rows).astype(f32)
    x0 = rng.uniform(-1, 1, cols).astype(f32)
    minv = rng.uniform(0.3, 0.5, rows).astype(f32) if precond else None
    for iters, shift in RUNS:
        x, r, info = cx.solve(k, solver, b, x0, minv, rtol=1e-6, max_iters=iters, check_every=0, shift=shift)
        mx, mr, minfo = model(cx, k, solver, b, x0, minv, 1e-6, iters)
        tag = (solver, precond, rows, iters, shift)
        assert info["status"] == minfo["status"] and info["iterations"] == minfo["iterations"] and info["products"] == minfo["products"], (tag, info, minfo)
        assert info["relres"] == minfo["relres"], (tag, info, minfo)
        assert np.array_equal(bits(x), bits(mx)), (tag, "x", int((bits(x) != bits(mx)).sum()))
        assert np.array_equal(bits(r), bits(mr)), (tag, "r", int((bits(r) != bits(mr)).sum()))


@pytest.fixture(scope="module")
def lock_ctx(torch_mod):
    mats = [km.tridiag(n) for n in km.TRIDIAG_SIZES] + [km.band(n) for n in km.TRIDIAG_SIZES] + [km.arrow(5000)]
    with Ctx(torch_mod, mats) as cx:
        yield cx


@pytest.mark.parametrize("k", range(len(km.TRIDIAG_SIZES)), ids=[str(n) for n in km.TRIDIAG_SIZES])
def test_lockstep_cg_tridiag(lock_ctx, k):
    lockstep(lock_ctx, k, "cg")
    lockstep(lock_ctx, k, "cg", precond=True)


@pytest.mark.parametrize("k", range(len(km.TRIDIAG_SIZES)), ids=[str(n) for n in km.TRIDIAG_SIZES])
def test_lockstep_bicgstab_band(lock_ctx, k):
    lockstep(lock_ctx, len(km.TRIDIAG_SIZES) + k, "bicgstab")


def test_lockstep_arrow_whose_first_row_is_cut_by_five_slices(lock_ctx):
    k = 2 * len(km.TRIDIAG_SIZES)
    info = lock_ctx.h.matrix_info(lock_ctx.idx[k])
    assert info["n_split_rows"] >= 1, info
    lockstep(lock_ctx, k, "cg")
    lockstep(lock_ctx, k, "cg", precond=True)
    lockstep(lock_ctx, k, "bicgstab")


def test_lockstep_cgls_over_a_stored_transpose(torch_mod):
    with Ctx(torch_mod, [km.least_squares(300, 200)], transposable="companion") as cx:
        assert cx.h.companion_info(cx.idx[0])["has"]
        ki = cx.h.krylov_info(cx.idx[0], "cgls")
        assert (ki["launches_per_iteration"], ki["products_per_iteration"], ki["products_t_per_iteration"]) == (4, 1, 1)
        lockstep(cx, 0, "cgls")


# ---- convergence -----------------------------------------------------------------------------------------------------------------------
def converge(cx, k, case, A_true=None):
    """The case on matrix k: CONVERGED, the fp64 true residual under twice the recorded one, iterations the lockstep model's."""
    A = cx.mats[k] if A_true is None else A_true
    b = km.rhs(A.shape[0])
    x0 = np.zeros(A.shape[1], f32)
    diag = A.diagonal() if isinstance(A, np.ndarray) else A.tocsr().diagonal()
    minv = (1.0 / diag).astype(f32) if case["precond"] else None
    x, r, info = cx.solve(k, case["solver"], b, x0, minv, rtol=case["rtol"], max_iters=case["max_iters"], check_every=8)
    mx, mr, minfo = model(cx, k, case["solver"], b, x0, minv, case["rtol"], case["max_iters"])
    A_sp = sp.coo_matrix(A)
    res = km.residual_of(case, A_sp, x, b)
    print(f"{info}, model {minfo}, true relative residual {res:.3e}, recorded on the CPU {case['attained']:.3e}")
    assert info["status"] == "CONVERGED", info
    assert info["iterations"] == minfo["iterations"] and info["relres"] == minfo["relres"], (info, minfo)
    assert info["relres"] <= case["rtol"]
    if case.get("bound", True):
        assert res <= 2 * case["attained"], (res, case["attained"])
    return x, info


@pytest.mark.parametrize("name", [n for n in sorted(km.CASES) if km.CASES[n]["solver"] != "cgls"])
def test_convergence(torch_mod, name):
    case = km.CASES[name]
    with Ctx(torch_mod, [case["make"]()]) as cx:
        converge(cx, 0, case)


def test_convergence_cgls_stored_transpose(torch_mod):
    case = km.CASES["cgls_300x200"]
    with Ctx(torch_mod, [case["make"]()], transposable="companion") as cx:
        converge(cx, 0, case)


def test_cgls_over_the_atomic_transposed_path(torch_mod):
    """set_transposable(True): the transposed product adds through float atomics, so no bit claims -- converged, and the residual of
    the normal equations under twice the CPU model's."""
    case = km.CASES["cgls_300x200"]
    A = case["make"]()
    b = km.rhs(300)
    with Ctx(torch_mod, [A], transposable=True) as cx:
        assert cx.h.transpose_info(cx.idx[0])["transposable"] and not cx.h.companion_info(cx.idx[0])["has"]
        x, r, info = cx.solve(0, "cgls", b, np.zeros(200, f32), rtol=case["rtol"], max_iters=case["max_iters"], check_every=8)
        res = km.normal_relres(A, x, b)
        print(f"{info}, normal-equation residual {res:.3e}, recorded on the CPU {case['attained']:.3e}")
        assert info["status"] == "CONVERGED" and info["relres"] <= case["rtol"], info
        assert res <= 2 * case["attained"]


# Handle kinds.  attained: the model with scipy products on the CPU, as in km.CASES.
def _tile_stream_system():
    """20 000 x 20 000, 70 000 scattered entries and a dominant diagonal: a tile stream under HISPMV_FORMAT=tts, not symmetric."""
    rng = np.random.default_rng(77)
    n, nnz = 20000, 70000
    r, c = rng.integers(0, n, nnz), rng.integers(0, n, nnz)
    v = rng.uniform(-0.5, 0.5, nnz).astype(f32)
    i = np.arange(n)
    return sp.coo_matrix((np.concatenate([v, np.full(n, 4.0, f32)]), (np.concatenate([r, i]), np.concatenate([c, i]))), shape=(n, n))


def _dense_spd(n=96):
    M = np.random.default_rng(96).standard_normal((n, n))
    return (M @ M.T / n + np.eye(n)).astype(f32)


def _bf16_system(n=1025):
    return km.tridiag(n, lo=-1.07, d=2.53, up=-1.07)


def _stray_split_system():
    """The stray-split band of the small-case generators (values in [-0.5, 0.5), 200 per row) with a dominant diagonal added as
    further entries of the same positions: not symmetric, so BiCGSTAB."""
    m = S.stray_split_band()
    n = m["rows"]
    i = np.arange(n)
    return sp.coo_matrix((np.concatenate([m["v"], np.full(n, 60.0, f32)]), (np.concatenate([m["r"], i]), np.concatenate([m["c"], i]))), shape=(n, n))


KINDS = {
    "tile_stream": dict(solver="bicgstab", make=_tile_stream_system, env=S.TTS, rtol=1e-6, max_iters=60, precond=False, attained=3.3e-7),
    "dense_spd_96": dict(solver="cg", make=_dense_spd, env=S.SLICES, rtol=1e-6, max_iters=200, precond=False, attained=4.8e-7),
    "bf16_storage": dict(solver="cg", make=_bf16_system, env=S.SLICES, rtol=1e-6, max_iters=100, precond=False, storage="bf16", attained=1.0e-6),
    "stray_split": dict(solver="bicgstab", make=_stray_split_system, env=S.SLICES, rtol=1e-6, max_iters=60, precond=False, attained=3.7e-7),
}


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_handle_kinds(torch_mod, kind):
    case = KINDS[kind]
    A = case["make"]()
    with Ctx(torch_mod, [A], env=case["env"], storage=case.get("storage", "fp32")) as cx:
        info = cx.h.matrix_info(cx.idx[0])
        A_true = A
        if kind == "tile_stream":
            assert info["format"] == 1, info
        elif kind == "dense_spd_96":
            assert info["is_dense"], info
        elif kind == "bf16_storage":          # the handle holds the rounded values: that system is the one solved
            assert cx.h.value_storage_info(cx.idx[0])["storage"] == "bf16"
            A_true = sp.coo_matrix((S.bf16_exact(A.data.astype(f32)), (A.row, A.col)), shape=A.shape)
            assert (A_true.data != A.data).any()
        else:
            assert info["tile_kind"] == 3 and info["col_tiles"] == 2, info
        converge(cx, 0, case, A_true=A_true)


# ---- freeze, breakdown, refusals -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["cg", "bicgstab", "cgls"])
def test_freeze_gives_the_same_answer_for_every_check_every(torch_mod, solver):
    A = {"cg": km.tridiag(4099), "bicgstab": km.band(4099), "cgls": km.least_squares(300, 200)}[solver]
    rtol = 1e-5 if solver == "cgls" else 1e-6
    b, x0 = km.rhs(A.shape[0]), np.zeros(A.shape[1], f32)
    with Ctx(torch_mod, [A], transposable="companion" if solver == "cgls" else None) as cx:
        runs = [cx.solve(0, solver, b, x0, rtol=rtol, max_iters=150, check_every=ce) for ce in (1, 7, 10 ** 6, 0)]
        x, r, info = runs[0]
        assert info["status"] == "CONVERGED" and 0 < info["iterations"] < 75, info
        for xo, ro, io in runs[1:]:
            assert np.array_equal(bits(xo), bits(x)) and np.array_equal(bits(ro), bits(r))
            assert (io["status"], io["iterations"], io["relres"]) == (info["status"], info["iterations"], info["relres"]), (io, info)
        per = cx.h.krylov_info(cx.idx[0], solver)
        per = per["products_per_iteration"] + per["products_t_per_iteration"]
        first = 3 if solver == "cgls" else 1
        assert runs[0][2]["products"] == first + per * info["iterations"]          # check_every = 1 stops at once
        assert runs[3][2]["products"] == first + per * 150                            # check_every = 0 enqueues them all


def test_breakdown_on_all_zero_values(torch_mod):
    A = km.zero_pattern(300)
    b, x0 = km.rhs(300), km.rhs(300, seed=2)
    with Ctx(torch_mod, [A], transposable=True) as cx:
        for solver in ("cg", "bicgstab", "cgls"):
            for ce in (0, 1):
                x, r, info = cx.solve(0, solver, b, x0, max_iters=5, check_every=ce)
                assert info["status"] == "BREAKDOWN" and info["iterations"] == 0, (solver, ce, info)
                assert np.array_equal(bits(x), bits(x0)), (solver, ce)
        for ce in (0, 1):          # b == 0: x = 0, converged, no iteration -- and no product where the host looks
            x, r, info = cx.solve(0, "cg", np.zeros(300, f32), x0, max_iters=5, check_every=ce)
            assert info["status"] == "CONVERGED" and info["iterations"] == 0 and not x.any(), info
            assert info["products"] == (6 if ce == 0 else 0)


def test_refusals_come_before_any_launch(torch_mod):
    torch = torch_mod
    tall = km.least_squares(300, 200)
    b300, x200 = km.rhs(300), km.rhs(200, seed=2)
    ts = S.tile_stream()
    ts = sp.coo_matrix((ts["v"], (ts["r"], ts["c"])), shape=(ts["rows"], ts["cols"]))
    with Ctx(torch, [ts, tall, km.tridiag(300)], env=S.AUTO) as cx:
        assert cx.h.matrix_info(cx.idx[0])["format"] == 1
        assert not cx.h.krylov_info(cx.idx[0], "cgls")["accepted"] and not cx.h.krylov_info(cx.idx[1], "cg")["accepted"]
        work = torch.zeros(cx.h.krylov_info(cx.idx[2], "bicgstab")["work_bytes"] + (4 << 20), dtype=torch.uint8, device=cx.dev)
        m = cx.mats[0]
        db, dx = cx.device(km.rhs(m.shape[0])), cx.device(km.rhs(m.shape[1], seed=2))
        before = dx.cpu().numpy().copy()
        with pytest.raises(NotImplementedError, match="set_transposable"):          # the message of spmv_device_t
            cx.h.cgls_device(cx.idx[0], db.data_ptr(), dx.data_ptr(), work=work.data_ptr(), work_bytes=work.numel())
        torch.cuda.synchronize()
        assert np.array_equal(bits(dx.cpu().numpy()), bits(before))
        db, dx = cx.device(b300), cx.device(x200)
        with pytest.raises(ValueError, match="square"):
            cx.h.cg_device(cx.idx[1], db.data_ptr(), dx.data_ptr(), work=work.data_ptr(), work_bytes=work.numel())
        with pytest.raises(ValueError, match="square"):
            cx.h.bicgstab_device(cx.idx[1], db.data_ptr(), dx.data_ptr(), work=work.data_ptr(), work_bytes=work.numel())
        dx = cx.device(b300)
        need = cx.h.krylov_info(cx.idx[2], "cg")["work_bytes"]
        for kw in (dict(work=work.data_ptr(), work_bytes=need - 1), dict(work=0, work_bytes=need), dict(work=work.data_ptr() + 4, work_bytes=need),
                   dict(work=work.data_ptr(), work_bytes=need, rtol=-1.0), dict(work=work.data_ptr(), work_bytes=need, max_iters=0),
                   dict(work=work.data_ptr(), work_bytes=need, check_every=-1)):
            for call in (cx.h.cg_device, cx.h.bicgstab_device):
                with pytest.raises(ValueError):
                    call(cx.idx[2], db.data_ptr(), dx.data_ptr(), **kw)
        with pytest.raises(IndexError):
            cx.h.cg_device(99, db.data_ptr(), dx.data_ptr(), work=work.data_ptr(), work_bytes=need)
        torch.cuda.synchronize()
        assert np.array_equal(bits(dx.cpu().numpy()), bits(b300))


def test_refused_before_load_matrices(torch_mod):
    import pyhispmv
    A = km.tridiag(64)
    h = pyhispmv.FpgaHandle(*HW)
    try:
        i = h.create_sparse_handle(A.row, A.col, A.data, 64, 64)
        d = torch_mod.zeros(1 << 20, dtype=torch_mod.float32, device="cuda")
        assert not h.krylov_info(i, "cg")["accepted"]
        for call in (h.cg_device, h.bicgstab_device, h.cgls_device):
            with pytest.raises(AssertionError, match="before load_matrices"):
                call(i, d.data_ptr(), d.data_ptr() + 1024, work=d.data_ptr() + 4096, work_bytes=(4 << 20) - 4096)
    finally:
        h.close()


def test_torch_front_end(torch_mod):
    """hispmv_amd.solvers on torch tensors and torch's current stream: the answer of the device entry, by another door."""
    from hispmv_amd import solvers
    torch = torch_mod
    case = km.CASES["cg_laplacian_48"]
    A = case["make"]()
    b = km.rhs(A.shape[0])
    with Ctx(torch, [A]) as cx:
        want, _, winfo = cx.solve(0, "cg", b, np.zeros(A.shape[1], f32), rtol=case["rtol"], max_iters=case["max_iters"], check_every=8)
        side = torch.cuda.Stream()
        tb = torch.from_numpy(b).to(cx.dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            x, info = solvers.cg(cx.h, cx.idx[0], tb, rtol=case["rtol"], max_iters=case["max_iters"])
        side.synchronize()
        assert info["status"] == "CONVERGED" and info["iterations"] == winfo["iterations"] and info["relres"] == winfo["relres"]
        assert np.array_equal(bits(x.cpu().numpy()), bits(want))
        with pytest.raises(TypeError):
            solvers.cg(cx.h, cx.idx[0], tb.double())
        with pytest.raises(ValueError):
            solvers.bicgstab(cx.h, cx.idx[0], tb[:-1].contiguous())


def test_torch_front_end_on_the_default_stream(torch_mod):
    """torch's default stream has the handle 0, which the library reads as the context's own stream -- not ordered with torch's
    kernels.  solvers.* order the two themselves there: b, x0 and minv made by torch ops that are still queued behind a long kernel
    when the solver is called give the bits of the same solve on a side stream, for check_every > 0 (x ready on return) and for
    check_every = 0 (x ready after krylov_status on stream 0)."""
    from hispmv_amd import solvers
    torch = torch_mod
    case = km.CASES["pcg_arrow_5000"]
    A = case["make"]()
    n = A.shape[0]
    bn, x0n = km.rhs(n), km.rhs(n, seed=4)
    minvn = (1.0 / A.tocsr().diagonal()).astype(f32)
    with Ctx(torch, [A]) as cx:
        side = torch.cuda.Stream()
        tb, tx, tm = (torch.from_numpy(a).to(cx.dev) for a in (bn, x0n, minvn))
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            want, winfo = solvers.cg(cx.h, cx.idx[0], tb, tx, minv=tm, rtol=case["rtol"], max_iters=case["max_iters"])
        side.synchronize()
        assert winfo["status"] == "CONVERGED"
        assert torch.cuda.current_stream().cuda_stream == 0
        long = torch.ones(1 << 26, dtype=torch.float32, device=cx.dev)
        for check_every in (8, 0):
            torch.cuda.synchronize()
            for _ in range(4):          # some milliseconds of work on the default stream, and the operands queued behind it
                long = long.sin()
            b, x0, minv = tb * 2.0 - tb, tx + 0.0, tm * 1.0
            x, info = solvers.cg(cx.h, cx.idx[0], b, x0, minv=minv, rtol=case["rtol"], max_iters=case["max_iters"], check_every=check_every)
            if check_every == 0:
                assert info["status"] == "IN_FLIGHT"
                info = dict(cx.h.krylov_status(info["work"].data_ptr(), 0), work=None)
            got = x.cpu().numpy()
            assert (info["status"], info["iterations"], info["relres"]) == (winfo["status"], winfo["iterations"], winfo["relres"]), (check_every, info, winfo)
            assert np.array_equal(bits(got), bits(want.cpu().numpy())), check_every
            assert np.array_equal(bits(x0.cpu().numpy()), bits(x0n))          # the caller's x0 is not written
