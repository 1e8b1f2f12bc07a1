"""The multi-right-hand-side Krylov entries on the device (include/hispmv.h: hispmv_dot_multi_device, hispmv_cg_multi_device,
hispmv_bicgstab_multi_device, hispmv_krylov_multi_status) against the single-vector numpy model of tests/krylov_model.py, driven by
spmm_device on ONE vector: column v of a batch is the model's solve of A x_v = b_v, bit for bit.

  dot           every column bit-equal to km.dot, for every width, ld and alignment of the operands; NaN pads are never read
  lockstep      X[:, v] and the workspace's R[:, v] after K iterations (check_every = 0) the model's bits, at the tile edges too
  independence  a column's x, iterations and relres do not depend on the batch: alone, or somewhere in 70 columns
  freeze        the same bits and results for every check_every, while columns stop at different iterations
  breakdown     an all-zero matrix: every column BREAKDOWN, X untouched; all-zero B: no product
  handle kinds  a stray split and bf16 storage converge, per column under twice the CPU model's residual
  refusals      before any launch, X untouched
"""
import numpy as np
import pytest
import scipy.sparse as sp

import krylov_model as km
import krylov_multi_cases as kc
import step_small_cases as S
from step_small_harness import HW, SHARED

pytestmark = pytest.mark.gpu

f32 = np.float32
SENTINEL = f32(-7.25e11)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


class Ctx:
    """One context with the given matrices (scipy COO, or a dense ndarray) loaded."""

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

    def vector(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, f32)).to(self.dev)

    def matrix(self, a, ld=None, shift=0, pad=np.nan):
        """a [n, m] on the device with leading dimension ld, `shift` floats off the 16-byte alignment of its allocation, the pad
        columns and everything around filled with `pad`: (the whole allocation, the pointer of a[0, 0])"""
        n, m = a.shape
        ld = m if ld is None else ld
        host = np.full(shift + n * ld + 4, pad, f32)
        host[shift:shift + n * ld].reshape(n, ld)[:, :m] = a
        t = self.torch.from_numpy(host).to(self.dev)
        return t, t.data_ptr() + 4 * shift

    @staticmethod
    def unpack(t, n, m, ld, shift):
        """(a [n, m], every other word of the allocation) of a tensor made by matrix()"""
        host = t.cpu().numpy()
        body = host[shift:shift + n * ld].reshape(n, ld)
        rest = np.concatenate([host[:shift], body[:, m:].ravel(), host[shift + n * ld:]])
        return body[:, :m].copy(), rest

    def products(self, k):
        """The model's callback over spmm_device on ONE vector of matrix k; a bias goes in place like the solvers' residual."""
        torch, h, idx = self.torch, self.h, self.idx[k]
        n = self.mats[k].shape[0]
        wb = h.spmm_info(idx, 1)["work_bytes"]
        work = torch.zeros(max(wb, 16), dtype=torch.uint8, device=self.dev)

        def prod(x, bias, alpha, beta):
            dx = self.vector(x)
            dy = self.vector(bias) if bias is not None else self.vector(np.full(n, np.nan, f32))
            torch.cuda.synchronize()          # the context's stream does not wait for torch's
            h.spmm_device(idx, dx.data_ptr(), 1, dy.data_ptr() if bias is not None else 0, dy.data_ptr(), alpha, beta,
                          bias_stride=1 if bias is not None else 0, work=work.data_ptr(), work_bytes=wb)
            h.synchronize()
            return dy.cpu().numpy()
        return prod

    def solve(self, k, solver, B, X0, minv=None, rtol=1e-6, max_iters=10, check_every=0, ld_b=None, ld_x=None, shift=0, stream=0):
        """One multi solve -> (X, R, the columns' results); check_every = 0 reads the outcome with krylov_multi_status.  The pads of B
        hold NaN; the pads of X and the words around it hold SENTINEL and are checked untouched."""
        torch, h, idx = self.torch, self.h, self.idx[k]
        n, m = B.shape
        ld_b, ld_x = m if ld_b is None else ld_b, m if ld_x is None else ld_x
        ki = h.krylov_multi_info(idx, solver, m)
        from hispmv_amd import prep
        lay = prep.krylov_multi(n, m)
        assert ki["accepted"] and ki["n"] == n and ki["ld"] == lay["ld"] and ki["groups"] == lay["groups"], ki
        assert ki["r_offset"] == lay["state_bytes"] + lay["partial_bytes"], (ki, lay)
        work = torch.zeros(ki["work_bytes"], dtype=torch.uint8, device=self.dev)
        tb, pb = self.matrix(B, ld_b, shift)
        tx, px = self.matrix(X0, ld_x, shift, pad=SENTINEL)
        dm = self.vector(minv) if minv is not None else None
        torch.cuda.synchronize()
        kw = dict(ld_b=ld_b, ld_x=ld_x, rtol=rtol, max_iters=max_iters, check_every=check_every, work=work.data_ptr(), work_bytes=ki["work_bytes"], stream=stream)
        if solver == "cg":
            res = h.cg_multi_device(idx, pb, px, m, dm.data_ptr() if dm is not None else 0, **kw)
        else:
            res = h.bicgstab_multi_device(idx, pb, px, m, **kw)
        assert len(res) == m
        if check_every == 0:
            assert all(r["status"] == "IN_FLIGHT" and r["products"] == res[0]["products"] for r in res), res
            enq = res[0]["products"]
            res = h.krylov_multi_status(work.data_ptr(), m, stream)
            assert all(r["products"] == enq for r in res)
        h.synchronize()
        torch.cuda.synchronize()
        X, rest = self.unpack(tx, n, m, ld_x, shift)
        assert (bits(rest) == bits(SENTINEL)).all(), "a pad of X was written"
        ld = ki["ld"]
        R = work[ki["r_offset"]:ki["r_offset"] + 4 * n * ld].cpu().numpy().view(f32).reshape(n, ld)[:, :m].copy()
        return X, R, res


def model(prod, solver, b, x0, minv, rtol, max_iters):
    b, x0 = np.ascontiguousarray(b), np.ascontiguousarray(x0)
    return km.cg(prod, b, x0, minv, rtol, max_iters) if solver == "cg" else km.bicgstab(prod, b, x0, rtol, max_iters)


def same_result(got, want, tag):
    assert (got["status"], got["iterations"], got["relres"]) == (want["status"], want["iterations"], want["relres"]), (tag, got, want)


# ---- dot_multi_device ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dot_ctx(torch_mod):
    with Ctx(torch_mod, [km.tridiag(8)]) as cx:
        yield cx


@pytest.mark.parametrize("n", (1, 3, 64, 65, 1023, 1025, 4099))
def test_dot_multi_device(torch_mod, dot_ctx, n):
    from hispmv_amd import prep
    torch, cx = torch_mod, dot_ctx
    rng = np.random.default_rng(n)
    A, B = rng.standard_normal((n, 65)).astype(f32), rng.standard_normal((n, 65)).astype(f32)
    want = np.array([km.dot(A[:, v], B[:, v]) for v in range(65)], np.float64)
    for m in (1, 3, 64, 65):
        lay = prep.krylov_multi(n, m)
        need = 8 * lay["groups"] * lay["ld"]
        work = torch.zeros(need + 16, dtype=torch.uint8, device=cx.dev)
        for ld in (m, m + 3):
            for sa, sb in ((0, 0), (1, 0), (0, 1)):          # operands 0 or 4 bytes off the 16-byte alignment
                ta, pa = cx.matrix(A[:, :m], ld, sa)
                tb, pb = cx.matrix(B[:, :m], ld, sb)
                out = torch.full((m + 1,), float("nan"), dtype=torch.float64, device=cx.dev)
                torch.cuda.synchronize()
                for tile in ("auto", "64"):          # the narrow tile a short grid takes, and the widest
                    with S.environment({} if tile == "auto" else {"HISPMV_KRYLOV_MULTI_TILE": tile}):
                        cx.h.dot_multi_device(n, m, pa, pb, out.data_ptr(), work.data_ptr(), need, ld_a=ld, ld_b=ld)
                    cx.h.synchronize()
                    got = out.cpu().numpy()
                    assert np.array_equal(got[:m].view(np.uint64), want[:m].view(np.uint64)), (n, m, ld, sa, sb, tile, got[:m], want[:m])
                    assert np.isnan(got[m])
                    out[:m] = float("nan")
                    torch.cuda.synchronize()
        with pytest.raises(ValueError, match="workspace"):
            cx.h.dot_multi_device(n, m, pa, pb, out.data_ptr(), work.data_ptr(), need - 8, ld_a=ld, ld_b=ld)
        with pytest.raises(ValueError):
            cx.h.dot_multi_device(n, m, pa, pb, out.data_ptr(), work.data_ptr() + 4, need, ld_a=ld, ld_b=ld)
        with pytest.raises(ValueError):
            cx.h.dot_multi_device(n, m, pa, pb, out.data_ptr(), work.data_ptr(), need, ld_a=m - 1, ld_b=ld)
    with pytest.raises(ValueError, match="1024"):
        cx.h.dot_multi_device(2 ** 20 + 1, 1, pa, pb, out.data_ptr(), work.data_ptr(), 1 << 30)


# ---- lockstep --------------------------------------------------------------------------------------------------------------------------
# (iterations, ld_b - m, ld_x - m rounded so that ld_x is even when `even`, floats off the 16-byte alignment): aligned and dense;
# 4 bytes off with ld_x != ld_b (4-byte accesses); 8 bytes off with an even ld_x (8-byte accesses)
RUNS = ((1, 0, 0, False, 0), (2, 3, 1, False, 1), (7, 2, 2, True, 2))


def checked_columns(m):
    return sorted({0, 1, m - 1} | {v for v in (63, 64, 255, 256) if v < m}) if m > 1 else [0]


def lockstep(cx, k, solver, m, precond=False):
    n = cx.mats[k].shape[0]
    rng = np.random.default_rng(1000 * m + n)
    B = rng.uniform(-1, 1, (n, m)).astype(f32)
    X0 = rng.uniform(-1, 1, (n, m)).astype(f32)
    minv = rng.uniform(0.3, 0.5, n).astype(f32) if precond else None
    prod = cx.products(k)
    per = cx.h.krylov_multi_info(cx.idx[k], solver, m)["products_per_iteration"]
    for iters, db, dx, even, shift in RUNS:
        ld_x = m + dx + ((m + dx) & 1 if even else 0)
        X, R, res = cx.solve(k, solver, B, X0, minv, rtol=1e-6, max_iters=iters, check_every=0, ld_b=m + db, ld_x=ld_x, shift=shift)
        for v in checked_columns(m):
            mx, mr, minfo = model(prod, solver, B[:, v], X0[:, v], minv, 1e-6, iters)
            tag = (solver, precond, n, m, iters, v)
            same_result(res[v], minfo, tag)
            assert res[v]["products"] == minfo["products"] == 1 + per * iters, (tag, res[v], minfo)
            assert np.array_equal(bits(X[:, v]), bits(mx)), (tag, "x", int((bits(X[:, v]) != bits(mx)).sum()))
            assert np.array_equal(bits(R[:, v]), bits(mr)), (tag, "r", int((bits(R[:, v]) != bits(mr)).sum()))


LOCK_SIZES = (1, 3, 65, 1025, 4099)


@pytest.fixture(scope="module")
def lock_ctx(torch_mod):
    mats = [km.tridiag(n) for n in LOCK_SIZES] + [km.band(n) for n in LOCK_SIZES] + [km.arrow(5000)]
    with Ctx(torch_mod, mats) as cx:
        yield cx


@pytest.mark.parametrize("k", range(len(LOCK_SIZES)), ids=[str(n) for n in LOCK_SIZES])
def test_lockstep_cg_tridiag(lock_ctx, k):
    lockstep(lock_ctx, k, "cg", 5)
    lockstep(lock_ctx, k, "cg", 5, precond=True)


@pytest.mark.parametrize("k", range(len(LOCK_SIZES)), ids=[str(n) for n in LOCK_SIZES])
def test_lockstep_bicgstab_band(lock_ctx, k):
    lockstep(lock_ctx, len(LOCK_SIZES) + k, "bicgstab", 5)


def test_lockstep_arrow_whose_first_row_is_cut_by_slices(lock_ctx):
    k = 2 * len(LOCK_SIZES)
    assert lock_ctx.h.matrix_info(lock_ctx.idx[k])["n_split_rows"] >= 1
    lockstep(lock_ctx, k, "cg", 3)
    lockstep(lock_ctx, k, "cg", 3, precond=True)
    lockstep(lock_ctx, k, "bicgstab", 3)


@pytest.mark.parametrize("tile", ("auto", "32", "64"))
@pytest.mark.parametrize("m", (64, 65, 260))
def test_lockstep_at_the_tile_edges(lock_ctx, m, tile):
    """64 fills the widest column tile of the vector kernels, 65 starts a second, 260 crosses the 256-vector tile of the product.  The
    vector kernels narrow their tile while the grid is short (here: to 16 columns); HISPMV_KRYLOV_MULTI_TILE holds it at 32 and 64,
    the widths a long system takes -- the bits do not depend on it."""
    k = LOCK_SIZES.index(1025)
    with S.environment({} if tile == "auto" else {"HISPMV_KRYLOV_MULTI_TILE": tile}):
        lockstep(lock_ctx, k, "cg", m, precond=True)
        lockstep(lock_ctx, len(LOCK_SIZES) + k, "bicgstab", m)


# ---- column independence, freeze -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def six_ctx(torch_mod):
    with Ctx(torch_mod, [km.tridiag(kc.N)]) as cx:
        yield cx


def six_columns():
    """B and X0 of the six columns: zero initial guesses, but the zero and the NaN column start from a guess that must be zeroed,
    respectively kept."""
    B = kc.columns()
    X0 = np.zeros_like(B)
    X0[:, 4] = km.rhs(kc.N, seed=2)
    X0[:, 5] = km.rhs(kc.N, seed=4)
    return B, X0


def test_a_column_does_not_depend_on_its_batch(six_ctx):
    cx = six_ctx
    B, X0 = six_columns()
    X, R, res = cx.solve(0, "cg", B, X0, rtol=kc.RTOL, max_iters=kc.MAX_ITERS, check_every=8)
    by = dict(zip(kc.NAMES, res))
    print({k: (v["status"], v["iterations"], v["relres"]) for k, v in by.items()})
    # the model on the GPU's own products says when the slowest and the smooth column stop
    prod = cx.products(0)
    for name in ("rhs1", "sin"):
        v = kc.NAMES.index(name)
        mx, mr, minfo = model(prod, "cg", B[:, v], X0[:, v], None, kc.RTOL, kc.MAX_ITERS)
        same_result(by[name], minfo, name)
        assert minfo["status"] == "CONVERGED" and np.array_equal(bits(X[:, v]), bits(mx)), name
    assert 0 < by["sin"]["iterations"] < by["rhs1"]["iterations"] <= kc.MAX_ITERS // 2
    assert all(by[k]["status"] == "CONVERGED" for k in ("rhs1", "e0", "A1", "sin", "zero"))
    assert by["zero"]["iterations"] == 0 and by["zero"]["relres"] == 0.0 and not X[:, 4].any()
    assert by["nan"]["status"] == "BREAKDOWN" and by["nan"]["iterations"] == 0 and np.array_equal(bits(X[:, 5]), bits(X0[:, 5]))
    # alone
    for v in range(6):
        x1, r1, res1 = cx.solve(0, "cg", B[:, v:v + 1], X0[:, v:v + 1], rtol=kc.RTOL, max_iters=kc.MAX_ITERS, check_every=8)
        same_result(res1[0], res[v], ("alone", v))
        assert np.array_equal(bits(x1[:, 0]), bits(X[:, v])), ("alone", v)
    # elsewhere in 70 columns, ld and alignment changed too
    rng = np.random.default_rng(70)
    B70, X70 = rng.uniform(-1, 1, (kc.N, 70)).astype(f32), np.zeros((kc.N, 70), f32)
    where = [69, 3, 64, 17, 65, 40]
    B70[:, where], X70[:, where] = B, X0
    Xw, Rw, resw = cx.solve(0, "cg", B70, X70, rtol=kc.RTOL, max_iters=kc.MAX_ITERS, check_every=8, ld_b=73, ld_x=71, shift=1)
    for v, w in enumerate(where):
        same_result(resw[w], res[v], ("in 70", v))
        assert np.array_equal(bits(Xw[:, w]), bits(X[:, v])), ("in 70", v)
    assert all(r["status"] == "CONVERGED" for w, r in enumerate(resw) if w != 40)


@pytest.mark.parametrize("solver", ["cg", "bicgstab"])
def test_freeze_gives_the_same_answer_for_every_check_every(six_ctx, solver):
    cx = six_ctx
    B, X0 = six_columns()
    runs = [cx.solve(0, solver, B, X0, rtol=kc.RTOL, max_iters=kc.MAX_ITERS, check_every=ce) for ce in (1, 7, 10 ** 6, 0)]
    X, R, res = runs[0]
    its = [r["iterations"] for r in res]
    print(solver, [(r["status"], r["iterations"]) for r in res])
    assert [r["status"] for r in res] == ["CONVERGED"] * 5 + ["BREAKDOWN"], res
    assert its[0] > its[3] > 0 and its[4] == its[5] == 0 and max(its) <= kc.MAX_ITERS // 2, its
    for Xo, Ro, reso in runs[1:]:
        assert np.array_equal(bits(Xo), bits(X)) and np.array_equal(bits(Ro), bits(R))
        for v in range(6):
            same_result(reso[v], res[v], (solver, v))
    per = cx.h.krylov_multi_info(cx.idx[0], solver, 6)["products_per_iteration"]
    assert per == (1 if solver == "cg" else 2)
    assert all(r["products"] == 1 + per * max(its) for r in runs[0][2])                    # check_every = 1 stops with the slowest column
    assert all(r["products"] == 1 + per * kc.MAX_ITERS for r in runs[3][2])                # check_every = 0 enqueues them all


# ---- breakdown -------------------------------------------------------------------------------------------------------------------------
def test_breakdown_on_all_zero_values(torch_mod):
    n, m = 300, 4
    B = np.stack([km.rhs(n, seed=s) for s in (1, 5, 6, 7)], axis=1)
    X0 = np.stack([km.rhs(n, seed=s) for s in (2, 8, 9, 10)], axis=1)
    with Ctx(torch_mod, [km.zero_pattern(n)]) as cx:
        for solver in ("cg", "bicgstab"):
            for ce in (0, 1):
                X, R, res = cx.solve(0, solver, B, X0, max_iters=5, check_every=ce, ld_x=m + 1)
                assert all(r["status"] == "BREAKDOWN" and r["iterations"] == 0 for r in res), (solver, ce, res)
                assert np.array_equal(bits(X), bits(X0)), (solver, ce)
        for ce in (0, 1):          # B == 0: X = 0, converged, no iteration -- and no product where the host looks
            X, R, res = cx.solve(0, "cg", np.zeros((n, m), f32), X0, max_iters=5, check_every=ce, ld_x=m + 1)
            assert all(r["status"] == "CONVERGED" and r["iterations"] == 0 and r["relres"] == 0.0 for r in res) and not X.any(), res
            assert all(r["products"] == (6 if ce == 0 else 0) for r in res), res


# ---- handle kinds ----------------------------------------------------------------------------------------------------------------------
def _stray_split_system():
    """test_gpu_krylov._stray_split_system: the stray-split band with a dominant diagonal added as further entries; not symmetric."""
    m = S.stray_split_band()
    n = m["rows"]
    i = np.arange(n)
    return sp.coo_matrix((np.concatenate([m["v"], np.full(n, 60.0, f32)]), (np.concatenate([m["r"], i]), np.concatenate([m["c"], i]))), shape=(n, n))


# attained: per column (b = km.rhs(n, seed) for seeds 1, 2, 3, x0 = 0) the fp64 true relative residual the single-vector model reaches
# with scipy products on the CPU; a column's bound is twice its figure
KINDS = {
    "stray_split": dict(solver="bicgstab", make=_stray_split_system, rtol=1e-6, max_iters=60, attained=(3.7e-7, 4.3e-7, 3.5e-7)),
    "bf16_storage": dict(solver="cg", make=lambda: km.tridiag(1025, lo=-1.07, d=2.53, up=-1.07), rtol=1e-6, max_iters=100, storage="bf16",
                         attained=(1.0e-6, 9.7e-7, 9.4e-7)),
}


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_handle_kinds(torch_mod, kind):
    case = KINDS[kind]
    A = case["make"]()
    n = A.shape[0]
    with Ctx(torch_mod, [A], storage=case.get("storage", "fp32")) as cx:
        info = cx.h.matrix_info(cx.idx[0])
        A_true = A
        if kind == "bf16_storage":          # the handle holds the rounded values: that system is the one solved
            assert cx.h.value_storage_info(cx.idx[0])["storage"] == "bf16"
            A_true = sp.coo_matrix((S.bf16_exact(A.data.astype(f32)), (A.row, A.col)), shape=A.shape)
        else:
            assert info["tile_kind"] == 3 and info["col_tiles"] == 2, info
        B = np.stack([km.rhs(n, seed=s) for s in (1, 2, 3)], axis=1)
        X, R, res = cx.solve(0, case["solver"], B, np.zeros_like(B), rtol=case["rtol"], max_iters=case["max_iters"], check_every=8)
        for v in range(3):
            true = km.true_relres(A_true, X[:, v], B[:, v])
            print(f"{kind} column {v}: {res[v]}, true relative residual {true:.3e}, recorded on the CPU {case['attained'][v]:.3e}")
            assert res[v]["status"] == "CONVERGED" and res[v]["relres"] <= case["rtol"], res[v]
            assert true <= 2 * case["attained"][v], (v, true, case["attained"][v])


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(torch_mod):
    torch = torch_mod
    ts = S.tile_stream()
    ts = sp.coo_matrix((ts["v"], (ts["r"], ts["c"])), shape=(ts["rows"], ts["cols"]))
    dense = np.eye(96, dtype=f32) * 3
    with Ctx(torch, [ts, dense, km.least_squares(300, 200), km.tridiag(300)], env=S.AUTO) as cx:
        h = cx.h
        assert h.matrix_info(cx.idx[0])["format"] == 1 and h.matrix_info(cx.idx[1])["is_dense"]
        m = 3
        work = torch.zeros(h.krylov_multi_info(cx.idx[3], "bicgstab", m)["work_bytes"] + (8 << 20), dtype=torch.uint8, device=cx.dev)
        wk = dict(work=work.data_ptr(), work_bytes=work.numel())
        calls = (h.cg_multi_device, h.bicgstab_multi_device)
        for k, err, match in ((0, NotImplementedError, "set_transposable"), (1, NotImplementedError, "GEMM"), (2, ValueError, "square")):
            rows = cx.mats[k].shape[0]
            for solver, call in zip(("cg", "bicgstab"), calls):
                assert not h.krylov_multi_info(cx.idx[k], solver, m)["accepted"]
                tb, pb = cx.matrix(np.ones((rows, m), f32))
                tx, px = cx.matrix(np.full((max(cx.mats[k].shape), m), SENTINEL, f32))
                with pytest.raises(err, match=match):
                    call(cx.idx[k], pb, px, m, **wk)
                torch.cuda.synchronize()
                assert (bits(tx.cpu().numpy()[:-4]) == bits(SENTINEL)).all()
        n = 300
        need = h.krylov_multi_info(cx.idx[3], "bicgstab", m)["work_bytes"]
        assert need >= h.krylov_multi_info(cx.idx[3], "cg", m)["work_bytes"] > 0
        tb, pb = cx.matrix(np.ones((n, m), f32))
        tx, px = cx.matrix(np.full((n, m), SENTINEL, f32))
        ok = dict(work=work.data_ptr(), work_bytes=need)
        bad = (dict(ok, ld_b=m - 1), dict(ok, ld_x=m - 1), dict(ok, work_bytes=h.krylov_multi_info(cx.idx[3], "cg", m)["work_bytes"] - 1),
               dict(ok, work=0), dict(ok, work=work.data_ptr() + 4), dict(ok, rtol=-1.0), dict(ok, max_iters=0), dict(ok, check_every=-1))
        for call in calls:
            for kw in bad:
                with pytest.raises(ValueError):
                    call(cx.idx[3], pb, px, m, **kw)
            with pytest.raises(ValueError, match="num_vecs"):
                call(cx.idx[3], pb, px, 0, ld_b=m, ld_x=m, **ok)
            with pytest.raises(IndexError):
                call(99, pb, px, m, **ok)
        with pytest.raises(ValueError):
            h.krylov_multi_info(cx.idx[3], "cg", 0)
        with pytest.raises(ValueError):
            h.krylov_multi_info(cx.idx[3], "cgls", 2)
        torch.cuda.synchronize()
        assert (bits(tx.cpu().numpy()[:-4]) == bits(SENTINEL)).all()


def test_refused_before_load_matrices(torch_mod):
    import pyhispmv
    A = km.tridiag(64)
    h = pyhispmv.FpgaHandle(*HW)
    try:
        i = h.create_sparse_handle(A.row, A.col, A.data, 64, 64)
        d = torch_mod.zeros(1 << 20, dtype=torch_mod.float32, device="cuda")
        assert not h.krylov_multi_info(i, "cg", 2)["accepted"]
        for call in (h.cg_multi_device, h.bicgstab_multi_device):
            with pytest.raises(AssertionError, match="before load_matrices"):
                call(i, d.data_ptr(), d.data_ptr() + 1024, 2, work=d.data_ptr() + 4096, work_bytes=(4 << 20) - 4096)
    finally:
        h.close()


# ---- the torch front end ---------------------------------------------------------------------------------------------------------------
def test_torch_front_end(six_ctx, torch_mod):
    """hispmv_amd.solvers.cg_multi on torch tensors: the bits of the device entry on a side stream and on the default stream (where
    the operands are still queued behind a long kernel when the solver is called), B a narrowed view of a wider tensor."""
    from hispmv_amd import solvers
    torch, cx = torch_mod, six_ctx
    B, X0 = six_columns()
    minv = np.full(kc.N, 0.4, f32)
    want, _, wres = cx.solve(0, "cg", B, X0, minv, rtol=kc.RTOL, max_iters=kc.MAX_ITERS, check_every=8)
    wide = torch.full((kc.N, 9), float("nan"), dtype=torch.float32, device=cx.dev)
    wide[:, 2:8] = torch.from_numpy(B).to(cx.dev)
    tb, tx, tm = wide[:, 2:8], torch.from_numpy(X0).to(cx.dev), torch.from_numpy(minv).to(cx.dev)
    assert tb.stride() == (9, 1) and not tb.is_contiguous()

    def same(X, info):
        assert info["status"] == [r["status"] for r in wres]
        assert info["iterations"].tolist() == [r["iterations"] for r in wres] and info["relres"].tolist() == [r["relres"] for r in wres]
        assert X.is_contiguous() and np.array_equal(bits(X.cpu().numpy()), bits(want))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        X, info = solvers.cg_multi(cx.h, cx.idx[0], tb, tx, minv=tm, rtol=kc.RTOL, max_iters=kc.MAX_ITERS)
    side.synchronize()
    same(X, info)
    assert info["products"] == wres[0]["products"] and info["work"].numel() == cx.h.krylov_multi_info(cx.idx[0], "cg", 6)["work_bytes"]
    assert torch.cuda.current_stream().cuda_stream == 0
    long = torch.ones(1 << 25, dtype=torch.float32, device=cx.dev)
    for check_every in (8, 0):
        torch.cuda.synchronize()
        for _ in range(4):          # some milliseconds of work on the default stream, and the operands queued behind it
            long = long.sin()
        b, x0 = (wide * 2.0 - wide)[:, 2:8], tx + 0.0
        X, info = solvers.cg_multi(cx.h, cx.idx[0], b, x0, minv=tm * 1.0, rtol=kc.RTOL, max_iters=kc.MAX_ITERS, check_every=check_every)
        if check_every == 0:
            assert info["status"] == ["IN_FLIGHT"] * 6
            res = cx.h.krylov_multi_status(info["work"].data_ptr(), 6, 0)
            info = dict(info, status=[r["status"] for r in res], iterations=np.array([r["iterations"] for r in res]),
                        relres=np.array([r["relres"] for r in res]))
        same(X, info)
        assert np.array_equal(bits(x0.cpu().numpy()), bits(X0))          # the caller's X0 is not written
    Xb, infob = solvers.bicgstab_multi(cx.h, cx.idx[0], tb, rtol=kc.RTOL, max_iters=kc.MAX_ITERS)
    assert infob["status"] == ["CONVERGED"] * 5 + ["BREAKDOWN"] and Xb.shape == (kc.N, 6)
    with pytest.raises(TypeError):
        solvers.cg_multi(cx.h, cx.idx[0], tb.double())
    with pytest.raises(TypeError):
        solvers.cg_multi(cx.h, cx.idx[0], tb[:, 0])
    with pytest.raises(ValueError):
        solvers.cg_multi(cx.h, cx.idx[0], tb[:-1])
    with pytest.raises(ValueError):
        solvers.cg_multi(cx.h, cx.idx[0], tb.t().contiguous().t()[:, :6])
    with pytest.raises(ValueError):
        solvers.cg_multi(cx.h, cx.idx[0], tb, tx[:, :5])
