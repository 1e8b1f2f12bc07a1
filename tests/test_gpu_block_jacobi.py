"""The block-Jacobi preconditioner on the device (include/hispmv.h: hispmv_block_jacobi_extract_device, hispmv_block_invert_device,
hispmv_block_jacobi_setup_device, _status, _apply_device, hispmv_cg_bj_device, hispmv_gmres_bj_device) against the numpy model of
tests/block_jacobi_model.py.

  inversion   blocks and flags bit for bit the model's, for every block size, block counts around a wavefront, every kind of block
  extraction  equal by == to the model's padded blocks; on every slice plan, storage and handle state the entry accepts:
              tests/test_gpu_block_jacobi_plans.py
  apply       bit for bit the model's multiply, for sizes around a chunk, operands aligned and 4 bytes off
  lockstep    x and the workspace's r (GMRES: the basis) after 1, 2 and 7 iterations bit for bit the model's, the model driven by the
              products spmv_device itself returns; with a buffer that holds the MODEL's inverse and with one the device set up
  convergence CONVERGED, the fp64 true residual under twice the model's recorded one, a tenth / a third of the iterations of minv
  bad block, freeze, refresh, refusals, streams
"""
import numpy as np
import pytest
import scipy.sparse as sp

import block_jacobi_model as bj
import gmres_model as gm
import krylov_model as km
import step_small_cases as S
from block_jacobi_harness import Ctx, bits, unpack
from hispmv_amd import prep
from step_small_harness import HW

pytestmark = pytest.mark.gpu

f32 = np.float32


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def plain_ctx(torch_mod):
    with Ctx(torch_mod, [km.tridiag(8)]) as cx:
        yield cx


# ---- inversion ---------------------------------------------------------------------------------------------------------------------------
def _block_counts(bs):
    return sorted({1, 2, 64 // bs - 1, 64 // bs, 64 // bs + 1, 257} - {0})


@pytest.mark.parametrize("bs,nb", [(bs, nb) for bs in bj.SIZES for nb in _block_counts(bs)])
def test_inversion_is_the_models_bit_for_bit(torch_mod, plain_ctx, bs, nb):
    torch, cx = torch_mod, plain_ctx
    rng = np.random.default_rng(1000 * bs + nb)
    kinds = [bj.KINDS[(k + nb) % len(bj.KINDS)] for k in range(nb)]          # every kind wherever there are 8 blocks; rotated with nb
    blocks = np.stack([bj.block_of(kind, bs, rng) for kind in kinds])
    want, wflags = bj.invert(blocks)
    for kind, flag in zip(kinds, wflags):
        assert flag == (1 if kind in bj.BAD_KINDS else 0), kind
    raw = bj.buffer_bytes(blocks, np.full(nb, 7, np.int32))
    side = torch.cuda.Stream()
    for stream in (0, side.cuda_stream):          # the call is run twice: the context's stream, a torch stream
        buf = cx.upload(raw)
        torch.cuda.synchronize()
        cx.h.block_invert_device(buf.data_ptr(), nb, bs, stream)
        assert cx.h.block_jacobi_status(buf.data_ptr(), nb * bs, bs, stream) == int(wflags.sum())
        got, gflags = unpack(buf, nb * bs, bs)
        assert np.array_equal(gflags, wflags), (kinds, gflags, wflags)
        bad = [(k, kinds[k]) for k in range(nb) if not np.array_equal(bits(got[k]), bits(want[k]))]
        assert not bad, bad


# ---- extraction --------------------------------------------------------------------------------------------------------------------------
def _dense_spd(n=96):
    M = np.random.default_rng(96).standard_normal((n, n))
    return (M @ M.T / n + np.eye(n)).astype(f32)


def _bf16_system(n=1025):
    return km.tridiag(n, lo=-1.07, d=2.53, up=-1.07)


def _stray_split_system():
    """The stray-split band of the small-case generators (values in [-0.5, 0.5), 200 per row) with a dominant diagonal added, every
    position stored once (redrawn columns may repeat a position; three values at one position have no fixed sum)."""
    m = S.stray_split_band()
    n = m["rows"]
    i = np.arange(n)
    A = sp.coo_matrix((np.concatenate([m["v"], np.full(n, 60.0, f32)]), (np.concatenate([m["r"], i]), np.concatenate([m["c"], i]))), shape=(n, n)).tocsr()
    A.sum_duplicates()
    return A.tocoo()


def _twice(A):
    A = A.tocoo()
    return sp.coo_matrix((np.concatenate([A.data, A.data]), (np.concatenate([A.row, A.row]), np.concatenate([A.col, A.col]))), shape=A.shape)


def check_extraction(cx, k, A_true):
    n = A_true.shape[0]
    for bs in bj.SIZES:
        want = bj.extract(A_true, bs)
        got, _ = unpack(cx.setup(k, bs, only_extract=True), n, bs)
        assert got.shape == want.shape
        assert (got == want).all(), (n, bs, int((got != want).sum()))


EXTRACT_SIZES = (1, 3, 63, 64, 65, 1023, 1025, 4099)


@pytest.fixture(scope="module")
def extract_ctx(torch_mod):
    mats = [km.tridiag(n) for n in EXTRACT_SIZES] + [km.arrow(5000), km.band(4099), _twice(km.band(1025)), _dense_spd()]
    with Ctx(torch_mod, mats) as cx:
        yield cx


@pytest.mark.parametrize("k", range(len(EXTRACT_SIZES)), ids=[str(n) for n in EXTRACT_SIZES])
def test_extraction_tridiag(extract_ctx, k):
    check_extraction(extract_ctx, k, extract_ctx.mats[k])


@pytest.mark.parametrize("which", ["arrow_5000", "band_4099", "every_entry_twice", "dense"])
def test_extraction_systems(extract_ctx, which):
    cx = extract_ctx
    k = len(EXTRACT_SIZES) + ["arrow_5000", "band_4099", "every_entry_twice", "dense"].index(which)
    info = cx.h.matrix_info(cx.idx[k])
    if which == "arrow_5000":
        assert info["n_split_rows"] >= 1, info
    if which == "dense":
        assert info["is_dense"] and cx.h.block_jacobi_info(cx.idx[k], 8)["setup_launches"] == 2
    check_extraction(cx, k, cx.mats[k])


def test_extraction_stray_split(torch_mod):
    A = _stray_split_system()
    with Ctx(torch_mod, [A]) as cx:
        info = cx.h.matrix_info(cx.idx[0])
        assert info["tile_kind"] == 3 and info["col_tiles"] == 2, info
        assert cx.h.block_jacobi_info(cx.idx[0], 8)["setup_launches"] == 4          # the fill, a walk per part, the inversion
        check_extraction(cx, 0, A)


def test_extraction_bf16_storage(torch_mod):
    """A bf16 handle holds the rounded values: those are the blocks, sparse and dense."""
    A, W = _bf16_system().tocoo(), _dense_spd()
    with Ctx(torch_mod, [A, W], storage="bf16") as cx:
        assert cx.h.value_storage_info(cx.idx[0])["storage"] == "bf16"
        A_true = sp.coo_matrix((S.bf16_exact(A.data.astype(f32)), (A.row, A.col)), shape=A.shape)
        assert (A_true.data != A.data).any()
        check_extraction(cx, 0, A_true)
        W_true = S.bf16_exact(W)
        assert (W_true != W).any()
        check_extraction(cx, 1, W_true)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def _tile_stream_system():
    """20 000 x 20 000, 70 000 scattered entries and a dominant diagonal: a tile stream under HISPMV_FORMAT=tts."""
    rng = np.random.default_rng(77)
    n, nnz = 20000, 70000
    r, c = rng.integers(0, n, nnz), rng.integers(0, n, nnz)
    v = rng.uniform(-0.5, 0.5, nnz).astype(f32)
    i = np.arange(n)
    return sp.coo_matrix((np.concatenate([v, np.full(n, 4.0, f32)]), (np.concatenate([r, i]), np.concatenate([c, i]))), shape=(n, n))


def test_refusals(torch_mod):
    from hispmv_amd import solvers
    torch = torch_mod
    with Ctx(torch, [_tile_stream_system(), km.least_squares(300, 200), km.tridiag(300)], env=S.TTS) as cx:
        assert cx.h.matrix_info(cx.idx[0])["format"] == 1
        assert not cx.h.block_jacobi_info(cx.idx[0], 8)["accepted"] and not cx.h.block_jacobi_info(cx.idx[1], 8)["accepted"]
        buf = torch.full((4 << 20,), 0xCD, dtype=torch.uint8, device=cx.dev)
        torch.cuda.synchronize()
        need = prep.block_jacobi(300, 8)["pre_bytes"]
        for call in (cx.h.block_jacobi_extract_device, cx.h.block_jacobi_setup_device):
            with pytest.raises(NotImplementedError, match="set_transposable"):          # the words of the transposed entries' refusal
                call(cx.idx[0], 8, buf.data_ptr(), buf.numel())
            with pytest.raises(ValueError, match="square"):
                call(cx.idx[1], 8, buf.data_ptr(), buf.numel())
            with pytest.raises(ValueError, match="block_size"):
                call(cx.idx[2], 5, buf.data_ptr(), buf.numel())
            with pytest.raises(ValueError, match="bytes"):
                call(cx.idx[2], 8, buf.data_ptr(), need - 4)
            with pytest.raises(ValueError):
                call(cx.idx[2], 8, 0, need)
            with pytest.raises(ValueError, match="aligned"):
                call(cx.idx[2], 8, buf.data_ptr() + 4, need)
            with pytest.raises(IndexError):
                call(99, 8, buf.data_ptr(), buf.numel())
        with pytest.raises(ValueError):
            cx.h.block_jacobi_info(cx.idx[2], 5)
        with pytest.raises(ValueError):
            cx.h.block_invert_device(buf.data_ptr(), 4, 5)
        with pytest.raises(ValueError):
            cx.h.block_jacobi_apply_device(buf.data_ptr(), 300, 64, buf.data_ptr(), buf.data_ptr() + 4096)
        with pytest.raises(ValueError):
            solvers.block_jacobi(cx.h, cx.idx[1], 8)
        with pytest.raises(NotImplementedError):
            solvers.block_jacobi(cx.h, cx.idx[0], 8)
        cx.h.synchronize()
        torch.cuda.synchronize()
        assert bool((buf == 0xCD).all())          # nothing was launched


def test_refused_before_load_matrices(torch_mod):
    import pyhispmv
    A = km.tridiag(64)
    h = pyhispmv.FpgaHandle(*HW)
    try:
        i = h.create_sparse_handle(A.row, A.col, A.data, 64, 64)
        d = torch_mod.zeros(1 << 20, dtype=torch_mod.float32, device="cuda")
        assert not h.block_jacobi_info(i, 8)["accepted"]
        for call in (h.block_jacobi_extract_device, h.block_jacobi_setup_device):
            with pytest.raises(AssertionError, match="before load_matrices"):
                call(i, 8, d.data_ptr(), 4 << 20)
        for call in (h.cg_bj_device, h.gmres_bj_device):
            with pytest.raises(AssertionError, match="before load_matrices"):
                call(i, d.data_ptr(), d.data_ptr() + 1024, d.data_ptr() + 8192, 8, work=d.data_ptr() + (1 << 20), work_bytes=2 << 20)
    finally:
        h.close()


# ---- apply -------------------------------------------------------------------------------------------------------------------------------
APPLY_CASES = [(bs, n) for bs in bj.SIZES for n in (1, 5, 63, 64, 65, 1023, 1024, 1025, 4099)] + [(4, 1024 * 1024 + 1029)]


@pytest.mark.parametrize("bs,n", APPLY_CASES)
def test_apply_is_the_models_bit_for_bit(torch_mod, plain_ctx, bs, n):
    torch, cx = torch_mod, plain_ctx
    rng = np.random.default_rng(7 * n + bs)
    nb = -(-n // bs)
    inv = rng.standard_normal((nb, bs, bs), dtype=f32)
    r = rng.standard_normal(n, dtype=f32)
    want = bj.BlockInverse(inv, n) * r
    buf = cx.upload(bj.buffer_bytes(inv, np.zeros(nb, np.int32))[:prep.block_jacobi(n, bs)["pre_bytes"]])
    side = torch.cuda.Stream()
    for shift_r, shift_z, stream in ((0, 0, 0), (1, 0, 0), (0, 1, side.cuda_stream), (1, 1, 0)):
        dr, dz = cx.device(r, shift_r), cx.device(np.full(n, np.nan, f32), shift_z)
        torch.cuda.synchronize()
        cx.h.block_jacobi_apply_device(buf.data_ptr(), n, bs, dr.data_ptr(), dz.data_ptr(), stream)
        cx.h.synchronize()
        side.synchronize()
        got = dz.cpu().numpy()
        assert np.array_equal(bits(got), bits(want)), (bs, n, shift_r, shift_z, int((bits(got) != bits(want)).sum()))
    dz = cx.device(r)          # in place
    torch.cuda.synchronize()
    cx.h.block_jacobi_apply_device(buf.data_ptr(), n, bs, dz.data_ptr(), dz.data_ptr())
    cx.h.synchronize()
    assert np.array_equal(bits(dz.cpu().numpy()), bits(want))


# ---- lockstep ----------------------------------------------------------------------------------------------------------------------------
LOCK_SIZES = (65, 1025, 4099)
LOCK_BS = (4, 8, 32)
CG_RUNS = ((1, 0), (2, 1), (7, 0))                    # (iterations, floats by which b and x are off the 16-byte alignment)
GMRES_RUNS = ((1, 30, 0), (2, 1, 1), (7, 3, 0))       # (iterations, restart, shift)


@pytest.fixture(scope="module")
def lock_ctx(torch_mod):
    with Ctx(torch_mod, [km.tridiag(n) for n in LOCK_SIZES] + [km.band(n) for n in LOCK_SIZES]) as cx:
        yield cx


def _buffers(cx, k, bs):
    """(the model's preconditioner, [a buffer holding the model's inverse, a buffer the device set up])"""
    A = cx.mats[k]
    n = A.shape[0]
    m = bj.setup(A, bs)
    assert not m.flags.any()
    by_model = cx.upload(bj.buffer_bytes(m.inv, m.flags)[:prep.block_jacobi(n, bs)["pre_bytes"]])
    by_device = cx.setup(k, bs)
    got, gflags = unpack(by_device, n, bs)
    assert np.array_equal(bits(got), bits(m.inv)) and not gflags.any()          # the extraction is exact on these systems
    return m, (by_model, by_device)


@pytest.mark.parametrize("bs", LOCK_BS)
@pytest.mark.parametrize("k", range(len(LOCK_SIZES)), ids=[str(n) for n in LOCK_SIZES])
def test_lockstep_cg_tridiag(torch_mod, lock_ctx, k, bs):
    torch, cx = torch_mod, lock_ctx
    n = cx.mats[k].shape[0]
    m, buffers = _buffers(cx, k, bs)
    rng = np.random.default_rng(1 + n)
    b, x0 = rng.uniform(-1, 1, n).astype(f32), rng.uniform(-1, 1, n).astype(f32)
    prod, _ = cx.products(k)
    ki = cx.h.krylov_info(cx.idx[k], "cg")
    assert ki["work_bytes"] == cx.h.block_jacobi_info(cx.idx[k], bs)["cg_work_bytes"]
    for iters, shift in CG_RUNS:
        mx, mr, minfo = km.cg(prod, b, x0, m, 1e-6, iters)
        for buf in buffers:
            work = torch.zeros(ki["work_bytes"], dtype=torch.uint8, device=cx.dev)
            db, dx = cx.device(b, shift), cx.device(x0, shift)
            torch.cuda.synchronize()
            info = cx.h.cg_bj_device(cx.idx[k], db.data_ptr(), dx.data_ptr(), buf.data_ptr(), bs, rtol=1e-6, max_iters=iters, check_every=0,
                                     work=work.data_ptr(), work_bytes=ki["work_bytes"])
            assert info["status"] == "IN_FLIGHT", info
            info = cx.h.krylov_status(work.data_ptr(), 0)
            torch.cuda.synchronize()
            x = dx.cpu().numpy()
            r = work[ki["r_offset"]:ki["r_offset"] + 4 * n].cpu().numpy().view(f32)
            tag = (n, bs, iters, shift)
            assert info == minfo, (tag, info, minfo)
            assert np.array_equal(bits(x), bits(mx)), (tag, "x", int((bits(x) != bits(mx)).sum()))
            assert np.array_equal(bits(r), bits(mr)), (tag, "r", int((bits(r) != bits(mr)).sum()))


@pytest.mark.parametrize("bs", LOCK_BS)
@pytest.mark.parametrize("k", range(len(LOCK_SIZES)), ids=[str(n) for n in LOCK_SIZES])
def test_lockstep_gmres_band(torch_mod, lock_ctx, k, bs):
    torch, cx = torch_mod, lock_ctx
    k = len(LOCK_SIZES) + k
    n = cx.mats[k].shape[0]
    m, buffers = _buffers(cx, k, bs)
    rng = np.random.default_rng(1 + n)
    b, x0 = rng.uniform(-1, 1, n).astype(f32), rng.uniform(-1, 1, n).astype(f32)
    prod, _ = cx.products(k)
    for iters, restart, shift in GMRES_RUNS:
        mx, mV, minfo = gm.gmres(prod, b, x0, m, 1e-6, iters, restart)
        gi = cx.h.gmres_info(cx.idx[k], restart, True)
        bi = cx.h.block_jacobi_info(cx.idx[k], bs)
        assert gi["work_bytes"] == bi["gmres_work_bytes"] + (restart - 1) * bi["gmres_step_bytes"]
        for buf in buffers:
            work = torch.zeros(gi["work_bytes"], dtype=torch.uint8, device=cx.dev)
            db, dx = cx.device(b, shift), cx.device(x0, shift)
            torch.cuda.synchronize()
            info = cx.h.gmres_bj_device(cx.idx[k], db.data_ptr(), dx.data_ptr(), buf.data_ptr(), bs, restart=restart, rtol=1e-6, max_iters=iters,
                                        check_every=0, work=work.data_ptr(), work_bytes=gi["work_bytes"])
            assert info["status"] == "IN_FLIGHT", info
            info = cx.h.krylov_status(work.data_ptr(), 0)
            torch.cuda.synchronize()
            x = dx.cpu().numpy()
            V = work[gi["v_offset"]:gi["v_offset"] + 4 * gi["stride"] * (restart + 1)].cpu().numpy().view(f32).reshape(restart + 1, gi["stride"])[:, :n]
            tag = (n, bs, iters, restart, shift)
            assert info == minfo, (tag, info, minfo)
            assert np.array_equal(bits(x), bits(mx)), (tag, "x", int((bits(x) != bits(mx)).sum()))
            for i in range(len(mV)):
                assert np.array_equal(bits(V[i]), bits(mV[i])), (tag, "basis vector", i)


# ---- convergence -------------------------------------------------------------------------------------------------------------------------
def _front_end_solve(torch, cx, case, b, precond=None, minv=None, **kw):
    from hispmv_amd import solvers
    tb = torch.from_numpy(b).to(cx.dev)
    args = dict(rtol=case["rtol"], max_iters=case["max_iters"], precond=precond, minv=minv, **kw)
    if case["solver"] == "cg":
        x, info = solvers.cg(cx.h, cx.idx[0], tb, **args)
    else:
        x, info = solvers.gmres(cx.h, cx.idx[0], tb, restart=case["restart"], **args)
    torch.cuda.synchronize()
    return x.cpu().numpy(), info


@pytest.mark.parametrize("name", sorted(bj.CASES))
def test_convergence(torch_mod, name):
    from hispmv_amd import solvers
    torch = torch_mod
    case = bj.CASES[name]
    A = case["make"]()
    b = km.rhs(A.shape[0])
    with Ctx(torch, [A]) as cx:
        pre = solvers.block_jacobi(cx.h, cx.idx[0], case["bs"])
        assert (pre.block_size, pre.n, pre.singular_blocks()) == (case["bs"], A.shape[0], 0)
        x, info = _front_end_solve(torch, cx, case, b, precond=pre)
        minv = torch.from_numpy((1.0 / A.tocsr().diagonal()).astype(f32)).to(cx.dev)
        xm, im = _front_end_solve(torch, cx, case, b, minv=minv)
        res = km.true_relres(A, x, b)
        print(f"{name}: blocks {info}, minv {im}, true relative residual {res:.3e}, recorded on the CPU {case['attained']:.3e}")
        assert info["status"] == "CONVERGED" and im["status"] == "CONVERGED", (info, im)
        assert info["relres"] <= case["rtol"]
        assert res <= 2 * case["attained"], (res, case["attained"])
        assert info["iterations"] <= case["ratio"] * im["iterations"], (info, im)
        # the multiply by the front end's door
        r = km.rhs(A.shape[0], seed=9)
        z = pre.apply(torch.from_numpy(r).to(cx.dev))
        torch.cuda.synchronize()
        assert np.array_equal(bits(z.cpu().numpy()), bits(bj.setup(A, case["bs"]) * r))


def test_a_bad_block_is_replaced_and_the_solve_goes_on(torch_mod):
    from hispmv_amd import solvers
    torch = torch_mod
    A = bj.zero_block_system()
    n = A.shape[0]
    b = km.rhs(n)
    with Ctx(torch, [A]) as cx:
        pre = solvers.block_jacobi(cx.h, cx.idx[0], 8)
        assert pre.singular_blocks() == 1
        blocks, flags = unpack(pre.buffer, n, 8)
        assert flags.tolist() == [0, 1, 0, 0, 0, 0, 0, 0] and np.array_equal(blocks[1], np.eye(8, dtype=f32))
        x, info = solvers.gmres(cx.h, cx.idx[0], torch.from_numpy(b).to(cx.dev), precond=pre, restart=30, rtol=1e-6, max_iters=200)
        torch.cuda.synchronize()
        x = x.cpu().numpy()
        assert info["status"] == "CONVERGED" and np.isfinite(x).all(), info
        assert km.true_relres(A, x, b) < 1e-4


# ---- freeze, refresh, argument order, streams --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(bj.CASES))
def test_freeze_gives_the_same_answer_for_every_check_every(torch_mod, name):
    from hispmv_amd import solvers
    torch = torch_mod
    case = dict(bj.CASES[name], max_iters=60)
    A = case["make"]()
    b = km.rhs(A.shape[0])
    with Ctx(torch, [A]) as cx:
        pre = solvers.block_jacobi(cx.h, cx.idx[0], case["bs"])
        runs = []
        for ce in (1, 7, 10 ** 6, 0):
            x, info = _front_end_solve(torch, cx, case, b, precond=pre, check_every=ce)
            if ce == 0:
                assert info["status"] == "IN_FLIGHT"
                info = cx.h.krylov_status(info["work"].data_ptr(), 0)
                torch.cuda.synchronize()
            runs.append((x, info))
        x, info = runs[0]
        assert info["status"] == "CONVERGED" and 0 < info["iterations"] < 60, info
        for xo, io in runs[1:]:
            assert np.array_equal(bits(xo), bits(x))
            assert (io["status"], io["iterations"], io["relres"]) == (info["status"], info["iterations"], info["relres"]), (io, info)


def test_refresh_after_a_value_update(torch_mod):
    from hispmv_amd import solvers
    torch = torch_mod
    A = bj.multidof(33, 8).tocoo()          # n = 264
    doubled = sp.coo_matrix((2 * A.data, (A.row, A.col)), shape=A.shape)
    with Ctx(torch, [doubled]) as fresh:
        want = solvers.block_jacobi(fresh.h, fresh.idx[0], 8).buffer.cpu().numpy().copy()
    with Ctx(torch, [A], updates=True) as cx:
        pre = solvers.block_jacobi(cx.h, cx.idx[0], 8)
        before = pre.buffer.cpu().numpy().copy()
        assert not np.array_equal(before, want)
        vals = torch.from_numpy((2 * A.data).astype(f32)).to(cx.dev)
        torch.cuda.synchronize()
        cx.h.update_values_device(cx.idx[0], vals.data_ptr(), len(A.data))
        cx.h.synchronize()
        assert pre.refresh() is pre
        torch.cuda.synchronize()
        assert np.array_equal(pre.buffer.cpu().numpy(), want)


def test_argument_order(torch_mod):
    from hispmv_amd import solvers
    torch = torch_mod
    A = km.tridiag(300)
    with Ctx(torch, [A, km.tridiag(64)]) as cx:
        pre = solvers.block_jacobi(cx.h, cx.idx[0], 4)
        other = solvers.block_jacobi(cx.h, cx.idx[1], 4)
        tb = torch.from_numpy(km.rhs(300)).to(cx.dev)
        minv = torch.ones(300, dtype=torch.float32, device=cx.dev)
        for solve in (solvers.cg, solvers.gmres):
            with pytest.raises(ValueError, match="not both"):
                solve(cx.h, cx.idx[0], tb, minv=minv, precond=pre)
            with pytest.raises(ValueError, match="unknowns"):
                solve(cx.h, cx.idx[0], tb, precond=other)
            with pytest.raises(TypeError):
                solve(cx.h, cx.idx[0], tb, precond=minv)
        # the entries refuse before any launch: x untouched
        x0 = km.rhs(300, seed=2)
        db, dx = cx.device(km.rhs(300)), cx.device(x0)
        work = torch.zeros(cx.h.gmres_info(cx.idx[0], 30, True)["work_bytes"], dtype=torch.uint8, device=cx.dev)
        torch.cuda.synchronize()
        kw = dict(work=work.data_ptr(), work_bytes=work.numel())
        for call in (cx.h.cg_bj_device, cx.h.gmres_bj_device):
            for d_pre, bs, more in ((pre.buffer.data_ptr(), 5, {}), (pre.buffer.data_ptr(), 0, {}), (pre.buffer.data_ptr() + 4, 4, {}), (0, 4, {}),
                                    (pre.buffer.data_ptr(), 4, dict(rtol=-1.0)), (pre.buffer.data_ptr(), 4, dict(max_iters=0)),
                                    (pre.buffer.data_ptr(), 4, dict(work_bytes=1024))):
                with pytest.raises(ValueError):
                    call(cx.idx[0], db.data_ptr(), dx.data_ptr(), d_pre, bs, **dict(kw, **more))
        cx.h.synchronize()
        torch.cuda.synchronize()
        assert np.array_equal(bits(dx.cpu().numpy()), bits(x0)) and not bool(work.any())


def test_front_end_on_a_side_stream_and_on_the_default_stream(torch_mod):
    """Setup and solve inside a side stream, and both on torch's default stream with the operands still queued behind a long kernel:
    the same buffer, the same x, the same info."""
    from hispmv_amd import solvers
    torch = torch_mod
    case = bj.CASES["cg_multidof_130x8"]
    A = case["make"]()
    n = A.shape[0]
    bn = km.rhs(n)
    with Ctx(torch, [A]) as cx:
        side = torch.cuda.Stream()
        tb = torch.from_numpy(bn).to(cx.dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            pre_s = solvers.block_jacobi(cx.h, cx.idx[0], case["bs"])
            want, winfo = solvers.cg(cx.h, cx.idx[0], tb, precond=pre_s, rtol=case["rtol"], max_iters=case["max_iters"])
            z_s = pre_s.apply(tb)
        side.synchronize()
        assert winfo["status"] == "CONVERGED" and pre_s.singular_blocks() == 0
        assert torch.cuda.current_stream().cuda_stream == 0
        long = torch.ones(1 << 26, dtype=torch.float32, device=cx.dev)
        for _ in range(4):          # some milliseconds of work on the default stream, and the operand queued behind it
            long = long.sin()
        b = tb * 2.0 - tb
        pre_d = solvers.block_jacobi(cx.h, cx.idx[0], case["bs"])
        x, info = solvers.cg(cx.h, cx.idx[0], b, precond=pre_d, rtol=case["rtol"], max_iters=case["max_iters"])
        z_d = pre_d.apply(b)
        assert np.array_equal(pre_d.buffer.cpu().numpy(), pre_s.buffer.cpu().numpy())
        assert (info["status"], info["iterations"], info["relres"]) == (winfo["status"], winfo["iterations"], winfo["relres"]), (info, winfo)
        assert np.array_equal(bits(x.cpu().numpy()), bits(want.cpu().numpy()))
        assert np.array_equal(bits(z_d.cpu().numpy()), bits(z_s.cpu().numpy()))
