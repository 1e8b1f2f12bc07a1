"""Thick-restart Golub-Kahan on the device (include/hispmv.h: hispmv_gk_steps_device, hispmv_gk_status, hispmv_svds_device, hispmv_gk_info)
against the numpy model of tests/gk_model.py.

  steps       both bases, Gc columns, alphas, betas and status bit for bit the model's on a companion context, the model driven by the
              products spmv_device and spmv_device_t themselves return; in one call and split over three; after a restart
  svds        status, found, products, cycles, values, residual estimates and both sets of vectors bit for bit the model's (library
              products, prep.bsvd); the fp64 true residual and the singular-value error under twice what the model attains on the CPU
  kinds       slice stream with atomics, tile stream, dense, bf16 storage: the singular values of the matrix the handle holds
  breakdown   a NaN in v0: BREAKDOWN, u and vt untouched; the all-zero matrix: INVARIANT with nothing found
  refusals    before any launch, the outputs and the workspace bit-unchanged
"""
import numpy as np
import pytest

import gk_model as gm
import lanczos_model as lm
import step_small_cases as S
from hispmv_amd import prep
from step_small_harness import HW, SHARED

pytestmark = pytest.mark.gpu

f32 = np.float32
f64 = np.float64


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, f64).view(np.uint64)


class Ctx:
    """One context with the given matrices (scipy COO, or a dense ndarray) loaded: the pattern of test_gpu_lanczos.py, with the state
    of set_transposable the handles are created under."""

    def __init__(self, torch, mats, env=S.SLICES, transposable="companion", storage="fp32"):
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

        def run(entry, x, n_out):
            dx = self.device(x)
            dy = self.device(np.full(n_out, np.nan, f32))
            self.torch.cuda.synchronize()          # the context's stream does not wait for torch's
            entry(self.idx[k], dx.data_ptr(), 0, dy.data_ptr(), 1.0, 0.0)
            self.h.synchronize()
            return dy.cpu().numpy()
        return (lambda x, bias, alpha, beta: run(self.h.spmv_device, x, rows)), (lambda x: run(self.h.spmv_device_t, x, cols))

    def workspace(self, k, ncv):
        rows, cols = self.mats[k].shape
        gi = self.h.gk_info(self.idx[k], ncv)
        p = prep.gk(rows, cols, ncv)
        assert gi["accepted"] and all(gi[key] == p[key] for key in ("work_bytes", "v_offset", "v_stride", "u_offset", "u_stride", "gc_offset", "yt_offset")), (gi, p)
        gi.update(rows=rows, cols=cols, ncv=ncv)
        return gi, self.torch.zeros(gi["work_bytes"], dtype=self.torch.uint8, device=self.dev)

    def read(self, gi, work):
        """(V [ncv + 1, cols], U [ncv, rows], Gc [64, 66], alphas [66], betas [66]) out of a workspace"""
        host = work.cpu().numpy()
        ncv = gi["ncv"]
        V = host[gi["v_offset"]:gi["v_offset"] + 4 * gi["v_stride"] * (ncv + 1)].view(f32).reshape(ncv + 1, gi["v_stride"])[:, :gi["cols"]]
        U = host[gi["u_offset"]:gi["u_offset"] + 4 * gi["u_stride"] * ncv].view(f32).reshape(ncv, gi["u_stride"])[:, :gi["rows"]]
        gc = host[gi["gc_offset"]:gi["gc_offset"] + 66 * 66 * 8].view(f64).reshape(66, 66)
        return V, U, gc[:64], gc[64], gc[65]

    def svds(self, k, v0, kk, ncv, tol=gm.TOL, max_products=None, stream=0, vectors=True):
        """One driver call -> (s, u [found, rows], vt [found, cols], info, the two output buffers as they are afterwards)"""
        torch = self.torch
        rows, cols = self.mats[k].shape
        gi, work = self.workspace(k, ncv)
        dv = self.device(v0)
        bu = torch.full((kk, gi["u_stride"]), -7.0, dtype=torch.float32, device=self.dev)
        bv = torch.full((kk, gi["v_stride"]), -7.0, dtype=torch.float32, device=self.dev)
        torch.cuda.synchronize()
        info = self.h.svds_device(self.idx[k], kk, dv.data_ptr(), bu.data_ptr(), gi["u_stride"], bv.data_ptr(), gi["v_stride"], ncv=ncv, tol=tol,
                                  max_products=max(20 * max(rows, cols), 2000) if max_products is None else max_products, work=work.data_ptr(),
                                  work_bytes=gi["work_bytes"], stream=stream, vectors=vectors)
        torch.cuda.synchronize()
        assert np.array_equal(bits(dv.cpu().numpy()), bits(v0))          # the start vector is not written
        ou, ov = bu.cpu().numpy(), bv.cpu().numpy()
        return info["s"], ou[:info["found"], :rows], ov[:info["found"], :cols], info, (ou, ov)


# ---- steps lockstep --------------------------------------------------------------------------------------------------------------------
def same_state(cx, gi, work, V, U, st, tag):
    """the comparison of test_gpu_lanczos.py's same_state, for two bases"""
    got = cx.h.gk_status(work.data_ptr())
    assert got == st.status(), (tag, got, st.status())
    assert cx.h.gk_status(work.data_ptr()) == got          # a second read gives the same answer
    dV, dU, dGc, dalpha, dbeta = cx.read(gi, work)
    for i in range(len(V)):
        assert np.array_equal(bits(dV[i]), bits(V[i])), (tag, "V slot", i, int((bits(dV[i]) != bits(V[i])).sum()))
    for i in range(len(U)):
        assert np.array_equal(bits(dU[i]), bits(U[i])), (tag, "U slot", i, int((bits(dU[i]) != bits(U[i])).sum()))
    for j in range(st.steps + (1 if st.closed else 0)):
        assert np.array_equal(bits64(dGc[j, :j]), bits64(st.Gc[j, :j])), (tag, "Gc column", j)
    assert np.array_equal(bits64(dalpha[:st.steps]), bits64(st.alphas[:st.steps])), (tag, "alphas")
    assert np.array_equal(bits64(dbeta[:st.steps]), bits64(st.betas[:st.steps])), (tag, "betas")


LOCK_SHAPES = ((1, 5), (2, 3), (63, 64), (65, 65), (255, 300), (1025, 700))


def lock_ncv(shape):
    return 64 if shape in ((63, 64), (65, 65)) else 20


@pytest.fixture(scope="module")
def lock_ctx(torch_mod):
    with Ctx(torch_mod, [gm.graded(*shape) for shape in LOCK_SHAPES]) as cx:
        yield cx


@pytest.fixture(scope="module")
def lock_models(lock_ctx):
    """The model's run over the device's products, once per shape: (V, U, state) after steps 0 .. ncv - 1."""
    out = {}
    for k, shape in enumerate(LOCK_SHAPES):
        rows, cols = shape
        ncv = lock_ncv(shape)
        prod, prod_t = lock_ctx.products(k)
        V, U, st = np.zeros((ncv + 1, cols), f32), np.zeros((ncv, rows), f32), gm.Run()
        gm.open_run(gm.start(cols, seed=cols), V, st)
        gm.steps(prod, prod_t, V, U, 0, ncv, st)
        out[shape] = (V, U, st)
    return out


@pytest.mark.parametrize("split", [False, True], ids=["one_call", "three_calls"])
@pytest.mark.parametrize("k", range(len(LOCK_SHAPES)), ids=[f"{r}x{c}" for r, c in LOCK_SHAPES])
def test_steps_lockstep(lock_ctx, lock_models, k, split):
    cx, shape = lock_ctx, LOCK_SHAPES[k]
    rows, cols = shape
    ncv = lock_ncv(shape)
    assert cx.h.transpose_info(cx.idx[k])["atomic_bytes"] == 0          # a companion handle: both products have a fixed order
    V, U, st = lock_models[shape]
    gi, work = cx.workspace(k, ncv)
    dv = cx.device(gm.start(cols, seed=cols), 1 if split else 0)
    cx.torch.cuda.synchronize()
    for j0, j1 in (((0, 1), (1, 7), (7, ncv)) if split else ((0, ncv),)):
        cx.h.gk_steps_device(cx.idx[k], ncv, j0, j1, j0 == 0, dv.data_ptr() if j0 == 0 else 0, work.data_ptr(), gi["work_bytes"])
    same_state(cx, gi, work, V, U, st, (shape, split))
    want = {(1, 5): (1, True, 3), (2, 3): (2, True, 5), (63, 64): (63, True, 127)}.get(shape)
    if want is not None:          # the space closes on the U side: frozen there, whatever was enqueued behind it
        assert (st.steps, st.closed, st.products) == want and st.inv and not st.brk, st.status()
    else:
        assert not st.frozen and st.steps == ncv and st.products == 2 * ncv, st.status()


def test_steps_after_a_restart(lock_ctx, lock_models):
    """Steps 12 .. 19 of graded(255, 300) on a state the model made: 20 steps, the small SVD, the two rotations with keep = 12."""
    torch, cx = lock_ctx.torch, lock_ctx
    shape = (255, 300)
    k = LOCK_SHAPES.index(shape)
    rows, cols = shape
    ncv, kk = 20, 4
    prod, prod_t = cx.products(k)
    V, U, st0 = lock_models[shape]
    V, U = V.copy(), U.copy()
    st = gm.Run()
    st.steps, st.products = st0.steps, st0.products
    B = np.zeros((64, 65), f64)
    gm.fill_b(B, st0, 0, ncv, False)
    r = prep.bsvd(B[:ncv, :ncv], kk, st0.betas[ncv - 1], gm.TOL)
    keep = lm.keep_of(kk, ncv)
    assert keep == 12
    new_u, new_v, last = lm.rotate(U[:ncv], r["Pt"][:keep].astype(f32)), lm.rotate(V[:ncv], r["Qt"][:keep].astype(f32)), V[ncv].copy()
    U[:keep], V[:keep], V[keep] = new_u, new_v, last
    gi, work = cx.workspace(k, ncv)
    block = np.zeros(16, f64)
    block[10], block[13] = st.products, st.steps          # products and steps, as the header numbers the words
    work[:128] = torch.from_numpy(block.view(np.uint8)).to(cx.dev)
    for off, stride, W in ((gi["v_offset"], gi["v_stride"], V), (gi["u_offset"], gi["u_stride"], U)):
        padded = np.zeros((len(W), stride), f32)
        padded[:, :W.shape[1]] = W
        work[off:off + padded.nbytes] = torch.from_numpy(padded.reshape(-1).view(np.uint8)).to(cx.dev)
    torch.cuda.synchronize()
    cx.h.gk_steps_device(cx.idx[k], ncv, keep, ncv, False, 0, work.data_ptr(), gi["work_bytes"])
    gm.steps(prod, prod_t, V, U, keep, ncv, st)
    assert st.steps == ncv and st.products == 2 * ncv + 2 * (ncv - keep) and not st.frozen
    got = cx.h.gk_status(work.data_ptr())
    assert got == st.status(), (got, st.status())
    dV, dU, dGc, dalpha, dbeta = cx.read(gi, work)
    for i in range(ncv + 1):
        assert np.array_equal(bits(dV[i]), bits(V[i])), ("V slot", i)
    for i in range(ncv):
        assert np.array_equal(bits(dU[i]), bits(U[i])), ("U slot", i)
    for j in range(keep, ncv):
        assert np.array_equal(bits64(dGc[j, :j]), bits64(st.Gc[j, :j])), ("Gc column", j)
    assert np.array_equal(bits64(dalpha[keep:ncv]), bits64(st.alphas[keep:ncv])) and np.array_equal(bits64(dbeta[keep:ncv]), bits64(st.betas[keep:ncv]))
    # the arrow column comes out of the U-side dots by itself
    assert np.abs(st.Gc[keep, :keep] - st0.betas[ncv - 1] * r["Pt"][:keep, ncv - 1]).max() <= 1e-5 * r["s"][0]


# ---- the driver --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(gm.GPU_CASES))
def test_svds_lockstep_and_accuracy(torch_mod, name):
    case = gm.CASES[name]
    A = case["make"]()
    rows, cols = A.shape
    with Ctx(torch_mod, [A]) as cx:
        v0 = gm.start(cols)
        s, u, vt, info, (ou, ov) = cx.svds(0, v0, case["k"], case["ncv"])
        ms, mu, mvt, minfo = gm.svds(*cx.products(0), prep.bsvd, v0, case["k"], case["ncv"], gm.TOL, max(20 * max(rows, cols), 2000), rows)
    res, err = gm.accuracy(A, s, u, vt, info["status"]) if info["found"] else (0.0, 0.0)
    print(f"{ {key: info[key] for key in ('status', 'found', 'products', 'cycles')} }, true residual {res:.3e}, singular-value error {err:.3e}, "
          f"recorded on the CPU {case['attained']}")
    for key in ("status", "found", "products", "cycles"):
        assert info[key] == minfo[key], (key, info, minfo)
    assert (info["status"], info["found"]) == (case["status"], case["found"]) and info["products"] <= 2 * case["prototype"], info
    assert np.array_equal(bits64(s), bits64(ms)) and np.array_equal(bits64(info["residuals"]), bits64(minfo["residuals"])), (s, ms)
    assert info["scale"] == minfo["scale"]
    assert np.array_equal(bits(u), bits(mu)), int((bits(u) != bits(mu)).sum())
    assert np.array_equal(bits(vt), bits(mvt)), int((bits(vt) != bits(mvt)).sum())
    assert res <= 2 * case["attained"][0] and err <= 2 * case["attained"][1], (res, err, case["attained"])
    assert (ou[info["found"]:] == -7.0).all() and (ov[info["found"]:] == -7.0).all()          # the rows behind `found` are not written


KINDS = {
    "slices_atomic": dict(env=S.SLICES, transposable=True),
    "tile_stream": dict(env=S.TTS, transposable="keep_format"),
    "dense_96x64": dict(env=S.SLICES, transposable=True),
    "bf16_storage": dict(env=S.SLICES, transposable=True, storage="bf16"),
}


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_handle_kinds(torch_mod, kind):
    """k = 4, ncv = 20: CONVERGED to the singular values of the matrix the handle holds, within twice what the model attains with scipy
    products on the CPU (tests/test_gk_host.py pins those figures); no bit claim on these routes, whose transposed product adds
    through atomics."""
    case = dict(gm.KIND_CASES[kind], **KINDS[kind])
    A_true = case["make"]()          # what the handle holds; a bf16 handle is created from the values before rounding
    A = gm.graded(1025, 700) if kind == "bf16_storage" else A_true
    with Ctx(torch_mod, [A], env=case["env"], transposable=case["transposable"], storage=case.get("storage", "fp32")) as cx:
        info = cx.h.matrix_info(cx.idx[0])
        if kind == "tile_stream":
            assert info["format"] == 1, info
        elif kind == "dense_96x64":
            assert info["is_dense"] and A.shape == (96, 64), info
        elif kind == "bf16_storage":
            assert cx.h.value_storage_info(cx.idx[0])["storage"] == "bf16" and (A_true.data != A.data).any()
        else:
            assert not cx.h.companion_info(cx.idx[0])["has"] and cx.h.transpose_info(cx.idx[0])["transposable"]
        s, u, vt, out, _ = cx.svds(0, gm.start(A.shape[1]), 4, 20)
    res, err = gm.accuracy(A_true, s, u, vt, out["status"])
    print(f"{kind}: {out['status']}, {out['products']} products, {out['cycles']} cycles, true residual {res:.3e}, singular-value error {err:.3e}")
    assert out["status"] == "CONVERGED" and out["found"] == 4, out
    assert res <= 2 * case["attained"][0] and err <= 2 * case["attained"][1], (res, err, case["attained"])


def test_a_default_switch_tile_stream_is_refused_before_any_launch(torch_mod):
    torch = torch_mod
    A = gm.tile_stream_rectangular()
    with Ctx(torch, [A], env=S.TTS, transposable=None) as cx:
        assert cx.h.matrix_info(cx.idx[0])["format"] == 1 and not cx.h.gk_info(cx.idx[0], 20)["accepted"]
        need = prep.gk(*A.shape, 20)["work_bytes"]
        pattern = (torch.arange(need, device=cx.dev) % 251).to(torch.uint8)
        work = pattern.clone()
        dv = cx.device(gm.start(A.shape[1]))
        bu = torch.full((4, A.shape[0]), -7.0, dtype=torch.float32, device=cx.dev)
        bv = torch.full((4, A.shape[1]), -7.0, dtype=torch.float32, device=cx.dev)
        with pytest.raises(NotImplementedError, match="spmv_device_t"):
            cx.h.svds_device(cx.idx[0], 4, dv.data_ptr(), bu.data_ptr(), A.shape[0], bv.data_ptr(), A.shape[1], ncv=20, work=work.data_ptr(), work_bytes=need)
        with pytest.raises(NotImplementedError, match="spmv_device_t"):
            cx.h.gk_steps_device(cx.idx[0], 20, 0, 4, True, dv.data_ptr(), work.data_ptr(), need)
        torch.cuda.synchronize()
        assert torch.equal(work, pattern) and bool((bu == -7.0).all()) and bool((bv == -7.0).all())


# ---- breakdown and refusals --------------------------------------------------------------------------------------------------------------
def test_breakdown_leaves_the_vectors_untouched_and_a_zero_matrix_is_not_one(torch_mod):
    A = gm.graded(300, 200)
    v0 = gm.start(200)
    nan_v0 = v0.copy()
    nan_v0[7] = np.nan
    with Ctx(torch_mod, [A, gm.zero_pattern()]) as cx:
        for start in (nan_v0, np.zeros(200, f32)):
            s, u, vt, info, (ou, ov) = cx.svds(0, start, 3, 10)
            assert info["status"] == "BREAKDOWN" and info["found"] == 0 and len(s) == 0 and len(info["residuals"]) == 0, info
            assert (ou == -7.0).all() and (ov == -7.0).all()
        s, u, vt, info, (ou, ov) = cx.svds(1, gm.start(30), 2, 8)
        assert info["status"] == "INVARIANT" and info["found"] == 0 and info["products"] == 1 and len(s) == 0, info
        assert (ou == -7.0).all() and (ov == -7.0).all()


def test_refusals_come_before_any_launch(torch_mod):
    torch = torch_mod
    A = gm.graded(300, 200)
    v0 = gm.start(200)
    with Ctx(torch, [A]) as cx:
        for ncv in (1, 65, 0):
            with pytest.raises(ValueError):
                cx.h.gk_info(cx.idx[0], ncv)
        with pytest.raises(IndexError):
            cx.h.gk_info(99, 20)
        gi = cx.h.gk_info(cx.idx[0], 20)
        need = gi["work_bytes"]
        assert need < cx.h.gk_info(cx.idx[0], 21)["work_bytes"]
        pattern = (torch.arange(need + 64, device=cx.dev) % 251).to(torch.uint8)
        work = pattern.clone()
        dv = cx.device(v0)
        bu = torch.full((4, gi["u_stride"]), -7.0, dtype=torch.float32, device=cx.dev)
        bv = torch.full((4, gi["v_stride"]), -7.0, dtype=torch.float32, device=cx.dev)
        base = dict(ncv=20, tol=1e-5, max_products=1000, work=work.data_ptr(), work_bytes=need)

        def call(idx=cx.idx[0], k=4, v0=dv.data_ptr(), u=bu.data_ptr(), ld_u=gi["u_stride"], v=bv.data_ptr(), ld_v=gi["v_stride"], **kw):
            return cx.h.svds_device(idx, k, v0, u, ld_u, v, ld_v, **dict(base, **kw))
        for kw in (dict(k=0), dict(k=201, ncv=64), dict(k=64, ncv=64), dict(ncv=4), dict(ncv=65), dict(tol=-1.0),
                   dict(tol=float("nan")), dict(max_products=1), dict(max_products=(1 << 30) + 1), dict(v0=0), dict(u=0), dict(v=0),
                   dict(v0=dv.data_ptr() + 2), dict(u=bu.data_ptr() + 1), dict(v=bv.data_ptr() + 2), dict(ld_u=299), dict(ld_v=199), dict(work=0),
                   dict(work_bytes=need - 1), dict(work=work.data_ptr() + 4)):
            with pytest.raises(ValueError):
                call(**kw)
        with pytest.raises(IndexError):
            call(idx=99)
        for kw in (dict(j0=0, j1=0), dict(j0=3, j1=2), dict(j0=0, j1=21), dict(j0=-1, j1=2), dict(j0=2, j1=4, first=True), dict(d_v0=0, first=True),
                   dict(ncv=1), dict(ncv=65), dict(work_bytes=need - 1)):
            a = dict(ncv=20, j0=0, j1=20, first=True, d_v0=dv.data_ptr(), work_bytes=need)
            a.update(kw)
            with pytest.raises(ValueError):
                cx.h.gk_steps_device(cx.idx[0], a["ncv"], a["j0"], a["j1"], a["first"], a["d_v0"], work.data_ptr(), a["work_bytes"])
        with pytest.raises(ValueError):
            cx.h.gk_status(work.data_ptr() + 8)
        torch.cuda.synchronize()
        assert torch.equal(work, pattern) and bool((bu == -7.0).all()) and bool((bv == -7.0).all())
        assert np.array_equal(bits(dv.cpu().numpy()), bits(v0))


def test_k_may_not_exceed_the_smaller_dimension(torch_mod):
    with Ctx(torch_mod, [gm.graded(5, 3)]) as cx:
        gi, work = cx.workspace(0, 8)
        dv = cx.device(gm.start(3))
        b = cx.torch.full((4, 8), -7.0, dtype=cx.torch.float32, device=cx.dev)
        with pytest.raises(ValueError, match="smaller"):
            cx.h.svds_device(cx.idx[0], 4, dv.data_ptr(), b.data_ptr(), 8, b.data_ptr(), 8, ncv=8, work=work.data_ptr(), work_bytes=gi["work_bytes"])
        assert bool((b == -7.0).all()) and not bool(work.any())


def test_refused_before_load_matrices(torch_mod):
    import pyhispmv
    A = gm.graded(64, 48)
    h = pyhispmv.FpgaHandle(*HW)
    try:
        h.set_transposable("companion")
        i = h.create_sparse_handle(A.row, A.col, A.data, 64, 48)
        d = torch_mod.zeros(1 << 20, dtype=torch_mod.float32, device="cuda")
        assert not h.gk_info(i, 20)["accepted"]
        with pytest.raises(AssertionError, match="before load_matrices"):
            h.svds_device(i, 2, d.data_ptr(), d.data_ptr() + 1024, 64, d.data_ptr() + 2048, 48, work=d.data_ptr() + 4096, work_bytes=(4 << 20) - 4096)
        with pytest.raises(AssertionError, match="before load_matrices"):
            h.gk_steps_device(i, 20, 0, 4, True, d.data_ptr(), d.data_ptr() + 4096, (4 << 20) - 4096)
    finally:
        h.close()


# ---- hispmv_amd.solvers.svds ---------------------------------------------------------------------------------------------------------------
def test_torch_front_end_on_a_side_stream_and_on_the_default_stream(torch_mod):
    """The answer of the device entry by another door: on a side stream everything is ordered there; on torch's default stream
    solvers.svds orders the two itself, also for a start vector still queued behind a long kernel."""
    from hispmv_amd import solvers
    torch = torch_mod
    case = gm.CASES["graded_1025x700"]
    A = case["make"]()
    rows, cols = A.shape
    v0n = gm.start(cols)
    kw = dict(ncv=case["ncv"], tol=gm.TOL)
    with Ctx(torch, [A]) as cx:
        ws, wu, wvt, winfo, _ = cx.svds(0, v0n, case["k"], case["ncv"])
        assert winfo["status"] == "CONVERGED"
        tv = torch.from_numpy(v0n).to(cx.dev)

        def same(s, u, vt, info):
            assert isinstance(s, np.ndarray) and s.dtype == np.float64 and u.dtype == torch.float32 and u.is_cuda and vt.is_cuda
            assert tuple(u.shape) == (rows, winfo["found"]) and tuple(vt.shape) == (winfo["found"], cols)
            assert set(info) == {"status", "found", "products", "cycles", "residuals", "scale", "work"}
            assert all(info[key] == winfo[key] for key in ("status", "found", "products", "cycles", "scale")), (info, winfo)
            assert np.array_equal(bits64(s), bits64(ws)) and np.array_equal(bits64(info["residuals"]), bits64(winfo["residuals"]))
            assert np.array_equal(bits(u.t().cpu().numpy()), bits(wu)) and np.array_equal(bits(vt.cpu().numpy()), bits(wvt))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            out = solvers.svds(cx.h, cx.idx[0], case["k"], v0=tv, **kw)
        side.synchronize()
        same(*out)
        assert torch.cuda.current_stream().cuda_stream == 0
        long = torch.ones(1 << 26, dtype=torch.float32, device=cx.dev)
        torch.cuda.synchronize()
        for _ in range(4):          # some milliseconds of work on the default stream, and the start vector queued behind it
            long = long.sin()
        v0 = tv * 2.0 - tv
        s, u, vt, info = solvers.svds(cx.h, cx.idx[0], case["k"], v0=v0, **kw)
        same(s, u, vt, info)
        assert np.array_equal(bits(v0.cpu().numpy()), bits(v0n))          # the caller's v0 is not written
        eye = torch.eye(len(s), device=cx.dev)
        assert float((u.t() @ u - eye).abs().max()) <= 1e-4 and float((vt @ vt.t() - eye).abs().max()) <= 1e-4
        # without the vectors: the same values, None for the vectors
        s2, u2, vt2, info2 = solvers.svds(cx.h, cx.idx[0], case["k"], v0=tv, return_vectors=False, **kw)
        assert u2 is None and vt2 is None and np.array_equal(bits64(s2), bits64(ws)) and info2["products"] == winfo["products"]
        norm = solvers.spectral_norm(cx.h, cx.idx[0])
        s1 = solvers.svds(cx.h, cx.idx[0], 1, tol=1e-4, return_vectors=False)[0]
        assert isinstance(norm, float) and norm == s1[0] and abs(norm - ws[0]) <= 4e-4 * ws[0]
        a = solvers.svds(cx.h, cx.idx[0], 2, seed=5)
        b = solvers.svds(cx.h, cx.idx[0], 2, seed=5)
        c = solvers.svds(cx.h, cx.idx[0], 2, seed=6)
        assert a[3]["status"] == "CONVERGED" and np.array_equal(bits64(a[0]), bits64(b[0])) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
        assert a[3]["products"] == b[3]["products"] and not torch.equal(a[2], c[2])
        assert np.abs(a[0] - c[0]).max() <= 4 * gm.TOL * a[0][0]          # another start, the same singular values
        with pytest.raises(TypeError):
            solvers.svds(cx.h, cx.idx[0], 2, v0=tv.double())
        with pytest.raises(ValueError):
            solvers.svds(cx.h, cx.idx[0], 2, v0=tv[:-1].contiguous())
