"""Thick-restart Lanczos on the device (include/hispmv.h: hispmv_basis_rotate_device, hispmv_lanczos_steps_device, hispmv_lanczos_status,
hispmv_eigsh_device, hispmv_lanczos_info) against the numpy model of tests/lanczos_model.py.

  rotate      every output bit-equal to the model's, in place and out of place, for every (m, k) around the kernel's register buckets,
              ld and alignment; NaN pads never read, slots at or above k untouched in place
  steps       basis slots, Hc columns, betas and status bit for bit the model's, the model driven by the products spmv_device itself
              returns; invariant subspaces freeze at the model's step and no vector kernel writes a later slot
  eigsh       status, found, products, cycles, values, residual estimates and vectors bit for bit the model's (library products,
              prep.ritz); the fp64 true residual and the eigenvalue error under twice what the model attains on the CPU (lm.CASES)
  kinds       tile stream, dense, bf16 storage: the eigenvalues of the matrix the handle holds
  breakdown   a NaN in v0, v0 = 0, a NaN among the values: BREAKDOWN, vecs untouched; the all-zero matrix: eigenvalue 0
  refusals    before any launch, the outputs and the workspace bit-unchanged
"""
import numpy as np
import pytest
import scipy.sparse as sp

import krylov_model as km
import lanczos_model as lm
import step_small_cases as S
from hispmv_amd import prep
from step_small_harness import HW, SHARED

pytestmark = pytest.mark.gpu

f32 = np.float32
f64 = np.float64
TILE = prep.gmres(1024, 30)["dot_tile"]


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
    """One context with the given matrices (scipy COO, or a dense ndarray) loaded: the pattern of test_gpu_gmres.py."""

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
            dy = self.device(np.full(rows, np.nan, f32))
            self.torch.cuda.synchronize()          # the context's stream does not wait for torch's
            self.h.spmv_device(self.idx[k], dx.data_ptr(), 0, dy.data_ptr(), alpha, beta)
            self.h.synchronize()
            return dy.cpu().numpy()
        return prod

    def workspace(self, k, ncv):
        n = self.mats[k].shape[0]
        li = self.h.lanczos_info(self.idx[k], ncv)
        p = prep.lanczos(n, ncv)
        assert li["accepted"] and li["n"] == n and li["launches_per_step"] == 5, li
        assert all(li[key] == p[key] for key in ("work_bytes", "v_offset", "stride", "hc_offset", "yt_offset")), (li, p)
        return li, self.torch.zeros(li["work_bytes"], dtype=self.torch.uint8, device=self.dev)

    def read(self, li, work, slots):
        """(basis [slots, n], Hc [64, 66], betas [66]) out of a workspace"""
        n, stride = li["n"], li["stride"]
        host = work.cpu().numpy()
        V = host[li["v_offset"]:li["v_offset"] + 4 * stride * slots].view(f32).reshape(slots, stride)[:, :n]
        hc = host[li["hc_offset"]:li["hc_offset"] + 65 * 66 * 8].view(f64).reshape(65, 66)
        return V, hc[:64], hc[64]

    def eigsh(self, k, v0, kk, ncv, which, tol=lm.TOL, max_products=None, stream=0):
        """One driver call -> (vals, vecs [found, n], info, the k rows of the output buffer as they are afterwards)"""
        torch = self.torch
        n = len(v0)
        li, work = self.workspace(k, ncv)
        dv = self.device(v0)
        rows = torch.full((kk, li["stride"]), -7.0, dtype=torch.float32, device=self.dev)
        torch.cuda.synchronize()
        info = self.h.eigsh_device(self.idx[k], kk, dv.data_ptr(), rows.data_ptr(), li["stride"], ncv=ncv, which=which, tol=tol,
                                   max_products=max(10 * n, 1000) if max_products is None else max_products, work=work.data_ptr(),
                                   work_bytes=li["work_bytes"], stream=stream)
        torch.cuda.synchronize()
        assert np.array_equal(bits(dv.cpu().numpy()), bits(v0))          # the start vector is not written
        out = rows.cpu().numpy()
        return info["vals"], out[:info["found"], :n], info, out


# ---- basis_rotate_device -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_ctx(torch_mod):
    with Ctx(torch_mod, [km.tridiag(8)]) as cx:
        yield cx


MK = ((1, 1), (2, 1), (9, 8), (20, 12), (64, 36), (65, 64))
SPLIT = 256 * 1024          # below this n the kernel splits the columns over a workgroup's wavefronts (hispmv_lanczos.h: kRotateSplitBelow)
BIG = 1024 * 1024 + 1029


def rotate_sample(n, rng):
    """The elements whose bits are compared: all of them up to n = 8192; above, the first and the last 1024, a stretch across 24
    boundaries of the 128 elements a wavefront serves and across 24 of the 512 a workgroup serves, and 2048 drawn at random.  The
    model is element-wise, so a subset of its columns is the same reference."""
    if n <= 8192:
        return np.arange(n)
    parts = [np.arange(1024), np.arange(n - 1024, n), rng.integers(0, n, 2048)]
    for unit in (128, 512):
        for b in rng.integers(1, n // unit, 24) * unit:
            parts.append(np.arange(b - 70, b + 70))
    return np.unique(np.concatenate(parts))


def shifted_clone(torch, t, shift):
    """a copy of the device vector t, `shift` floats off the 16-byte alignment of its allocation"""
    c = torch.empty(t.numel() + shift + 4, dtype=t.dtype, device=t.device)[shift:shift + t.numel()]
    c.copy_(t)
    return c


def same_bits(torch, a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("n", (1, 3, 255, 1023, 1025, 4099, SPLIT - 1, SPLIT + 5, BIG))
def test_basis_rotate_device(torch_mod, small_ctx, n):
    """Every (m, k) at every n: the small n and SPLIT - 1 take the kernels that split the columns, SPLIT + 5 and the largest n those
    that do not.  Above n = 8192 the bits are compared on the elements of rotate_sample, every element is held against torch's own
    product to a rounding bound, and the pads and the untouched slots are checked over the full vectors, on the device."""
    torch, cx = torch_mod, small_ctx
    rng = np.random.default_rng(n)
    slots = max(m for m, k in MK)
    V = rng.standard_normal((slots, n), dtype=f32)
    stride = (n + 3) // 4 * 4
    idx = rotate_sample(n, rng)
    tidx = torch.from_numpy(idx).to(cx.dev)
    Vs = np.ascontiguousarray(V[:, idx])
    wants = {}
    for ld, shift in ((stride, 0), (stride + 1, 1)):
        host = np.full(slots * ld, np.nan, f32)          # the pads between two vectors are never read
        for i in range(slots):
            host[i * ld:i * ld + n] = V[i]
        pristine = cx.device(host, shift)
        for m, k in MK:
            if (m, k) not in wants:          # once per (n, m, k): a value depends neither on ld, on the alignment nor on the place
                Yt = rng.standard_normal((k, m), dtype=f32)
                wants[(m, k)] = (Yt, lm.rotate(Vs[:m], Yt))
            Yt, want = wants[(m, k)]
            dY = cx.device(Yt.flatten())
            P = pristine.view(slots, ld)[:m, :n]
            near = torch.from_numpy(Yt).to(cx.dev) @ P
            slack = (m + 2) * 2.0 ** -23 * (torch.from_numpy(np.abs(Yt)).to(cx.dev) @ P.abs()) + 1e-30
            for in_place in (False, True):
                dV = shifted_clone(torch, pristine, shift)
                dO = dV if in_place else cx.device(np.full(k * ld + 8, np.nan, f32), shift)
                torch.cuda.synchronize()
                cx.h.basis_rotate_device(n, m, k, dV.data_ptr(), dY.data_ptr(), dO.data_ptr(), ld_v=ld, ld_out=ld)
                cx.h.synchronize()
                tag = (n, m, k, ld, shift, in_place)
                R = dO[:k * ld].view(k, ld)
                got = R[:, :n][:, tidx].cpu().numpy()
                for c in range(k):
                    assert np.array_equal(bits(got[c]), bits(want[c])), (tag, c, int((bits(got[c]) != bits(want[c])).sum()))
                assert bool(((R[:, :n] - near).abs() <= slack).all()), (tag, "an element off torch's product")
                assert bool(torch.isnan(R[:, n:]).all()), (tag, "pads")
                if in_place:          # slots at or above k are untouched
                    assert same_bits(torch, dV[k * ld:], pristine[k * ld:]), tag
                else:
                    assert bool(torch.isnan(dO[k * ld:]).all()), tag
                    assert same_bits(torch, dV, pristine), tag
    args = (dV.data_ptr(), dY.data_ptr(), dO.data_ptr())
    for bad in (dict(m=0, k=1), dict(m=66, k=1), dict(m=4, k=0), dict(m=4, k=65)):
        with pytest.raises(ValueError):
            cx.h.basis_rotate_device(n, bad["m"], bad["k"], *args, ld_v=ld, ld_out=ld)
    if n > 1:
        with pytest.raises(ValueError):
            cx.h.basis_rotate_device(n, 4, 2, *args, ld_v=n - 1, ld_out=ld)
    with pytest.raises(ValueError):
        cx.h.basis_rotate_device(n, 4, 2, dV.data_ptr() + 2, dY.data_ptr(), dO.data_ptr(), ld_v=ld, ld_out=ld)
    with pytest.raises(ValueError):
        cx.h.basis_rotate_device(n, 4, 2, dV.data_ptr(), 0, dO.data_ptr(), ld_v=ld, ld_out=ld)
    with pytest.raises(ValueError):
        cx.h.basis_rotate_device(n, 4, 2, dV.data_ptr(), dY.data_ptr(), dV.data_ptr(), ld_v=ld, ld_out=ld + 4)


# ---- steps lockstep --------------------------------------------------------------------------------------------------------------------
def same_state(cx, li, work, V, st, slots, tag):
    got = cx.h.lanczos_status(work.data_ptr())
    assert got == st.status(), (tag, got, st.status())
    assert cx.h.lanczos_status(work.data_ptr()) == got          # a second read gives the same answer
    dV, dHc, dbeta = cx.read(li, work, slots)
    for i in range(slots):
        assert np.array_equal(bits(dV[i]), bits(V[i])), (tag, "basis slot", i, int((bits(dV[i]) != bits(V[i])).sum()))
    for j in range(st.steps):
        assert np.array_equal(bits64(dHc[j, :j + 1]), bits64(st.Hc[j, :j + 1])), (tag, "Hc column", j)
    assert np.array_equal(bits64(dbeta[:st.steps]), bits64(st.betas[:st.steps])), (tag, "betas")


def steps_lockstep(cx, k, spans):
    n = cx.mats[k].shape[0]
    v0 = lm.start(n, seed=n)
    prod = cx.products(k)
    for j1, shift in spans:
        li, work = cx.workspace(k, max(j1, 2))
        dv = cx.device(v0, shift)
        cx.torch.cuda.synchronize()
        cx.h.lanczos_steps_device(cx.idx[k], 0, j1, True, dv.data_ptr(), work.data_ptr(), li["work_bytes"])
        V, st = np.zeros((max(j1, 2) + 1, n), f32), lm.Run()
        lm.open_run(v0, V, st)
        lm.steps(prod, V, 0, j1, st)
        same_state(cx, li, work, V, st, j1 + 1, (n, j1, shift))
    return st


@pytest.fixture(scope="module")
def lock_ctx(torch_mod):
    with Ctx(torch_mod, [km.tridiag(n) for n in km.TRIDIAG_SIZES] + [km.arrow(5000)]) as cx:
        yield cx


SPANS = ((1, 0), (3, 1), (TILE + 2, 0), (64, 1))


@pytest.mark.parametrize("k", range(len(km.TRIDIAG_SIZES)), ids=[str(n) for n in km.TRIDIAG_SIZES])
def test_steps_lockstep_tridiag(lock_ctx, k):
    n = km.TRIDIAG_SIZES[k]
    st = steps_lockstep(lock_ctx, k, SPANS)
    if n <= 64:          # the Krylov space closes at step n: frozen there, whatever was enqueued behind it
        assert st.inv and not st.brk and st.steps == n and st.products == n, st.status()
    else:
        assert not st.frozen and st.steps == 64 and st.products == 64, st.status()


def test_steps_lockstep_arrow_whose_first_row_is_cut_by_five_slices(lock_ctx):
    k = len(km.TRIDIAG_SIZES)
    assert lock_ctx.h.matrix_info(lock_ctx.idx[k])["n_split_rows"] >= 1
    st = steps_lockstep(lock_ctx, k, ((1, 0), (3, 0), (TILE + 2, 1)))
    assert st.inv and st.steps == 3 and st.products == 3, st.status()          # 2.5 I plus rank two: three steps, then rounding noise
    ratio = lm.invariance_ratio(st, 2)
    print(f"arrow(5000), library products: invariance ratio {ratio:.3e} at step 2, tiny {2.0 ** -12:.3e}")
    assert ratio <= 2.0 ** -12          # rounding noise of w: below tiny, which is what freezes the run


def test_steps_after_a_restart(lock_ctx):
    """Steps 12 .. 19 on a state the model made: 20 steps, the Ritz step, the rotation with keep = 12."""
    torch, cx = lock_ctx.torch, lock_ctx
    k = km.TRIDIAG_SIZES.index(1025)
    n, ncv, kk = 1025, 20, 4
    prod = cx.products(k)
    v0 = lm.start(n)
    V, st = np.zeros((ncv + 1, n), f32), lm.Run()
    lm.open_run(v0, V, st)
    lm.steps(prod, V, 0, ncv, st)
    H = np.zeros((64, 64), f64)
    lm.mirror(H, st, 0, ncv)
    r = prep.ritz(H[:ncv, :ncv], kk, "LA", st.betas[ncv - 1], lm.TOL)
    keep = lm.keep_of(kk, ncv)
    assert keep == 12
    new, last = lm.rotate(V[:ncv], r["Yt"][:keep].astype(f32)), V[ncv].copy()
    V[:keep], V[keep] = new, last
    li, work = cx.workspace(k, ncv)
    block = np.zeros(16, f64)
    block[10], block[13] = st.products, st.steps          # products and steps, as the header numbers the words
    work[:128] = torch.from_numpy(block.view(np.uint8)).to(cx.dev)
    padded = np.zeros((ncv + 1, li["stride"]), f32)
    padded[:, :n] = V
    work[li["v_offset"]:li["v_offset"] + padded.nbytes] = torch.from_numpy(padded.reshape(-1).view(np.uint8)).to(cx.dev)
    torch.cuda.synchronize()
    cx.h.lanczos_steps_device(cx.idx[k], keep, ncv, False, 0, work.data_ptr(), li["work_bytes"])
    lm.steps(prod, V, keep, ncv, st)
    assert st.steps == ncv and st.products == 2 * ncv - keep and not st.frozen
    got = cx.h.lanczos_status(work.data_ptr())
    assert got == st.status(), (got, st.status())
    dV, dHc, dbeta = cx.read(li, work, ncv + 1)
    for i in range(ncv + 1):
        assert np.array_equal(bits(dV[i]), bits(V[i])), ("basis slot", i)
    for j in range(keep, ncv):
        assert np.array_equal(bits64(dHc[j, :j + 1]), bits64(st.Hc[j, :j + 1])), ("Hc column", j)
    assert np.array_equal(bits64(dbeta[keep:ncv]), bits64(st.betas[keep:ncv]))
    # the arrowhead column comes out of the dots by itself: beta_19 * Y[19, c] of the look, to fp32 rounding of the vectors
    arrow = st.Hc[keep, :keep]
    assert np.abs(np.abs(arrow) - r["res"][:keep]).max() <= 1e-5 * np.abs(r["theta"]).max()


# ---- the driver --------------------------------------------------------------------------------------------------------------------------
def eigsh_lockstep(cx, k, case, A_true=None):
    A = cx.mats[k] if A_true is None else A_true
    n = A.shape[0]
    v0 = lm.start(n)
    vals, vecs, info, _ = cx.eigsh(k, v0, case["k"], case["ncv"], case["which"])
    mvals, mvecs, minfo = lm.eigsh(cx.products(k), prep.ritz, v0, case["k"], case["ncv"], case["which"], lm.TOL, max(10 * n, 1000))
    res, err = lm.accuracy(A, vals, vecs, case["k"], case["which"], info["status"])
    print(f"{ {key: info[key] for key in ('status', 'found', 'products', 'cycles')} }, true residual {res:.3e}, eigenvalue error {err:.3e}, "
          f"recorded on the CPU {case['attained']}")
    for key in ("status", "found", "products", "cycles"):
        assert info[key] == minfo[key], (key, info, minfo)
    assert (info["status"], info["found"]) == (case["status"], case["found"]) and info["products"] <= 2 * case["prototype"], info
    assert np.array_equal(bits64(vals), bits64(mvals)) and np.array_equal(bits64(info["residuals"]), bits64(minfo["residuals"])), (vals, mvals)
    assert info["scale"] == minfo["scale"]
    assert np.array_equal(bits(vecs), bits(mvecs)), int((bits(vecs) != bits(mvecs)).sum())
    assert res <= 2 * case["attained"][0] and err <= 2 * case["attained"][1], (res, err, case["attained"])
    norms = np.linalg.norm(vecs.astype(f64), axis=1)
    assert np.abs(norms - 1.0).max() <= 64 * 2.0 ** -23, norms          # not renormalised: 1 to a few fp32 ulps
    return info


@pytest.mark.parametrize("name", sorted(lm.GPU_CASES))
def test_eigsh_lockstep_and_accuracy(torch_mod, name):
    case = lm.CASES[name]
    with Ctx(torch_mod, [case["make"]()]) as cx:
        eigsh_lockstep(cx, 0, case)


ATT_TILE, ATT_DENSE, ATT_BF16 = (8.15e-6, lm.FLOOR), (2.15e-7, lm.FLOOR), (3.26e-6, lm.FLOOR)
KINDS = {
    "tile_stream": dict(make=lm.tile_stream_symmetric, env=S.TTS, attained=ATT_TILE),
    "dense_96": dict(make=lm.dense_symmetric, env=S.SLICES, attained=ATT_DENSE),
    "bf16_storage": dict(make=lambda: lm.ramp(1025), env=S.SLICES, storage="bf16", attained=ATT_BF16),
}


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_handle_kinds(torch_mod, kind):
    """k = 4, LA, ncv = 20: CONVERGED to the eigenvalues of the matrix the handle holds, within twice what the model attains with
    scipy products on the CPU."""
    case = KINDS[kind]
    A = case["make"]()
    A_true = A
    if kind == "bf16_storage":
        A_true = sp.coo_matrix((S.bf16_exact(A.data.astype(f32)), (A.row, A.col)), shape=A.shape)
    with Ctx(torch_mod, [A], env=case["env"], storage=case.get("storage", "fp32")) as cx:
        info = cx.h.matrix_info(cx.idx[0])
        if kind == "tile_stream":
            assert info["format"] == 1, info
        elif kind == "dense_96":
            assert info["is_dense"] and np.array_equal(A, A.T), info
        else:
            assert cx.h.value_storage_info(cx.idx[0])["storage"] == "bf16" and (A_true.data != A.data).any()
        n = A.shape[0]
        vals, vecs, out, _ = cx.eigsh(0, lm.start(n), 4, 20, "LA")
        res, err = lm.accuracy(A_true, vals, vecs, 4, "LA", out["status"])
        print(f"{kind}: {out['status']}, {out['products']} products, {out['cycles']} cycles, true residual {res:.3e}, eigenvalue error {err:.3e}")
        assert out["status"] == "CONVERGED" and out["found"] == 4, out
        assert res <= 2 * case["attained"][0] and err <= 2 * case["attained"][1], (res, err, case["attained"])


# ---- breakdown and refusals --------------------------------------------------------------------------------------------------------------
def test_breakdown_leaves_vecs_untouched_and_a_zero_matrix_is_not_one(torch_mod):
    n = 300
    v0 = lm.start(n)
    nan_v0 = v0.copy()
    nan_v0[7] = np.nan
    A_nan = km.tridiag(n)
    A_nan.data[5] = np.nan
    with Ctx(torch_mod, [km.tridiag(n), A_nan, km.zero_pattern(n)]) as cx:
        for k, start in ((0, nan_v0), (0, np.zeros(n, f32)), (1, v0)):
            vals, vecs, info, out = cx.eigsh(k, start, 3, 10, "LA")
            assert info["status"] == "BREAKDOWN" and info["found"] == 0 and len(vals) == 0 and len(info["residuals"]) == 0, (k, info)
            assert (out == -7.0).all(), k
        vals, vecs, info, out = cx.eigsh(2, v0, 3, 10, "LA")
        assert info["status"] in ("INVARIANT", "CONVERGED") and info["found"] == 1 and info["products"] == 1, info
        assert vals[0] == 0.0 and info["residuals"][0] == 0.0
        assert np.array_equal(bits(vecs[0]), bits(lm.rotate(np.array([f32(1.0 / np.sqrt(km.dot(v0, v0))) * v0]), np.ones((1, 1), f32))[0]))
        assert (out[1:] == -7.0).all()


def test_refusals_come_before_any_launch(torch_mod):
    torch = torch_mod
    tall = km.least_squares(300, 200)
    v300 = lm.start(300)
    with Ctx(torch, [tall, km.tridiag(300)]) as cx:
        assert not cx.h.lanczos_info(cx.idx[0], 20)["accepted"]
        for ncv in (1, 65, 0):
            with pytest.raises(ValueError):
                cx.h.lanczos_info(cx.idx[1], ncv)
        with pytest.raises(IndexError):
            cx.h.lanczos_info(99, 20)
        li = cx.h.lanczos_info(cx.idx[1], 20)
        need = li["work_bytes"]
        assert need < cx.h.lanczos_info(cx.idx[1], 21)["work_bytes"]
        pattern = torch.arange(need + 64, device=cx.dev).to(torch.uint8)
        work = pattern.clone()
        dv = cx.device(v300)
        rows = torch.full((4, li["stride"]), -7.0, dtype=torch.float32, device=cx.dev)
        base = dict(ncv=20, which="LA", tol=1e-5, max_products=1000, work=work.data_ptr(), work_bytes=need)

        def call(idx=cx.idx[1], k=4, v0=dv.data_ptr(), vecs=rows.data_ptr(), ld=li["stride"], **kw):
            return cx.h.eigsh_device(idx, k, v0, vecs, ld, **dict(base, **kw))
        with pytest.raises(ValueError, match="square"):
            call(idx=cx.idx[0])
        for kw in (dict(k=0), dict(ncv=4), dict(ncv=65), dict(k=64, ncv=64), dict(tol=-1.0), dict(tol=float("nan")), dict(max_products=0), dict(which="XX"),
                   dict(v0=0), dict(vecs=0), dict(v0=dv.data_ptr() + 2), dict(vecs=rows.data_ptr() + 1), dict(ld=299), dict(work=0),
                   dict(work_bytes=need - 1), dict(work=work.data_ptr() + 4)):
            with pytest.raises(ValueError):
                call(**kw)
        with pytest.raises(IndexError):
            call(idx=99)
        for kw in (dict(j0=0, j1=0), dict(j0=3, j1=2), dict(j0=0, j1=65), dict(j0=-1, j1=2), dict(j0=2, j1=4, first=True), dict(d_v0=0, first=True),
                   dict(work_bytes=prep.lanczos(300, 20)["work_bytes"] - 1)):
            a = dict(j0=0, j1=20, first=True, d_v0=dv.data_ptr(), work_bytes=need)
            a.update(kw)
            with pytest.raises(ValueError):
                cx.h.lanczos_steps_device(cx.idx[1], a["j0"], a["j1"], a["first"], a["d_v0"], work.data_ptr(), a["work_bytes"])
        with pytest.raises(ValueError, match="square"):
            cx.h.lanczos_steps_device(cx.idx[0], 0, 4, True, dv.data_ptr(), work.data_ptr(), need)
        with pytest.raises(ValueError):
            cx.h.lanczos_status(work.data_ptr() + 8)
        torch.cuda.synchronize()
        assert torch.equal(work, pattern) and bool((rows == -7.0).all())
        assert np.array_equal(bits(dv.cpu().numpy()), bits(v300))


def test_refused_before_load_matrices(torch_mod):
    import pyhispmv
    A = km.tridiag(64)
    h = pyhispmv.FpgaHandle(*HW)
    try:
        i = h.create_sparse_handle(A.row, A.col, A.data, 64, 64)
        d = torch_mod.zeros(1 << 20, dtype=torch_mod.float32, device="cuda")
        assert not h.lanczos_info(i, 20)["accepted"]
        with pytest.raises(AssertionError, match="before load_matrices"):
            h.eigsh_device(i, 2, d.data_ptr(), d.data_ptr() + 1024, 64, work=d.data_ptr() + 4096, work_bytes=(4 << 20) - 4096)
        with pytest.raises(AssertionError, match="before load_matrices"):
            h.lanczos_steps_device(i, 0, 4, True, d.data_ptr(), d.data_ptr() + 4096, (4 << 20) - 4096)
    finally:
        h.close()


# ---- hispmv_amd.solvers.eigsh --------------------------------------------------------------------------------------------------------------
def test_torch_front_end_on_a_side_stream_and_on_the_default_stream(torch_mod):
    """The answer of the device entry by another door: on a side stream everything is ordered there; on torch's default stream
    solvers.eigsh orders the two itself, also for a start vector still queued behind a long kernel."""
    from hispmv_amd import solvers
    torch = torch_mod
    case = lm.CASES["ramp_1025_LA"]
    A = case["make"]()
    n = A.shape[0]
    v0n = lm.start(n)
    kw = dict(which=case["which"], ncv=case["ncv"], tol=lm.TOL)
    with Ctx(torch, [A]) as cx:
        want_vals, want_vecs, winfo, _ = cx.eigsh(0, v0n, case["k"], case["ncv"], case["which"])
        assert winfo["status"] == "CONVERGED"
        tv = torch.from_numpy(v0n).to(cx.dev)

        def same(vals, vecs, info):
            assert isinstance(vals, np.ndarray) and vals.dtype == np.float64 and vecs.dtype == torch.float32 and vecs.is_cuda
            assert tuple(vecs.shape) == (n, winfo["found"]) and set(info) == {"status", "found", "products", "cycles", "residuals", "work"}
            assert all(info[key] == winfo[key] for key in ("status", "found", "products", "cycles")), (info, winfo)
            assert np.array_equal(bits64(vals), bits64(want_vals)) and np.array_equal(bits64(info["residuals"]), bits64(winfo["residuals"]))
            assert np.array_equal(bits(vecs.t().cpu().numpy()), bits(want_vecs))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            out = solvers.eigsh(cx.h, cx.idx[0], case["k"], v0=tv, **kw)
        side.synchronize()
        same(*out)
        assert torch.cuda.current_stream().cuda_stream == 0
        long = torch.ones(1 << 26, dtype=torch.float32, device=cx.dev)
        torch.cuda.synchronize()
        for _ in range(4):          # some milliseconds of work on the default stream, and the start vector queued behind it
            long = long.sin()
        v0 = tv * 2.0 - tv
        same(*solvers.eigsh(cx.h, cx.idx[0], case["k"], v0=v0, **kw))
        assert np.array_equal(bits(v0.cpu().numpy()), bits(v0n))          # the caller's v0 is not written
        a = solvers.eigsh(cx.h, cx.idx[0], 2, seed=5)
        b = solvers.eigsh(cx.h, cx.idx[0], 2, seed=5)
        c = solvers.eigsh(cx.h, cx.idx[0], 2, seed=6)
        assert a[2]["status"] == "CONVERGED" and np.array_equal(bits64(a[0]), bits64(b[0])) and torch.equal(a[1], b[1])
        assert a[2]["products"] == b[2]["products"] and not torch.equal(a[1], c[1])
        assert np.abs(a[0] - c[0]).max() <= 4 * lm.TOL * np.abs(a[0]).max()          # another start, the same eigenvalues
        with pytest.raises(TypeError):
            solvers.eigsh(cx.h, cx.idx[0], 2, v0=tv.double())
        with pytest.raises(ValueError):
            solvers.eigsh(cx.h, cx.idx[0], 2, v0=tv[:-1].contiguous())
        with pytest.raises(ValueError):
            solvers.eigsh(cx.h, cx.idx[0], 2, which="XX")
