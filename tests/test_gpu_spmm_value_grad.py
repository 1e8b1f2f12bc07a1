"""The wide-batch value gradient grad[k] = alpha * sum_v gyt[row_k, v] * xt[col_k, v] + beta * grad[k] on feature-major operands
(hispmv_spmm_value_grad_device; hispmv_spmm_grad.hip) and sparse_linear(..., spmm=True, wide_grad=True), at the small shapes of
tests/step_small_cases.py through the updatable Ctx of tests/test_gpu_value_grad.py: the plan classes of tests/test_gpu_spmm.py, each
asserted the same way.

EXACT BY CONSTRUCTION.  Per matrix and operand a pool of 16 integer vectors in [-3, 3]; vector v is pool[v % 16] * 2^((v // 16) % 5 - 2)
(the scaling of tests/test_gpu_spmm.py, on both operands); grad0 holds integers in [-8, 8].  Every product is a multiple of 1/16 of
magnitude <= 9 * 16 = 144; with B <= 257 and |alpha| <= 2 every partial sum, in any order, stays below 2 * 257 * 144 * 16 + 8 * 16 <
2^24 units of 1/16, so fp32 is exact and grad must equal the numpy result bit for bit at all n positions.  The reference is
sum_p w_p(B) * GYpool[p, r] * Xpool[p, c] with w_p(B) the sum of the squared scales of the vectors v = p (mod 16): 16 gathers per entry.

B in {1, 64, 65, 130, 257} with ld = B rounded up to 4: VL 1 (B = 1, 64); one VL 2 tile whose lane 32 is half live (65, ld 68); one
VL 4 tile whose lane 32 holds two live and two pad floats (130, ld 132); a full VL 4 tile, then a one-vector VL 1 tile that accumulates
(257, ld 260).  Once per class B = 65, ld = 68 with every pointer moved by one float (VL 1, two tiles).  (alpha, beta) in {(1, 0),
(2, -1), (0, 1), (0, 0)}; alpha = 0 gives exactly beta * grad0, or +0.  The pad columns of gyt and xt hold NaN, grad starts as NaN for
beta = 0 and lies between sentinel guards.  (That table holds up to 8192 columns; the 1024-thread matrices of the small cases have
20 000 and more and take VL 1 in up to five tiles, so test_wide_lanes_at_1024_threads adds such plans at 8000 columns.)
spmm_value_grad_info must report the VL and tiles of prep.spmm_tiles and launches = tiles *
parts (0 for n = 0): a fall-back to passes of 4 would pass every numeric gate.

RANDOM FLOATS on big_band, stray_split_band and a windowless matrix: the pool draws of tests/test_gpu_spmm.py, (alpha, beta) =
(0.85, -2.06), gate |grad - g64| <= TOL * (|alpha| sum |gy x| + |beta grad0|).  An entry sees at most VL + 6 + tiles + 2 <= 14
roundings, about 8e-7 of that magnitude, more than 10x below TOL = 1e-5.  A second identical call gives identical bits."""
import numpy as np
import pytest

import step_small_cases as S
from conftest import TOL
from test_gpu_spmm import POOL, bits, pool_of, scale_of
from test_gpu_spmm_companion import Pair
from test_gpu_transpose import GUARD, SENTINEL, Ctx as TCtx
from test_gpu_value_grad import Ctx as VCtx, entries, ints

pytestmark = pytest.mark.gpu

BATCHES = (1, 64, 65, 130, 257)
PAIRS = ((1.0, 0.0), (2.0, -1.0), (0.0, 1.0), (0.0, 0.0))
EXPECT = {1: (1, 1), 64: (1, 1), 65: (2, 1), 130: (4, 1), 257: (4, 2)}      # B -> (VL of the first tile, tiles) at ld = B rounded up to 4


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def weights(B):
    """w_p(B) = sum of scale(v)^2 over the vectors v < B with v = p (mod 16): exact in fp64"""
    w = np.zeros(POOL)
    for v in range(B):
        w[v % POOL] += float(scale_of(v)) ** 2
    return w


def batch_t(pool, B, ld):
    """[n, ld] feature-major: column v is pool[v % 16] * scale(v), the pad columns hold NaN"""
    out = np.full((pool.shape[1], ld), np.nan, np.float32)
    sc = np.array([scale_of(v) for v in range(B)], np.float32)
    out[:, :B] = pool[np.arange(B) % POOL].T * sc
    return out


class Ctx(VCtx):
    """The updatable context of tests/test_gpu_value_grad.py; updates="any_storage" for bf16 matrices."""

    def __init__(self, torch, env, mats, transposable=None, updates=True):
        TCtx.__init__(self, torch, env, mats, transposable=transposable, updates=updates)
        self.n, self.refs, self._ops = [], {}, {}
        for k, m in enumerate(mats):
            u = self.h.value_update_info(self.idx[k])
            assert u["updatable"] and u["n"] == m["r"].size, (m["name"], u)
            self.n.append(u["n"])

    def pools(self, k, kind):
        """(GYpool [16, rows], Xpool [16, cols]): integers in [-3, 3], or the float draws of tests/test_gpu_spmm.py"""
        m = self.mats[k]
        if kind == "ints":
            return (np.stack([ints(m, "wide_gy", p, m["rows"]) for p in range(POOL)]), np.stack([ints(m, "wide_x", p, m["cols"]) for p in range(POOL)]))
        return pool_of(dict(m, pool_key=m["name"] + "_rows"), m["rows"]), pool_of(m, m["cols"])

    def sums(self, k, kind, B, magnitudes=False):
        """(sum_v gy x, sum_v |gy x| or None) per entry in fp64, from the pools: computed once per (matrix, kind), weighted per B"""
        m = self.mats[k]
        key = (m["name"], kind)
        if key not in self.refs:
            r, c = entries(m)
            GY, X = self.pools(k, kind)
            self.refs[key] = np.stack([GY[p].astype(np.float64)[r] * X[p].astype(np.float64)[c] for p in range(POOL)]) if r.size else np.zeros((POOL, 0))
        t, w = self.refs[key], weights(B)
        return w @ t, (w @ np.abs(t) if magnitudes else None)

    def operands(self, k, kind, B, ld, shift):
        """gyt and xt on the device (pad columns NaN, moved by `shift` floats), kept for the pairs of one (kind, B, ld, shift)"""
        key = (k, kind, B, ld, shift)
        if key not in self._ops:
            GY, X = self.pools(k, kind)
            pad = np.full(shift, np.nan, np.float32)
            self._ops = {key: (self.device(np.concatenate([pad, batch_t(GY, B, ld).reshape(-1)])), self.device(np.concatenate([pad, batch_t(X, B, ld).reshape(-1)])))}
        return self._ops[key]

    def wide(self, k, kind, B, grad0, alpha, beta, ld=None, shift=0):
        """One call on matrix k -> grad (numpy).  grad0 None: grad starts as NaN.  The guards on both sides of grad must survive."""
        torch, m, n = self.torch, self.mats[k], self.n[k]
        ld = (B + 3) & ~3 if ld is None else ld
        dG, dX = self.operands(k, kind, B, ld, shift)
        lo = GUARD + shift
        full = np.full(n + 2 * GUARD + shift, SENTINEL, np.int32).view(np.float32)
        full[lo:lo + n] = np.nan if grad0 is None else grad0
        dR = self.device(full)
        torch.cuda.synchronize()
        self.h.spmm_value_grad_device(self.idx[k], dG.data_ptr() + 4 * shift, dX.data_ptr() + 4 * shift, B, dR.data_ptr() + 4 * lo, alpha, beta, ld_gy=ld, ld_x=ld)
        self.h.synchronize()
        out = dR.cpu().numpy()
        guard = np.ones(out.size, bool)
        guard[lo:lo + n] = False
        assert (out.view(np.int32)[guard] == SENTINEL).all(), f'{m["name"]}: floats outside grad were written (B={B}, ld={ld})'
        return out[lo:lo + n].copy()

    def exact(self, k, B, alpha, beta, ld=None, shift=0):
        m, n = self.mats[k], self.n[k]
        g0 = ints(m, "wide_grad0", 0, n, -8, 8)
        s, _ = self.sums(k, "ints", B)
        # (alpha == 0: gyt and xt are not read, the result is beta * grad0 -- or +0 -- and not 0 * s, which is -0 where s < 0)
        want = ((alpha * s if alpha != 0.0 else np.zeros(n)) + (beta * g0.astype(np.float64) if beta != 0.0 else 0.0)).astype(np.float32)
        got = self.wide(k, "ints", B, None if beta == 0.0 else g0, alpha, beta, ld=ld, shift=shift)
        bad = np.flatnonzero(bits(got) != bits(want))
        assert bad.size == 0, (m["name"], B, alpha, beta, shift, bad.size, bad[:8], got[bad[:8]], want[bad[:8]])

    def check_info(self, k, B):
        from hispmv_amd import prep
        m = self.mats[k]
        ld = (B + 3) & ~3
        info, tiles = self.h.spmm_value_grad_info(self.idx[k], B, ld), prep.spmm_tiles(m["cols"], B, ld, 16)
        if m["cols"] <= 8192:                       # (past 8192 columns the tile rule caps VL: 1 from 16385 columns on)
            assert (tiles["vl"], tiles["tiles"]) == EXPECT[B], (m["name"], B, tiles)
        else:
            assert m["cols"] > 16384 and (tiles["vl"], tiles["tiles"]) == (1, (B + 63) // 64), (m["name"], B, tiles)
        assert info["accepted"] and (info["vl"], info["tiles"]) == (tiles["vl"], tiles["tiles"]), (m["name"], B, info, tiles)
        parts = self.info[k]["col_tiles"]
        assert info["launches"] == (tiles["tiles"] * parts if self.n[k] > 0 else 0), (m["name"], B, info, parts)

    def floats(self, k, B):
        m, n = self.mats[k], self.n[k]
        alpha, beta = 0.85, -2.06
        g0 = (np.random.default_rng(200 + k).random(n, dtype=np.float32) - np.float32(0.5))
        s, a = self.sums(k, "floats", B, magnitudes=True)
        g64 = alpha * s + beta * g0.astype(np.float64)
        mag = abs(alpha) * a + np.abs(beta * g0.astype(np.float64))
        got = self.wide(k, "floats", B, g0, alpha, beta)
        err = np.abs(got.astype(np.float64) - g64)
        print(f'{m["name"]}: B={B} worst |grad - g64| / mag = {float((err / np.maximum(mag, 1e-300)).max()) if n else 0.0:.3e}')
        assert np.isfinite(got).all() and (err <= TOL * mag).all(), (m["name"], B, float((err - TOL * mag).max()))
        again = self.wide(k, "floats", B, g0, alpha, beta)
        assert np.array_equal(bits(got), bits(again)), (m["name"], B, "a second identical call gave other bits")

    def run_class(self, k, floats=False):
        """Every gate of the module docstring on matrix k; spmv_device gives identical bits before and after the gradient calls."""
        from hispmv_amd import prep
        m = self.mats[k]
        before = self.spmv(k, m["x"], m["b"], 0.85, -2.06)
        for B in BATCHES:
            self.check_info(k, B)
            for alpha, beta in PAIRS:
                self.exact(k, B, alpha, beta)
        assert prep.spmm_tiles(m["cols"], 65, 68, 4) == dict(vl=1, tiles=2, last_vecs=1, vl_last=1)
        self.exact(k, 65, 2.0, -1.0, ld=68, shift=1)
        if floats:
            for B in (130, 257):
                self.floats(k, B)
        after = self.spmv(k, m["x"], m["b"], 0.85, -2.06)
        assert np.array_equal(bits(before), bits(after)), m["name"]


# ---- plan classes (those of tests/test_gpu_spmm.py) ---------------------------------------------------------------------------------------
def test_plans_without_a_window(torch_mod):
    """256 threads, no window: the six plain matrices of case A (nnz = 0 and 1024 among them)."""
    mats = S.case_a()[:6]
    with Ctx(torch_mod, S.SLICES, mats) as cx:
        assert cx.n[0] == 0 and cx.n[1] == 1024
        for k in range(len(mats)):
            assert cx.info[k]["block_threads"] == 256 and cx.info[k]["lds_bytes"] == 0, cx.info[k]
            cx.run_class(k, floats=(k == 2))


@pytest.mark.parametrize("make", [S.one_by_one, S.single_row, S.single_row_long, S.sparse_rows],
                         ids=["one_by_one", "single_row", "single_row_long", "sparse_rows"])
def test_chains_and_fillers(torch_mod, make):
    """The 1 x 1 matrix; one row over many slices (the row never changes and the header row is the chain's row); 50 live rows among
    49 950 fillers, whose map words are 0."""
    m = make()
    with Ctx(torch_mod, S.SLICES, [m]) as cx:
        assert cx.info[0]["block_threads"] == 256 and cx.info[0]["lds_bytes"] == 0, cx.info[0]
        if m["name"].startswith("single_row"):
            assert cx.h.spmm_info(cx.idx[0], 4)["launches"] == 2, m["name"]          # (the forward wide call has a cut row to fix up; the gradient has none)
            assert cx.h.spmm_value_grad_info(cx.idx[0], 4)["launches"] == 1, m["name"]
        cx.run_class(0)


def test_compact_windows_256_threads(torch_mod):
    mats = S.case_a()[6:8]
    with Ctx(torch_mod, S.SLICES, mats) as cx:
        assert all(i["block_threads"] == 256 and i["lds_bytes"] > 0 and i["compact_slices"] == i["n_slices"] for i in cx.info), cx.info
        for k in range(2):
            cx.run_class(k)


def test_wide_groups_with_a_window_and_l2_elements(torch_mod):
    m = S.two_way_band()
    with Ctx(torch_mod, S.NOSPLIT, [m]) as cx:
        assert cx.info[0]["compact_slices"] == 0 and cx.info[0]["lds_bytes"] > 0, cx.info[0]
        cx.run_class(0)


def test_1024_threads_compact(torch_mod):
    m = S.big_band()
    with Ctx(torch_mod, S.SLICES, [m]) as cx:
        assert cx.info[0]["block_threads"] == 1024 and cx.info[0]["compact_slices"] == cx.info[0]["n_slices"], cx.info[0]
        cx.run_class(0, floats=True)


def test_stray_slots(torch_mod):
    m = S.stray_slot_band()
    with Ctx(torch_mod, S.SLICES, [m]) as cx:
        assert cx.info[0]["block_threads"] == 1024 and cx.info[0]["compact_slices"] == cx.info[0]["n_slices"], cx.info[0]
        cx.run_class(0)


def test_two_parts_of_a_stray_split(torch_mod):
    m = S.stray_split_band()
    with Ctx(torch_mod, S.SLICES, [m]) as cx:
        assert cx.info[0]["tile_kind"] == 3 and cx.info[0]["col_tiles"] == 2, cx.info[0]
        assert cx.h.spmm_value_grad_info(cx.idx[0], 64)["launches"] == 2
        cx.run_class(0, floats=True)


def test_eight_column_parts(torch_mod):
    m = S.column_tiled()
    with Ctx(torch_mod, S.COLTILES, [m]) as cx:
        assert cx.info[0]["tile_kind"] == 1 and cx.info[0]["col_tiles"] == 8, cx.info[0]
        assert cx.h.spmm_value_grad_info(cx.idx[0], 64)["launches"] == 8
        cx.run_class(0)


@pytest.mark.parametrize("make", [S.big_band, S.stray_slot_band], ids=["big_band", "stray_slot_band"])
def test_half_groups(torch_mod, make):
    m = S.as_bf16(make())
    with Ctx(torch_mod, S.SLICES, [m], updates="any_storage") as cx:
        st = cx.h.value_storage_info(cx.idx[0])
        assert st["storage"] == "bf16" and st["slots_2byte"] > 0, st
        cx.run_class(0)


def short_band(rows, cols, per_row, seed, redraw=0.0):
    """Row i holds per_row columns from i * cols / rows on (mod cols); `redraw`: that share of the entries gets a random column."""
    rng = np.random.default_rng(seed)
    r = np.repeat(np.arange(rows, dtype=np.int64), per_row)
    c = (r * cols // rows + np.tile(np.arange(per_row, dtype=np.int64), rows)) % cols
    if redraw > 0:
        c = np.where(rng.random(r.size) < redraw, rng.integers(0, cols, r.size), c)
    return S._finish(f"short_band_{rows}x{cols}x{per_row}_r{redraw}_s{seed}", rows, cols, r, c, seed, dict(format=0, threads=1024, window=True))


@pytest.mark.parametrize("kind", ["compact", "stray_slots", "stray_slots_bf16"])
def test_wide_lanes_at_1024_threads(torch_mod, kind):
    """The 1024-thread matrices above have 20 000 columns and more, where the tile rule leaves VL 1: the bodies with the least
    registers to spare would run VL 2 and 4 in no test.  big_band and stray_slot_band squeezed into 8000 columns keep their plans
    (1024 threads, compact groups of 16 and 18 slices, stray slots in every slice of the second) and take VL 2 at B = 65 and VL 4 at
    B = 130 and 257 (check_info asserts it)."""
    m = short_band(20000, 8000, 200, 231) if kind == "compact" else short_band(22000, 8000, 210, 244, redraw=0.02)
    if kind != "compact":
        with S.environment(S.SLICES):
            stray, compact, n_slices = S.stray_layout(m)
        assert stray == compact == n_slices > 0, (stray, compact, n_slices)
    if kind.endswith("bf16"):
        m = S.as_bf16(m)
    with Ctx(torch_mod, S.SLICES, [m], updates="any_storage" if kind.endswith("bf16") else True) as cx:
        i = cx.info[0]
        assert i["block_threads"] == 1024 and i["compact_slices"] == i["n_slices"] and i["col_tiles"] == 1 and m["cols"] <= 8192, i
        if kind.endswith("bf16"):
            assert cx.h.value_storage_info(cx.idx[0])["slots_2byte"] > 0
        cx.run_class(0, floats=True)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_tile_stream_and_dense_handles_are_refused(torch_mod):
    m, d = S.tile_stream(), S.dense_shapes()[1]
    with TCtx(torch_mod, S.AUTO, [m, d], updates=True) as cx:
        assert cx.info[0]["format"] == 1
        for k, match in ((0, "set_transposable"), (1, "GEMM")):
            mm = cx.mats[k]
            assert cx.h.spmm_value_grad_info(cx.idx[k], 8) == dict(accepted=False, vl=0, tiles=0, launches=0)
            t = torch_mod.zeros(8 * (mm["rows"] + mm["cols"]) + cx.h.value_update_info(cx.idx[k])["n"], dtype=torch_mod.float32, device="cuda")
            with pytest.raises(NotImplementedError, match=match):
                cx.h.spmm_value_grad_device(cx.idx[k], t.data_ptr(), t.data_ptr() + 32 * mm["rows"], 8, t.data_ptr() + 32 * (mm["rows"] + mm["cols"]))


def test_refused_without_value_updates(torch_mod):
    m = S.case_a()[7]
    with TCtx(torch_mod, S.SLICES, [m], updates=False) as cx:
        assert cx.h.spmm_value_grad_info(cx.idx[0], 4) == dict(accepted=False, vl=0, tiles=0, launches=0)
        d = cx.device(np.zeros(4 * (m["rows"] + m["cols"]) + m["r"].size, np.float32))
        args = (d.data_ptr(), d.data_ptr() + 16 * m["rows"], 4, d.data_ptr() + 16 * (m["rows"] + m["cols"]))
        with pytest.raises(AssertionError, match="set_value_updates") as wide:
            cx.h.spmm_value_grad_device(cx.idx[0], *args)
        with pytest.raises(AssertionError, match="set_value_updates") as narrow:
            cx.h.value_grad_device(cx.idx[0], *args)
        assert type(wide.value) is type(narrow.value)


def test_argument_errors_come_before_any_launch(torch_mod):
    """ld < B, NULL operands, an aliased or misaligned pointer and num_vecs < 1 are HISPMV_EINVAL (ValueError); grad is untouched."""
    m = S.case_a()[7]
    with Ctx(torch_mod, S.SLICES, [m]) as cx:
        h, idx, B, n = cx.h, cx.idx[0], 8, cx.n[0]
        gyt = torch_mod.zeros(m["rows"] * B, dtype=torch_mod.float32, device="cuda")
        xt = torch_mod.zeros(m["cols"] * B, dtype=torch_mod.float32, device="cuda")
        grad = torch_mod.full((n,), 7.0, dtype=torch_mod.float32, device="cuda")
        pg, px, pr = gyt.data_ptr(), xt.data_ptr(), grad.data_ptr()
        with pytest.raises(ValueError, match="at least num_vecs"):
            h.spmm_value_grad_device(idx, pg, px, B, pr, ld_gy=B - 1)
        with pytest.raises(ValueError, match="at least num_vecs"):
            h.spmm_value_grad_device(idx, pg, px, B, pr, ld_x=B - 1)
        for args in ((0, px, B, pr), (pg, 0, B, pr), (pg, px, B, 0), (pg, px, 0, pr), (pg, px, B, pg), (pg, px, B, px), (pg + 2, px, B, pr)):
            with pytest.raises(ValueError):
                h.spmm_value_grad_device(idx, *args)
        with pytest.raises(ValueError):
            h.spmm_value_grad_info(idx, 8, 7)
        with pytest.raises(ValueError):
            h.spmm_value_grad_info(idx, 0)
        with pytest.raises(IndexError):
            h.spmm_value_grad_device(99, pg, px, B, pr)
        with pytest.raises(IndexError):
            h.spmm_value_grad_info(99, 1)
        h.synchronize()
        assert (grad == 7.0).all()


# ---- sparse_linear(..., spmm=True, wide_grad=True) ----------------------------------------------------------------------------------------
def test_sparse_linear_wide_grad(torch_mod):
    """On the windowed uniform matrix with a stored transpose, B = 65: grad_values within TOL * mag of the fp64 truth and of the
    spmm=False route, two backward passes bit-equal, y and grad_x with the bits of spmm=True, wide_grad=False."""
    from hispmv_amd.torch_ops import sparse_linear
    torch = torch_mod
    B = 65
    m = S.case_a()[6]
    rng = np.random.default_rng(13)
    X = rng.random((B, m["cols"]), dtype=np.float32) - np.float32(0.3)
    G = rng.random((B, m["rows"]), dtype=np.float32) - np.float32(0.5)
    r, c = entries(m)
    with Pair(torch_mod, m, updates=True) as cx:
        h, P = cx.h, cx.idx[0]
        assert h.spmm_info(P, B, 68)["accepted_t"] and h.spmm_value_grad_info(P, B, 68) == dict(accepted=True, vl=2, tiles=1, launches=1)

        def passes(**kw):
            x = cx.device(X).requires_grad_(True)
            v = cx.device(m["v"] * np.float32(2.0)).requires_grad_(True)
            y = sparse_linear(h, P, x, None, values=v, **kw)
            y.backward(cx.device(G))
            torch.cuda.synchronize()
            h.synchronize()
            return y.detach().cpu().numpy(), x.grad.cpu().numpy(), v.grad.cpu().numpy()

        for scope in ("default stream", "own stream"):
            with torch.cuda.stream(torch.cuda.Stream() if scope == "own stream" else None):
                narrow = passes(spmm=False)
                spmm = passes(spmm=True)
                wide = passes(spmm=True, wide_grad=True)
                again = passes(spmm=True, wide_grad=True)
            g64 = sum(G[u].astype(np.float64)[r] * X[u].astype(np.float64)[c] for u in range(B))
            mag = sum(np.abs(G[u].astype(np.float64)[r] * X[u].astype(np.float64)[c]) for u in range(B))
            assert wide[2].shape == (m["r"].size,) and np.isfinite(wide[2]).all(), scope
            assert (np.abs(wide[2].astype(np.float64) - g64) <= TOL * mag).all(), scope
            assert (np.abs(wide[2].astype(np.float64) - narrow[2]) <= TOL * mag).all(), scope
            assert np.array_equal(bits(wide[2]), bits(again[2])), scope
            assert np.array_equal(bits(wide[0]), bits(spmm[0])) and np.array_equal(bits(wide[1]), bits(spmm[1])), scope
            assert np.array_equal(bits(spmm[2]), bits(narrow[2])), scope                      # the default route is what it was
        x, v = cx.device(X), cx.device(m["v"])
        with pytest.raises(ValueError, match="spmm=True"):
            sparse_linear(h, P, x, None, values=v, wide_grad=True)
        with pytest.raises(ValueError, match="values"):
            sparse_linear(h, P, x, None, spmm=True, wide_grad=True)


def test_three_training_steps_reduce_the_loss(torch_mod):
    """loss(v) = 1/2 sum_b |A(v) x_b - t_b|^2, t = A(v*) x: three steps v -= lr * v.grad through the wide route reduce it every time.
    The Hessian in v is block diagonal per row, its largest eigenvalue at most B * (entries of the fullest row) * max x^2 =: L, and a
    step of 1 / L cannot increase a quadratic loss."""
    from hispmv_amd.torch_ops import sparse_linear
    torch = torch_mod
    B = 65
    m = S.case_a()[6]
    with Pair(torch_mod, m, updates=True) as cx:
        rng = np.random.default_rng(11)
        X = rng.random((B, m["cols"]), dtype=np.float32) - np.float32(0.3)
        lr = 1.0 / (B * np.bincount(m["r"]).max() * float((X * X).max()))
        x = cx.device(X)
        kw = dict(spmm=True, wide_grad=True)
        with torch.no_grad():
            t = sparse_linear(cx.h, cx.idx[0], x, None, values=cx.device(m["v"]), **kw).clone()
        v = cx.device(m["v"] + np.float32(0.25) * (rng.random(m["v"].size, dtype=np.float32) - np.float32(0.5))).requires_grad_(True)
        losses = []
        for _ in range(4):
            y = sparse_linear(cx.h, cx.idx[0], x, None, values=v, **kw)
            loss = 0.5 * ((y - t) ** 2).sum()
            losses.append(float(loss.detach()))
            loss.backward()
            with torch.no_grad():
                v -= lr * v.grad
                v.grad = None
            torch.cuda.synchronize()
        print("losses", losses)
        assert losses[0] > 0 and all(b < a for a, b in zip(losses, losses[1:])), losses
