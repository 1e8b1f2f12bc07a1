"""The wide-batch value gradient with bf16 activations (hispmv_spmm_value_grad_device_bf16; hispmv_spmm_grad.hip) and
sparse_linear(..., spmm=True, wide_grad="bf16"), at the small shapes of tests/step_small_cases.py with the plan classes, the Ctx and the
helpers of tests/test_gpu_spmm_value_grad.py.

1. EXACT BY CONSTRUCTION.  The integer pools and power-of-two scales of that file; every operand value is exactly a bf16.  The reference
is the numpy sum.  Every product is a multiple of 1/16 of magnitude <= 9 * 16 = 144 = 2304 units; the largest B = 513 and |alpha| <= 2
give at most 2 * 513 * 2304 + 128 < 2^24 units of 1/16 in any partial sum, so any order is exact and grad must equal the reference bit
for bit at all n positions.  (alpha, beta) in {(1, 0), (2, -1), (0, 1), (0, 0)}; pad columns hold bf16 NaN; grad starts as NaN for
beta = 0 and lies between sentinel guards.  B -> ld, lanes at up to 8192 columns:
    1 -> 8: VB 1;  64 -> 64: VB 1;  65 -> 72: VB 2, a half-live lane;  130 -> 136: VB 4, a lane with 2 live + 2 pad;
    257 -> 260 (ld % 8 = 4): a full VB 4 tile, then a VB 1 tile;  258 -> 264: VB 8, a lane with 2 live + 6 pad;
    513 -> 520: a full VB 8 tile, then a VB 1 tile that accumulates.
Once per class B = 65 with both operands moved by one bf16 (alignment 2: VB 1, two tiles) and by two (alignment 4: VB 2).
spmm_value_grad_bf16_info must equal prep.spmm_bf16_tiles and launches = tiles * parts (0 for n = 0): a fall-back to narrower lanes
would pass every numeric gate.  The 1024-thread matrices of the small cases have 20 000 columns and more, where the rule caps VB at 2,
so test_wide_lanes_at_1024_threads runs the same plans at 8000 columns.

2. BITS, random bf16 operands (the float pools of tests/test_gpu_spmm.py rounded once to bf16) on big_band, on its 8000-column form
(VB 8 at 1024 threads), on stray_split_band and on a windowless matrix: equal, with no tolerance, to the order model of
tests/spmm_grad_bf16_cases.py at every B of the table -- on every entry of a matrix of up to 32 768 entries, otherwise on the first and
last 1024 entries and 30 720 seeded draws (the model holds [entries, B] float32 arrays; 4 M entries at B = 513 are 8 GB).  At B = 65,
130, 257 with ld = 68, 132, 260 both tile rules give the same lanes and tiles (asserted), and ALL entries equal spmm_value_grad_device
on the widened operands bit for bit.  A second identical call gives identical bits.

3. NON-FINITE.  Column 0 (the row of xt an element without a place reads) and one live column of xt hold +Inf, -Inf and NaN in three
vectors: every entry has the model's bits, or for a NaN the model's class.  Zeros instead of NaN in the pad columns change no bit.

4. REFUSALS with their exception types.    5. sparse_linear(wide_grad="bf16")."""
import numpy as np
import pytest

import spmm_grad_bf16_cases as M
import step_small_cases as S
from test_gpu_spmm import POOL, bits, scale_of
from test_gpu_spmm_companion import Pair
from test_gpu_transpose import GUARD, SENTINEL, Ctx as TCtx
from test_gpu_spmm_value_grad import PAIRS, Ctx as FCtx, batch_t, short_band
from test_gpu_value_grad import entries, ints

pytestmark = pytest.mark.gpu

NAN16 = 0x7FC0
LD = {1: 8, 64: 64, 65: 72, 130: 136, 257: 260, 258: 264, 513: 520}
EXPECT = {1: (1, 1), 64: (1, 1), 65: (2, 1), 130: (4, 1), 257: (4, 2), 258: (8, 1), 513: (8, 2)}      # (VB of the first tile, tiles) up to 8192 columns
SAME_AS_FP32 = ((65, 68), (130, 132), (257, 260))
SAMPLE = 32768


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def vb_cap(cols):
    return 8 if cols <= 8192 else 4 if cols <= 16384 else 2 if cols <= 32768 else 1


class Ctx(FCtx):
    """The context of tests/test_gpu_spmm_value_grad.py with `wide` running the bf16 entry (so that its `exact` checks it against the
    numpy sum) and `wide32` the fp32 entry on the widened operands."""

    def pools(self, k, kind):
        GY, X = super().pools(k, kind)
        if kind == "floats":          # rounded once; the power-of-two scales keep them bf16
            GY, X = M.widen(M.to_bf16_bits(GY)).reshape(GY.shape), M.widen(M.to_bf16_bits(X)).reshape(X.shape)
        return GY, X

    def words(self, a16):
        return self.torch.from_numpy(np.ascontiguousarray(a16, np.uint16).view(np.int16)).to(self.dev)

    def operands16(self, k, kind, B, ld, shift, pad=NAN16, poke=None):
        """gyt and xt as bf16 words on the device (pad columns `pad`, moved by `shift` elements); poke(xt [cols, ld] float32) edits xt"""
        key = (k, kind, B, ld, shift, pad, poke is not None)
        ops = self.__dict__.setdefault("_ops16", {})
        if key not in ops:
            GY, X = self.pools(k, kind)
            out = []
            for pool, edit in ((GY, None), (X, poke)):
                t = batch_t(pool, B, ld)
                if edit is not None:
                    edit(t)
                w = M.to_bf16_bits(t)
                assert np.array_equal(bits(M.widen(w)[np.isfinite(t)]), bits(t[np.isfinite(t)])), "an operand is not a bf16"
                w[np.isnan(t) & (np.arange(ld) >= B)] = pad
                out.append(self.words(np.concatenate([np.full(shift, NAN16, np.uint16), w.reshape(-1)])))
            ops.clear()
            ops[key] = tuple(out)
        return ops[key]

    def wide(self, k, kind, B, grad0, alpha, beta, ld=None, shift=0, pad=NAN16, poke=None):
        """One bf16 call on matrix k -> grad (numpy).  grad0 None: grad starts as NaN.  The guards on both sides of grad must survive."""
        torch, m, n = self.torch, self.mats[k], self.n[k]
        ld = LD[B] if ld is None else ld
        dG, dX = self.operands16(k, kind, B, ld, shift, pad, poke)
        full = np.full(n + 2 * GUARD, SENTINEL, np.int32).view(np.float32)
        full[GUARD:GUARD + n] = np.nan if grad0 is None else grad0
        dR = self.device(full)
        torch.cuda.synchronize()
        self.h.spmm_value_grad_device_bf16(self.idx[k], dG.data_ptr() + 2 * shift, dX.data_ptr() + 2 * shift, B, dR.data_ptr() + 4 * GUARD, alpha, beta, ld_gy=ld, ld_x=ld)
        self.h.synchronize()
        out = dR.cpu().numpy()
        guard = np.ones(out.size, bool)
        guard[GUARD:GUARD + n] = False
        assert (out.view(np.int32)[guard] == SENTINEL).all(), f'{m["name"]}: floats outside grad were written (B={B}, ld={ld})'
        return out[GUARD:GUARD + n].copy()

    def wide32(self, k, kind, B, grad0, alpha, beta, ld):
        return FCtx.wide(self, k, kind, B, grad0, alpha, beta, ld=ld)

    def check_info(self, k, B):
        from hispmv_amd import prep
        m = self.mats[k]
        info, tiles = self.h.spmm_value_grad_bf16_info(self.idx[k], B, LD[B]), prep.spmm_bf16_tiles(m["cols"], B, LD[B], 16)
        if m["cols"] <= 8192:
            assert (tiles["vb"], tiles["tiles"]) == EXPECT[B], (m["name"], B, tiles)
        else:
            assert tiles["vb"] == min(EXPECT[B][0], vb_cap(m["cols"])), (m["name"], B, tiles)
        assert info["accepted"] and (info["vb"], info["tiles"]) == (tiles["vb"], tiles["tiles"]), (m["name"], B, info, tiles)
        parts = self.info[k]["col_tiles"]
        assert info["launches"] == (tiles["tiles"] * parts if self.n[k] > 0 else 0), (m["name"], B, info, parts)

    def sample(self, k):
        n = self.n[k]
        if n <= SAMPLE:
            return np.arange(n)
        rng = np.random.default_rng(300 + k)
        return np.unique(np.concatenate([np.arange(1024), np.arange(n - 1024, n), rng.integers(0, n, SAMPLE - 2048)]))

    def modelled(self, k, kind, B, ld, align, alpha, beta, g0, poke=None):
        """(entries, the order model's grad on them) for the call's operands"""
        from hispmv_amd import prep
        m = self.mats[k]
        r, c = entries(m)
        e = self.sample(k)
        GY, X = self.pools(k, kind)
        xt = batch_t(X, B, ld)
        if poke is not None:
            poke(xt)
        gy, x = batch_t(GY, B, ld)[r[e], :B], xt[c[e], :B]
        tiles = M.tile_list(prep.spmm_bf16_tiles(m["cols"], B, ld, align))
        return e, M.model(gy, x, tiles, alpha, beta, None if g0 is None else g0[e])

    def same_bits_or_class(self, got, want, what):
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), what
        bad = np.flatnonzero(bits(got)[~nan] != bits(want)[~nan])
        assert bad.size == 0, (what, bad.size, bad[:8], got[~nan][bad[:8]], want[~nan][bad[:8]])

    def order(self, k, batches=tuple(LD)):
        """gate 2 on matrix k"""
        from hispmv_amd import prep
        m, n = self.mats[k], self.n[k]
        alpha, beta = 0.85, -2.06
        g0 = np.random.default_rng(200 + k).random(n, dtype=np.float32) - np.float32(0.5)
        for B in batches:
            got = self.wide(k, "floats", B, g0, alpha, beta)
            e, want = self.modelled(k, "floats", B, LD[B], 16, alpha, beta, g0)
            assert np.isfinite(got).all() and np.abs(got).max() > 0
            self.same_bits_or_class(got[e], want, (m["name"], B, "order model"))
            assert np.array_equal(bits(got), bits(self.wide(k, "floats", B, g0, alpha, beta))), (m["name"], B, "a second identical call gave other bits")
        for B, ld in SAME_AS_FP32:
            if m["cols"] > 8192:
                continue
            a, b = self.h.spmm_value_grad_info(self.idx[k], B, ld), self.h.spmm_value_grad_bf16_info(self.idx[k], B, ld)
            assert (a["vl"], a["tiles"], a["launches"]) == (b["vb"], b["tiles"], b["launches"]), (m["name"], B, ld, a, b)
            assert M.tile_list(prep.spmm_bf16_tiles(m["cols"], B, ld, 16)) == M.tile_list(prep.spmm_tiles(m["cols"], B, ld, 16), key="vl")
            got, ref = self.wide(k, "floats", B, g0, alpha, beta, ld=ld), self.wide32(k, "floats", B, g0, alpha, beta, ld)
            assert np.array_equal(bits(got), bits(ref)), (m["name"], B, ld, "not the bits of spmm_value_grad_device on the widened operands")

    def run_class(self, k, order=False):
        """Gate 1 (and 2 with `order`) on matrix k; spmv_device gives identical bits before and after the gradient calls."""
        from hispmv_amd import prep
        m = self.mats[k]
        before = self.spmv(k, m["x"], m["b"], 0.85, -2.06)
        for B in LD:
            self.check_info(k, B)
            for alpha, beta in PAIRS:
                self.exact(k, B, alpha, beta)
        assert prep.spmm_bf16_tiles(m["cols"], 65, 72, 2) == dict(vb=1, tiles=2, last_vecs=1, vb_last=1)
        self.exact(k, 65, 2.0, -1.0, ld=72, shift=1)
        if m["cols"] <= 32768:
            assert prep.spmm_bf16_tiles(m["cols"], 65, 72, 4) == dict(vb=2, tiles=1, last_vecs=65, vb_last=2)
        self.exact(k, 65, 2.0, -1.0, ld=72, shift=2)
        if order:
            self.order(k)
        after = self.spmv(k, m["x"], m["b"], 0.85, -2.06)
        assert np.array_equal(bits(before), bits(after)), m["name"]


# ---- plan classes (those of tests/test_gpu_spmm_value_grad.py) ----------------------------------------------------------------------------
def test_plans_without_a_window(torch_mod):
    """256 threads, no window: the six plain matrices of case A (nnz = 0 and 1024 among them)."""
    mats = S.case_a()[:6]
    with Ctx(torch_mod, S.SLICES, mats) as cx:
        assert cx.n[0] == 0 and cx.n[1] == 1024
        for k in range(len(mats)):
            assert cx.info[k]["block_threads"] == 256 and cx.info[k]["lds_bytes"] == 0, cx.info[k]
            cx.run_class(k, order=(k == 2))


@pytest.mark.parametrize("make", [S.one_by_one, S.single_row_long, S.sparse_rows], ids=["one_by_one", "single_row_long", "sparse_rows"])
def test_chains_and_fillers(torch_mod, make):
    m = make()
    with Ctx(torch_mod, S.SLICES, [m]) as cx:
        assert cx.info[0]["block_threads"] == 256 and cx.info[0]["lds_bytes"] == 0, cx.info[0]
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
        cx.run_class(0, order=True)


def test_stray_slots(torch_mod):
    m = S.stray_slot_band()
    with Ctx(torch_mod, S.SLICES, [m]) as cx:
        assert cx.info[0]["block_threads"] == 1024 and cx.info[0]["compact_slices"] == cx.info[0]["n_slices"], cx.info[0]
        cx.run_class(0)


def test_two_parts_of_a_stray_split(torch_mod):
    m = S.stray_split_band()
    with Ctx(torch_mod, S.SLICES, [m]) as cx:
        assert cx.info[0]["tile_kind"] == 3 and cx.info[0]["col_tiles"] == 2, cx.info[0]
        assert cx.h.spmm_value_grad_bf16_info(cx.idx[0], 64)["launches"] == 2
        cx.run_class(0, order=True)


def test_eight_column_parts(torch_mod):
    m = S.column_tiled()
    with Ctx(torch_mod, S.COLTILES, [m]) as cx:
        assert cx.info[0]["tile_kind"] == 1 and cx.info[0]["col_tiles"] == 8, cx.info[0]
        assert cx.h.spmm_value_grad_bf16_info(cx.idx[0], 64)["launches"] == 8
        cx.run_class(0)


@pytest.mark.parametrize("make", [S.big_band, S.stray_slot_band], ids=["big_band", "stray_slot_band"])
def test_half_groups(torch_mod, make):
    m = S.as_bf16(make())
    with Ctx(torch_mod, S.SLICES, [m], updates="any_storage") as cx:
        st = cx.h.value_storage_info(cx.idx[0])
        assert st["storage"] == "bf16" and st["slots_2byte"] > 0, st
        cx.run_class(0)


@pytest.mark.parametrize("kind", ["compact", "stray_slots", "stray_slots_bf16"])
def test_wide_lanes_at_1024_threads(torch_mod, kind):
    """big_band and stray_slot_band squeezed into 8000 columns keep their plans (1024 threads, compact groups, stray slots in every slice
    of the second) and take VB 4 and VB 8 (check_info asserts it): the bodies with the least registers to spare."""
    m = short_band(20000, 8000, 200, 231) if kind == "compact" else short_band(22000, 8000, 210, 244, redraw=0.02)
    if kind.endswith("bf16"):
        m = S.as_bf16(m)
    with Ctx(torch_mod, S.SLICES, [m], updates="any_storage" if kind.endswith("bf16") else True) as cx:
        i = cx.info[0]
        assert i["block_threads"] == 1024 and i["compact_slices"] == i["n_slices"] and i["col_tiles"] == 1 and m["cols"] <= 8192, i
        if kind.endswith("bf16"):
            assert cx.h.value_storage_info(cx.idx[0])["slots_2byte"] > 0
        cx.run_class(0, order=True)


# ---- non-finite operands ------------------------------------------------------------------------------------------------------------------
def test_non_finite_operands_follow_the_model(torch_mod):
    m = S.case_a()[3]
    with Ctx(torch_mod, S.SLICES, [m]) as cx:
        live = int(np.bincount(m["c"], minlength=m["cols"])[1:].argmax()) + 1
        live2 = int(np.argsort(np.bincount(m["c"], minlength=m["cols"])[1:])[-2]) + 1          # (a second live column treated like column 0)
        assert (m["c"] == live).any() and (m["c"] == live2).any() and live2 != live and cx.n[0] <= SAMPLE

        def poke(xt):          # column 0 and a second live one: one Inf (entries of +-Inf, by the sign of gy); the live column: +-Inf and NaN (NaN)
            xt[0, 3], xt[live2, 3] = np.inf, -np.inf
            xt[live, 3], xt[live, 70], xt[live, 200] = np.inf, -np.inf, np.nan

        g0 = np.random.default_rng(7).random(cx.n[0], dtype=np.float32) - np.float32(0.5)
        for B in (258, 513):
            got = cx.wide(0, "floats", B, g0, 0.85, -2.06, poke=poke)
            e, want = cx.modelled(0, "floats", B, LD[B], 16, 0.85, -2.06, g0, poke=poke)
            assert e.size == cx.n[0] and np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).any()
            cx.same_bits_or_class(got, want, (m["name"], B, "non-finite"))
        # the pad columns: NaN or zeros, no bit changes (B = 258: lane 32 of the VB 8 tile holds 2 live + 6 pad halves)
        for B in (65, 130, 258):
            a = cx.wide(0, "floats", B, g0, 0.85, -2.06)
            b = cx.wide(0, "floats", B, g0, 0.85, -2.06, pad=0)
            assert np.isfinite(a).all() and np.array_equal(bits(a), bits(b)), B


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_tile_stream_and_dense_handles_are_refused(torch_mod):
    m, d = S.tile_stream(), S.dense_shapes()[1]
    with TCtx(torch_mod, S.AUTO, [m, d], updates=True) as cx:
        assert cx.info[0]["format"] == 1
        for k, match in ((0, "set_transposable"), (1, "GEMM")):
            mm = cx.mats[k]
            assert cx.h.spmm_value_grad_bf16_info(cx.idx[k], 8) == dict(accepted=False, vb=0, tiles=0, launches=0)
            t = torch_mod.zeros(8 * (mm["rows"] + mm["cols"]) + cx.h.value_update_info(cx.idx[k])["n"], dtype=torch_mod.float32, device="cuda")
            with pytest.raises(NotImplementedError, match=match):
                cx.h.spmm_value_grad_device_bf16(cx.idx[k], t.data_ptr(), t.data_ptr() + 16 * mm["rows"], 8, t.data_ptr() + 32 * (mm["rows"] + mm["cols"]))


def test_refused_without_value_updates(torch_mod):
    m = S.case_a()[7]
    with TCtx(torch_mod, S.SLICES, [m], updates=False) as cx:
        assert cx.h.spmm_value_grad_bf16_info(cx.idx[0], 4) == dict(accepted=False, vb=0, tiles=0, launches=0)
        d = cx.device(np.zeros(4 * (m["rows"] + m["cols"]) + m["r"].size, np.float32))
        with pytest.raises(AssertionError, match="set_value_updates"):
            cx.h.spmm_value_grad_device_bf16(cx.idx[0], d.data_ptr(), d.data_ptr() + 8 * m["rows"], 4, d.data_ptr() + 16 * (m["rows"] + m["cols"]))


def test_argument_errors_come_before_any_launch(torch_mod):
    """ld < B, NULL operands, an aliased pointer, operands off 2 bytes, grad off 4 bytes and num_vecs < 1 are HISPMV_EINVAL (ValueError);
    grad is untouched."""
    m = S.case_a()[7]
    with Ctx(torch_mod, S.SLICES, [m]) as cx:
        h, idx, B, n = cx.h, cx.idx[0], 8, cx.n[0]
        gyt = torch_mod.zeros(m["rows"] * B + 8, dtype=torch_mod.bfloat16, device="cuda")
        xt = torch_mod.zeros(m["cols"] * B + 8, dtype=torch_mod.bfloat16, device="cuda")
        grad = torch_mod.full((n + 1,), 7.0, dtype=torch_mod.float32, device="cuda")
        pg, px, pr = gyt.data_ptr(), xt.data_ptr(), grad.data_ptr()
        with pytest.raises(ValueError, match="at least num_vecs"):
            h.spmm_value_grad_device_bf16(idx, pg, px, B, pr, ld_gy=B - 1)
        with pytest.raises(ValueError, match="at least num_vecs"):
            h.spmm_value_grad_device_bf16(idx, pg, px, B, pr, ld_x=B - 1)
        for args in ((0, px, B, pr), (pg, 0, B, pr), (pg, px, B, 0), (pg, px, 0, pr), (pg, px, B, pg), (pg, px, B, px)):
            with pytest.raises(ValueError):
                h.spmm_value_grad_device_bf16(idx, *args)
        for args, match in (((pg + 1, px, B, pr), "2-byte"), ((pg, px + 1, B, pr), "2-byte"), ((pg, px, B, pr + 2), "4-byte")):
            with pytest.raises(ValueError, match=match):
                h.spmm_value_grad_device_bf16(idx, *args)
        with pytest.raises(ValueError):
            h.spmm_value_grad_bf16_info(idx, 8, 7)
        with pytest.raises(ValueError):
            h.spmm_value_grad_bf16_info(idx, 0)
        with pytest.raises(IndexError):
            h.spmm_value_grad_device_bf16(99, pg, px, B, pr)
        with pytest.raises(IndexError):
            h.spmm_value_grad_bf16_info(99, 1)
        h.synchronize()
        assert (grad == 7.0).all()


# ---- sparse_linear(..., spmm=True, wide_grad="bf16") --------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [65, 130, 258])
def test_sparse_linear_wide_grad_bf16(torch_mod, B):
    """On the windowed uniform matrix with a stored transpose: y and x.grad have the bits of the wide_grad=True route; values.grad is bit
    for bit a direct call of the new entry on the same feature-major copies (ld = B rounded up to 8); at B = 130 (VB 4 = VL 4, one tile
    either way, exact widening) it is also bit for bit the wide_grad=True route's; two backward passes are bit-equal; on the default
    stream and on a side stream."""
    from hispmv_amd.torch_ops import sparse_linear
    torch = torch_mod
    m = S.case_a()[6]
    rng = np.random.default_rng(23)
    X = rng.random((B, m["cols"]), dtype=np.float32) - np.float32(0.3)
    G = rng.random((B, m["rows"]), dtype=np.float32) - np.float32(0.5)
    ld = (B + 7) & ~7
    with Pair(torch_mod, m, updates=True) as cx:
        h, P = cx.h, cx.idx[0]
        assert h.spmm_bf16_info(P, B, ld)["accepted_t"] and h.spmm_value_grad_bf16_info(P, B, ld)["accepted"]
        x16, g16 = cx.device(X).to(torch.bfloat16), cx.device(G).to(torch.bfloat16)

        def passes(wide_grad):
            x = x16.clone().requires_grad_(True)
            v = cx.device(m["v"] * np.float32(2.0)).requires_grad_(True)
            y = sparse_linear(h, P, x, None, values=v, spmm=True, wide_grad=wide_grad)
            y.backward(g16)
            torch.cuda.synchronize()
            h.synchronize()
            return y.detach().clone(), x.grad.clone(), v.grad.clone()

        def direct():
            xt = torch.zeros((m["cols"], ld), dtype=torch.bfloat16, device=x16.device)
            gt = torch.zeros((m["rows"], ld), dtype=torch.bfloat16, device=x16.device)
            xt[:, :B], gt[:, :B] = x16.t(), g16.t()
            out = torch.empty(m["r"].size, dtype=torch.float32, device=x16.device)
            torch.cuda.synchronize()
            h.spmm_value_grad_device_bf16(P, gt.data_ptr(), xt.data_ptr(), B, out.data_ptr(), 1.0, 0.0, ld_gy=ld, ld_x=ld)
            h.synchronize()
            return out

        want = direct()
        assert torch.isfinite(want).all() and want.abs().max() > 0
        for scope in ("default stream", "own stream"):
            with torch.cuda.stream(torch.cuda.Stream() if scope == "own stream" else None):
                wide = passes(True)
                half = passes("bf16")
                again = passes("bf16")
            assert half[0].dtype == torch.bfloat16 and torch.equal(half[0], wide[0]) and half[1].dtype == torch.bfloat16 and torch.equal(half[1], wide[1]), scope
            assert half[2].dtype == torch.float32 and torch.equal(half[2].view(torch.int32), want.view(torch.int32)), scope
            assert torch.equal(half[2].view(torch.int32), again[2].view(torch.int32)), scope
            if B == 130:
                assert h.spmm_value_grad_info(P, B, 132)["vl"] == 4 == h.spmm_value_grad_bf16_info(P, B, ld)["vb"]
                assert torch.equal(half[2].view(torch.int32), wide[2].view(torch.int32)), scope
