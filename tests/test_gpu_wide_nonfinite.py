"""Zero slots, non-finite operands and bf16 edge rounding in the wide-batch entries (spmm_device, spmm_device_t, spmm_device_bf16,
spmm_device_t_bf16, spmm_value_grad_device), whose other tests use finite operands only.  Three promises of include/hispmv.h:

ZERO SLOTS: a stored slot whose value is +-0 contributes nothing, whatever xt holds.  A wrong keep mask, a mask on the wrong half of a
packed dword or a filler that slips through is 0 * x on finite data and passes every other gate; with Inf or NaN in xt it is NaN.
ISOLATION: the bits of vector v depend neither on num_vecs nor on the tile or lane width that carried it -- a non-finite value in
one vector must leave every other vector's bits alone.
BF16 OUTPUT ROUNDING: nearest, ties to even; +-Inf stay; overflow becomes Inf; a NaN becomes a quiet NaN.

Per matrix m of tests/step_small_cases.py (one context each), Z, L = choose_columns(m) and mz = zeroed(m, Z) of
tests/wide_nonfinite_cases.py, whose builders tests/test_wide_nonfinite_host.py checks against a brute force.  The context asserts
that mz got the plan of m (check_expect).  Batches B = 65 and 257: fp32 at ld 68 and 260 (VL 2 with lane 32 half live; VL 4 and a
one-vector tail tile), bf16 at ld 72 and 264 (VB 2; VB 8 with lane 32 straddling n_vecs); matrices of more than 8192 columns take
narrower lanes.  Poisoned vectors P = {0, 37, B - 1}: vector 0 is what lanes past the batch gather, 36 and 38 share a lane with 37,
B - 1 sits in the masked last lane or in the tail tile.  (alpha, beta) = (0.85, -2.06) and (-1.5, 0.5).  Per entry and B:
  1. the call on the finite batch, Y0, passes the fp64 gate of tests/test_gpu_spmm.py (bf16: equals the rounded fp32 entry, which does);
  2. xt[Z] = +Inf, -Inf, NaN in the vectors of P (and in genuinely empty columns where the matrix has some): Y == Y0 bit for bit.
     Column 0 is always among the zeroed and poisoned ones: a skipped element gathers row 0 of xt, so only a non-finite row 0 shows
     a mask that is missing (found by dropping the mask: without row 0 the gate passed on every matrix whose Z lacks column 0);
  3. xt[L[0]] = +Inf, xt[L[1]] = NaN in the vectors of P: every other vector and every row the reference calls untouched keep the bits
     of Y0, every other row has exactly the reference's class (+Inf, -Inf, NaN); alpha = 0 gives exactly beta * bias;
  4. (big_band, updatable) zeros pushed into the Z entries through update_values_device make them zero slots, the original values
     pushed back make them propagate.
The transposed entries repeat 2 and 3 with poisoned ROWS on a handle with a stored transpose and must also equal, bit for bit, the
forward call on the handle of the swapped matrix.  STORED VALUE DECIDES: entries of +-1e-41 (an fp32 subnormal that rounds to a bf16
zero) are zero slots on a bf16-storage handle and live on an fp32 one.  The value gradient has no zero-slot rule: an explicit zero gets
its gradient, so on zeroed(m, Z) the entries of column Z[0] must turn non-finite with xt[Z[0]].

EDGE ROUNDING: the shared fp32 bias holds SPECIAL_BITS of tests/test_gpu_value_updates_bf16.py tiled over the rows, the batch is all
zeros, so (alpha, beta) = (1, 1) finishes every row through its own store site with 0 + special and (0, 1) through the bias launch.
The fp32 entry must return every special that is neither NaN nor +-0 bit for bit (it saw the value and flushed nothing); the bf16
word must be the integer rule of hispmv_format.h (S.bf16_exact) of the fp32 entry's output wherever that is no NaN, and a NaN word
where it is.  NaN payloads are not pinned.  No tolerance anywhere except the existing TOL on the finite baselines."""
import numpy as np
import pytest

import step_small_cases as S
import wide_nonfinite_cases as N
from conftest import TOL
from test_gpu_spmm import ALL_PAIRS, Wide, batch, bits
from test_gpu_spmm_bf16 import Oracle, WideBf16, to_bf16, widen
from test_gpu_spmm_companion import Pair, scatter_truth
from test_gpu_spmm_value_grad import Ctx as GradCtx, batch_t
from test_gpu_transpose import _PACKS, Ctx
from test_gpu_value_updates_bf16 import SPECIAL_BITS
from util import bwd_err

pytestmark = pytest.mark.gpu

INF, NAN = np.float32(np.inf), np.float32(np.nan)
WORD = {"inf": 0x7F80, "-inf": 0xFF80, "nan": 0x7FC0}
PAIRS = (S.PAIRS[0], (-1.5, 0.5))
BATCHES = (65, 257)
assert PAIRS[1] in ALL_PAIRS and PAIRS[1][0] < 0


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def poisoned(B):
    return [0, 37, B - 1]


def gather_row(Z, L):
    """A skipped element gathers row 0 of xt before its floats are masked, so a dropped mask shows only when row 0 is not finite:
    column 0 joins the zeroed, poisoned columns (it is one of Z in every band; not where it is one of the live columns L)."""
    return [] if 0 in list(Z) + list(L) else [0]


class Fp32Entry:
    """spmm_device (t: spmm_device_t) on matrix k of a context.  Every call uploads its xt: the cache of Wide goes by the first
    features of the batch, which a poisoned column further on does not change."""
    name = "fp32"

    def __init__(self, cx, k, t=False):
        self.cx, self.t, self.m = cx, t, cx.mats[k]
        self.w = Wide(cx, k, t)
        self.pool, self._sums = self.w.pool, None

    def ld(self, B):
        return (B + 3) & ~3

    def finite(self, B):
        return batch(self.pool, B)

    def poison(self, X, special, B):
        X = X.copy()
        for col, x in special.items():
            X[poisoned(B), col] = x
        return X

    def call(self, X, b, alpha, beta):
        self.w._xt = {}
        return self.w.call(X, b, alpha, beta, ld=self.ld(X.shape[0]))

    def forward_truth(self, B, b, alpha, beta):
        return self.w.truth(range(B), b, alpha, beta)

    def truth(self, B, b, alpha, beta):
        """(y64, mag) [B, n_out] of the finite batch; transposed: the fp64 scatter of tests/test_gpu_spmm_companion.py, its sums taken
        once per entry for the largest batch."""
        if not self.t:
            return self.forward_truth(B, b, alpha, beta)
        if self._sums is None:
            self._sums = scatter_truth(self.m, self.pool, range(max(BATCHES)), np.zeros(self.m["cols"]), 1.0, 0.0)
        bb = beta * np.asarray(b, np.float64)
        return alpha * self._sums[0][:B] + bb, abs(alpha) * self._sums[1][:B] + np.abs(bb)

    def gate(self, Y0, X, b, alpha, beta):
        B = X.shape[0]
        y64, mag = self.truth(B, b, alpha, beta)
        err = max(bwd_err(Y0[i], y64[i], mag[i]) for i in range(B))
        print(f'{self.m["name"]}: {self.name}{" transposed" if self.t else ""} B={B} alpha={alpha} beta={beta} baseline backward error {err:.3e}')
        assert np.isfinite(Y0).all() and err < TOL, (self.m["name"], self.name, B, alpha, beta, err)

    raw = staticmethod(bits)
    classes = staticmethod(N.class_of)

    def same(self, a, b):
        return np.array_equal(self.raw(a), self.raw(b))

    def bias_only(self, b, beta):
        return np.float32(beta) * np.asarray(b, np.float32)


class Bf16Entry(Fp32Entry):
    """spmm_device_bf16 (t: spmm_device_t_bf16); the baseline is gated through the fp32 entry on the widened operands."""
    name = "bf16"

    def __init__(self, cx, k, t=False):
        self.cx, self.t, self.m = cx, t, cx.mats[k]
        self.o = Oracle(cx, k, t)
        self.w = WideBf16(cx, k, t)
        self.pool, self._sums = self.o.pool, None

    def ld(self, B):
        return (B + 7) & ~7

    def finite(self, B):
        return to_bf16(self.cx.torch, batch(self.pool, B))

    def poison(self, X16, special, B):
        X16 = X16.copy()
        for col, x in special.items():
            X16[poisoned(B), col] = WORD[str(float(x))]
        return X16

    def forward_truth(self, B, b, alpha, beta):
        return self.o.truth(range(B), b, alpha, beta)

    def gate(self, Y0, X16, b, alpha, beta):
        X = widen(X16)
        assert np.array_equal(bits(X), bits(batch(self.pool, X16.shape[0])))
        ref = self.o.call(X, b, alpha, beta)
        Fp32Entry.gate(self, ref, X, b, alpha, beta)
        assert np.array_equal(Y0, to_bf16(self.cx.torch, ref)), (self.m["name"], "bf16 baseline", alpha, beta)

    raw = staticmethod(lambda a: np.asarray(a, np.uint16))
    classes = staticmethod(N.class_of_bf16)

    def bias_only(self, b, beta):
        return S.bf16_exact(np.float32(beta) * np.asarray(b, np.float32)).view(np.uint32) >> 16


def check_propagation(e, Y, Y0, want, B, what):
    """Gate 3: the vectors outside P and the untouched rows keep the bits of Y0; every other row has the reference's class."""
    P = poisoned(B)
    others = np.setdiff1d(np.arange(B), P)
    assert e.same(Y[others], Y0[others]), (what, "a vector that is not poisoned changed")
    assert (want != N.UNTOUCHED).any(), (what, "vacuous")
    same = want == N.UNTOUCHED
    for v in P:
        got = e.classes(Y[v])
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (what, v, bad.size, bad[:8], got[bad[:8]], want[bad[:8]])
        assert e.same(Y[v][same], Y0[v][same]), (what, v, "an untouched row changed")


def run_gates(e, ref, b, Z, L, empty=(), mirror=None, batches=BATCHES, pairs=PAIRS, zero_slots=True):
    """Gates 1 to 3 of the module docstring for entry e.  ref: the matrix the classes come from (its columns are the poisoned index);
    empty: further columns without a live entry, poisoned with the zeroed ones; mirror: an entry that must give the same bits on every
    call (the forward call on the swapped handle)."""
    name = ref["name"]
    zeros = dict(zip(Z, (INF, -INF, NAN)))
    zeros.update(zip(empty, (NAN, INF, -INF, NAN)))
    if zero_slots:
        assert 0 in zeros or 0 in L, name
        for col in zeros:
            assert (N.row_class(ref, col, NAN, 1.0) == N.UNTOUCHED).all(), (name, col, "a poisoned column of gate 2 holds a live entry")
    live = {L[0]: INF, L[1]: NAN}
    assert len(set(Z) | set(L)) == len(Z) + 2 and not (set(empty) & (set(Z) | set(L)))
    for B in batches:
        X = e.finite(B)

        def call(X, alpha, beta):
            Y = e.call(X, b, alpha, beta)
            if mirror is not None:
                assert e.same(Y, mirror.call(X, b, alpha, beta)), (name, e.name, B, alpha, beta, "differs from the forward call on the swapped handle")
            return Y

        for alpha, beta in pairs:
            tag = (name, e.name, B, alpha, beta)
            Y0 = call(X, alpha, beta)
            e.gate(Y0, X, b, alpha, beta)                                                            # 1
            if zero_slots:
                Y = call(e.poison(X, zeros, B), alpha, beta)
                diff = np.argwhere(e.raw(Y) != e.raw(Y0))
                assert e.same(Y, Y0), (tag, "zero slots", len(diff), diff[:8].tolist())              # 2
            want = N.row_classes(ref, live, alpha)
            if ref["r"].size == 0:
                assert (want == N.UNTOUCHED).all()
                assert e.same(call(e.poison(X, live, B), alpha, beta), Y0) and all(e.same(Y0[v], e.bias_only(b, beta)) for v in range(B)), tag
            else:
                check_propagation(e, call(e.poison(X, live, B), alpha, beta), Y0, want, B, tag)      # 3
        Y = call(e.poison(X, live, B), 0.0, 1.0)
        assert all(e.same(Y[v], e.bias_only(b, 1.0)) for v in range(B)) and (e.classes(Y) == N.UNTOUCHED).all(), (name, e.name, B, "alpha = 0")


# ---- gates 1 to 3, one context per plan class ---------------------------------------------------------------------------------------------
def _no_window():
    a = S.case_a()
    return S.SLICES, [a[0], a[4], a[10]]


CLASSES = {
    "no_window_nnz0_fillers": _no_window,
    "long_chain": lambda: (S.SLICES, [S.single_row_long()]),
    "compact_256": lambda: (S.SLICES, [S.case_a()[7]]),
    "wide_groups": lambda: (S.NOSPLIT, [S.two_way_band()]),
    "compact_1024": lambda: (S.SLICES, [S.big_band()]),
    "stray_slots": lambda: (S.SLICES, [S.stray_slot_band()]),
    "stray_split": lambda: (S.SLICES, [S.stray_split_band()]),
    "eight_column_parts": lambda: (S.COLTILES, [S.column_tiled()]),
    "half_groups": lambda: (S.SLICES, [S.as_bf16(S.big_band())]),
}


def empty_columns(m):
    """Three columns without any entry, for the matrices the issue names: 755 of sparse_rows and 148 131 of column_tiled among them."""
    if m["name"] not in ("sparse_rows", S.column_tiled()["name"]):
        return ()
    free = np.setdiff1d(np.arange(m["cols"]), m["c"])
    must = 755 if m["name"] == "sparse_rows" else 148131
    assert must in free and free.size >= 3
    return (must, int(free[0]) if free[0] != must else int(free[1]), int(free[-1]) if free[-1] != must else int(free[-2]))


@pytest.mark.parametrize("kind", list(CLASSES))
def test_zero_slots_propagation_and_isolation(torch_mod, kind):
    env, mats = CLASSES[kind]()
    picks = [N.choose_columns(m) for m in mats]
    zs = [N.zeroed(m, Z + gather_row(Z, L)) if m["r"].size else m for m, (Z, L) in zip(mats, picks)]
    with Ctx(torch_mod, env, zs) as cx:                                     # (check_expect: the zeroed matrix got the plan of the original)
        if kind == "half_groups":
            st = cx.h.value_storage_info(cx.idx[0])
            assert st["storage"] == "bf16" and st["slots_2byte"] > 0, st
        for k, (m, mz, (Z, L)) in enumerate(zip(mats, zs, picks)):
            for entry in (Fp32Entry, Bf16Entry):
                run_gates(entry(cx, k), mz, m["b"], Z, L, empty=empty_columns(m) + tuple(gather_row(Z, L)))


# ---- gate 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_updated_zeros_become_zero_slots_and_updated_values_leave_them(torch_mod):
    m = S.big_band()
    Z, L = N.choose_columns(m)
    assert 0 in Z
    mz = N.zeroed(m, Z)
    torch = torch_mod
    with Ctx(torch, S.SLICES, [m], updates=True) as cx:
        assert cx.h.value_update_info(cx.idx[0])["updatable"]

        def push(v):
            dv = cx.device(v)
            torch.cuda.synchronize()
            cx.h.update_values_device(cx.idx[0], dv.data_ptr(), dv.numel())
            cx.h.synchronize()

        for entry in (Fp32Entry, Bf16Entry):
            push(mz["v"])
            cx.mats[0] = mz                                                 # (the truth of the baseline goes by the values the handle holds)
            run_gates(entry(cx, 0), mz, m["b"], Z, L, batches=(65,), pairs=PAIRS[:1])
            push(m["v"])
            cx.mats[0] = m
            run_gates(entry(cx, 0), m, m["b"], [], Z[:2], batches=(65,), pairs=PAIRS[:1], zero_slots=False)


# ---- the transposed entries -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [S.big_band, lambda: S.case_a()[6]], ids=["big_band", "windowed_uniform"])
def test_transposed_entries(torch_mod, make):
    """The poisoned index is a ROW of the matrix.  P is the handle with the stored transpose, R the handle of the swapped matrix."""
    m = make()
    Z, L = N.choose_columns(N.transposed_view(m))
    mz = N.zeroed_rows(m, Z + gather_row(Z, L))
    with Pair(torch_mod, mz) as cx:
        ref = dict(cx.mats[1], v=mz["v"])
        assert np.array_equal(ref["c"], m["r"]) and np.array_equal(ref["r"], m["c"]) and (ref["v"][np.isin(ref["c"], Z)] == 0.0).all()
        assert cx.h.spmm_info(cx.idx[0], 65, 68)["accepted_t"] and cx.h.spmm_bf16_info(cx.idx[0], 65, 72)["accepted_t"]
        bias = np.resize(m["b"], m["cols"]).astype(np.float32)
        for entry in (Fp32Entry, Bf16Entry):
            e, mirror = entry(cx, 0, t=True), entry(cx, 1)
            assert np.array_equal(e.pool, mirror.pool)
            run_gates(e, ref, bias, Z, L, empty=tuple(gather_row(Z, L)), mirror=mirror)


# ---- the stored value decides ---------------------------------------------------------------------------------------------------------------
def test_the_stored_value_decides(torch_mod):
    """Entries of +-1e-41: an fp32 subnormal below 0x00008000, which rounds to a bf16 zero.  On the bf16-storage handle (the loader
    rounds) they are zero slots; on the fp32 handle they are live and 1e-41 * Inf is Inf -- fp32 denormals are not flushed, the
    compiler's default for gfx950.  A NaN there instead would be 0 * Inf from a flushed denormal."""
    m = S.big_band()
    Z, L = N.choose_columns(m)
    assert 0 in Z
    tiny = N.with_values(m, Z, 1e-41, "tiny")
    at = np.isin(m["c"], Z)
    assert (tiny["v"][at] != 0.0).all() and (np.abs(tiny["v"][at]).view(np.uint32) < 0x8000).all() and (S.bf16_exact(tiny["v"])[at] == 0.0).all()
    half = dict(tiny, name=tiny["name"] + "_bf16_storage", storage="bf16")
    with Ctx(torch_mod, S.SLICES, [tiny, half]) as cx:
        assert cx.h.value_storage_info(cx.idx[0])["storage"] == "fp32" and cx.h.value_storage_info(cx.idx[1])["storage"] == "bf16"
        cx.mats[1] = dict(half, v=S.bf16_exact(half["v"]))                  # (what the handle stores: the truth of its baseline)
        for entry in (Fp32Entry, Bf16Entry):
            run_gates(entry(cx, 1), cx.mats[1], m["b"], Z, L, batches=(65,))
            # fp32 storage: the three columns propagate by the sign rule
            e = entry(cx, 0)
            X = e.finite(65)
            for alpha, beta in PAIRS:
                want = N.row_classes(tiny, dict(zip(Z, (INF, -INF, NAN))), alpha)
                assert (want == N.POS_INF).any() and (want == N.NEG_INF).any() and (want == N.NAN).any()
                Y0 = e.call(X, m["b"], alpha, beta)
                e.gate(Y0, X, m["b"], alpha, beta)
                check_propagation(e, e.call(e.poison(X, dict(zip(Z, (INF, -INF, NAN))), 65), m["b"], alpha, beta), Y0, want, 65, (tiny["name"], e.name, alpha))
                only = N.row_classes(tiny, {Z[0]: INF}, alpha)
                assert not (only == N.NAN).any() and (only != N.UNTOUCHED).sum() == 200
                check_propagation(e, e.call(e.poison(X, {Z[0]: INF}, 65), m["b"], alpha, beta), Y0, only, 65, (tiny["name"], e.name, alpha, "one column"))


# ---- the value gradient ---------------------------------------------------------------------------------------------------------------------
class ExplicitGrad(GradCtx):
    """The wide-gradient context with operands given as arrays: wide(k, "explicit", ...) takes self.explicit = (gyt [rows, ld], xt [cols, ld])."""
    explicit = None

    def operands(self, k, kind, B, ld, shift):
        if kind != "explicit":
            return super().operands(k, kind, B, ld, shift)
        gyt, xt = self.explicit
        assert gyt.shape == (self.mats[k]["rows"], ld) and xt.shape == (self.mats[k]["cols"], ld) and shift == 0
        return self.device(gyt.reshape(-1)), self.device(xt.reshape(-1))

    def grad(self, k, gyt, xt, B, g0, alpha, beta):
        self.explicit = (gyt, xt)
        return self.wide(k, "explicit", B, g0, alpha, beta, ld=gyt.shape[1])


@pytest.mark.parametrize("make", [S.big_band, S.stray_split_band, lambda: S.case_a()[4]], ids=["big_band", "stray_split_band", "no_window"])
def test_value_gradient(torch_mod, make):
    """(a) xt[L[0]] = +Inf, (b) gyt[fullest row] = NaN on m; (c) both on zeroed(m, Z) with the column Z[0], whose zero-valued entries
    must turn non-finite.  The gradient never reads the values, so the finite baseline of the zeroed handle has the bits of m's."""
    m = make()
    Z, L = N.choose_columns(m)
    mz = N.zeroed(m, Z)
    r_star = int(np.argmax(np.bincount(m["r"], minlength=m["rows"])))
    in_z0 = m["c"] == Z[0]
    assert (mz["v"][in_z0] == 0.0).all() and in_z0.sum() > 0
    with ExplicitGrad(torch_mod, S.SLICES, [m, mz]) as cx:
        n = cx.n[0]
        GY, X = cx.pools(0, "floats")
        g0 = np.random.default_rng(300).random(n, dtype=np.float32) - np.float32(0.5)
        for B in BATCHES:
            ld, P = (B + 3) & ~3, poisoned(B)
            gyt, xt = batch_t(GY, B, ld), batch_t(X, B, ld)
            gy_p, x_p = gyt[:, P].T.copy(), xt[:, P].T.copy()
            s, a = cx.sums(0, "floats", B, magnitudes=True)
            for alpha, beta in ((1.0, 0.0), (2.0, -1.0)):
                start = None if beta == 0.0 else g0
                tag = (m["name"], B, alpha, beta)
                G0 = cx.grad(0, gyt, xt, B, start, alpha, beta)
                g64 = alpha * s + beta * g0.astype(np.float64)
                mag = abs(alpha) * a + np.abs(beta * g0.astype(np.float64))
                assert np.isfinite(G0).all() and (np.abs(G0.astype(np.float64) - g64) <= TOL * mag).all(), tag
                assert np.array_equal(bits(cx.grad(1, gyt, xt, B, start, alpha, beta)), bits(G0)), (tag, "the zeroed handle's baseline")

                def check(got, want, what):
                    assert (want != N.UNTOUCHED).any(), (tag, what, "vacuous")
                    bad = np.flatnonzero(N.class_of(got) != want)
                    assert bad.size == 0, (tag, what, bad.size, bad[:8], got[bad[:8]], want[bad[:8]])
                    same = want == N.UNTOUCHED
                    assert np.array_equal(bits(got[same]), bits(G0[same])), (tag, what, "an untouched entry changed")

                xa = xt.copy()
                xa[L[0], P] = INF
                check(cx.grad(0, gyt, xa, B, start, alpha, beta), N.entry_class(m, alpha, gy_p, x_p, col_star=L[0], x_special=INF), "(a)")
                gb = gyt.copy()
                gb[r_star, P] = NAN
                check(cx.grad(0, gb, xt, B, start, alpha, beta), N.entry_class(m, alpha, gy_p, x_p, row_star=r_star, gy_special=NAN), "(b)")
                xc = xt.copy()
                xc[Z[0], P] = INF
                got = cx.grad(1, gb, xc, B, start, alpha, beta)
                check(got, N.entry_class(mz, alpha, gy_p, x_p, row_star=r_star, gy_special=NAN, col_star=Z[0], x_special=INF), "(c)")
                assert not np.isfinite(got[in_z0]).any(), (tag, "an explicit zero gets its gradient")


# ---- bf16 edge rounding ---------------------------------------------------------------------------------------------------------------------
def is_nan_bits(u):
    return (np.asarray(u, np.uint32) & 0x7FFFFFFF) > 0x7F800000


EDGE = {
    "slice_store": lambda: (S.SLICES, S.case_a()[4]),
    "fix_up_launch": lambda: (S.SLICES, S.single_row_long()),
    "fix_up_every_special": lambda: (S.SLICES, S.case_a()[7]),
    "tile_accumulator": lambda: (S.COLTILES, S.column_tiled()),
    "half_groups": lambda: (S.SLICES, S.as_bf16(S.big_band())),
}


@pytest.mark.parametrize("kind", list(EDGE))
def test_bf16_edge_rounding(torch_mod, kind):
    env, m = EDGE[kind]()
    rows = m["rows"]
    sp = np.resize(SPECIAL_BITS, rows).astype(np.uint32)
    bias = sp.view(np.float32)
    nan_sp, zero_sp = is_nan_bits(sp), (sp & 0x7FFFFFFF) == 0
    assert is_nan_bits(SPECIAL_BITS).sum() == 4 and SPECIAL_BITS.size == 32
    with Ctx(torch_mod, env, [m]) as cx:
        info = cx.info[0]
        if kind == "fix_up_launch":
            assert rows == 1 and cx.h.spmm_bf16_info(cx.idx[0], 8)["launches"] == 2
        if kind == "tile_accumulator":
            assert info["col_tiles"] == 8
        if kind == "fix_up_every_special":      # (single_row_long has one row, so one special; here 1156 rows are cut between slices,
            # each finished by the fix-up launch alone, and they meet every special)
            key = (m["name"], info["format"], info["col_tiles"], info["tile_kind"], info["col_tile_width"], info["col_tile_base"], info["group_slices"])
            cut = np.concatenate([np.asarray(p.fix[:, 0]) for p in _PACKS[key]])
            assert set((cut % 32).tolist()) == set(range(32)), "the cut rows do not meet every special"
        o, w = Oracle(cx, 0), WideBf16(cx, 0)
        for B, ld, shift in ((65, 72, 0), (130, 136, 0), (257, 264, 0), (65, 68, 1)):
            X = np.zeros((B, m["cols"]), np.float32)
            X16 = np.zeros((B, m["cols"]), np.uint16)
            for alpha, beta in ((1.0, 1.0), (0.0, 1.0)):
                tag = (m["name"], B, ld, shift, alpha)
                F = bits(o.call(X, bias, alpha, beta, ld=ld, shift=shift)).view(np.uint32)
                Y = w.call(X16, bias, alpha, beta, ld=ld, shift=shift)
                exact = ~nan_sp & ~zero_sp
                assert (F[:, exact] == sp[exact]).all(), (tag, "the fp32 entry did not return the special")
                assert (is_nan_bits(F) == nan_sp).all() and ((F[:, zero_sp] & 0x7FFFFFFF) == 0).all(), tag
                want = S.bf16_exact(F.view(np.float32)).view(np.uint32) >> 16
                bad = np.argwhere((Y != want) & ~nan_sp)
                assert bad.size == 0, (tag, len(bad), bad[:8].tolist(), [hex(int(Y[i, j])) for i, j in bad[:8]], [hex(int(F[i, j])) for i, j in bad[:8]])
                assert (N.class_of_bf16(Y[:, nan_sp]) == N.NAN).all(), (tag, "a NaN did not stay a NaN")
        # in place: the matrix bias holds the specials' bf16 words; widening is exact, 0 + b is b (and +0 for b = -0)
        B = 65
        w16 = (sp >> 16).astype(np.uint16)
        Y = w.call(np.zeros((B, m["cols"]), np.uint16), np.broadcast_to(w16, (B, rows)), 1.0, 1.0, bias="in_place")
        nan16 = N.class_of_bf16(w16) == N.NAN
        want = np.where(w16 == 0x8000, 0, w16).astype(np.uint16)
        assert (Y[:, ~nan16] == want[~nan16]).all(), (m["name"], "in place")
        assert (N.class_of_bf16(Y[:, nan16]) == N.NAN).all(), (m["name"], "in place: a NaN did not stay a NaN")


def test_no_free_was_rejected():
    from hispmv_amd._lib import lib
    assert lib.hispmv_free_failures() == 0
