"""The reference of tests/test_gpu_wide_nonfinite.py, tested first and without a GPU: the class builders of
tests/wide_nonfinite_cases.py against a brute-force evaluation (numpy float64, a loop over the entries) on three hand-written matrices
of at most 8 x 8 that hold a duplicate pair of opposite signs, an explicit zero, an empty row and an empty column; and what the
construction gives on the real inputs, pinned, so that the GPU gates cannot be vacuous: how many entries every zeroed column holds and
how many rows the first live column turns into +Inf, -Inf and NaN."""
import numpy as np
import pytest

import step_small_cases as S
import wide_nonfinite_cases as N

SPECIALS = (np.inf, -np.inf, np.nan)
ALPHAS = (0.85, -1.5, 0.0)


def tiny(name, rows, cols, entries, storage=None):
    r, c, v = (np.array(a) for a in zip(*entries))
    rng = np.random.default_rng(len(name))
    m = dict(name=name, rows=rows, cols=cols, r=r.astype(np.int32), c=c.astype(np.int32), v=v.astype(np.float32),
             b=rng.random(rows, dtype=np.float32), x=rng.random(cols, dtype=np.float32) - np.float32(0.3))
    return dict(m, storage=storage) if storage else m


def tiny_cases():
    """Row 3 and column 4 of the first are empty; (1, 2) is a duplicate pair of opposite signs, (0, 1) an explicit zero, (5, 0) a -0."""
    a = tiny("tiny_a", 6, 6, [(0, 0, 1.5), (0, 1, 0.0), (1, 2, 2.0), (1, 2, -2.0), (2, 2, -0.5), (2, 5, 3.0), (4, 1, -1.0), (5, 0, -0.0),
                              (5, 5, 0.25), (4, 5, -4.0), (0, 3, 1.0), (1, 3, 1.0)])
    b = tiny("tiny_b", 8, 5, [(0, 0, -1.0), (0, 0, 1.0), (0, 0, 1.0), (1, 1, 0.0), (1, 1, 2.0), (2, 3, -0.0), (3, 3, 5.0), (4, 3, -5.0),
                              (6, 0, 0.5), (7, 1, -0.5), (7, 3, 0.125), (6, 4, 1e-41), (7, 4, -1e-41)])            # row 5 and column 2 empty
    c = tiny("tiny_c", 7, 8, [(0, 7, 1.0), (0, 7, -1.0), (1, 7, 1e-41), (2, 7, -1e-41), (3, 0, 0.0), (3, 1, 1.0), (5, 2, -2.0), (5, 3, 2.0),
                              (6, 4, 1.0), (6, 4, 1.0), (6, 6, -3.0)], storage="bf16")                               # row 4 and column 5 empty; 1e-41 is a bf16 zero
    return [a, b, c]


def brute_forward(m, X, alpha, beta):
    """y [B, rows] in float64, entry by entry; a slot whose stored value is +-0 is skipped; alpha == 0 reads nothing."""
    v = N.stored_values(m)
    with np.errstate(all="ignore"):
        Y = np.zeros((X.shape[0], m["rows"]))
        if alpha != 0.0:
            for k in range(m["r"].size):
                if v[k] == 0.0:
                    continue
                Y[:, m["r"][k]] += np.float64(v[k]) * X[:, m["c"][k]].astype(np.float64)
            Y = alpha * Y
        return Y + beta * m["b"].astype(np.float64)


def brute_grad(m, GY, X, alpha, beta, g0):
    with np.errstate(all="ignore"):
        out = np.zeros(m["r"].size)
        for k in range(m["r"].size):
            s = 0.0
            for u in range(GY.shape[0]):
                s += np.float64(GY[u, m["r"][k]]) * np.float64(X[u, m["c"][k]])
            out[k] = (alpha * s if alpha != 0.0 else 0.0) + beta * np.float64(g0[k])
        return out


def test_tiny_cases_hold_what_they_are_for():
    for m in tiny_cases():
        pairs = list(zip(m["r"].tolist(), m["c"].tolist(), m["v"].tolist()))
        dup = [(r, c) for r, c, v in pairs if sum(1 for r2, c2, v2 in pairs if (r2, c2) == (r, c) and v2 * v < 0) > 0]
        assert dup, m["name"]
        assert (m["v"] == 0.0).any(), m["name"]
        assert np.setdiff1d(np.arange(m["rows"]), m["r"]).size > 0 and np.setdiff1d(np.arange(m["cols"]), m["c"]).size > 0, m["name"]
        assert m["rows"] <= 8 and m["cols"] <= 8
    assert (N.stored_values(tiny_cases()[2]) == 0.0).sum() == 3 and (tiny_cases()[1]["v"] != 0.0).sum() == 11      # 1e-41 lives in fp32 only


@pytest.mark.parametrize("k", range(3))
def test_row_class_against_brute_force(k):
    m = tiny_cases()[k]
    rng = np.random.default_rng(40 + k)
    B, P = 5, (0, 3, 4)
    X0 = rng.random((B, m["cols"])).astype(np.float32) - np.float32(0.3)
    for alpha in ALPHAS:
        for beta in (0.0, -2.06):
            Y0 = brute_forward(m, X0, alpha, beta)
            assert np.isfinite(Y0).all()
            for col in range(m["cols"]):
                for special in SPECIALS:
                    X = X0.copy()
                    X[list(P), col] = special
                    Y = brute_forward(m, X, alpha, beta)
                    want = N.row_class(m, col, special, alpha)
                    for v in range(B):
                        if v in P:
                            assert np.array_equal(N.class_of(Y[v]), want), (m["name"], alpha, beta, col, special, v)
                            same = want == N.UNTOUCHED
                            assert np.array_equal(Y[v][same], Y0[v][same])
                        else:
                            assert np.array_equal(Y[v], Y0[v])
            # two columns at once, as the GPU module poisons them
            for c0, c1 in ((0, 1), (2, 3), (m["cols"] - 1, 0)):
                X = X0.copy()
                X[list(P), c0], X[list(P), c1] = np.inf, np.nan
                want = N.row_classes(m, {c0: np.inf, c1: np.nan}, alpha)
                assert np.array_equal(N.class_of(brute_forward(m, X, alpha, beta)[0]), want), (m["name"], alpha, c0, c1)


def test_duplicates_stay_separate_and_zeros_are_skipped():
    a, b, c = tiny_cases()
    assert N.row_class(a, 2, np.inf, 1.0).tolist() == [0, N.NAN, N.NEG_INF, 0, 0, 0]          # (1, 2) twice with opposite signs: NaN, not a summed 0
    assert N.row_class(a, 1, np.inf, 1.0).tolist() == [0, 0, 0, 0, N.NEG_INF, 0]              # the explicit zero at (0, 1) is skipped
    assert N.row_class(a, 0, np.nan, -1.0).tolist() == [N.NAN, 0, 0, 0, 0, 0]                 # the -0 at (5, 0) as well
    assert N.row_class(a, 4, np.nan, 1.0).tolist() == [0] * 6                                 # an empty column
    assert N.row_class(b, 0, -np.inf, 2.0).tolist() == [N.NAN, 0, 0, 0, 0, 0, N.NEG_INF, 0]
    assert N.row_class(b, 4, np.inf, -1.0).tolist() == [0, 0, 0, 0, 0, 0, N.NEG_INF, N.POS_INF]   # fp32 storage: 1e-41 is live
    assert N.row_class(c, 7, np.inf, 1.0).tolist() == [N.NAN, 0, 0, 0, 0, 0, 0]                # bf16 storage: 1e-41 is a zero slot
    assert N.row_class(c, 4, -np.inf, 1.0).tolist() == [0, 0, 0, 0, 0, 0, N.NEG_INF]           # a duplicate pair of one sign


@pytest.mark.parametrize("k", range(3))
def test_entry_class_against_brute_force(k):
    m = tiny_cases()[k]
    rng = np.random.default_rng(50 + k)
    B, P = 5, (0, 3, 4)
    GY0 = rng.random((B, m["rows"])).astype(np.float32) - np.float32(0.3)
    X0 = rng.random((B, m["cols"])).astype(np.float32) - np.float32(0.3)
    GY0[3, 1] = 0.0                                                                           # a 0 * Inf among the products
    g0 = rng.random(m["r"].size).astype(np.float32)
    for alpha, beta in ((1.0, 0.0), (2.0, -1.0), (-1.0, 0.5), (0.0, 1.0)):
        G0 = brute_grad(m, GY0, X0, alpha, beta, g0)
        assert np.isfinite(G0).all()
        for row in range(m["rows"]):
            for col in range(m["cols"]):
                for gs, xs in ((None, np.inf), (np.nan, None), (np.nan, np.inf), (-np.inf, np.inf), (np.inf, None)):
                    GY, X = GY0.copy(), X0.copy()
                    if gs is not None:
                        GY[list(P), row] = gs
                    if xs is not None:
                        X[list(P), col] = xs
                    want = N.entry_class(m, alpha, GY0[list(P)], X0[list(P)], row_star=row, gy_special=gs, col_star=col, x_special=xs)
                    got = brute_grad(m, GY, X, alpha, beta, g0)
                    assert np.array_equal(N.class_of(got), want), (m["name"], alpha, beta, row, col, gs, xs)
                    same = want == N.UNTOUCHED
                    assert np.array_equal(got[same], G0[same])
                    if alpha != 0.0 and xs is not None:                                       # zero-valued entries of the column get their gradient
                        assert (want[(m["c"] == col)] != N.UNTOUCHED).all()


def test_zeroed_keeps_the_pattern_and_alternates_signs():
    m = tiny_cases()[0]
    z = N.zeroed(m, [2, 5])
    assert z["name"] != m["name"] and z["pool_key"] == m["name"] and z["r"] is m["r"] and z["c"] is m["c"]
    at = np.flatnonzero(np.isin(m["c"], [2, 5]))
    assert (z["v"][at] == 0.0).all() and np.signbit(z["v"][at]).tolist() == [bool(i & 1) for i in range(at.size)]
    rest = np.setdiff1d(np.arange(m["v"].size), at)
    assert np.array_equal(z["v"][rest].view(np.uint32), m["v"][rest].view(np.uint32)) and m["v"][at].any()
    assert N.zeroed(z, [0])["pool_key"] == m["name"]
    for col in (2, 5):
        for special in SPECIALS:
            assert (N.row_class(z, col, special, 1.0) == N.UNTOUCHED).all()
    zr = N.zeroed_rows(m, [1, 5])
    assert (zr["v"][np.isin(m["r"], [1, 5])] == 0.0).all() and np.array_equal(zr["v"][~np.isin(m["r"], [1, 5])], m["v"][~np.isin(m["r"], [1, 5])])


def test_choose_columns():
    m = tiny_cases()[0]                       # entries per column: 2, 2, 3, 2, 0, 3
    assert N.choose_columns(m) == ([2, 5, 0], [1, 3])
    assert N.choose_columns(S.case_a()[0]) == ([0, 1, 2], [3, 4])


def test_classes_of_words():
    f = np.array([1.0, np.inf, -np.inf, np.nan, -0.0, 3e38], np.float32)
    assert N.class_of(f).tolist() == [0, N.POS_INF, N.NEG_INF, N.NAN, 0, 0]
    w = np.array([0x3F80, 0x7F80, 0xFF80, 0x7FC0, 0xFF81, 0x8000, 0x7F7F], np.uint16)
    assert N.class_of_bf16(w).tolist() == [0, N.POS_INF, N.NEG_INF, N.NAN, N.NAN, 0, 0]


@pytest.mark.parametrize("name", list(N.table()))
def test_the_construction_is_not_vacuous_on_the_real_inputs(name):
    m, transposed, per_z, classes = N.table()[name]
    view = N.transposed_view(m) if transposed else m
    Z, L = N.choose_columns(view)
    assert len(set(Z + L)) == 5
    counts = np.bincount(view["c"], minlength=view["cols"])
    assert tuple(int(counts[c]) for c in Z) == per_z, (name, Z, counts[Z])
    cls = N.row_class(view, L[0], np.inf, 0.85)
    got = tuple(int((cls == k).sum()) for k in (N.POS_INF, N.NEG_INF, N.NAN))
    assert got == classes, (name, L, got)
    assert np.array_equal(N.row_class(N.zeroed(view, Z), L[0], np.inf, 0.85), cls)               # zeroing Z leaves the L columns alone
    flipped = N.row_class(view, L[0], -np.inf, 0.85)
    assert np.array_equal(flipped, N.row_class(view, L[0], np.inf, -1.5))
    assert (flipped == N.POS_INF).sum() == classes[1] and (flipped == N.NEG_INF).sum() == classes[0] and (flipped == N.NAN).sum() == classes[2]
    assert (N.row_class(view, L[1], np.nan, 0.85) == N.NAN).sum() == np.unique(view["r"][(view["c"] == L[1]) & (view["v"] != 0.0)]).size > 0
    z = N.zeroed(view, Z)
    for col, special in zip(Z, SPECIALS):
        assert (N.row_class(z, col, special, 0.85) == N.UNTOUCHED).all()
        assert (N.row_class(view, col, special, 0.85) != N.UNTOUCHED).any()                     # ... which the original values would not give


def test_further_facts_about_the_inputs():
    """stray_slot_band holds one value that is exactly 0.0 by chance: a zero slot for the reference.  In the redrawn bands the Z and L
    columns hold entries of the band (window slots) and redrawn ones far from it (strays, or elements of the other part)."""
    m = S.stray_slot_band()
    zero = np.flatnonzero(m["v"] == 0.0)
    assert zero.size == 1
    col = int(m["c"][zero[0]])
    assert N.row_class(m, col, np.nan, 1.0)[m["r"][zero[0]]] == N.UNTOUCHED or ((m["r"] == m["r"][zero[0]]) & (m["c"] == col)).sum() > 1
    for make, per_row in ((S.stray_slot_band, 210), (S.stray_split_band, 200), (S.two_way_band, 300)):
        m = make()
        Z, L = N.choose_columns(m)
        off = (m["c"].astype(np.int64) - m["r"]) % m["cols"]
        for col in Z + L:
            at = m["c"] == col
            assert (off[at] < per_row).any() and (off[at] >= per_row).any(), (m["name"], col)
    # the genuinely empty columns the GPU module poisons on top
    assert not np.isin([755], S.sparse_rows()["c"]).any() and not np.isin([148131], S.column_tiled()["c"]).any()
