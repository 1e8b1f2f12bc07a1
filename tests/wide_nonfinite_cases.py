"""Expectations of tests/test_gpu_wide_nonfinite.py (zero slots, non-finite operands and isolation in the wide-batch entries), in one
place: which columns are poisoned, the matrix variant whose entries in some columns are +-0, and the IEEE class every output row (or,
for the value gradient, every entry) must have when one operand element is +-Inf or NaN.  tests/test_wide_nonfinite_host.py checks
the builders against a brute-force evaluation and pins what they give on the real inputs.  No product code; not a test module and not
a conftest.

The rules, from include/hispmv.h:
  forward (hispmv_spmm_device and its bf16 / transposed forms): a stored slot whose value is +-0 contributes nothing, whatever xt
    holds; every other ENTRY contributes a_k * xt[col_k, v] on its own (duplicates of the input stay separate slots).  A contribution
    of a_k * (+-Inf) is an infinity of sign(a_k) * sign(x); both signs in one row, or a NaN, give NaN; then alpha * sum + beta * bias
    keeps the class and multiplies the sign by sign(alpha).  alpha == 0 reads neither xt nor the matrix.
  value gradient (hispmv_spmm_value_grad_device): grad[k] = alpha * sum_v gyt[row_k, v] * xt[col_k, v] + beta * grad[k] whatever the
    entry's value: an explicit zero gets its gradient.  0 * Inf is NaN."""
from __future__ import annotations

import numpy as np

import step_small_cases as S

UNTOUCHED, POS_INF, NEG_INF, NAN = 0, 1, 2, 3
_POS, _NEG, _NAN = 1, 2, 4


def stored_values(m):
    """The values the handle multiplies with: those of the input, rounded to bf16 where the matrix asks for bf16 storage."""
    v = np.ascontiguousarray(m["v"], np.float32)
    return S.bf16_exact(v) if m.get("storage") == "bf16" else v


def choose_columns(m):
    """-> (Z, L): the columns by entry count descending, ties by index; Z the first three, L the next two (nnz = 0: columns 0 .. 4)."""
    counts = np.bincount(np.asarray(m["c"], np.int64), minlength=m["cols"])
    order = np.argsort(-counts, kind="stable")
    return [int(c) for c in order[:3]], [int(c) for c in order[3:5]]


def zeroed(m, Z):
    """The matrix with every entry whose column is in Z set to zero, +0 and -0 alternating in entry order.  Same pattern, so the same
    plan (the chooser never reads values); a name of its own and the vector pool of m."""
    v = np.array(m["v"], np.float32, copy=True)
    at = np.flatnonzero(np.isin(np.asarray(m["c"], np.int64), list(Z)))
    v[at[0::2]] = np.float32(0.0)
    v[at[1::2]] = np.float32(-0.0)
    return dict(m, name=m["name"] + "_zero_" + "_".join(str(int(c)) for c in Z), pool_key=m.get("pool_key", m["name"]), v=v)


def with_values(m, Z, value, tag):
    """The matrix with the entries of the columns Z set to +value, -value alternating in entry order."""
    v = np.array(m["v"], np.float32, copy=True)
    at = np.flatnonzero(np.isin(np.asarray(m["c"], np.int64), list(Z)))
    v[at[0::2]] = np.float32(value)
    v[at[1::2]] = -np.float32(value)
    return dict(m, name=m["name"] + "_" + tag, pool_key=m.get("pool_key", m["name"]), v=v)


def _classes(mask):
    out = np.full(mask.shape, UNTOUCHED, np.int8)
    out[mask == _POS] = POS_INF
    out[mask == _NEG] = NEG_INF
    out[((mask & _NAN) != 0) | (mask == (_POS | _NEG))] = NAN
    return out


def _row_mask(m, col, x_special, alpha):
    mask = np.zeros(m["rows"], np.int8)
    if alpha == 0.0:
        return mask
    v = stored_values(m)
    hit = np.flatnonzero((np.asarray(m["c"], np.int64) == col) & (v != 0.0))      # (-0.0 != 0.0 is False: both zeros are skipped)
    rows = np.asarray(m["r"], np.int64)[hit]
    if np.isnan(x_special):
        mask[rows] |= _NAN
        return mask
    assert np.isinf(x_special)
    sign = np.sign(v[hit].astype(np.float64)) * np.sign(x_special) * np.sign(alpha)
    np.bitwise_or.at(mask, rows[sign > 0], _POS)
    np.bitwise_or.at(mask, rows[sign < 0], _NEG)
    return mask


def row_class(m, col, x_special, alpha):
    """Per row of the product: UNTOUCHED, POS_INF, NEG_INF or NAN for xt[col, v] = x_special (+-Inf or NaN), every other element finite."""
    return _classes(_row_mask(m, col, x_special, alpha))


def row_classes(m, poison, alpha):
    """The same for several poisoned columns at once: poison = {col: x_special}."""
    mask = np.zeros(m["rows"], np.int8)
    for col, x in poison.items():
        mask |= _row_mask(m, col, x, alpha)
    return _classes(mask)


def entry_class(m, alpha, gy, x, row_star=None, gy_special=None, col_star=None, x_special=None):
    """Per entry of the value gradient: its class when, in each poisoned vector, gyt[row_star] = gy_special and / or xt[col_star] =
    x_special.  gy [n_poisoned, rows] and x [n_poisoned, cols] hold the finite values of those vectors; every other vector is finite
    and changes no class.  An entry is touched when its row is row_star or its column col_star, whatever its value."""
    r, c = np.asarray(m["r"], np.int64), np.asarray(m["c"], np.int64)
    mask = np.zeros(r.size, np.int8)
    if alpha == 0.0:
        return _classes(mask)
    on_row = (r == row_star) if gy_special is not None else np.zeros(r.size, bool)
    on_col = (c == col_star) if x_special is not None else np.zeros(r.size, bool)
    at = np.flatnonzero(on_row | on_col)
    for p in range(gy.shape[0]):
        g = np.where(on_row[at], np.float64(gy_special if gy_special is not None else 0.0), gy[p].astype(np.float64)[r[at]])
        xx = np.where(on_col[at], np.float64(x_special if x_special is not None else 0.0), x[p].astype(np.float64)[c[at]])
        nan = np.isnan(g) | np.isnan(xx) | (np.isinf(g) & (xx == 0.0)) | (np.isinf(xx) & (g == 0.0))
        inf = (np.isinf(g) | np.isinf(xx)) & ~nan
        sign = np.sign(g) * np.sign(xx) * np.sign(alpha)
        mask[at[nan]] |= _NAN
        mask[at[inf & (sign > 0)]] |= _POS
        mask[at[inf & (sign < 0)]] |= _NEG
    return _classes(mask)


def class_of(a):
    """The class of every float of an output: finite values are UNTOUCHED."""
    a = np.asarray(a)
    out = np.full(a.shape, UNTOUCHED, np.int8)
    out[np.isposinf(a)] = POS_INF
    out[np.isneginf(a)] = NEG_INF
    out[np.isnan(a)] = NAN
    return out


def class_of_bf16(w):
    """The same for bf16 words (uint16)."""
    w = np.asarray(w, np.uint16)
    out = np.full(w.shape, UNTOUCHED, np.int8)
    top = (w & 0x7F80) == 0x7F80
    out[top & ((w & 0x007F) != 0)] = NAN
    out[w == 0x7F80] = POS_INF
    out[w == 0xFF80] = NEG_INF
    return out


# ---- what the construction gives on the real inputs: tests/test_wide_nonfinite_host.py re-derives and pins these figures ------------------
def table():
    """name -> (matrix, transposed, entries per Z column, (rows +Inf, -Inf, NaN) for xt[L[0]] = +Inf with alpha > 0).  `transposed`: the
    poisoned index is a row of the matrix (spmm_device_t), the figures are those of the swapped matrix.  The figures 294, 290, 289 and
    144 / 119 / 7 of the windowed uniform matrix belong to its COLUMNS (the forward orientation); the transposed pair poisons its rows
    and big_band's, whose figures are the two last lines."""
    a = S.case_a()
    return {
        "no_window": (a[4], False, (15, 14, 13), (6, 7, 0)),
        "single_row_long": (S.single_row_long(), False, (24, 24, 23), (0, 0, 1)),
        "compact_256": (a[7], False, (300, 300, 300), (150, 150, 0)),
        "two_way_band": (S.two_way_band(), False, (309, 308, 308), (155, 153, 0)),
        "big_band": (S.big_band(), False, (200, 200, 200), (99, 101, 0)),
        "stray_slot_band": (S.stray_slot_band(), False, (221, 221, 221), (113, 107, 0)),
        "stray_split_band": (S.stray_split_band(), False, (214, 211, 211), (109, 100, 1)),
        "column_tiled": (S.column_tiled(), False, (6, 5, 5), (1, 1, 1)),
        "windowed_uniform": (a[6], False, (294, 290, 289), (144, 119, 7)),
        "windowed_uniform_t": (a[6], True, (250, 248, 248), (108, 122, 4)),
        "big_band_t": (S.big_band(), True, (200, 200, 200), (109, 91, 0)),
    }


def transposed_view(m):
    """The swapped COO of m with its values: rows and columns exchanged, entry order kept (what spmm_device_t multiplies with)."""
    return dict(m, name=m["name"] + "_T", rows=m["cols"], cols=m["rows"], r=m["c"], c=m["r"], expect=dict(format=0))


def zeroed_rows(m, Z):
    """m with the entries of the ROWS Z set to +-0: zeroed() on the swapped matrix, swapped back."""
    z = zeroed(transposed_view(m), Z)
    return dict(m, name=m["name"] + "_zero_rows_" + "_".join(str(int(c)) for c in Z), v=z["v"])
