"""Inputs of tests/test_gpu_block_jacobi_plans.py (the block-Jacobi extraction on every slice plan include/hispmv.h promises), in one
place: name -> the switches of the context, the value storages, the generator, and the plan the case exists for.
tests/test_block_jacobi_plans_host.py checks those plans on the host (no GPU), the GPU module checks them again from matrix_info of
the loaded handles.  Every case is square, built from generators the suite already has, and reduced so that every position is stored
ONCE (two duplicates in pairs_256, never three): three values at one position have no fixed sum (include/hispmv.h), and the tests
compare exactly.  A band of fewer than 4 M entries never gets 1024 threads, stray slots or band tiles (hispmv_choose.cpp,
hispmv_plan.cpp: stray_slots_possible): these are the smallest inputs found that still take each plan.  The row counts are no
multiples of 4 wherever the plan survives it, so that the last block is partial at every block size and the slice padding behind the
last row meets the filters of a windowed group.  No product code; not a test module and not a conftest."""
from functools import lru_cache

import numpy as np
import scipy.sparse as sp

import step_small_cases as S

f32 = np.float32

# group words of hispmv_format.h
COMPACT, STRAYS, HALF = 1, 2, 4

COLUMN_TILES = {"HISPMV_FORMAT": "slices", "HISPMV_BAND_TILES": "0", "HISPMV_COL_TILE_BYTES": "65536"}
DEFAULT = {}


def once(r, c, v, n):
    """The COO matrix with every position stored once (duplicates summed in float32: the result IS the input of the case)."""
    A = sp.coo_matrix((np.asarray(v, f32), (np.asarray(r, np.int64), np.asarray(c, np.int64))), shape=(n, n)).tocsr()
    A.sum_duplicates()
    A = A.tocoo()
    return sp.coo_matrix((A.data.astype(f32), (A.row.astype(np.int32), A.col.astype(np.int32))), shape=(n, n))


def _s_band(n, per_row, seed, redraw=0.0):
    m = S.band(n, per_row, seed, {}, redraw=redraw)
    return once(m["r"], m["c"], m["v"], n)


def _updates_band(n, per_row, half, seed):
    """The band of tests/test_gpu_value_updates.py (columns within +-half of the row, clipped) with random values."""
    from test_gpu_value_updates import _band
    r, c = _band(n, per_row, half)
    v = np.random.default_rng(seed).random(r.size, dtype=f32) - f32(0.5)
    return once(r, c, v, n)


# ---- holes_1024 ------------------------------------------------------------------------------------------------------------------------
HOLE_ROWS = tuple(range(64, 96)) + (5, 1000, 20000)          # rows 64 .. 95: diagonal block 2 (bs = 32), 4 - 5 (16), 8 - 11 (8), 16 - 23 (4)
NAN_AT, INF_AT = (200, 201), (3000, 3000)                     # inside one diagonal block each, at every block size


def _holes():
    A = _s_band(20001, 200, 31)
    keep = ~np.isin(A.row, HOLE_ROWS)
    r, c, v = A.row[keep], A.col[keep], A.data[keep].copy()
    for (i, j), val in ((NAN_AT, np.nan), (INF_AT, np.inf)):
        at = np.flatnonzero((r == i) & (c == j))
        assert at.size == 1, (i, j)
        v[at[0]] = val
    return sp.coo_matrix((v, (r, c)), shape=A.shape)


def holes_flagged(bs):
    """The blocks of holes_1024 that cannot be inverted: those with an emptied row (the band holds columns i .. i + 199 of row i, so a
    diagonal block is upper triangular and an empty row leaves an exact zero pivot; blocks of rows 64 .. 95 are zero altogether) and
    the two that hold the NaN and the Inf."""
    return sorted({i // bs for i in HOLE_ROWS} | {NAN_AT[0] // bs, INF_AT[0] // bs})


def holes_zero_blocks(bs):
    """... and those among them that are exactly zero."""
    return list(range(64 // bs, 96 // bs))


# ---- pairs_256 -------------------------------------------------------------------------------------------------------------------------
def _pairs():
    A = _s_band(4001, 300, 18)
    rng = np.random.default_rng(256)
    again = rng.choice(A.nnz, A.nnz // 50, replace=False)          # without replacement: no position is stored three times
    r, c = np.concatenate([A.row, A.row[again]]), np.concatenate([A.col, A.col[again]])
    v = np.concatenate([A.data, rng.random(again.size, dtype=f32) - f32(0.5)])
    p = rng.permutation(r.size)
    return sp.coo_matrix((v[p], (r[p], c[p])), shape=A.shape)          # (a COO keeps its duplicates: never converted)


def _stray_split():
    from test_gpu_block_jacobi import _stray_split_system
    A = _stray_split_system()
    return sp.coo_matrix((A.data.astype(f32), (A.row.astype(np.int32), A.col.astype(np.int32))), shape=A.shape)


def _exact(make):
    def run():
        A = make()
        return sp.coo_matrix((S.bf16_exact(A.data), (A.row, A.col)), shape=A.shape)
    return run


_band_1024 = lambda: _s_band(20001, 200, 31)
_band_strays = lambda: _s_band(22002, 210, 44, redraw=0.02)

# expect: threads / group (slices per group) / window / tile_kind / parts as matrix_info and the host planner name them (parts that
# all hold slices); compact and strays: "all", 0 or None (not pinned: a cut matrix); words: {storage: the value of EVERY group word},
# None where the plan has no window; odd_n: n is no multiple of 4; stored: the most entries at one position.
CASES = {
    "window_compact_256": dict(env=S.SLICES, storages=("fp32",), make=lambda: _s_band(4001, 300, 18),
                               expect=dict(threads=256, group=4, window=True, compact="all", strays=0, words={"fp32": COMPACT}, odd_n=True)),
    "window_wide_256": dict(env=S.SLICES, storages=("fp32",), make=lambda: _s_band(4001, 300, 43, redraw=0.01),
                            expect=dict(threads=256, group=4, window=True, compact=0, strays=0, words={"fp32": 0}, odd_n=True)),
    "window_compact_1024": dict(env=S.SLICES, storages=("fp32",), make=_band_1024,
                                expect=dict(threads=1024, group=16, window=True, compact="all", strays=0, words={"fp32": COMPACT}, odd_n=True)),
    "half_1024": dict(env=S.SLICES, storages=("bf16",), make=_exact(_band_1024),
                      expect=dict(threads=1024, group=16, window=True, compact="all", strays=0, words={"bf16": COMPACT | HALF}, odd_n=True)),
    "strays_1024": dict(env=S.SLICES, storages=("fp32",), make=_band_strays,
                        expect=dict(threads=1024, group=18, window=True, compact="all", strays="all", words={"fp32": COMPACT | STRAYS}, odd_n=True)),
    "half_strays_1024": dict(env=S.SLICES, storages=("bf16",), make=_exact(_band_strays),
                             expect=dict(threads=1024, group=18, window=True, compact="all", strays="all", words={"bf16": COMPACT | STRAYS | HALF},
                                         odd_n=True)),
    "holes_1024": dict(env=S.SLICES, storages=("fp32", "bf16"), make=_holes,
                       expect=dict(threads=1024, group=16, window=True, compact="all", strays=0, words={"fp32": COMPACT, "bf16": COMPACT | HALF},
                                   odd_n=True)),
    "pairs_256": dict(env=S.SLICES, storages=("fp32", "bf16"), make=_pairs,
                      expect=dict(threads=256, group=4, window=True, compact="all", strays=0, words={"fp32": COMPACT, "bf16": COMPACT | HALF},
                                  odd_n=True, stored=2)),
    "column_tiles_8": dict(env=COLUMN_TILES, storages=("fp32",), make=lambda: _updates_band(70001, 8, 30000, 8),
                           expect=dict(threads=256, window=False, tile_kind=1, parts=8, compact=None, strays=None, words=None, odd_n=True)),
    # (at n = 210001 the chooser takes a tile stream instead: keep 250000)
    "band_tiles": dict(env=DEFAULT, storages=("fp32",), make=lambda: _updates_band(250000, 20, 30000, 20),
                       expect=dict(threads=1024, window=True, tile_kind=2, parts=3, compact=None, strays=None, words=None, odd_n=False)),
    "stray_split": dict(env=S.SLICES, storages=("fp32", "bf16"), make=_stray_split,
                        expect=dict(tile_kind=3, parts=2, compact=None, strays=None, words=None, odd_n=False)),
}


@lru_cache(maxsize=None)
def matrix(name):
    """The input of the case (scipy COO, float32, int32 indices): what create_sparse_handle gets.  Built once, never changed."""
    A = CASES[name]["make"]()
    for a in (A.row, A.col, A.data):
        a.setflags(write=False)
    return A


def stored(A, storage):
    """The matrix the handle holds: a bf16 handle rounds every entry on its own, once (duplicates are summed in fp32 afterwards)."""
    return A if storage == "fp32" else sp.coo_matrix((S.bf16_exact(A.data), (A.row, A.col)), shape=A.shape)


def as_case(name):
    """The case in the form of the small-case generators (step_small_cases.host_info takes it)."""
    A = matrix(name)
    return dict(name=name, rows=A.shape[0], cols=A.shape[1], r=A.row, c=A.col, v=A.data)


def most_stored(A):
    """The most entries any one position holds."""
    key = A.row.astype(np.int64) * A.shape[1] + A.col
    return int(np.unique(key, return_counts=True)[1].max())
