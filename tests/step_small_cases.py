"""Inputs of tests/test_gpu_step_small.py (the step kernel and the chunked batch tails at small shapes), in one place: the
generators, the plan every input is expected to get from the loader at 256 CUs, and the environment switches of each case.
tests/test_step_small_inputs.py checks those expectations on the host (no GPU), the GPU module checks them again from
matrix_info of the loaded handles.  No product code; not a test module and not a conftest."""
from __future__ import annotations

import os
from contextlib import contextmanager

import numpy as np

SLICES = {"HISPMV_FORMAT": "slices"}
AUTO = {"HISPMV_FORMAT": "auto", "HISPMV_TTS_MIN_NNZ": "20000"}
COLTILES = {"HISPMV_FORMAT": "slices", "HISPMV_COL_TILE_BYTES": "65536"}
NOSPLIT = {"HISPMV_FORMAT": "slices", "HISPMV_STRAY_SPLIT": "0"}
TTS = {"HISPMV_FORMAT": "tts"}                                   # every candidate of >= 64 K entries becomes a tile stream, the rest stay slice streams
TTS_XLDS = {"HISPMV_FORMAT": "tts", "HISPMV_TTS_XLDS": "1"}      # ... and x of <= 16 K floats is kept in the LDS
TTS_SMALL = {"HISPMV_FORMAT": "tts", "HISPMV_TTS_SMALL": "1"}    # ... in the 13 K-slot geometry where a gather touches <= 8 lines


@contextmanager
def environment(env):
    """The switches of a case, set for the duration of the block (the loader reads most of them when a context is created,
    HISPMV_NO_XCD_PIN when a batch plan is built) and restored afterwards."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _finish(name, rows, cols, r, c, seed, expect):
    rng = np.random.default_rng(1000 + seed)
    r = np.asarray(r, np.int32)
    c = np.asarray(c, np.int32)
    v = rng.random(r.size, dtype=np.float32) - np.float32(0.5)
    x = rng.random(cols, dtype=np.float32) - np.float32(0.3)
    b = rng.random(rows, dtype=np.float32)
    return dict(name=name, rows=rows, cols=cols, r=r, c=c, v=v, x=x, b=b, expect=expect)


def uniform(rows, cols, nnz, seed, expect, heavy_row=None, name=None):
    """nnz entries anywhere; heavy_row = (row, share): that share of the entries sits in one row (a row cut over many slices)."""
    rng = np.random.default_rng(seed)
    r = rng.integers(0, rows, nnz)
    c = rng.integers(0, cols, nnz)
    if heavy_row is not None:
        r[: int(nnz * heavy_row[1])] = heavy_row[0]
    return _finish(name or f"uniform_{rows}x{cols}_{nnz}_s{seed}", rows, cols, r, c, seed, expect)


def band(n, per_row, seed, expect, redraw=0.0, name=None):
    """Row i holds columns i .. i + per_row - 1 (mod n); `redraw`: that share of the entries gets a random column instead."""
    rng = np.random.default_rng(seed)
    r = np.repeat(np.arange(n, dtype=np.int64), per_row)
    c = (r + np.tile(np.arange(per_row, dtype=np.int64), n)) % n
    if redraw > 0:
        c = np.where(rng.random(r.size) < redraw, rng.integers(0, n, r.size), c)
    return _finish(name or f"band_{n}x{per_row}_r{redraw}_s{seed}", n, n, r, c, seed, expect)


def one_by_one():
    return _finish("one_by_one", 1, 1, [0], [0], 91, dict(format=0, threads=256, groups=1, window=False))


def single_row(seed=92):
    """One row of 30 000 entries: cut over some thirty slices, every one of them carries into the next."""
    rng = np.random.default_rng(seed)
    return _finish("single_row", 1, 4096, np.zeros(30000, np.int64), rng.integers(0, 4096, 30000), seed,
                   dict(format=0, threads=256, cut_rows=True))


def sparse_rows(seed=93):
    """50 000 rows, 50 of them with 40 entries each, the others empty."""
    rng = np.random.default_rng(seed)
    live = np.sort(rng.choice(50000, 50, replace=False))
    return _finish("sparse_rows", 50000, 2000, np.repeat(live, 40), rng.integers(0, 2000, 2000), seed, dict(format=0, threads=256))


def tile_stream_cut_row(seed=94):
    """The "empty_and_heavy_rows" pattern of tests/test_gpu_tts.py scaled down: a quarter of the rows empty, one row of 60 000
    entries that the tile stream cuts into pieces (carry tiles + a fix-up in the tail)."""
    rng = np.random.default_rng(seed)
    rows, cols, nnz = 3000, 400000, 120000
    r = rng.integers(0, rows, nnz)
    r[r % 4 == 0] = 31
    r[:60000] = rows - 1
    return _finish("tts_cut_row", rows, cols, r, rng.integers(0, cols, nnz), seed, dict(format=1, cut_rows=True))


# ---- case A: 256-thread parts whose group counts cover every residue mod 4 --------------------------------------------------------
def case_a():
    plain = [uniform(3000, 2500, nnz, 10 + k, dict(format=0, threads=256, group=4, window=False, groups=g))
             for k, (nnz, g) in enumerate([(0, 1), (1024, 1), (4096, 2), (9000, 3), (13000, 4), (17000, 5)])]
    windowed = [uniform(3000, 2500, 600000, 17, dict(format=0, threads=256, window=True, groups=147)),
                band(4000, 300, 18, dict(format=0, threads=256, window=True, groups=293, cut_rows=True))]
    return plain + windowed + [one_by_one(), single_row(), sparse_rows()]


# ---- case C: every item kind ------------------------------------------------------------------------------------------------------
def big_band():
    return band(20000, 200, 31, dict(format=0, threads=1024, group=16, groups=250, window=True))


def tile_stream(seed=32):
    return uniform(3000, 400000, 60000, seed, dict(format=1))


def case_c():
    a = case_a()
    return [big_band(), tile_stream(), tile_stream_cut_row(), a[3], a[5], a[6], a[7]]


# ---- tile streams whose x fits the LDS (HISPMV_TTS_XLDS=1), the small geometry, a chain of more than 32 slices --------------------------
TTS_XLDS_MAX = 16 * 1024           # kTtsXldsMax (hispmv_kernels.h): the longest x the kernels keep in the LDS
DYN_LDS_MAX = 160 * 1024 - 256     # kDynLdsMax


def tts_nv_lds_bytes(tts, cols, nv, xlds):
    """tts_nv_lds_bytes (hispmv_kernels.hip) from the packer's arrays: per vector the accumulators, a staging area of the largest
    block in whole chunks + the dummy slot, 64 tails and -- xlds -- x rounded up to 64 floats."""
    acc = (tts["max_rows"] + 63) & ~63
    stage = -(-tts["max_slots"] // 1024) * 1024 + 64
    return (acc + stage + 64 + (((cols + 63) & ~63) if xlds else 0)) * nv * 4


def x_in_lds(tts, cols, nv=1):
    """tts_x_in_lds under HISPMV_TTS_XLDS=1: a one-part stream with stream words for every row, x short enough, the LDS large enough."""
    return (not isinstance(tts, (list, tuple)) and not tts["zero_fill"] and tts["flags_hi"] is None and cols <= TTS_XLDS_MAX
            and tts_nv_lds_bytes(tts, cols, nv, True) <= DYN_LDS_MAX)


def tts_widths(tts, cols):
    """-> (from the LDS, through the cache): the most vectors (4, 2, 1; 0 = none) that share a pass over the words with x in the LDS,
    and with x gathered through the cache -- what tts_batch_width returns for a call of >= 4 vectors with and without the switch."""
    lds = next((nv for nv in (4, 2, 1) if x_in_lds(tts, cols, nv)), 0)
    cache = next((nv for nv in (4, 2) if tts_nv_lds_bytes(tts, cols, nv, False) <= DYN_LDS_MAX), 1)
    return lds, cache


def linear_passes(tts, cols, vecs, xlds_on):
    """The passes of a `linear` call of `vecs` vectors (forward_width + tts_batch_width): [(vectors, x in the LDS)]."""
    out, k = [], 0
    while k < vecs:
        left, nv, lds = vecs - k, 1, False
        if left >= 2:
            nv = next((n for n in (4, 2) if n <= left and xlds_on and x_in_lds(tts, cols, n)), 0)
            lds = nv > 0
            if not nv:
                nv = next((n for n in (4, 2) if n <= left and tts_nv_lds_bytes(tts, cols, n, False) <= DYN_LDS_MAX), 1)
            if nv < 2:
                nv, lds = min(left, 8), False                      # (one after the other inside one launch: kTtsMaxVectors)
        if nv == 1:
            lds = xlds_on and x_in_lds(tts, cols, 1)
        out.append((nv, lds))
        k += nv
    return out


def xlds_cases():
    """Uniform random columns, every column count but D's odd.  name -> matrix; expect["widths"] = tts_widths of its packed stream.
    A has 72 000 entries, not 60 000: under HISPMV_FORMAT=tts the loader keeps a matrix of fewer than 64 K entries a slice stream
    (hispmv_choose.cpp), so the smaller one never reaches a tile-stream kernel; shape, heavy row and share are unchanged."""
    return dict(
        A=uniform(2000, 2047, 72000, 301, dict(format=1, group=28, cut_rows=True, widths=(4, 4), xlds=True), heavy_row=(7, 1.0 / 3), name="xlds_A"),
        B=uniform(3000, 8191, 120000, 302, dict(format=1, group=28, widths=(2, 4), xlds=True), name="xlds_B"),
        C=uniform(3000, 16383, 120000, 303, dict(format=1, group=28, cut_rows=True, widths=(1, 4), xlds=True), heavy_row=(7, 1.0 / 3), name="xlds_C"),
        D=uniform(300, 16384, 70000, 304, dict(format=1, group=28, xlds=True), name="xlds_D"),
        E=uniform(300, 16385, 70000, 305, dict(format=1, group=28, xlds=False), name="xlds_E"))


def small_band(seed=306):
    """6 entries per row within +-100 columns of the row: 1.4 lines of x per gather, so HISPMV_TTS_SMALL=1 packs it in 13 K-slot blocks."""
    rng = np.random.default_rng(seed)
    n = 20000
    r = np.repeat(np.arange(n, dtype=np.int64), 6)
    c = np.clip(r + rng.integers(-100, 101, r.size), 0, n - 1)
    return _finish("small_band", n, n, r, c, seed, dict(format=1, group=13))


def single_row_long(seed=95):
    """One row of 40 000 entries: a chain of more than 32 slices (kFixShortMax), finished by a launch of its own behind the tail."""
    rng = np.random.default_rng(seed)
    return _finish("single_row_long", 1, 4096, np.zeros(40000, np.int64), rng.integers(0, 4096, 40000), seed,
                   dict(format=0, threads=256, cut_rows=True, long_chain=True))


def tall(m, geometry):
    """The tile stream under HISPMV_TTS_GEOMETRY=tall / tallgap: two column parts of 16 K-row tiles, part 1 through a partial vector."""
    return dict(m, name=f'{m["name"]}_{geometry}', expect=dict(format=1, group=23, parts=2, tile_kind=1, geometry=geometry))


def tall_env(geometry):
    return dict(TTS, HISPMV_TTS_GEOMETRY=geometry)


def as_slices(m, **expect):
    """The same matrix where the context's switches keep it a slice stream (HISPMV_FORMAT=tts: fewer than 64 K entries)."""
    return dict(m, expect=dict(format=0, **expect))


def bf16_exact(a):
    """fp32 values rounded to bfloat16 once (round to nearest even), kept as fp32: a bf16 handle stores exactly these."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32).reshape(np.shape(a))


def as_bf16(m):
    """The matrix with bf16-exact values, to be created under set_value_storage("bf16"): the CPU models apply unchanged."""
    key = "W" if m.get("dense") else "v"
    return dict(m, name=m["name"] + "_bf16", storage="bf16", **{key: bf16_exact(m[key])})


# ---- case D -----------------------------------------------------------------------------------------------------------------------
def stray_split_band():
    return band(20000, 200, 41, dict(format=0, tile_kind=3, parts=2), redraw=0.02)


def column_tiled(seed=42, heavy=True):
    """Eight L2-sized column parts under HISPMV_COL_TILE_BYTES=65536; a third of the entries in row 7, so that every part has
    a row cut between slices."""
    return uniform(3000, 200000, 60000, seed, dict(format=0, tile_kind=1, parts=8, threads=256, l2_tiles=True, cut_rows=True),
                   heavy_row=(7, 1.0 / 3) if heavy else None)


def two_way_band():
    return band(4000, 300, 43, dict(format=0, threads=256, window=True, compact=0, groups_mod4=1), redraw=0.01)


def stray_slot_band():
    """4.6 M entries: the smallest band probed whose resident 1024-thread plan has more than 16 slices per group (18), so that
    its compact groups keep stray slots (hispmv_plan.cpp: stray_slots_possible) under the default switches."""
    return band(22000, 210, 44, dict(format=0, threads=1024, parts=1, window=True, stray_slots=True, cut_rows=True), redraw=0.02)


def pick(ms, *names):
    by = {m["name"]: m for m in ms}
    return [by[n] for n in names]


# ---- case E -----------------------------------------------------------------------------------------------------------------------
def case_e_sparse():
    """40 matrices of 256-thread plans with different slice counts, each with a row cut over several slices."""
    return [uniform(3000, 2500, 6000 + 700 * k, 50 + k, dict(format=0, threads=256, window=False, cut_rows=True), heavy_row=(7 + k, 0.3))
            for k in range(40)]


def case_e_column_tiled():
    return [column_tiled(100 + k) for k in range(34)]


def case_e_tile_streams():
    return [tile_stream(200 + k) for k in range(33)]


def dense_shapes():
    rng = np.random.default_rng(61)
    shapes = [(64, 64), (301, 520), (17, 4099), (1, 1), (130, 1001)] + [(32 + 8 * k, 96 + 4 * k) for k in range(30)]
    out = []
    for k, (rows, cols) in enumerate(shapes):
        out.append(dict(name=f"dense_{k}_{rows}x{cols}", dense=True, rows=rows, cols=cols, W=rng.standard_normal((rows, cols), dtype=np.float32),
                        x=rng.random(cols, dtype=np.float32) - np.float32(0.3), b=rng.random(rows, dtype=np.float32)))
    return out


# ---- the plan of a matrix, from the host planner or from matrix_info of a loaded handle ----------------------------------------
def csr_of(m):
    order = np.lexsort((m["c"], m["r"]))
    rp = np.zeros(m["rows"] + 1, np.int64)
    np.add.at(rp, m["r"].astype(np.int64) + 1, 1)
    return np.cumsum(rp), m["c"][order], m["v"][order]


def host_info(m, env):
    """The loader's decision at 256 CUs under the case's switches (hispmv_prep_choose_format), under the names matrix_info uses
    for the same facts; + "l2_tiles", which only the planner tells."""
    from hispmv_amd import prep
    with environment(env):
        rp, ci, va = csr_of(m)
        ch = prep.choose_format_from_csr(rp, ci, va, m["rows"], m["cols"], 256)
    return dict(format=ch["format"], tile_kind=ch["tile_kind"], col_tiles=ch["parts"], col_tile_width=ch["tile_width"], col_tile_base=ch["tile_base"],
                block_threads=ch["threads"], group_slices=ch["group"], lds_bytes=4 * ch["lds_floats"], batch_group_slices=0, l2_tiles=ch["l2_tiles"])


def packed(m, info):
    """The streams of the matrix from the host packer, cut the way `info` says the loader cut it: the list of its slice parts
    (util.prepared_tiles), or, for a tile stream, the Prepared object whose .tts holds the packer's arrays."""
    from hispmv_amd.prep import prep_from_coo
    from util import prepared_tiles
    if info["format"] == 1:
        if info["group_slices"] == 23:                                                    # the two column parts of the tall geometries
            assert info["col_tiles"] == 2 and m["expect"]["geometry"] in ("tall", "tallgap"), info
            return prep_from_coo(m["r"], m["c"], m["v"], m["rows"], m["cols"], tts=(0, m["expect"]["geometry"]))
        assert info["col_tiles"] == 1 and info["group_slices"] in (28, 13), info          # the standard or the small geometry
        return prep_from_coo(m["r"], m["c"], m["v"], m["rows"], m["cols"], tts=(0, {28: 0, 13: 1}[info["group_slices"]]))
    return prepared_tiles(info, m["r"], m["c"], m["v"], m["rows"], m["cols"])


def groups_of(n_slices, group_slices):
    return -(-int(n_slices) // int(group_slices)) if n_slices > 0 else 0


def part_plans(info, pk, shared_chip=True):
    """Per slice part (threads, slices per group) as the call queues it: from matrix_info for a whole-matrix stream (with its batch
    layout's group length in a call that shares the chip, where it has one), from the host planner for the parts of a cut matrix
    (every part is planned on its own; part 0 must agree with what matrix_info reports)."""
    if len(pk) == 1:
        gs = info["batch_group_slices"] if (shared_chip and info["batch_group_slices"] > 0) else info["group_slices"]
        return [(info["block_threads"], gs)]
    assert (pk[0].plan["threads"], pk[0].plan["group_slices"]) == (info["block_threads"], info["group_slices"]), (info, pk[0].plan)
    return [(P.plan["threads"], P.plan["group_slices"]) for P in pk]


def queue_items(info, pk, shared_chip=True):
    """Queue items of the matrix in a step-kernel call, counted without the library: a group of a 1024-thread part is an item,
    four groups of a 256-thread part share one, a tile of a tile stream is one."""
    if info["format"] == 1:
        return sum(int(t["n_tiles"]) for t in _tts_parts(pk))
    n = 0
    for P, (threads, gs) in zip(pk, part_plans(info, pk, shared_chip)):
        assert threads in (256, 1024), (info, threads)
        g = groups_of(P.n_slices, gs)
        n += g if threads == 1024 else -(-g // 4)
    return n


def _tts_parts(pk):
    return pk.tts if isinstance(pk.tts, (list, tuple)) else [pk.tts]


def cut_rows(info, pk):
    """Per part: the number of rows the packer cut between slices (or, in a tile stream, into pieces)."""
    return [int(t["fix"].shape[0]) for t in _tts_parts(pk)] if info["format"] == 1 else [int(P.fix.shape[0]) for P in pk]


def check_expect(m, info, pk):
    """The plan the case needs (m["expect"]) against `info` (host_info, or matrix_info of the loaded handle)."""
    e, tag = m["expect"], (m["name"], info)
    assert info["format"] == e["format"], tag
    if "threads" in e:
        assert info["block_threads"] == e["threads"], tag
    if "group" in e:
        assert info["group_slices"] == e["group"], tag
    if "window" in e:
        assert (info["lds_bytes"] > 0) == e["window"], tag
    assert info["col_tiles"] == e.get("parts", 1) and info["tile_kind"] == e.get("tile_kind", 0), tag
    if e["format"] == 0:
        g0 = groups_of(pk[0].n_slices, info["group_slices"])
        if "groups" in e:
            assert g0 == e["groups"], (tag, g0)
        if "groups_mod4" in e:
            assert g0 % 4 == e["groups_mod4"], (tag, g0)
    if e.get("cut_rows"):
        assert all(n > 0 for n in cut_rows(info, pk)) if e.get("tile_kind") == 1 else sum(cut_rows(info, pk)) > 0, (tag, cut_rows(info, pk))
    if "l2_tiles" in e and "l2_tiles" in info:
        assert bool(info["l2_tiles"]) == e["l2_tiles"], tag
    if "compact" in e and "compact_slices" in info:
        assert info["compact_slices"] == e["compact"], tag
    if "widths" in e:
        assert tts_widths(pk.tts, m["cols"]) == e["widths"], (tag, tts_widths(pk.tts, m["cols"]))
    if "xlds" in e:
        assert x_in_lds(pk.tts, m["cols"]) == e["xlds"], tag
    if e.get("long_chain"):
        assert int(pk[0].fix[:, 2].max()) > 32, (tag, pk[0].fix)                          # more slices than kFixShortMax: a fix_long entry


def stray_layout(m):
    """Host-only: slices with stray slots / compact slices / all slices under the plan the loader takes for a single-part matrix."""
    from hispmv_amd import prep
    lay = prep.device_layout_from_coo(m["r"], m["c"], m["v"], m["rows"], m["cols"])
    return lay["stray_slices"], lay["compact_slices"], lay["n_slices"]


PAIRS = ((0.85, -2.06), (1.0, 0.0))               # (ALPHA, BETA) of tests/conftest.py, and beta = 0: no bias table
MORE_PAIRS = ((0.0, 1.0), (-1.5, 0.5))


def reference(m, info, pk, alpha, beta, mode=0):
    """-> (ye, y64, mag): the CPU model of the matrix's format on the packer's arrays (a batch call always uses the fix-up carry
    variant of the slice stream, mode 0; 1 = the look-back variant of a single launch) and the fp64 accumulation with the magnitude
    sum of its terms."""
    import oracle
    from util import csr_truth, emulate_tiles
    if m.get("dense"):
        W64, x64 = m["W"].astype(np.float64), m["x"].astype(np.float64)
        return (oracle.emu_gemv(m["W"], m["x"], m["b"], alpha, beta), alpha * (W64 @ x64) + beta * m["b"].astype(np.float64),
                abs(alpha) * (np.abs(W64) @ np.abs(x64)) + np.abs(beta * m["b"].astype(np.float64)))
    if info["format"] == 1:
        ye = oracle.emu_tts(pk.tts, m["x"], m["b"], alpha, beta, m["rows"])
    else:
        ye = emulate_tiles(pk, m["x"], m["b"], alpha, beta, m["rows"], mode)
    y64, mag = csr_truth(m["r"], m["c"], m["v"], m["rows"], m["x"], m["b"], alpha, beta)
    return ye, y64, mag
