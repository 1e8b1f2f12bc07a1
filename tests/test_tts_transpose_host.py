"""Host side of the transposed product and the value gradient on tile streams (hispmv_tts_transpose.hip), no GPU: a NumPy model of
the kernel's two phases -- EXPAND (row-major: row(slot) = chunk_info.x + the row ends at earlier slots of the chunk, staging[slot] =
x[row(slot)]) and SCATTER (column order: a word whose value is not +-0 adds value * staging[slot] to y[col_base + col_off]) -- run on
the arrays of the host packer for the inputs tests/test_gpu_tts_transpose.py uses.  It pins what the kernel relies on:
  * every slot below n_slots maps to a row inside its tile,
  * every non-zero word has slot < n_slots and col < cols,
  * the row of a carry tile is found through `fix`,
and that the model reproduces the fp64 scatter.  The same walk with the values replaced by index payloads (the bits of k + 1, as an
updatable handle is packed) finds every input entry exactly once, at its own row and column: the addressing of the value gradient.

The model sums in fp64 in another order than np.bincount: n terms differ by at most n * 2^-53 * sum |terms|, far below the 1e-10 *
magnitude asserted here."""
import numpy as np
import pytest

import step_small_cases as S
from tts_transpose_cases import CASES, case


def cases():
    """(matrix, environment, packer geometry, pass width) of every case of tests/tts_transpose_cases.py."""
    return [case(name) for name in CASES]


def pack(m, geometry, values=None):
    from hispmv_amd.prep import prep_from_coo
    return prep_from_coo(m["r"], m["c"], m["v"] if values is None else values, m["rows"], m["cols"], tts=(0, geometry)).tts


def walk(tts, rows, cols):
    """The kernel's walk over a packed stream -> per stored non-zero word (value bits, row, col), tile by tile, with the invariants
    asserted on the way; + counts of what it met."""
    vals, meta = tts["words"][:, 0, :], tts["words"][:, 1, :]
    lane = np.arange(64)
    out_bits, out_row, out_col = [], [], []
    seen = dict(tiles=0, carry_tiles=0, max_blocks=0, fillers=0, cut_rows=0)
    for row0, n_rows, block_begin, n_blocks in tts["tiles"]:
        seen["tiles"] += 1
        seen["max_blocks"] = max(seen["max_blocks"], int(n_blocks))
        if row0 < 0:                                   # a piece of a long row: its row is the fix entry whose carry range holds it
            ci = -int(row0) - 1
            hit = [f for f in tts["fix"] if f[1] <= ci < f[1] + f[2]]
            assert len(hit) == 1 and n_rows == 1, (row0, n_rows, hit)
            row = int(hit[0][0])
            seen["carry_tiles"] += 1
        else:
            row = int(row0)
        assert 0 <= row and row + n_rows <= rows
        for b in range(block_begin, block_begin + n_blocks):
            slice_begin, n_slices, chunk_begin, n_chunks, n_slots = (int(q) for q in tts["blocks"][b][:5])
            assert (n_chunks - 1) * 1024 < n_slots <= n_chunks * 1024 <= tts["max_slots"] + 1023
            fl = tts["flags"][chunk_begin:chunk_begin + n_chunks].astype(np.int64)
            ends = np.zeros((n_chunks, 1024), np.int64)
            for j in range(4):
                for k in range(4):
                    ends[:, 256 * j + 4 * lane + k] = (fl >> (4 * j + k)) & 1
            before = np.cumsum(ends, axis=1) - ends                                  # row ends at earlier slots of the chunk
            row_of = (tts["chunk_info"][chunk_begin:chunk_begin + n_chunks, 0].astype(np.int64)[:, None] + before).ravel()
            assert row_of[:n_slots].min() >= 0 and row_of[:n_slots].max() < n_rows, (b, n_rows)
            assert ends.ravel()[n_slots:].sum() == 0 and ends.sum() == n_rows           # every row of the tile ends once in every block
            v = vals[slice_begin:slice_begin + n_slices].ravel()
            m = meta[slice_begin:slice_begin + n_slices].ravel().astype(np.int64)
            col = np.repeat(tts["col_base"][slice_begin:slice_begin + n_slices].astype(np.int64), 1024) + (m >> 16)
            slot = m & 0xFFFF
            nz = (v & 0x7FFFFFFF) != 0
            assert (slot[nz] < n_slots).all() and (col[nz] < cols).all() and (col[nz] >= 0).all()
            seen["fillers"] += int(((slot < n_slots) & ~nz).sum())
            out_bits.append(v[nz])
            out_row.append(row + row_of[slot[nz]])
            out_col.append(col[nz])
    seen["cut_rows"] = len(tts["fix"])
    return np.concatenate(out_bits), np.concatenate(out_row), np.concatenate(out_col), seen


@pytest.fixture(scope="module")
def walked():
    out = {}
    for m, env, geometry, width in cases():
        info = S.host_info(m, env)
        assert info["format"] == 1 and info["group_slices"] == (13 if geometry else 28) and info["col_tiles"] == 1, (m["name"], info)
        tts = pack(m, geometry)
        assert not tts["zero_fill"] and tts["flags_hi"] is None
        assert S.tts_widths(tts, m["cols"])[1] == width, (m["name"], S.tts_widths(tts, m["cols"]))
        out[m["name"]] = (m, tts, walk(tts, m["rows"], m["cols"]))
    return out


def test_the_model_reproduces_the_fp64_scatter(walked):
    for name, (m, tts, (bits, row, col, seen)) in walked.items():
        rng = np.random.default_rng(5)
        x = rng.random(m["rows"]) - 0.3
        t = bits.view(np.float32).astype(np.float64) * x[row]
        y = np.bincount(col, weights=t, minlength=m["cols"])
        t0 = m["v"].astype(np.float64) * x[m["r"]]
        y64 = np.bincount(m["c"], weights=t0, minlength=m["cols"])
        mag = np.bincount(m["c"], weights=np.abs(t0), minlength=m["cols"])
        assert bits.size == np.count_nonzero(m["v"]), name
        assert (np.abs(y - y64) <= 1e-10 * mag).all(), name
        print(name, seen, "widths", S.tts_widths(tts, m["cols"]))


def test_the_cases_reach_what_they_are_there_for(walked):
    """One block per tile and rows cut by chunk boundaries; carry tiles; two blocks per tile with fillers; the three pass widths."""
    seen = {name: w[2][3] for name, w in walked.items()}
    assert seen["uniform_3000x400000_60000_s32"]["max_blocks"] == 1 and seen["uniform_3000x400000_60000_s32"]["carry_tiles"] == 0
    assert seen["tts_cut_row"]["carry_tiles"] >= 2 and seen["tts_cut_row"]["fillers"] > 0
    assert seen["xlds_A"]["carry_tiles"] >= 1
    assert seen["two_blocks_3000"]["max_blocks"] >= 2
    assert seen["two_blocks_20000"]["max_blocks"] >= 2 and seen["two_blocks_20000"]["fillers"] > 0
    assert sorted({c[3] for c in CASES.values()}) == [1, 2, 4]
    assert walked["small_band"][1]["max_slots"] <= 13 * 1024


def test_index_payloads_name_every_entry_once_at_its_row_and_column():
    """An updatable handle is packed from the bits of k + 1 in place of the values: the walk then meets every input entry exactly once,
    at (r[k], c[k]) -- what the gradient kernel stores grad[k] from.  Duplicates of the input are entries of their own."""
    for m, env, geometry, width in cases()[:5]:
        n = m["v"].size
        payload = np.arange(1, n + 1, dtype=np.uint32).view(np.float32)
        bits, row, col, _ = walk(pack(m, geometry, payload), m["rows"], m["cols"])
        k = bits.astype(np.int64) - 1
        assert k.size == n and np.array_equal(np.sort(k), np.arange(n)), m["name"]
        assert np.array_equal(row, m["r"][k]) and np.array_equal(col, m["c"][k]), m["name"]


def test_constants_of_the_switch():
    from hispmv_amd import _lib
    assert (_lib.HISPMV_TRANSPOSABLE_OFF, _lib.HISPMV_TRANSPOSABLE_SLICES, _lib.HISPMV_TRANSPOSABLE_KEEP_FORMAT) == (0, 1, 2)
    assert _lib.lib.hispmv_set_transposable(None, 2) == _lib.HISPMV_EINVAL
