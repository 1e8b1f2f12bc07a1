"""Shared helpers for the tests (no product code)."""
from __future__ import annotations

import numpy as np

import oracle


class MT19937:
    """std::mt19937 (32-bit Mersenne Twister, init_genrand seeding) -- needed to regenerate the
    input sequence of KAT-0, which is defined in terms of it."""

    def __init__(self, seed: int):
        self.mt = [0] * 624
        self.mt[0] = seed & 0xFFFFFFFF
        for i in range(1, 624):
            self.mt[i] = (1812433253 * (self.mt[i - 1] ^ (self.mt[i - 1] >> 30)) + i) & 0xFFFFFFFF
        self.idx = 624

    def __call__(self) -> int:
        if self.idx >= 624:
            mt = self.mt
            for i in range(624):
                y = (mt[i] & 0x80000000) | (mt[(i + 1) % 624] & 0x7FFFFFFF)
                mt[i] = mt[(i + 397) % 624] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)
            self.idx = 0
        y = self.mt[self.idx]
        self.idx += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9D2C5680
        y ^= (y << 15) & 0xEFC60000
        y ^= y >> 18
        return y & 0xFFFFFFFF


def kat0_coo():
    """KAT-0 input: rows=1000, cols=900, 20 000 entries, every ~10th in row 7."""
    g = MT19937(1)
    rows, cols = 1000, 900
    r, c, v = [], [], []
    for _ in range(20000):
        rr = 7 if g() % 10 == 0 else g() % rows
        r.append(rr)
        c.append(g() % cols)
        v.append(np.float32(g() % 1000) / np.float32(1000.0) + np.float32(0.001))
    return rows, cols, np.array(r, np.int32), np.array(c, np.int32), np.array(v, np.float32)


def bwd_err(y, y64, mag):
    """max_i |y_i - y64_i| / (|alpha| sum_j |a_ij x_j| + |beta b_i|): the backward-error form of the
    1e-5 gate (BASELINE.json north_star; SURVEY.md section 7, hard part 1)."""
    mag = np.maximum(mag, np.finfo(np.float64).tiny)
    return float(np.max(np.abs(np.asarray(y, np.float64) - y64) / mag))


def prepared_tiles(info, r, c, v, rows, cols):
    """The slice streams of the handle's column tiles, packed on the host the way the loader packs them."""
    from hispmv_amd.prep import prep_from_coo
    r, c, v = np.asarray(r), np.asarray(c), np.asarray(v, np.float32)
    if info["col_tiles"] <= 1:
        return [prep_from_coo(r, c, v, rows, cols)]
    if info.get("tile_kind") == 3:
        # stray split: part 0 = the entries inside the x window of their workgroup (under the plan of the WHOLE matrix), part 1 the rest
        from hispmv_amd.prep import window_membership
        inside, order = window_membership(r, c, v, rows, cols, 256)
        keep = np.zeros(r.size, dtype=bool)
        keep[order] = inside.astype(bool)
        return [prep_from_coo(r[keep], c[keep], v[keep], rows, cols), prep_from_coo(r[~keep], c[~keep], v[~keep], rows, cols)]
    width, base, n = info["col_tile_width"], info["col_tile_base"], info["col_tiles"]
    # tile_kind 2 (band tiles): base / width are ranges of the OFFSET from the scaled diagonal, col - row*cols/rows
    key = c.astype(np.int64) - (r.astype(np.int64) * cols // rows) if info.get("tile_kind") == 2 else c.astype(np.int64)
    tiles = []
    for t in range(n):                                     # the end tiles are open-ended (hispmv.h: col_tile_base)
        lo = -(1 << 40) if t == 0 else base + t * width
        hi = (1 << 40) if t == n - 1 else base + (t + 1) * width
        sel = (key >= lo) & (key < hi)
        tiles.append(prep_from_coo(r[sel], c[sel], v[sel], rows, cols))
    return tiles


def emulate_tiles(tiles, x, b, alpha, beta, rows, mode):
    """Tile 0 computes alpha*A_0*x + beta*bias; every further column tile computes alpha*A_t*x into a partial vector
    (its own cut rows fixed up there), and the merge pass adds the partial vectors to y in tile order."""
    ye = None
    for t, P in enumerate(tiles):
        if t == 0:
            ye = oracle.emu_spmv(P.words, P.hdr, P.fix, x, b, alpha, beta, rows, mode)
        else:
            ye = (ye + oracle.emu_spmv(P.words, P.hdr, P.fix, x, np.zeros(rows, np.float32), alpha, 0.0, rows, mode)).astype(np.float32)
    return ye


def emulate_device(info, r, c, v, rows, cols, x, b, alpha, beta, carry=None):
    """The wavefront model applied the way the device runs the handle: one stream per column tile (tile 0
    with beta*bias, later tiles into partial vectors added afterwards), carry variant as reported by matrix_info (or `carry`:
    a batched pass always uses the fix-up variant, 0)."""
    return emulate_tiles(prepared_tiles(info, r, c, v, rows, cols), x, b, alpha, beta, rows,
                         info["carry_lookback"] if carry is None else carry)


def csr_truth(r, c, v, rows, x, b, alpha, beta):
    order = np.lexsort((c, r))
    rp = np.zeros(rows + 1, np.int64)
    np.add.at(rp, np.asarray(r, np.int64) + 1, 1)
    rp = np.cumsum(rp).astype(np.int32)
    return oracle.spmv_f64(rp, np.asarray(c, np.int32)[order], np.asarray(v, np.float32)[order], x, b, alpha, beta)
