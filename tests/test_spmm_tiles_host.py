"""The vector tiles of the wide-batch product (hispmv_prep_spmm_tiles; hispmv_spmm.h: spmm_tiles), host-only.  A lane owns VL in
{4, 2, 1} consecutive vectors, a tile is 64 * VL vectors, and every tile takes the largest VL such that (a) 64 * (VL / 2) < vectors
left, (b) cols * 64 * VL * 4 <= kSpmmTileBytes, (c) ld % VL == 0 and align_bytes % (4 * VL) == 0.

kSpmmTileBytes is 8 MiB, so (b) caps the columns: VL 4 up to 8192, VL 2 up to 16384, VL 1 above.  The table pins, at 2048 columns,
what (a) and (c) decide (the batch, the leading dimension, the alignment); at B = 256, the cap from both sides -- 4096 and 8192
columns take VL 4 in one tile, 16384 VL 2 in two, 32768 VL 1 in four."""
import ctypes as C

import pytest

from hispmv_amd import _lib, prep

# cols, B, ld, align -> (VL of the first tile, tiles, vectors in the last tile, VL of the last tile)
CASES = [
    (2048, 1, 1, 16, (1, 1, 1, 1)),
    (2048, 64, 64, 16, (1, 1, 64, 1)),
    (2048, 65, 68, 16, (2, 1, 65, 2)),
    (2048, 200, 200, 16, (4, 1, 200, 4)),
    (2048, 257, 260, 16, (4, 2, 1, 1)),          # VL 4, then a last tile of 1 vector with VL 1
    (32768, 256, 256, 16, (1, 4, 64, 1)),        # 32768 * 64 * 2 * 4 = 16 MiB: not even VL 2
    (16384, 256, 256, 16, (2, 2, 128, 2)),       # 16384 * 64 * 2 * 4 = 8 MiB fits, VL 4 would be 16 MiB
    (8192, 256, 256, 16, (4, 1, 256, 4)),        # 8192 * 64 * 4 * 4 = 8 MiB: the widest matrix that takes VL 4
    (4096, 256, 256, 16, (4, 1, 256, 4)),
    (2048, 256, 258, 16, (2, 2, 128, 2)),        # ld % 4 != 0
    (2048, 256, 256, 4, (1, 4, 64, 1)),          # pointers aligned to 4 bytes only
]


@pytest.mark.parametrize("cols,B,ld,align,expected", CASES, ids=[f"{c[0]}x{c[1]}_ld{c[2]}_a{c[3]}" for c in CASES])
def test_tile_rule(cols, B, ld, align, expected):
    t = prep.spmm_tiles(cols, B, ld, align)
    assert (t["vl"], t["tiles"], t["last_vecs"], t["vl_last"]) == expected, t


def test_the_tiles_cover_the_batch_and_only_the_last_differs():
    """For every batch up to 600 on four column counts (below, at and twice the cap of VL 4, and past the cap of VL 2): full tiles of the first VL, then one last tile, together B vectors; 8-byte
    alignment allows VL 2 at the most."""
    for cols in (100, 8192, 16384, 40000):
        for B in range(1, 601):
            ld = (B + 3) & ~3
            t = prep.spmm_tiles(cols, B, ld, 16)
            assert (t["tiles"] - 1) * 64 * t["vl"] + t["last_vecs"] == B, (cols, B, t)
            assert 1 <= t["last_vecs"] <= 64 * t["vl_last"] and t["vl_last"] <= t["vl"], (cols, B, t)
            assert cols * 64 * t["vl"] * 4 <= 8 << 20 or t["vl"] == 1, (cols, B, t)
            assert prep.spmm_tiles(cols, B, ld, 8)["vl"] <= 2


def test_arguments_below_one_are_refused():
    out = (C.c_int64 * 4)(7, 7, 7, 7)
    for args in ((0, 1, 1, 16), (1, 0, 1, 16), (1, 1, 0, 16), (1, 1, 1, 0), (-5, 8, 8, 16), (8, 8, 4, 16)):
        assert _lib.lib.hispmv_prep_spmm_tiles(*args, out) == _lib.HISPMV_EINVAL, args
        with pytest.raises(ValueError):
            prep.spmm_tiles(*args)
    assert list(out) == [7, 7, 7, 7]
    assert _lib.lib.hispmv_prep_spmm_tiles(8, 8, 8, 16, None) == _lib.HISPMV_EINVAL


def test_entry_points_check_their_arguments_before_touching_the_device():
    lib = _lib.lib
    out = (C.c_int64 * 8)()
    assert lib.hispmv_spmm_device(None, 0, None, 1, 1, None, 0, None, 1, 1.0, 0.0, None, 0, None) == _lib.HISPMV_EINVAL
    assert lib.hispmv_spmm_device_t(None, 0, None, 1, 1, None, 0, None, 1, 1.0, 0.0, None, 0, None) == _lib.HISPMV_EINVAL
    assert lib.hispmv_spmm_info(None, 0, 1, 1, out) == _lib.HISPMV_EINVAL
