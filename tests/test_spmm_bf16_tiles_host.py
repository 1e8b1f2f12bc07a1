"""The tile rule of the wide-batch product with bf16 activations (hispmv_prep_spmm_bf16_tiles; hispmv_spmm.h), host-only.

Every tile takes the largest VB in {8, 4, 2} with (a) 64 * (VB / 2) < vectors left, (b) cols * 64 * VB * 2 <= 8 MiB, (c) ld % VB == 0 and
align_bytes % (2 * VB) == 0, otherwise VB 1; a tile is 64 * VB vectors.  The library's answer is compared with the restatement below
over a grid of (cols, B, ld, align) that holds the edges of all three conditions.  The fp32 rule (prep.spmm_tiles) must answer what it
answered before the bf16 entries existed: it is restated here as well."""
import ctypes as C

import pytest

from hispmv_amd import _lib, prep

TILE_BYTES = 8 << 20


def rule(cols, B, ld, align, widths, elem):
    """-> (lanes' width of the first tile, tiles, vectors in the last tile, width of the last tile)"""
    first = last = None
    tiles, k, n = 0, 0, 0
    while k < B:
        left, w = B - k, 1
        for cand in widths:
            if 64 * (cand // 2) < left and cols * 64 * cand * elem <= TILE_BYTES and ld % cand == 0 and align % (elem * cand) == 0:
                w = cand
                break
        n = min(left, 64 * w)
        first = w if first is None else first
        last = w
        tiles += 1
        k += n
    return first, tiles, n, last


BATCHES = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1024, 1100)
COLS = (1, 1000, 8192, 8193, 16384, 16385, 32768, 32769)


def lds(B):
    return sorted({B, (B + 7) & ~7, (B + 3) & ~3, (B + 1) & ~1, B + 3, ((B + 7) & ~7) + 8, 2 * B + 1})


@pytest.mark.parametrize("cols", COLS)
def test_the_rule_over_the_grid(cols):
    for B in BATCHES:
        for ld in lds(B):
            for align in (2, 4, 6, 8, 16, 32, 48):
                got = prep.spmm_bf16_tiles(cols, B, ld, align)
                want = rule(cols, B, ld, align, (8, 4, 2), 2)
                assert (got["vb"], got["tiles"], got["last_vecs"], got["vb_last"]) == want, (cols, B, ld, align, got, want)


def test_the_edges_by_hand():
    t = prep.spmm_bf16_tiles
    # (a): a width is taken only past half of its tile
    assert [t(1000, B, (B + 7) & ~7)["vb"] for B in (1, 64, 65, 128, 129, 256, 257, 512, 513)] == [1, 1, 2, 2, 4, 4, 8, 8, 8]
    assert t(1000, 513, 520) == dict(vb=8, tiles=2, last_vecs=1, vb_last=1)
    assert t(1000, 512, 512) == dict(vb=8, tiles=1, last_vecs=512, vb_last=8)
    assert t(1000, 257, 264) == dict(vb=8, tiles=1, last_vecs=257, vb_last=8)
    assert t(1000, 1100, 1104) == dict(vb=8, tiles=3, last_vecs=76, vb_last=2)
    # (b): VB 8 up to 8192 columns, VB 4 up to 16384, VB 2 up to 32768
    assert [t(c, 513, 520)["vb"] for c in (8192, 8193, 16384, 16385, 32768, 32769)] == [8, 4, 4, 2, 2, 1]
    # (c): an odd ld and 2-byte alignment give VB 1; ld % 8 and the alignment cap the width
    assert t(1000, 513, 521)["vb"] == 1 and t(1000, 65, 68, 2) == dict(vb=1, tiles=2, last_vecs=1, vb_last=1)
    assert t(1000, 513, 516)["vb"] == 4 and t(1000, 513, 514)["vb"] == 2
    assert [t(1000, 513, 520, a)["vb"] for a in (2, 4, 8, 16)] == [1, 2, 4, 8]
    assert t(1000, 7)["vb"] == 1 and t(1000, 520)["vb"] == 8          # ld defaults to num_vecs


@pytest.mark.parametrize("cols", COLS)
def test_the_fp32_rule_is_unchanged(cols):
    for B in BATCHES:
        for ld in lds(B):
            for align in (4, 8, 12, 16, 32):
                got = prep.spmm_tiles(cols, B, ld, align)
                want = rule(cols, B, ld, align, (4, 2), 4)
                assert (got["vl"], got["tiles"], got["last_vecs"], got["vl_last"]) == want, (cols, B, ld, align, got, want)
    assert prep.spmm_tiles(1000, 65, 68, 4) == dict(vl=1, tiles=2, last_vecs=1, vl_last=1)
    assert prep.spmm_tiles(1000, 257, 260, 16) == dict(vl=4, tiles=2, last_vecs=1, vl_last=1)


@pytest.mark.parametrize("entry", ["hispmv_prep_spmm_bf16_tiles", "hispmv_prep_spmm_tiles"])
def test_bad_arguments(entry):
    f = getattr(_lib.lib, entry)
    out = (C.c_int64 * 4)()
    assert f(1000, 8, 8, 16, out) == _lib.HISPMV_OK
    for args in ((0, 8, 8, 16), (1000, 0, 8, 16), (1000, 8, 0, 16), (1000, 8, 8, 0), (1000, 8, 7, 16), (-1, 8, 8, 16)):
        assert f(*args, out) == _lib.HISPMV_EINVAL, args
    assert f(1000, 8, 8, 16, None) == _lib.HISPMV_EINVAL
    for wrapper in (prep.spmm_bf16_tiles, prep.spmm_tiles):
        with pytest.raises(ValueError):
            wrapper(1000, 8, 7)


def test_the_new_symbols_are_declared():
    for name in ("hispmv_spmm_device_bf16", "hispmv_spmm_device_t_bf16", "hispmv_spmm_bf16_info", "hispmv_prep_spmm_bf16_tiles"):
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.lib, name), name
    assert _lib.SIGNATURES["hispmv_spmm_device_bf16"] == _lib.SIGNATURES["hispmv_spmm_device"]
    assert _lib.SIGNATURES["hispmv_spmm_device_t_bf16"] == _lib.SIGNATURES["hispmv_spmm_device_t"]
    assert _lib.SIGNATURES["hispmv_spmm_bf16_info"] == _lib.SIGNATURES["hispmv_spmm_info"]
