"""The transposed product (include/hispmv.h: hispmv_spmv_device_t) without a GPU: the argument checks of its three entries, the
Python surface, and a numpy DECODER of the host-packed device layout -- the (row, column, value) triplet of every non-zero slot,
rebuilt the way hispmv_transpose.hip rebuilds it: the row of an element is its slice's row_base plus the row ends before it, its
column is the meta (a plain column, a window index mapped back through the group's fragment table, or a stray slot looked up in the
slice's stray columns).  The triplets must be the input as a multiset.  This passes on the layouts as they were before the
transposed kernels existed: it pins the decoding they rely on."""
import ctypes as C

import numpy as np
import pytest

import step_small_cases as S

ROW_END, GLOBAL_COL = 0x80000000, 0x40000000
SLICE_UNIT, STRAY_SLOTS = 2048, 64


def test_entries_refuse_a_null_context():
    from hispmv_amd import _lib
    lib = _lib.lib
    out = (C.c_int64 * 4)()
    assert lib.hispmv_spmv_device_t(None, 0, None, None, None, 1.0, 0.0, None) == _lib.HISPMV_EINVAL
    assert lib.hispmv_set_transposable(None, 1) == _lib.HISPMV_EINVAL
    assert lib.hispmv_transpose_info(None, 0, out) == _lib.HISPMV_EINVAL
    assert _lib.HISPMV_ENOTSUP == -8


def test_python_surface():
    from hispmv_amd.fpga_handle import FpgaHandle
    for name in ("set_transposable", "spmv_device_t", "transpose_info"):
        assert callable(getattr(FpgaHandle, name)), name


def decode_layout(lay, hdr):
    """-> (rows, cols, value bits) of every non-zero slot of a layout of hispmv_amd.prep.device_layout_from_coo; hdr = the slice
    headers of the same stream (row_base in column 0)."""
    n, G, win = lay["n_slices"], lay["group_slices"], lay["window_floats"]
    raw, frags = lay["bytes"], lay["frags"]
    rr, cc, vv = [], [], []
    kinds = set()
    for g, (fb, fc, off, gw) in enumerate(lay["dgroups"]):
        s0, s1 = g * G, min(n, (g + 1) * G)
        half, compact, strays = bool(gw & 4), bool(gw & 1), bool(gw & 2)
        nbytes = 4096 if half else 6144 if compact else 8192
        fr = frags[fb:fb + fc]
        for sl in range(s0, s1):
            b = raw[off * SLICE_UNIT + (sl - s0) * nbytes:][:nbytes]
            if half:
                q = b.view(np.uint16).reshape(256, 8)
                vals = (q[:, :4].astype(np.uint32) << 16).reshape(-1)
                meta = q[:, 4:].reshape(-1).astype(np.uint32)
            else:
                vals = b[:4096].view(np.uint32)
                meta = b[4096:].view(np.uint16).astype(np.uint32) if compact else b[4096:].view(np.uint32)
            end = (meta >> (15 if compact else 31)) & 1
            row = hdr[sl, 0] + np.cumsum(end) - end                   # row ends BEFORE the element
            idx = meta & (0x7FFF if compact else 0x7FFFFFFF)
            col = np.full(1024, -1, np.int64)
            if win > 0 and fc > 0:
                if compact:
                    stray = idx >= win
                    assert strays or not stray.any()
                    if stray.any():
                        sc = lay["stray_cols"][sl][(idx[stray] - win) & (STRAY_SLOTS - 1)]
                        live = (vals[stray] & 0x7FFFFFFF) != 0
                        assert (sc[live] != 0xFFFFFFFF).all()
                        col[stray] = sc
                        kinds.add("stray")
                    inwin = ~stray
                    kinds.add("half" if half else "compact")
                else:
                    outside = (idx & GLOBAL_COL) != 0
                    col[outside] = idx[outside] & ~np.uint32(GLOBAL_COL)
                    inwin = ~outside
                    kinds.add("wide+window")
                    if outside.any():
                        kinds.add("wide+L2")
                f = np.searchsorted(fr[:, 2], idx[inwin], side="right") - 1
                assert (f >= 0).all() and (idx[inwin] - fr[f, 2] < fr[f, 1]).all()
                col[inwin] = fr[f, 0] + (idx[inwin] - fr[f, 2])
            else:
                assert not compact
                col[:] = idx & ~np.uint32(GLOBAL_COL)
                kinds.add("no window")
            live = (vals & 0x7FFFFFFF) != 0
            rr.append(row[live])
            cc.append(col[live])
            vv.append(vals[live])
    return np.concatenate(rr), np.concatenate(cc), np.concatenate(vv), kinds


def _multiset(r, c, vbits):
    a = np.stack([np.asarray(r, np.int64), np.asarray(c, np.int64), np.asarray(vbits, np.int64)], axis=1)
    return a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]


@pytest.mark.parametrize("case", ["compact", "wide_with_window", "stray_slots", "half"])
def test_decoder_rebuilds_the_input_triplets(case):
    from hispmv_amd import prep
    m, storage = {"compact": (lambda: S.case_a()[7], "fp32"), "wide_with_window": (S.two_way_band, "fp32"),
                  "stray_slots": (S.stray_slot_band, "fp32"), "half": (lambda: S.as_bf16(S.big_band()), "bf16")}[case]
    m = m()
    with S.environment(S.SLICES):
        lay = prep.device_layout_from_coo(m["r"], m["c"], m["v"], m["rows"], m["cols"], value_storage=storage)
        hdr = prep.prep_from_coo(m["r"], m["c"], m["v"], m["rows"], m["cols"], value_storage=storage).hdr
    assert lay["n_slices"] == hdr.shape[0]
    r, c, vb, kinds = decode_layout(lay, hdr)
    want = {"compact": {"compact"}, "wide_with_window": {"wide+window", "wide+L2"}, "stray_slots": {"compact", "stray"}, "half": {"half"}}[case]
    assert want <= kinds, kinds
    assert (c >= 0).all() and (c < m["cols"]).all() and (r >= 0).all() and (r < m["rows"]).all()
    vin = np.ascontiguousarray(m["v"], np.float32).view(np.uint32)
    live = (vin & 0x7FFFFFFF) != 0
    assert np.array_equal(_multiset(r, c, vb), _multiset(m["r"][live], m["c"][live], vin[live]))
