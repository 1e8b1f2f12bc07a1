"""The stored transpose (hispmv_set_transposable state HISPMV_TRANSPOSABLE_COMPANION) as far as a box without a GPU can see it: the
new entry is exported, the Python spellings of the state, and the expansion of a CSR input to the swapped COO in input order from
which hispmv_create_sparse_handle_from_csr makes the companion."""
import ctypes as C

import numpy as np
import pytest


def test_library_exports_the_companion_entries():
    from hispmv_amd import _lib
    raw = C.CDLL(str(_lib.LIB_PATH))
    assert hasattr(raw, "hispmv_companion_info")
    assert hasattr(raw, "hispmv_prep_swapped_coo_from_csr")
    assert _lib.HISPMV_TRANSPOSABLE_COMPANION == 3
    out = (C.c_int64 * 6)(*([7] * 6))
    assert _lib.lib.hispmv_companion_info(None, 0, out) == _lib.HISPMV_EINVAL      # no context: refused, nothing written
    assert list(out) == [7] * 6


def test_set_transposable_spellings():
    from hispmv_amd import _lib
    from hispmv_amd.fpga_handle import FpgaHandle
    import pyhispmv
    assert pyhispmv.FpgaHandle is FpgaHandle or issubclass(pyhispmv.FpgaHandle, FpgaHandle)
    state = FpgaHandle.transposable_state
    assert state("companion") == 3 == _lib.HISPMV_TRANSPOSABLE_COMPANION
    assert state("keep_format") == 2
    assert [state(e) for e in (False, True, 0, 1, 2)] == [0, 1, 0, 1, 2]
    # other strings are refused; so is the bare integer 3, which Python callers spell "companion" (the C ABI takes the constant)
    for bad in ("Companion", "stored", "", "3", 3):
        with pytest.raises(ValueError, match="companion"):
            state(bad)


def test_csr_expands_to_the_swapped_coo_in_input_order():
    """5 x 4: row 1 empty, row 2 with unsorted columns, row 3 with a duplicated entry.  Entry k of the swapped COO is
    (col_idx[k], row of k) for k ascending: the expansion happens before any per-row sort and merges nothing."""
    from hispmv_amd import _lib
    row_ptr = np.array([0, 2, 2, 5, 8, 9], np.int32)
    col_idx = np.array([0, 3,   3, 0, 1,   2, 2, 0,   1], np.int32)
    row_of = np.array([0, 0,   2, 2, 2,   3, 3, 3,   4], np.int32)
    out_r = np.full(9, -1, np.int32)
    out_c = np.full(9, -1, np.int32)
    rc = _lib.lib.hispmv_prep_swapped_coo_from_csr(row_ptr.ctypes.data, col_idx.ctypes.data, 5, out_r.ctypes.data, out_c.ctypes.data)
    assert rc == _lib.HISPMV_OK
    assert out_r.tolist() == col_idx.tolist()
    assert out_c.tolist() == row_of.tolist()
    # row_ptr that does not start at 0, or decreases: refused, nothing written
    out_r[:] = -1
    for bad in (np.array([1, 2, 2, 5, 8, 9], np.int32), np.array([0, 2, 1, 5, 8, 9], np.int32)):
        assert _lib.lib.hispmv_prep_swapped_coo_from_csr(bad.ctypes.data, col_idx.ctypes.data, 5, out_r.ctypes.data, out_c.ctypes.data) == _lib.HISPMV_EINVAL
    assert (out_r == -1).all()
