"""The widths of the multi-vector passes of hispmv_linear_device / hispmv_linear_device_t, from the host (hispmv_prep_vector_widths: no
device), and the argument checks both entries make before any device call.

A pass of NV vectors keeps NV windows in the LDS: NV is the largest of {4, 2} with (NV * window + wavefronts * row tile) * 4 bytes
<= 160 KiB - 256.  The two W-matrices below (4000 rows x 200 entries, the columns of row i drawn from [i, i + W)) get, at 32 CUs under
HISPMV_FORMAT=slices, the 1024-thread plan with 16 row tiles of 64 floats and a window of
  W = 12000: 12128 floats -> 2 x 12128 + 1024 = 25280 floats (101 120 B) fit, 4 x 12128 + 1024 (198 144 B) do not: width 2;
  W = 26000: 26144 floats -> 2 x 26144 + 1024 (213 248 B) do not fit: width 1.
(The window is the widest group's span of columns in whole 64-byte blocks, W + the group's ~128 rows: the last block depends on the draw.)
tests/test_gpu_linear_device.py loads the same two under HISPMV_PLAN_CUS=32."""
import ctypes as C

import numpy as np
import pytest

import step_small_cases as S
from hispmv_amd import _lib, prep
from hispmv_amd._lib import lib

N_CUS = 32


def w_matrix(W, seed=7):
    """4000 rows x 200 entries per row, the columns of row i uniform in [i, i + W)."""
    rng = np.random.default_rng(seed + W)
    rows, per = 4000, 200
    r = np.repeat(np.arange(rows, dtype=np.int64), per)
    c = r + rng.integers(0, W, r.size)
    return S._finish(f"w_{W}", rows, rows + W, r, c, seed, dict(format=0, threads=1024, window=True))


def plan_at(m, n_cus):
    with S.environment(S.SLICES):
        rp, ci, va = S.csr_of(m)
        return prep.choose_format_from_csr(rp, ci, va, m["rows"], m["cols"], n_cus)


def widths(m, n_cus, vecs):
    with S.environment(S.SLICES):
        return prep.vector_widths_from_coo(m["r"], m["c"], m["v"], m["rows"], m["cols"], n_cus, vecs)


@pytest.mark.parametrize("W, window, width", [(12000, 12128, 2), (26000, 26144, 1)])
def test_wide_windows_narrow_the_pass(W, window, width):
    m = w_matrix(W)
    ch = plan_at(m, N_CUS)
    assert (ch["format"], ch["parts"], ch["threads"], ch["lds_floats"]) == (0, 1, 1024, window), ch
    for vecs in (4, 9):
        assert widths(m, N_CUS, vecs) == dict(forward=width, transposed=width), vecs
    assert widths(m, N_CUS, 1) == dict(forward=1, transposed=1)


def test_small_window_and_no_window_take_four():
    a = S.case_a()
    band = a[7]                                    # band_4000x300: 256 threads, a window of a few hundred floats
    assert plan_at(band, 256)["lds_floats"] > 0
    assert widths(band, 256, 4) == dict(forward=4, transposed=4)
    assert widths(band, 256, 3) == dict(forward=2, transposed=2)
    assert widths(band, 256, 2) == dict(forward=2, transposed=2)
    plain = a[4]                                   # uniform 3000 x 2500, 13 000 entries: no window
    assert plan_at(plain, 256)["lds_floats"] == 0
    assert widths(plain, 256, 7)["transposed"] == 4
    assert widths(plain, 256, 1)["transposed"] == 1


def test_widths_refuse_bad_arguments():
    out = (C.c_int64 * 2)()
    assert lib.hispmv_prep_vector_widths(None, N_CUS, 4, out) == _lib.HISPMV_EINVAL
    m = S.case_a()[1]
    with pytest.raises(ValueError):
        prep.vector_widths_from_coo(m["r"], m["c"], m["v"], m["rows"], m["cols"], N_CUS, 0)
    with pytest.raises(ValueError):
        prep.vector_widths_from_coo(m["r"], m["c"], m["v"], m["rows"], m["cols"], 0, 4)


def test_null_context_is_refused_by_both_entries():
    """NULL context -> HISPMV_EINVAL before anything else, whatever the other arguments are."""
    p = C.c_void_p(4096)
    assert lib.hispmv_linear_device(None, 0, p, 4, p, C.c_void_p(8192), 1.0, 1.0, None) == _lib.HISPMV_EINVAL
    assert lib.hispmv_linear_device_t(None, 0, p, 4, p, 0, C.c_void_p(8192), 1.0, 1.0, None) == _lib.HISPMV_EINVAL
    assert lib.hispmv_linear_device(None, 0, None, 0, None, None, 1.0, 1.0, None) == _lib.HISPMV_EINVAL
    assert lib.hispmv_linear_device_t(None, 0, None, 0, None, 7, None, 1.0, 1.0, None) == _lib.HISPMV_EINVAL
    out = (C.c_int64 * 5)()
    assert lib.hispmv_linear_info(None, 0, 4, out) == _lib.HISPMV_EINVAL
