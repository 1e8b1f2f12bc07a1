"""The wide-batch value gradient without a device: the two C entries refuse a NULL context and a leading dimension below the batch,
FpgaHandle has the two methods with their documented defaults, and sparse_linear has wide_grad=False."""
import ctypes as C
import inspect


def test_null_context_is_refused():
    from hispmv_amd import _lib
    lib = _lib.lib
    out = (C.c_int64 * 4)()
    assert lib.hispmv_spmm_value_grad_device(None, 0, None, 1, None, 1, 1, None, 1.0, 0.0, None) == _lib.HISPMV_EINVAL
    assert lib.hispmv_spmm_value_grad_info(None, 0, 1, 1, out) == _lib.HISPMV_EINVAL


def test_info_refuses_a_leading_dimension_below_the_batch():
    """(a context needs a device: the same check on a real context is in tests/test_gpu_spmm_value_grad.py)"""
    from hispmv_amd import _lib
    out = (C.c_int64 * 4)(7, 7, 7, 7)
    assert _lib.lib.hispmv_spmm_value_grad_info(None, 0, 8, 7, out) == _lib.HISPMV_EINVAL
    assert _lib.lib.hispmv_spmm_value_grad_info(None, 0, 8, 8, None) == _lib.HISPMV_EINVAL
    assert list(out) == [7, 7, 7, 7]


def test_methods_and_defaults():
    from hispmv_amd.fpga_handle import FpgaHandle
    p = inspect.signature(FpgaHandle.spmm_value_grad_device).parameters
    assert list(p) == ["self", "matrix_idx", "d_gyt", "d_xt", "num_vecs", "d_grad", "alpha", "beta", "ld_gy", "ld_x", "stream"]
    assert (p["alpha"].default, p["beta"].default, p["ld_gy"].default, p["ld_x"].default, p["stream"].default) == (1.0, 0.0, None, None, 0)
    q = inspect.signature(FpgaHandle.spmm_value_grad_info).parameters
    assert list(q) == ["self", "matrix_idx", "num_vecs", "ld"] and q["ld"].default is None


def test_sparse_linear_has_wide_grad():
    from hispmv_amd.torch_ops import sparse_linear
    p = inspect.signature(sparse_linear).parameters
    assert p["wide_grad"].default is False and list(p)[-2:] == ["spmm", "wide_grad"]
