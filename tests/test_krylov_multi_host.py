"""The multi-right-hand-side Krylov entries' host side, no device: the layout rule on both sides of the ABI, the argument errors of the
new entries without a context, and the numpy model on the columns the GPU tests batch -- the check that those inputs are fair (the
columns stop at different iterations, well inside the budget; the zero column never iterates; the NaN column breaks down alone)."""
import ctypes as C

import numpy as np
import pytest

import krylov_model as km
import krylov_multi_cases as kc


def test_layout_rule_on_both_sides_of_the_abi():
    from hispmv_amd import _lib, prep
    out = (C.c_int64 * 4)()
    for n in (0, 1, 3, 1023, 1024, 1025, 4099, 2 ** 20 - 1, 2 ** 20):
        for m in (1, 2, 3, 4, 5, 63, 64, 65, 256, 260, 2 ** 20):
            assert _lib.lib.hispmv_prep_krylov_multi(n, m, out) == _lib.HISPMV_OK
            got = prep.krylov_multi(n, m)
            groups, ld = -(-n // 1024), -(-m // 4) * 4
            want = {"groups": groups, "ld": ld, "state_bytes": 2 * 128 * ld + 8 * ld, "partial_bytes": 8 * groups * ld * 8}
            assert got == want == dict(zip(want, (int(x) for x in out))), (n, m)
            # every workgroup owns one chunk, so the order of a column's dot product is the single-vector one for this n
            assert groups == prep.krylov_groups(n) == km.groups(n)
            assert ld % 4 == 0 and ld >= m and (got["state_bytes"] + got["partial_bytes"]) % 16 == 0
    for n, m in ((-1, 1), (2 ** 20 + 1, 1), (5, 0), (5, -3), (5, 2 ** 20 + 1)):
        assert _lib.lib.hispmv_prep_krylov_multi(n, m, out) == _lib.HISPMV_EINVAL
        with pytest.raises(ValueError):
            prep.krylov_multi(n, m)
    assert _lib.lib.hispmv_prep_krylov_multi(5, 1, None) == _lib.HISPMV_EINVAL


def test_argument_errors_without_a_context():
    from hispmv_amd import _lib
    lib = _lib.lib
    res = (_lib.KrylovResult * 2)()
    out = (C.c_int64 * 8)()
    assert lib.hispmv_krylov_multi_info(None, 0, 0, 2, out) == _lib.HISPMV_EINVAL
    assert lib.hispmv_dot_multi_device(None, 4, 2, None, 2, None, 2, None, None, 0, None) == _lib.HISPMV_EINVAL
    assert lib.hispmv_cg_multi_device(None, 0, None, 2, None, 2, 2, None, 1e-6, 10, 1, None, 0, None, res) == _lib.HISPMV_EINVAL
    assert lib.hispmv_bicgstab_multi_device(None, 0, None, 2, None, 2, 2, 1e-6, 10, 1, None, 0, None, res) == _lib.HISPMV_EINVAL
    assert lib.hispmv_krylov_multi_status(None, None, 2, None, res) == _lib.HISPMV_EINVAL


@pytest.mark.parametrize("solver", ["cg", "bicgstab"])
def test_the_columns_stop_at_different_iterations(solver):
    prod, _ = km.scipy_products(km.tridiag(kc.N))
    infos = [info for _, _, info in kc.run_models(prod, kc.columns(), solver=solver)]
    by = dict(zip(kc.NAMES, infos))
    print({k: (v["status"], v["iterations"]) for k, v in by.items()})
    its = [by[k]["iterations"] for k in ("rhs1", "e0", "A1", "sin")]
    assert all(by[k]["status"] == "CONVERGED" for k in ("rhs1", "e0", "A1", "sin", "zero"))
    assert its[0] > its[1] > its[2] > its[3] > 0, its
    assert all(i <= kc.MAX_ITERS // 2 for i in its), its
    assert by["zero"]["iterations"] == 0 and by["zero"]["relres"] == 0.0
    assert by["nan"]["status"] == "BREAKDOWN" and by["nan"]["iterations"] == 0
    x_nan = kc.run_models(prod, kc.columns()[:, 5:6], solver=solver)[0][0]
    assert not x_nan.any()          # x stays the initial guess
