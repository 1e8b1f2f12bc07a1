"""The value gradient (include/hispmv.h: hispmv_value_grad_device) without a GPU: its two entries and the Python surface, and the
relation its slice kernel rests on -- DECODE + MAP.  The layouts of an updatable handle are packed with the index payloads bits(k + 1)
in the place of the values (the packers do no arithmetic on values); the value map is those payloads read back.  With the decoder of
tests/test_transpose_host.py (row = the slice's row_base + the row ends before the slot, column = the meta through fragment table or
stray columns) the payload of a slot then names the input entry whose row and column the kernel decodes for it: the payloads must be
exactly 1 .. n, each once, and rows == r[k], cols == c[k] for every slot.  That passes on the packer as it is, and pins it."""
import ctypes as C
import inspect

import numpy as np
import pytest

import step_small_cases as S
from test_transpose_host import decode_layout


def test_entries_refuse_a_null_context():
    from hispmv_amd import _lib
    lib = _lib.lib
    out = (C.c_int64 * 4)()
    assert lib.hispmv_value_grad_device(None, 0, None, None, 1, None, 1.0, 0.0, None) == _lib.HISPMV_EINVAL
    assert lib.hispmv_value_grad_info(None, 0, 1, out) == _lib.HISPMV_EINVAL


def test_python_surface():
    from hispmv_amd.fpga_handle import FpgaHandle
    from hispmv_amd.torch_ops import sparse_linear
    for name in ("value_grad_device", "value_grad_info"):
        assert callable(getattr(FpgaHandle, name)), name
    sig = inspect.signature(FpgaHandle.value_grad_device)
    assert list(sig.parameters)[1:] == ["matrix_idx", "d_gy", "d_x", "num_vecs", "d_grad", "alpha", "beta", "stream"]
    assert (sig.parameters["alpha"].default, sig.parameters["beta"].default, sig.parameters["stream"].default) == (1.0, 0.0, 0)
    p = inspect.signature(sparse_linear).parameters
    assert "values" in p and p["values"].default is None


def shuffled_with_duplicates():
    """case_a()[7] (band_4000x300) with its entries shuffled and 5000 of them entered a second time."""
    m = S.case_a()[7]
    rng = np.random.default_rng(404)
    again = rng.choice(m["r"].size, 5000, replace=False)
    r, c = np.concatenate([m["r"], m["r"][again]]), np.concatenate([m["c"], m["c"][again]])
    order = rng.permutation(r.size)
    return dict(m, name="band_shuffled_duplicates", r=r[order], c=c[order], v=np.ones(r.size, np.float32))


CASES = {"compact": lambda: S.case_a()[7], "wide_with_window": S.two_way_band, "stray_slots": S.stray_slot_band,
         "shuffled_duplicates": shuffled_with_duplicates}
KINDS = {"compact": {"compact"}, "wide_with_window": {"wide+window", "wide+L2"}, "stray_slots": {"compact", "stray"},
         "shuffled_duplicates": {"compact"}}


@pytest.mark.parametrize("case", list(CASES))
def test_payload_of_a_slot_names_the_entry_the_decode_gives(case):
    from hispmv_amd import prep
    m = CASES[case]()
    n = m["r"].size
    payload = np.arange(1, n + 1, dtype=np.uint32).view(np.float32)
    with S.environment(S.SLICES):
        lay = prep.device_layout_from_coo(m["r"], m["c"], payload, m["rows"], m["cols"])
        hdr = prep.prep_from_coo(m["r"], m["c"], payload, m["rows"], m["cols"]).hdr
    assert lay["n_slices"] == hdr.shape[0]
    rows, cols, q, kinds = decode_layout(lay, hdr)
    assert KINDS[case] <= kinds, kinds
    q = q.astype(np.int64)
    assert q.size == n and np.array_equal(np.sort(q), np.arange(1, n + 1)), "the payloads are not 1 .. n, each once"
    assert np.array_equal(rows, m["r"][q - 1].astype(np.int64)), "a slot's decoded row is not the row of the entry its payload names"
    assert np.array_equal(cols, m["c"][q - 1].astype(np.int64)), "a slot's decoded column is not the column of the entry its payload names"
