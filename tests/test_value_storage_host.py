"""bf16 value storage without a device (hispmv_set_value_storage / hispmv_prep_set_value_storage): the rounding R, the HALF slice
layout the host packer writes for every group that is compact under fp32 storage, and the promise that format choice and launch
plan do not look at the storage.

R is what CPU torch gives: v.to(torch.bfloat16).to(torch.float32).  A half slice is 1024 x 4 bytes: per lane and step one 16-byte
piece {v0 | v1 << 16, v2 | v3 << 16, m0 | m1 << 16, m2 | m3 << 16} of four consecutive elements (hispmv_format.h)."""
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
SLICE = 1024
UNIT = 2048


def R(v):
    import torch
    return torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def _band(rows, per_row, half, seed=3):
    rng = np.random.default_rng(seed)
    r = np.repeat(np.arange(rows, dtype=np.int64), per_row)
    c = np.clip(r + rng.integers(-half, half + 1, size=r.size), 0, rows - 1)
    return r.astype(np.int32), c.astype(np.int32)


def _strays(share, rows=300000):
    r, c = _band(rows, 16, 1500)
    far = np.random.default_rng(5).random(c.size) < share
    return r, np.where(far, np.random.default_rng(6).integers(0, rows, c.size), c).astype(np.int32)


def _mixed(rows=100000):
    """Stray couplings in the first third of the rows only: compact and wide groups side by side."""
    r, c = _band(rows, 16, 1500)
    far = (np.random.default_rng(5).random(c.size) < 0.2) & (r < rows / 3)
    return r, np.where(far, np.random.default_rng(6).integers(0, rows, c.size), c).astype(np.int32)


def _values(n, seed=11):
    """Random values over many decades, both signs."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * 10.0 ** rng.uniform(-30, 30, n)).astype(np.float32)


def _split(lay):
    """Per group of a device layout: (kind bits, values as fp32 bits [n, 1024], metas [n, 1024], the group's raw bytes)."""
    G, ns = lay["group_slices"], lay["n_slices"]
    out = []
    for g, (_, _, off, w) in enumerate(lay["dgroups"]):
        n = min(G, ns - g * G)
        size = SLICE * (4 if w & 4 else 6 if w else 8)
        raw = lay["bytes"][off * UNIT: off * UNIT + n * size]
        assert raw.size == n * size
        if w & 4:
            q = raw.view(np.uint16).reshape(n, SLICE // 4, 8)
            vals = q[:, :, :4].reshape(n, SLICE).astype(np.uint32) << 16
            meta = q[:, :, 4:].reshape(n, SLICE).astype(np.uint32)
        elif w:
            s = raw.reshape(n, SLICE * 6)
            vals = s[:, :SLICE * 4].copy().view(np.uint32)
            meta = s[:, SLICE * 4:].copy().view(np.uint16).astype(np.uint32)
        else:
            s = raw.reshape(n, SLICE * 8)
            vals = s[:, :SLICE * 4].copy().view(np.uint32)
            meta = s[:, SLICE * 4:].copy().view(np.uint32)
        out.append((int(w), vals, meta, raw))
    return out


def test_rounding_read_back_from_a_half_layout():
    from hispmv_amd.prep import device_layout_from_coo
    r, c = _band(200000, 12, 400)
    v = _values(r.size)
    edge = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1e-39, -3e-39, 1.1754942e-38, 3.4028235e38, -3.4028235e38, 3.3895314e38, 3.39e38,
                     1.00390625, 1.01171875, -1.00390625, -1.01171875, 1.0039063692092896, 1.0039061307907104, 65280.0, 1.0, -2.5], np.float32)
    at = np.arange(edge.size) * 1009 + 5
    v[at] = edge
    nan_at = 7777
    v[nan_at] = np.nan
    # the ties named in the issue, and the overflow to Inf, so that the reference itself is what this test believes it is
    assert R(np.float32([1.00390625, 1.01171875, 3.4028235e38])).tolist() == [1.0, 1.015625, np.inf]
    lay = device_layout_from_coo(r, c, v, 200000, 200000, 256, value_storage="bf16")
    groups = _split(lay)
    assert all(w & 4 for w, *_ in groups), "every group of this matrix is half"
    got = np.concatenate([vals.reshape(-1) for _, vals, _, _ in groups])
    # v in the order of the stream: the value halves of the host words under fp32 storage (fillers and padding are zeros)
    vs = (device_layout_from_coo(r, c, v, 200000, 200000, 256)["words"] & 0xffffffff).astype(np.uint32)
    assert vs.size == got.size
    assert np.array_equal(np.sort(vs[vs != 0]), np.sort(v.view(np.uint32)[v.view(np.uint32) != 0])), "the stream holds the input's values"
    want = R(vs.view(np.float32))
    nan = np.isnan(vs.view(np.float32))
    assert nan.sum() == 1 and np.isnan(got.view(np.float32)[nan]).all() and not np.isnan(got.view(np.float32)[~nan]).any()
    assert np.array_equal(got[~nan], want.view(np.uint32)[~nan])
    u = vs[~nan].astype(np.uint64)
    assert np.array_equal(got[~nan], ((u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000).astype(np.uint32))
    for e in edge:          # every edge value really went through the packer
        assert (vs == np.float32(e).view(np.uint32)).any(), e


MATRICES = {
    # name -> (matrix, (slices, groups, compact groups, wide groups, kind bits of the compact groups, layout bytes or None))
    "band": (lambda: _band(200000, 12, 400), (2353, 589, 589, 0, 1, 14456832)),
    "strays": (lambda: _strays(0.03), (4688, 247, 247, 0, 3, None)),
    "mixed": (_mixed, (None, 391, 260, 131, None, None)),
}


@pytest.mark.parametrize("name", sorted(MATRICES))
def test_half_layout_of_the_host_packer(name):
    from hispmv_amd.prep import device_layout_from_coo, prep_from_coo
    make, (n_slices, n_groups, n_compact, n_wide, kind, n_bytes) = MATRICES[name]
    r, c = make()
    rows = int(max(r.max(), c.max())) + 1
    v = _values(r.size, seed=13)
    f = device_layout_from_coo(r, c, v, rows, rows, 256)
    # what the packer makes of the matrix with fp32 storage (checked first: the rest must not pass vacuously)
    fw = f["dgroups"][:, 3]
    assert f["dgroups"].shape[0] == n_groups and int((fw != 0).sum()) == n_compact and int((fw == 0).sum()) == n_wide, (f["dgroups"].shape, int((fw != 0).sum()))
    if n_slices is not None:
        assert f["n_slices"] == n_slices
    if kind is not None:
        assert set(fw[fw != 0].tolist()) == {kind}
    if n_bytes is not None:
        assert f["bytes"].size == n_bytes
    assert f["compact_slices"] > 0 and not (fw & 4).any()
    h = device_layout_from_coo(r, c, v, rows, rows, 256, value_storage="bf16")
    p = device_layout_from_coo(r, c, R(v), rows, rows, 256)          # fp32 storage of the pre-rounded values
    # shorter by exactly one unit per slice of a compact group
    assert h["bytes"].size == f["bytes"].size - f["compact_slices"] * UNIT
    assert h["compact_slices"] == f["compact_slices"] and h["stray_slices"] == f["stray_slices"] and h["n_slices"] == f["n_slices"]
    # same plan, groups, fragments, stray columns; the group table differs in the half bit and the offsets only
    for k in ("threads", "group_slices", "window_floats", "stray_floats"):
        assert h[k] == f[k], k
    assert np.array_equal(h["groups"], f["groups"]) and np.array_equal(h["frags"], f["frags"]) and np.array_equal(h["stray_cols"], f["stray_cols"])
    assert np.array_equal(h["dgroups"][:, :2], f["dgroups"][:, :2])
    assert np.array_equal(h["dgroups"][:, 3], np.where(fw != 0, fw | 4, 0))
    G = f["group_slices"]
    here = np.minimum(G, f["n_slices"] - np.arange(n_groups) * G)
    sizes = here * np.where(fw != 0, 2, 4)
    assert np.array_equal(h["dgroups"][:, 2], np.concatenate([[0], np.cumsum(sizes)[:-1]])), "a group's offset follows from the sizes before it"
    assert int(sizes.sum()) * UNIT == h["bytes"].size
    # the slices themselves
    for (hw, hv, hm, hraw), (pw, pv, pm, praw), (_, _, fm, _) in zip(_split(h), _split(p), _split(f)):
        assert np.array_equal(hm, fm) and np.array_equal(hm, pm), "the metas of a half slice are the compact metas"
        assert np.array_equal(hv, pv), "the values are R(v), widened"
        if not hw:
            assert np.array_equal(hraw, praw), "a wide group is the fp32 layout of R(v), byte for byte"
    # headers and fix lists do not know the storage
    a, b = prep_from_coo(r, c, v, rows, rows), prep_from_coo(r, c, v, rows, rows, value_storage="bf16")
    assert np.array_equal(a.hdr, b.hdr) and np.array_equal(a.fix, b.fix) and a.plan == b.plan
    assert np.array_equal(b.values.view(np.uint32), R(a.values).view(np.uint32))
    assert np.array_equal(b.words >> 32, a.words >> 32)
    assert np.array_equal((b.words & 0xffffffff).astype(np.uint32), R((a.words & 0xffffffff).astype(np.uint32).view(np.float32)).view(np.uint32))


def test_plan_and_format_choice_do_not_depend_on_the_storage():
    """hispmv_prep_plan and hispmv_prep_choose_format on the golden cases of tests/golden/format_choices.json: the bf16 outputs are
    the fp32 ones (which test_format_choice.py pins against the golden file)."""
    from hispmv_amd._lib import lib, HISPMV_OK
    sys.path.insert(0, str(ROOT / "tests" / "golden"))
    import make_format_choices as G
    gold = json.loads((ROOT / "tests" / "golden" / "format_choices.json").read_text())
    seen = 0
    for name, rows, cols, rp, ci, va in G.cases():
        rr = np.repeat(np.arange(rows, dtype=np.int32), np.diff(np.asarray(rp, np.int64)))
        cc = np.ascontiguousarray(ci, np.int32)
        vv = np.ascontiguousarray(va, np.float32)
        outs = []
        for storage in (0, 1):
            p = C.c_void_p()
            assert lib.hispmv_prep_from_coo(C.byref(p), C.c_void_p(rr.ctypes.data), C.c_void_p(cc.ctypes.data), C.c_void_p(vv.ctypes.data), rr.size, rows, cols) == HISPMV_OK
            try:
                assert lib.hispmv_prep_set_value_storage(p, storage) == HISPMV_OK
                plan, choice = (C.c_int64 * 6)(), (C.c_int64 * 16)()
                assert lib.hispmv_prep_plan(p, 256, plan) == HISPMV_OK
                assert lib.hispmv_prep_choose_format(p, 256, choice) == HISPMV_OK
                outs.append((list(plan), list(choice)))
            finally:
                lib.hispmv_prep_free(p)
        assert outs[0] == outs[1], name
        from hispmv_amd.prep import FORMAT_FIELDS
        got = dict(zip(FORMAT_FIELDS, outs[1][1]))
        assert {k: got[k] for k in G.KEYS} == gold[name], name
        seen += 1
    assert seen == len(gold)


def test_argument_errors_without_a_device():
    from hispmv_amd import _lib
    lib = _lib.lib
    out = (C.c_int64 * 4)(7, 7, 7, 7)
    assert lib.hispmv_set_value_storage(None, _lib.HISPMV_VALUES_BF16) == _lib.HISPMV_EINVAL
    assert lib.hispmv_set_value_storage(None, 7) == _lib.HISPMV_EINVAL
    assert lib.hispmv_value_storage_info(None, 0, out) == _lib.HISPMV_EINVAL
    assert list(out) == [7, 7, 7, 7]
    assert lib.hispmv_prep_set_value_storage(None, _lib.HISPMV_VALUES_BF16) == _lib.HISPMV_EINVAL
    # an unknown storage on a prepared matrix: refused, the matrix keeps its fp32 values
    r, c = np.int32([0, 1]), np.int32([1, 0])
    v = np.float32([1.00390625, 3.0])
    p = C.c_void_p()
    assert lib.hispmv_prep_from_coo(C.byref(p), C.c_void_p(r.ctypes.data), C.c_void_p(c.ctypes.data), C.c_void_p(v.ctypes.data), 2, 2, 2) == _lib.HISPMV_OK
    try:
        assert lib.hispmv_prep_set_value_storage(p, 2) == _lib.HISPMV_EINVAL
        assert np.ctypeslib.as_array(lib.hispmv_prep_csr_val(p), shape=(2,)).tolist() == [1.00390625, 3.0]
        assert lib.hispmv_prep_set_value_storage(p, _lib.HISPMV_VALUES_BF16) == _lib.HISPMV_OK
        assert np.ctypeslib.as_array(lib.hispmv_prep_csr_val(p), shape=(2,)).tolist() == [1.0, 3.0]
    finally:
        lib.hispmv_prep_free(p)
    from hispmv_amd.prep import prep_from_coo
    with pytest.raises(ValueError):
        prep_from_coo(r, c, v, 2, 2, value_storage="fp16")
