"""In-place value updates (hispmv_set_value_updates / hispmv_update_values*), the parts that need no device:

* the value map: every device layout of a handle packed with the real values and with the index payloads of an updatable handle
  (hispmv_prep_value_layouts) -- gathering the values through the map read out of the payload layouts must give the real layouts
  byte for byte, for every golden fixture and for every format the defaults can choose (slices compact and wide, tile stream,
  column tiles, band tiles, stray split, stray slots, batch layouts);
* argument errors of the new entry points without a device;
* Shard.local_values against shard_csr(...).values."""
import ctypes as C

import numpy as np
import pytest

from conftest import GOLDEN_CASES


def gather_through_map(d, values):
    """What update_values_kernel writes: for every chunk, values[map - 1] (0 where the map holds 0) at both destinations."""
    out = d["index"].view(np.uint32).copy()
    vb = np.ascontiguousarray(values, np.float32).view(np.uint32)
    m = d["map"].reshape(-1, 1024)
    for k, (o0, o1) in enumerate(d["chunks"]):
        idx = m[k].astype(np.int64)
        chunk = np.where(idx > 0, vb[np.maximum(idx - 1, 0)], 0).astype(np.uint32)
        for o in (o0, o1):
            if o >= 0:
                assert o % 16 == 0
                out[o // 4:o // 4 + 1024] = chunk
    return out


def check_map(r, c, v, rows, cols):
    from hispmv_amd.prep import value_layouts_from_coo
    d = value_layouts_from_coo(r, c, v, rows, cols, 256)
    nnz = len(v)
    assert d["bytes"] > 0 and d["map_slots"] == 1024 * d["chunks"].shape[0]
    # every input entry sits in exactly one slot of the first layouts; the rest are fillers / padding (0)
    got = np.sort(d["map"][d["map"] > 0])
    assert np.array_equal(got, np.arange(1, nnz + 1)), "map is not a permutation of the input positions"
    assert d["written"] == 1024 * int(d["chunks"].shape[0] + (d["chunks"][:, 1] >= 0).sum())
    # the meta bytes did not depend on the values, and the gather reproduces the value slots
    assert np.array_equal(gather_through_map(d, v), d["real"].view(np.uint32))
    # a second set of values gathered into the same map is what a fresh packing of that set gives
    v2 = (np.arange(nnz, dtype=np.float32) * np.float32(0.37) - np.float32(11.0))
    d2 = value_layouts_from_coo(r, c, v2, rows, cols, 256)
    assert np.array_equal(gather_through_map(d, v2), d2["real"].view(np.uint32))
    return d


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_value_map_reproduces_every_golden_layout(golden, name):
    g = golden(name)
    r, c, v = g["coo_r"], g["coo_c"], g["coo_v"]
    check_map(r, c, v, int(g["rows"]), int(g["cols"]))


def _band(rows, per_row, half, seed=3):
    rng = np.random.default_rng(seed)
    r = np.repeat(np.arange(rows, dtype=np.int64), per_row)
    c = np.clip(r + rng.integers(-half, half + 1, size=r.size), 0, rows - 1)
    v = rng.random(r.size, dtype=np.float32) - np.float32(0.5)
    return r.astype(np.int32), c.astype(np.int32), v


def _strays(share, rows=300000):
    r, c, v = _band(rows, 16, 1500)
    far = np.random.default_rng(5).random(c.size) < share
    c = np.where(far, np.random.default_rng(6).integers(0, rows, c.size), c).astype(np.int32)
    return r, c, v


def _shuffled(r, c, v, seed=1):
    p = np.random.default_rng(seed).permutation(r.size)      # input order that differs from CSR order
    return r[p], c[p], v[p]


CASES = {
    # (env, matrix, expected (format, tile_kind, parts) -- None = not checked, batch layout expected)
    "slices_compact": ({}, lambda: _band(200000, 12, 400), (0, 0, 1), False),
    "slices_wide_l2": ({"HISPMV_FORMAT": "slices"}, lambda: _band(100000, 8, 45000), (0, 0, 1), False),
    "plan_global": ({"HISPMV_PLAN": "global", "HISPMV_FORMAT": "slices"}, lambda: _band(200000, 12, 400), (0, 0, 1), False),
    "tile_stream": ({"HISPMV_FORMAT": "tts"}, lambda: _band(100000, 8, 45000), (1, 0, 1), False),
    "column_tiles": ({"HISPMV_FORMAT": "slices", "HISPMV_BAND_TILES": "0", "HISPMV_COL_TILE_BYTES": "65536"},
                     lambda: _band(100000, 8, 45000), (0, 1, None), False),
    "band_tiles": ({}, lambda: _band(250000, 20, 30000), (0, 2, None), False),
    "stray_split": ({"HISPMV_STRAY_SLOTS": "0"}, lambda: _strays(0.03), (0, 3, 2), False),
    "stray_slots": ({}, lambda: _strays(0.03), (0, 0, 1), False),
    "batch_layout": ({"HISPMV_BATCH_MIN_SLICES": "1"}, lambda: _band(400000, 12, 400), (0, 0, 1), True),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_value_map_reproduces_every_format(monkeypatch, case):
    env, make, want, batch = CASES[case]
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    r, c, v = _shuffled(*make())
    d = check_map(r, c, v, int(r.max()) + 1, int(r.max()) + 1)
    got = (d["format"], d["tile_kind"], d["parts"])
    assert all(w is None or w == g for w, g in zip(want, got)), (case, got)
    if want[2] is None:
        assert d["parts"] >= 2
    if batch:
        assert d["batch_layouts"] > 0 and d["written"] > d["map_slots"]


def test_value_map_with_duplicates_and_empty_rows():
    rng = np.random.default_rng(4)
    rows, cols = 5000, 3000
    r = rng.integers(0, rows // 2, 40000).astype(np.int32)               # the upper half of the rows stays empty (fillers)
    c = rng.integers(0, cols, 40000).astype(np.int32)
    r[:5000], c[:5000] = 17, 5                                         # 5000 duplicates of one coordinate
    v = rng.random(r.size, dtype=np.float32)
    check_map(r, c, v, rows, cols)


def test_index_payloads_survive_the_host_path():
    """Payloads below 2^23 are fp32 denormals: nothing on the way may flush or compare them.  The CSR of a payload array is the
    stable CSR order of the input positions."""
    from hispmv_amd.prep import prep_from_coo
    rng = np.random.default_rng(8)
    rows, cols, nnz = 700, 900, 20000
    r = rng.integers(0, rows, nnz).astype(np.int32)
    c = rng.integers(0, cols, nnz).astype(np.int32)
    pay = (np.arange(nnz, dtype=np.uint32) + 1).view(np.float32)
    p = prep_from_coo(r, c, pay, rows, cols)
    order = np.lexsort((np.arange(nnz), c, r))
    assert np.array_equal(np.asarray(p.values).view(np.uint32), order.astype(np.uint32) + 1)


def test_value_update_entry_points_check_their_arguments_without_a_device():
    from hispmv_amd import _lib
    lib = _lib.lib
    out = (C.c_int64 * 4)(7, 7, 7, 7)
    v = (C.c_float * 4)()
    assert lib.hispmv_set_value_updates(None, 1) == _lib.HISPMV_EINVAL
    assert lib.hispmv_update_values(None, 0, v, 4) == _lib.HISPMV_EINVAL
    assert lib.hispmv_update_values(None, 0, None, 4) == _lib.HISPMV_EINVAL
    assert lib.hispmv_update_values_device(None, 0, v, 4, None) == _lib.HISPMV_EINVAL
    assert lib.hispmv_update_values_device(None, -1, None, -1, None) == _lib.HISPMV_EINVAL
    assert lib.hispmv_value_update_info(None, 0, out) == _lib.HISPMV_EINVAL
    assert list(out) == [7, 7, 7, 7]
    # the host-only packing entry
    p = C.c_void_p()
    cnt = (C.c_int64 * 8)()
    r = np.zeros(4, np.int32)
    assert lib.hispmv_prep_value_layouts(C.byref(p), None, None, None, 4, 10, 10, 256, cnt) == _lib.HISPMV_EINVAL
    assert lib.hispmv_prep_value_layouts(C.byref(p), r.ctypes.data, r.ctypes.data, r.ctypes.data, 4, 0, 10, 256, cnt) == _lib.HISPMV_EINVAL
    assert lib.hispmv_prep_value_layouts(C.byref(p), r.ctypes.data, r.ctypes.data, r.ctypes.data, 4, 10, 10, 0, cnt) == _lib.HISPMV_EINVAL
    assert lib.hispmv_prep_value_layouts(None, r.ctypes.data, r.ctypes.data, r.ctypes.data, 4, 10, 10, 256, cnt) == _lib.HISPMV_EINVAL
    assert not p.value
    assert lib.hispmv_prep_value_array(None, 0) is None


def test_value_layouts_refuse_the_experiment_geometries(monkeypatch):
    from hispmv_amd.prep import value_layouts_from_coo
    r, c, v = _band(1000, 4, 20)
    monkeypatch.setenv("HISPMV_TTS_GEOMETRY", "tall")
    with pytest.raises(ValueError, match="experiment"):
        value_layouts_from_coo(r, c, v, 1000, 1000)


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_shard_local_values_match_shard_csr(world):
    from hispmv_amd.dist import shard_csr
    rng = np.random.default_rng(world)
    rows, cols = 3000, 2000
    lens = rng.integers(0, 30, rows)
    lens[::7] = 0                                                    # empty rows: fillers count in the cut
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = rng.integers(0, cols, int(rp[-1])).astype(np.int32)
    va = rng.random(int(rp[-1]), dtype=np.float32)
    va2 = rng.random(int(rp[-1]), dtype=np.float32)
    total = 0
    for rank in range(world):
        sh = shard_csr(rp, ci, va, world, rank)
        assert np.array_equal(sh.local_values(va), sh.values)
        assert np.array_equal(sh.local_values(va2), shard_csr(rp, ci, va2, world, rank).values)
        assert sh.local_values(va).dtype == np.float32
        total += sh.values.size
    assert total == va.size
    with pytest.raises(ValueError):
        shard_csr(rp, ci, va, world, 0).local_values(va[:-1])
