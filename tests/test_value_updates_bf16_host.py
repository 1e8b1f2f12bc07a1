"""Value updates of bf16 handles (hispmv_set_value_updates in state HISPMV_VALUE_UPDATES_ANY_STORAGE), the parts that need no device.

hispmv_prep_value_layouts_storage packs every device layout of an updatable bf16 handle on the host: `real` from R(values) with its
half groups, `index` with the payloads, the `map` as the loader uploads it and one kind per chunk destination.  For every format the
defaults can choose (the matrices and switches of test_value_updates.py, whose builders are copied here):

* the map equals the fp32 map of the same input word for word and is a permutation of 1..nnz plus zeros;
* a numpy emulation of update_values_bf16_kernel -- gather through the map, round with R, write by chunk kind at both destinations,
  8 of every 16 bytes of a half slice -- turns `index` into `real` byte for byte, so metas and headers are never written;
* a second value set gathered the same way equals a fresh packing of that set;
* the cases with compact groups really have half slices (kind 1), the batch layout really has second destinations.

R is checked against torch's own bf16 rounding for every non-NaN value."""
import numpy as np
import pytest


def R_bits(v):
    """round_bits_to_bf16 (hispmv_format.h) over an fp32 array, as uint32 bits."""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    rounded = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return np.where(nan, (u & 0xFFFF0000) | 0x00400000, rounded).astype(np.uint32)


def test_rounding_rule_is_torch_bf16():
    import torch
    rng = np.random.default_rng(0)
    bits = np.concatenate([
        rng.integers(0, 2**32, 200000, dtype=np.uint64).astype(np.uint32),
        np.array([0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0x7F7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0x7F800000, 0xFF800000,
                  0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x80000001, 0x00000000, 0x80000000], np.uint32)])
    v = bits.view(np.float32)
    keep = ~np.isnan(v)
    want = torch.from_numpy(v.copy()).bfloat16().float().numpy().view(np.uint32)
    assert np.array_equal(R_bits(v)[keep], want[keep])
    # a NaN stays a NaN with its sign
    nan = R_bits(np.array([0x7F800001, 0xFFC12345], np.uint32).view(np.float32))
    assert list(nan) == [0x7FC00000, 0xFFC10000]


def emulate_update(d, values):
    """What update_values_bf16_kernel writes into the payload layouts: per chunk R(values[map - 1]) (0 where the map holds 0) at both
    destinations -- 1024 fp32 slots, or the first 8 bytes of each of the 256 pieces of a half slice."""
    out = d["index"].copy()
    rb = R_bits(values)
    m = d["map"].reshape(-1, 1024)
    for k in range(m.shape[0]):
        idx = m[k].astype(np.int64)
        chunk = np.where(idx > 0, rb[np.maximum(idx - 1, 0)], 0).astype(np.uint32)
        for o, kind in zip(d["chunks"][k], d["kinds"][k]):
            if o < 0:
                continue
            assert o % 16 == 0 and kind in (0, 1)
            if kind == 0:
                out[o:o + 4096] = chunk.view(np.uint8)
            else:
                halves = (chunk >> 16).astype(np.uint16).reshape(256, 4)          # piece t = elements 4t .. 4t + 3
                out[o:o + 4096].reshape(256, 16)[:, :8] = halves.view(np.uint8).reshape(256, 8)
    return out


def value_slot_mask(d):
    mask = np.zeros(d["bytes"], bool)
    for k in range(d["chunks"].shape[0]):
        for o, kind in zip(d["chunks"][k], d["kinds"][k]):
            if o < 0:
                continue
            if kind == 0:
                mask[o:o + 4096] = True
            else:
                mask[o:o + 4096].reshape(256, 16)[:, :8] = True
    return mask


def check_map_bf16(r, c, v, rows, cols):
    from hispmv_amd.prep import value_layouts_from_coo
    d = value_layouts_from_coo(r, c, v, rows, cols, 256, value_storage="bf16")
    f = value_layouts_from_coo(r, c, v, rows, cols, 256)
    nnz = len(v)
    assert d["bytes"] > 0 and d["map_slots"] == 1024 * d["chunks"].shape[0] and d["kinds"].shape == d["chunks"].shape
    # format choice and plan do not depend on the storage: same chunks, same map
    assert (d["format"], d["tile_kind"], d["parts"], d["batch_layouts"]) == (f["format"], f["tile_kind"], f["parts"], f["batch_layouts"])
    assert np.array_equal(d["map"], f["map"]), "the map of the bf16 handle is not the fp32 map"
    assert np.array_equal(np.sort(d["map"][d["map"] > 0]), np.arange(1, nnz + 1)), "map is not a permutation of the input positions"
    assert d["written"] == 1024 * int(d["chunks"].shape[0] + (d["chunks"][:, 1] >= 0).sum()) == f["written"]
    assert not f["kinds"].any() and not d["kinds"][d["chunks"] < 0].any()          # fp32: 32-bit slots only; no kind without a destination
    half = int((d["kinds"] == 1).sum())
    assert d["bytes"] == f["bytes"] - 2048 * half              # a half slice is one 2 KiB unit shorter than a compact one
    # metas and headers do not depend on the values ...
    outside = ~value_slot_mask(d)
    assert np.array_equal(d["index"][outside], d["real"][outside])
    # ... and the update reproduces every value slot, writing nothing else
    got = emulate_update(d, v)
    assert np.array_equal(got, d["real"])
    assert np.array_equal(got[outside], d["index"][outside])
    # a second set of values through the same map is a fresh packing of that set
    v2 = (np.arange(nnz, dtype=np.float32) * np.float32(0.37) - np.float32(11.0))
    d2 = value_layouts_from_coo(r, c, v2, rows, cols, 256, value_storage="bf16")
    assert np.array_equal(emulate_update(d, v2), d2["real"])
    return d


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
    # (env, matrix, expected (format, tile_kind, parts) -- None = not checked, batch layout expected): test_value_updates.py
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
HALF_CASES = {"slices_compact", "stray_slots", "batch_layout"}       # compact groups: they must come out as half slices


@pytest.mark.parametrize("case", sorted(CASES))
def test_bf16_value_map_reproduces_every_format(monkeypatch, case):
    env, make, want, batch = CASES[case]
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    r, c, v = _shuffled(*make())
    d = check_map_bf16(r, c, v, int(r.max()) + 1, int(r.max()) + 1)
    got = (d["format"], d["tile_kind"], d["parts"])
    assert all(w is None or w == g for w, g in zip(want, got)), (case, got)
    if want[2] is None:
        assert d["parts"] >= 2
    if case in HALF_CASES:
        assert (d["kinds"][:, 0] == 1).any(), "no half slice: the case does not test what it is for"
    if batch:
        assert d["batch_layouts"] > 0 and d["written"] > d["map_slots"]
        assert (d["kinds"][:, 1] == 1).any()                       # the batch layout's copy is a half layout too


def test_bf16_value_map_with_duplicates_and_empty_rows():
    rng = np.random.default_rng(4)
    rows, cols = 5000, 3000
    r = rng.integers(0, rows // 2, 40000).astype(np.int32)               # the upper half of the rows stays empty (fillers)
    c = rng.integers(0, cols, 40000).astype(np.int32)
    r[:5000], c[:5000] = 17, 5                                         # 5000 duplicates of one coordinate
    v = rng.random(r.size, dtype=np.float32)
    check_map_bf16(r, c, v, rows, cols)


def test_storage_entry_checks_its_arguments():
    import ctypes as C
    from hispmv_amd import _lib
    from hispmv_amd.prep import value_layouts_from_coo
    lib = _lib.lib
    p = C.c_void_p()
    cnt = (C.c_int64 * 8)()
    r = np.zeros(4, np.int32)
    assert lib.hispmv_prep_value_layouts_storage(C.byref(p), r.ctypes.data, r.ctypes.data, r.ctypes.data, 4, 10, 10, 256, 2, cnt) == _lib.HISPMV_EINVAL
    assert lib.hispmv_prep_value_layouts_storage(None, r.ctypes.data, r.ctypes.data, r.ctypes.data, 4, 10, 10, 256, 1, cnt) == _lib.HISPMV_EINVAL
    assert lib.hispmv_prep_value_layouts_storage(C.byref(p), None, None, None, 4, 10, 10, 256, 1, cnt) == _lib.HISPMV_EINVAL
    assert not p.value
    with pytest.raises(ValueError):
        value_layouts_from_coo(r, r, r.astype(np.float32), 10, 10, value_storage="fp16")
    assert lib.hispmv_set_value_updates(None, _lib.HISPMV_VALUE_UPDATES_ANY_STORAGE) == _lib.HISPMV_EINVAL
