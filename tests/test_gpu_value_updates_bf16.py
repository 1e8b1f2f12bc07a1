"""In-place value updates of bf16 handles on the MI355X (hispmv_set_value_updates in state HISPMV_VALUE_UPDATES_ANY_STORAGE).

No tolerance anywhere: after update_values*(v) an updatable bf16 handle returns, through every forward entry, BIT FOR BIT what a plain
bf16 handle freshly created from v returns -- the update rounds on the device with the R of the host packer.  The handle kinds are
the case builders of tests/test_gpu_value_storage.py (copied: that file stays as it is), the smallest shapes the project has for
each layout.  Special values (ties of both parities, overflow to Inf, Inf, NaN, subnormals, signed zeros) are read back through
y = A * ones.  Bookkeeping: the three states of the switch, device bytes, the arena."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HW = ("tests.xclbin", 0, 24, 1, 1, 2, 5, True, False, True)
ALPHA, BETA = 0.85, -2.06


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def R(v):
    import torch
    v = np.ascontiguousarray(v, np.float32)
    return torch.from_numpy(v).to(torch.bfloat16).to(torch.float32).numpy()


def make_handle(storage="fp32", updates=False, arena=64 << 30):
    import pyhispmv
    h = pyhispmv.FpgaHandle(*HW)
    h.set_arena_bytes(arena)
    h.set_value_storage(storage)
    h.set_value_updates(updates)
    return h


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def _band(rows, per_row, half, seed=3):
    rng = np.random.default_rng(seed)
    r = np.repeat(np.arange(rows, dtype=np.int64), per_row)
    c = np.clip(r + rng.integers(-half, half + 1, size=r.size), 0, rows - 1)
    return r.astype(np.int32), c.astype(np.int32)


def _strays(share, rows=300000):
    r, c = _band(rows, 16, 1500)
    far = np.random.default_rng(5).random(c.size) < share
    return r, np.where(far, np.random.default_rng(6).integers(0, rows, c.size), c).astype(np.int32)


def _shuffled_with_duplicates(r, c, seed=1):
    """Input order differs from CSR order, and some coordinates come twice (duplicates are summed, not coalesced)."""
    rng = np.random.default_rng(seed)
    dup = rng.integers(0, r.size, r.size // 50)
    r, c = np.concatenate([r, r[dup]]), np.concatenate([c, c[dup]])
    p = rng.permutation(r.size)
    return r[p], c[p]


# name -> (env, matrix, check on matrix_info): tests/test_gpu_value_storage.py
CASES = {
    "slices_compact": ({}, lambda: _band(200000, 12, 400), lambda i: i["format"] == 0 and i["col_tiles"] == 1 and i["compact_slices"] > 0),
    "slices_wide": ({"HISPMV_FORMAT": "slices"}, lambda: _band(100000, 8, 45000), lambda i: i["format"] == 0 and i["compact_slices"] < i["n_slices"]),
    "plan_global": ({"HISPMV_FORMAT": "slices", "HISPMV_PLAN": "global"}, lambda: _band(200000, 12, 400), lambda i: i["format"] == 0),
    "tile_stream": ({"HISPMV_FORMAT": "tts"}, lambda: _band(100000, 8, 45000), lambda i: i["format"] == 1),
    "column_tiles": ({"HISPMV_FORMAT": "slices", "HISPMV_BAND_TILES": "0", "HISPMV_COL_TILE_BYTES": "65536"}, lambda: _band(100000, 8, 45000),
                     lambda i: i["tile_kind"] == 1 and i["col_tiles"] >= 2),
    "stray_split": ({"HISPMV_STRAY_SLOTS": "0"}, lambda: _strays(0.03), lambda i: i["tile_kind"] == 3),
    "stray_slots": ({}, lambda: _strays(0.03), lambda i: i["tile_kind"] == 0 and i["compact_slices"] == i["n_slices"]),
    "batch_layout": ({"HISPMV_BATCH_MIN_SLICES": "1"}, lambda: _band(400000, 12, 400), lambda i: i["batch_group_slices"] > 0),
}
NO_HALF = {"tile_stream", "plan_global"}
HALF = {"slices_compact", "stray_split", "stray_slots", "batch_layout"}      # compact groups, so half slices; column tiles and the wide case gather through L2


def _runs(torch, h, idx, rows, cols, x, b, xs3, xs5):
    """y of run_kernel, linear (3 and 5 vectors), spmv_device and linear_device (3 vectors, alpha and beta of their own) for handle idx."""
    y = np.full(rows, np.nan, np.float32)
    h.select_matrix(idx)
    h.run_kernel(x, b, y, ALPHA, BETA)
    lin3, lin5 = h.linear(idx, xs3, b), h.linear(idx, xs5, b)
    dev = torch.device("cuda", 0)
    dx, db, dx3 = torch.from_numpy(x).to(dev), torch.from_numpy(b).to(dev), torch.from_numpy(xs3).to(dev)
    dy = torch.full((rows,), float("nan"), dtype=torch.float32, device=dev)
    dy3 = torch.full((3 * rows,), float("nan"), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    h.spmv_device(idx, dx.data_ptr(), db.data_ptr(), dy.data_ptr(), ALPHA, BETA)
    h.linear_device(idx, dx3.data_ptr(), 3, db.data_ptr(), dy3.data_ptr(), 0.5, 0.25)
    h.synchronize()
    return y, lin3, lin5, dy.cpu().numpy(), dy3.cpu().numpy()


def _assert_same_runs(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.all(np.isfinite(g)), (what, k)
        assert same_bits(g, w), f"{what}: path {k} differs from the fresh bf16 handle"


def _update_device(torch, h, idx, v):
    dv = torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    h.update_values_device(idx, dv.data_ptr(), dv.numel())
    h.synchronize()


@pytest.mark.parametrize("case", sorted(CASES))
def test_updated_bf16_handle_gives_the_bits_of_a_fresh_one(torch_mod, monkeypatch, case):
    env, make, check = CASES[case]
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    r, c = _shuffled_with_duplicates(*make())
    rows = cols = int(max(r.max(), c.max())) + 1
    rng = np.random.default_rng(17)
    v0 = rng.random(r.size, dtype=np.float32) - np.float32(0.5)
    v1 = rng.random(r.size, dtype=np.float32) * np.float32(3.0) - np.float32(1.0)
    x = rng.random(cols, dtype=np.float32) - np.float32(0.3)
    b = rng.random(rows, dtype=np.float32)
    xs3, xs5 = rng.random(3 * cols, dtype=np.float32), rng.random(5 * cols, dtype=np.float32)
    hu, hp = make_handle("bf16", "any_storage"), make_handle("bf16")
    try:
        u = hu.create_sparse_handle(r, c, v0, rows, cols)
        p0, p1 = hp.create_sparse_handle(r, c, v0, rows, cols), hp.create_sparse_handle(r, c, v1, rows, cols)
        assert min(u, p0, p1) >= 0
        hu.load_matrices()
        hp.load_matrices()
        iu, ip = hu.matrix_info(u), hp.matrix_info(p0)
        for k in ("format", "tile_kind", "col_tiles", "n_slices", "n_elems", "n_split_rows", "compact_slices", "block_threads", "group_slices", "lds_bytes",
                  "batch_group_slices", "carry_lookback", "col_tile_width", "col_tile_base"):
            assert iu[k] == ip[k], (k, iu[k], ip[k])
        assert check(iu), (case, iu)
        su, sp, up = hu.value_storage_info(u), hp.value_storage_info(p0), hu.value_update_info(u)
        print(case, iu, su, up)
        assert su == sp and su["storage"] == "bf16"                      # value_storage_info does not know about updates
        assert (su["slots_2byte"] > 0) == (iu["compact_slices"] > 0), su      # (column tiles gather through L2: no window, no half group)
        assert su["slots_2byte"] == 0 if case in NO_HALF else su["slots_2byte"] > 0 or case not in HALF, su
        assert up["updatable"] and up["n"] == r.size and up["map_slots"] % 1024 == 0 and up["map_slots"] >= r.size
        assert up["written"] == su["slots_2byte"] + su["slots_4byte"] and up["written"] >= up["map_slots"]
        if case == "batch_layout":
            assert up["written"] == 2 * up["map_slots"]
        assert iu["device_bytes"] == ip["device_bytes"] + 4 * up["map_slots"] + 24 * (up["map_slots"] // 1024)
        assert not hp.value_update_info(p0)["updatable"]

        ref0 = _runs(torch_mod, hp, p0, rows, cols, x, b, xs3, xs5)
        ref1 = _runs(torch_mod, hp, p1, rows, cols, x, b, xs3, xs5)
        assert not same_bits(ref0[0], ref1[0])
        # the load wrote the creation values through the update kernel
        _assert_same_runs(_runs(torch_mod, hu, u, rows, cols, x, b, xs3, xs5), ref0, f"{case} after load")
        _update_device(torch_mod, hu, u, v1)
        _assert_same_runs(_runs(torch_mod, hu, u, rows, cols, x, b, xs3, xs5), ref1, f"{case} after update_values_device")
        hu.update_values(u, v0)
        _assert_same_runs(_runs(torch_mod, hu, u, rows, cols, x, b, xs3, xs5), ref0, f"{case} after update_values")
    finally:
        hu.close()
        hp.close()
    from hispmv_amd._lib import lib
    assert lib.hispmv_free_failures() == 0


@pytest.mark.parametrize("shape", [(1000, 1003), (1000, 1004), (37, 1003)])
def test_updated_dense_bf16_handle_gives_the_bits_of_a_fresh_one(torch_mod, shape):
    """(37, 1003): 37111 values, not a multiple of 4 -- the element tail of the convert-and-copy kernel."""
    rows, cols = shape
    rng = np.random.default_rng(5)
    W0 = rng.random(rows * cols, dtype=np.float32) - np.float32(0.5)
    W1 = rng.random(rows * cols, dtype=np.float32) * np.float32(3.0) - np.float32(1.0)
    x = rng.random(cols, dtype=np.float32) - np.float32(0.3)
    b = rng.random(rows, dtype=np.float32)
    xs3, xs5 = rng.random(3 * cols, dtype=np.float32), rng.random(5 * cols, dtype=np.float32)
    hu, hp = make_handle("bf16", "any_storage"), make_handle("bf16")
    try:
        u = hu.create_dense_handle(W0, rows, cols)
        p0, p1 = hp.create_dense_handle(W0, rows, cols), hp.create_dense_handle(W1, rows, cols)
        hu.load_matrices()
        hp.load_matrices()
        assert hu.value_update_info(u) == {"updatable": True, "n": rows * cols, "map_slots": 0, "written": rows * cols}
        assert hu.value_storage_info(u) == hp.value_storage_info(p0)
        assert hu.matrix_info(u)["device_bytes"] == hp.matrix_info(p0)["device_bytes"] == 2 * rows * cols
        ref0 = _runs(torch_mod, hp, p0, rows, cols, x, b, xs3, xs5)
        ref1 = _runs(torch_mod, hp, p1, rows, cols, x, b, xs3, xs5)
        assert not same_bits(ref0[0], ref1[0])
        _assert_same_runs(_runs(torch_mod, hu, u, rows, cols, x, b, xs3, xs5), ref0, "dense after load")
        _update_device(torch_mod, hu, u, W1)
        _assert_same_runs(_runs(torch_mod, hu, u, rows, cols, x, b, xs3, xs5), ref1, "dense after update_values_device")
        hu.update_values(u, W0)
        _assert_same_runs(_runs(torch_mod, hu, u, rows, cols, x, b, xs3, xs5), ref0, "dense after update_values")
    finally:
        hu.close()
        hp.close()
    from hispmv_amd._lib import lib
    assert lib.hispmv_free_failures() == 0


# exact ties of both parities, their neighbours, the largest fp32, the smallest value that overflows to Inf and its lower neighbour,
# +-Inf, NaNs (quiet, signalling, negative with payload), fp32 subnormals (to 0, a tie to even 0, up, up to the smallest normal), +-0
SPECIAL_BITS = np.array([
    0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF, 0x3F818001, 0x3F817FFF,
    0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0xFF7F8000, 0x7F800000, 0xFF800000,
    0x7FC00000, 0x7F800001, 0xFFC12345, 0x7FFFFFFF,
    0x00000001, 0x00008000, 0x00008001, 0x00018000, 0x007FFFFF, 0x80000001, 0x80018000, 0x00400000,
    0x00000000, 0x80000000, 0x3F800000, 0xC0490FDB, 0x42F6E979], np.uint32)


def _expect_stored(y, v, what, strict_zero=True):
    """y = A * ones holds the stored values: R(v) bit for bit where v is not NaN and R(v) is not +-0, NaN where NaN, and +0 where the
    stored value is +-0 (the sum starts at +0, and +0 + -0 = +0): v = +-0 and the subnormals that round to +-0.  strict_zero=False
    (cases beyond the one the feature was specified with): a zero of either sign, its sign being the forward kernel's business."""
    want = R(v)
    nan, zero = np.isnan(v), want == 0
    rest = ~nan & ~zero
    assert np.all(np.isnan(y[nan])), what
    assert np.all(y[zero] == 0), what
    if strict_zero:
        assert np.array_equal(y[zero].view(np.uint32), np.zeros(int(zero.sum()), np.uint32)), what
    assert np.array_equal(y[rest].view(np.uint32), want[rest].view(np.uint32)), (what, [hex(q) for q in v[rest].view(np.uint32)[y[rest].view(np.uint32) != want[rest].view(np.uint32)][:8]])


def _one_per_row(n=2048):
    rng = np.random.default_rng(2)
    return rng.permutation(n).astype(np.int32), rng.integers(0, n, n).astype(np.int32), np.arange(n)


def _one_value_per_row_of_a_band(rows=50000, per_row=12):
    """Twelve entries per row, enough for a plan with a window (half slices); eleven of them will hold +0."""
    r, c = _band(rows, per_row, 400)
    at = np.arange(rows) * per_row + np.random.default_rng(3).integers(0, per_row, rows)
    p = np.random.default_rng(4).permutation(r.size)
    inv = np.empty_like(p)
    inv[p] = np.arange(p.size)
    return r[p], c[p], inv[at]


# name -> (env, matrix -> (r, c, positions of the one live entry of every row), half slices expected, +0 for stored zeros required)
SPECIAL_CASES = {
    "one_per_row": ({}, _one_per_row, False, True),
    "one_per_row_plan_global": ({"HISPMV_FORMAT": "slices", "HISPMV_PLAN": "global"}, _one_per_row, False, False),
    "half_slices": ({}, _one_value_per_row_of_a_band, True, False),
}


@pytest.mark.parametrize("case", sorted(SPECIAL_CASES))
def test_special_values_through_a_sparse_update(torch_mod, monkeypatch, case):
    """2048 x 2048 with one entry per row (32-bit slots: a matrix this small gets no window), the same under HISPMV_PLAN=global, and a
    band matrix whose compact groups are half slices, every row with one live entry among explicit +0 entries: y = A * ones."""
    env, make, half, strict = SPECIAL_CASES[case]
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    r, c, at = make()
    n = int(r.max()) + 1
    rows_at = r[at]
    assert np.array_equal(np.sort(rows_at), np.arange(n))
    rng = np.random.default_rng(2)
    special = np.resize(SPECIAL_BITS, n).view(np.float32)[rng.permutation(n)].copy()
    live0 = rng.random(n, dtype=np.float32) + np.float32(0.5)

    def values(live):
        v = np.zeros(r.size, np.float32)
        v[at] = live
        return v
    ones, zeros = np.ones(n, np.float32), np.zeros(n, np.float32)
    hu, hp = make_handle("bf16", "any_storage"), make_handle("bf16")
    try:
        u, s = hu.create_sparse_handle(r, c, values(live0), n, n), hu.create_sparse_handle(r, c, values(special), n, n)
        p = hp.create_sparse_handle(r, c, values(special), n, n)
        hu.load_matrices()
        hp.load_matrices()
        assert (hu.value_storage_info(u)["slots_2byte"] > 0) == half

        def stored(h, idx):
            y = np.full(n, np.nan, np.float32)
            h.select_matrix(idx)
            h.run_kernel(ones, zeros, y, 1.0, 0.0)
            return y[rows_at]
        assert np.array_equal(stored(hu, u), R(live0))
        _expect_stored(stored(hu, s), special, "created from the special values (the load's update)", strict)
        fresh = stored(hp, p)
        _expect_stored(fresh, special, "plain bf16 handle (host rounding)", strict)
        keep = ~np.isnan(fresh)
        _update_device(torch_mod, hu, u, values(special))
        y = stored(hu, u)
        _expect_stored(y, special, "update_values_device", strict)
        assert np.array_equal(np.isnan(y), ~keep) and same_bits(y[keep], fresh[keep])
        hu.update_values(u, values(live0))
        assert np.array_equal(stored(hu, u), R(live0))
        hu.update_values(u, values(special))
        y = stored(hu, u)
        _expect_stored(y, special, "update_values", strict)
        assert np.array_equal(np.isnan(y), ~keep) and same_bits(y[keep], fresh[keep])
    finally:
        hu.close()
        hp.close()
    from hispmv_amd._lib import lib
    assert lib.hispmv_free_failures() == 0


def test_special_values_through_a_dense_update(torch_mod):
    """64 x 64 with one non-zero per row: every other term of a row sum is +0, so y = W * ones holds the stored value of the row."""
    n = 64
    rng = np.random.default_rng(3)
    col = rng.integers(0, n, n)
    special = np.resize(SPECIAL_BITS, n).view(np.float32).copy()
    def dense(vals):
        W = np.zeros((n, n), np.float32)
        W[np.arange(n), col] = vals
        return W.reshape(-1)
    v0 = rng.random(n, dtype=np.float32) + np.float32(0.5)
    ones, zeros = np.ones(n, np.float32), np.zeros(n, np.float32)
    hu = make_handle("bf16", "any_storage")
    try:
        u, s = hu.create_dense_handle(dense(v0), n, n), hu.create_dense_handle(dense(special), n, n)
        hu.load_matrices()
        def stored(idx):
            y = np.full(n, np.nan, np.float32)
            hu.select_matrix(idx)
            hu.run_kernel(ones, zeros, y, 1.0, 0.0)
            return y
        assert np.array_equal(stored(u), R(v0))
        _expect_stored(stored(s), special, "created from the special values")
        _update_device(torch_mod, hu, u, dense(special))
        _expect_stored(stored(u), special, "update_values_device")
        hu.update_values(u, dense(v0))
        assert np.array_equal(stored(u), R(v0))
        hu.update_values(u, dense(special))
        _expect_stored(stored(u), special, "update_values")
    finally:
        hu.close()
    from hispmv_amd._lib import lib
    assert lib.hispmv_free_failures() == 0


def test_batch_call_after_an_update_equals_a_batch_call_on_fresh_handles(torch_mod, monkeypatch):
    """The batch layout's copy of the slices (a half layout too) is what a batch call may read: it must have been kept current."""
    monkeypatch.setenv("HISPMV_BATCH_MIN_SLICES", "1")
    torch = torch_mod
    mats = [_band(400000, 12, 400), _band(60000, 10, 300, seed=4)]
    dims = [int(max(r.max(), c.max())) + 1 for r, c in mats]
    rng = np.random.default_rng(31)
    v0 = [rng.random(r.size, dtype=np.float32) - np.float32(0.5) for r, _ in mats]
    v1 = [rng.random(r.size, dtype=np.float32) * np.float32(2.0) - np.float32(0.7) for r, _ in mats]
    vecs = [(rng.random(n, dtype=np.float32) - np.float32(0.3), rng.random(n, dtype=np.float32)) for n in dims]
    dev = torch.device("cuda", 0)

    def batch(h, idx):
        dx = [torch.from_numpy(x).to(dev) for x, _ in vecs]
        db = [torch.from_numpy(b).to(dev) for _, b in vecs]
        dy = [torch.full((n,), float("nan"), dtype=torch.float32, device=dev) for n in dims]
        prepared = h.prepare_batch(idx, [t.data_ptr() for t in dx], [t.data_ptr() for t in db], [t.data_ptr() for t in dy])
        for _ in range(2):                   # (the second call replays the cached plan)
            torch.cuda.synchronize()
            h.spmv_device_batch(prepared, ALPHA, BETA)
            h.synchronize()
        return [t.cpu().numpy() for t in dy]

    hu, hp = make_handle("bf16", "any_storage"), make_handle("bf16")
    try:
        iu = [hu.create_sparse_handle(r, c, v, n, n) for (r, c), v, n in zip(mats, v0, dims)]
        ip = [hp.create_sparse_handle(r, c, v, n, n) for (r, c), v, n in zip(mats, v1, dims)]
        hu.load_matrices()
        hp.load_matrices()
        assert hu.matrix_info(iu[0])["batch_group_slices"] > 0
        up = hu.value_update_info(iu[0])
        assert up["written"] > up["map_slots"]
        before = batch(hu, iu)
        for i, v in zip(iu, v1):
            _update_device(torch, hu, i, v)
        got, want = batch(hu, iu), batch(hp, ip)
        for k in range(2):
            assert np.all(np.isfinite(got[k])) and not same_bits(got[k], before[k])
            assert same_bits(got[k], want[k]), f"matrix {k} of the batch call after the update"
    finally:
        hu.close()
        hp.close()
    from hispmv_amd._lib import lib
    assert lib.hispmv_free_failures() == 0


def test_states_of_the_switch_bookkeeping_and_arena(torch_mod):
    from hispmv_amd import _lib
    r, c = _band(50000, 12, 400)
    rows = cols = 50000
    v = np.random.default_rng(1).random(r.size, dtype=np.float32) + np.float32(0.25)
    W = np.random.default_rng(2).random(64 * 48, dtype=np.float32)
    order = np.lexsort((c, r))
    rp = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=rows))]).astype(np.int32)
    h = make_handle()
    try:
        with pytest.raises(ValueError):
            h.set_value_updates("all")
        # state 1: as ever, bf16 creation refused for COO, CSR and dense; the context stays usable
        h.set_value_updates(True)
        f1, d1 = h.create_sparse_handle(r, c, v, rows, cols), h.create_dense_handle(W, 64, 48)
        h.set_value_storage("bf16")
        for create in (lambda: h.create_sparse_handle(r, c, v, rows, cols),
                       lambda: h.create_sparse_handle_from_csr(rp, c[order], v[order], rows, cols),
                       lambda: h.create_dense_handle(W, 64, 48)):
            with pytest.raises(ValueError, match="value updates"):
                create()
        # any other non-zero value of the C entry means "on"
        assert _lib.lib.hispmv_set_value_updates(h._ctx, 7) == _lib.HISPMV_OK
        with pytest.raises(ValueError, match="value updates"):
            h.create_dense_handle(W, 64, 48)
        assert h.num_matrices() == 2
        # state 2: an fp32 handle is the handle of state 1; bf16 handles are accepted, from COO, CSR and dense
        h.set_value_updates("any_storage")
        h.set_value_storage("fp32")
        f2, d2 = h.create_sparse_handle(r, c, v, rows, cols), h.create_dense_handle(W, 64, 48)
        h.set_value_storage("bf16")
        a = h.create_sparse_handle(r, c, v, rows, cols)
        a_csr = h.create_sparse_handle_from_csr(rp, c[order], v[order], rows, cols)
        e = h.create_dense_handle(W, 64, 48)
        h.set_value_updates(False)
        plain = h.create_sparse_handle(r, c, v, rows, cols)
        assert min(f2, d2, a, a_csr, e, plain) >= 0
        h.load_matrices()
        for one, two in ((f1, f2), (d1, d2)):
            assert h.value_update_info(one) == h.value_update_info(two) and h.value_update_info(one)["updatable"]
            assert h.matrix_info(one)["device_bytes"] == h.matrix_info(two)["device_bytes"]
            assert h.value_storage_info(one) == h.value_storage_info(two)
        ua, uf = h.value_update_info(a), h.value_update_info(f2)
        assert ua == uf == h.value_update_info(a_csr)                 # {1, n, map slots, slots written} by the rules of an fp32 handle
        assert h.value_storage_info(a) == h.value_storage_info(plain) and h.value_storage_info(a)["slots_2byte"] > 0
        bytes_a = h.matrix_info(a)["device_bytes"]
        assert bytes_a == h.matrix_info(plain)["device_bytes"] + 4 * ua["map_slots"] + 24 * (ua["map_slots"] // 1024)
        assert h.matrix_info(e)["device_bytes"] == 2 * W.size and h.value_update_info(e) == h.value_update_info(d2)
        # the CSR handle updates in the order of its input, as the COO handle in its own
        x, b = np.random.default_rng(2).random(cols, dtype=np.float32), np.zeros(rows, np.float32)
        v2 = np.random.default_rng(3).random(r.size, dtype=np.float32) - np.float32(0.5)
        h.update_values(a, v2)
        h.update_values(a_csr, v2[order])
        ya, yc = np.full(rows, np.nan, np.float32), np.full(rows, np.nan, np.float32)
        h.select_matrix(a)
        h.run_kernel(x, b, ya, 1.0, 0.0)
        h.select_matrix(a_csr)
        h.run_kernel(x, b, yc, 1.0, 0.0)
        assert np.all(np.isfinite(ya)) and same_bits(ya, yc)
        with pytest.raises(AssertionError):
            h.update_values(plain, v2)
    finally:
        h.close()
    # an arena one byte short of the updatable bf16 handle is full; the exact size takes it
    for arena, want in ((bytes_a - 1, -1), (bytes_a, 0)):
        h = make_handle("bf16", "any_storage", arena=arena)
        try:
            assert h.create_sparse_handle(r, c, v, rows, cols) == want
            assert h.arena_bytes_used() == (bytes_a if want == 0 else 0)
        finally:
            h.close()
    assert _lib.lib.hispmv_free_failures() == 0
