"""In-place value updates on the MI355X (hispmv_set_value_updates, hispmv_update_values / _device, hispmv_value_update_info).

An updatable handle created with values v1, loaded and updated to v2 must give the BITS of a plain handle created from v2 in a
second context under the same switches -- for every format and variant the loader can choose -- through run_kernel, linear with
several vectors and spmv_device, within the 1e-5 backward-error gate against fp64.  An updatable handle that is never updated
gives the bits of a plain one (the load itself runs the update kernel).  Batch calls keep their cached plans and step-kernel
queues across an update; an update on a stream orders with an SpMV on the same stream; the arena charge of the map is honest."""
import os

import numpy as np
import pytest

import oracle
from conftest import ALPHA, BETA, TOL
from util import bwd_err

pytestmark = pytest.mark.gpu

HW = ("tests.xclbin", 0, 24, 1, 1, 2, 5, True, False, True)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def make_handle(env=None, updates=False, arena=64 << 30):
    """An FpgaHandle created under `env` (the switches are read when the context is created), value updates on or off."""
    import pyhispmv
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        h = pyhispmv.FpgaHandle(*HW)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    h.set_arena_bytes(arena)
    if updates:
        h.set_value_updates(True)
    return h


def truth(r, c, v, rows, x, b, alpha, beta):
    order = np.lexsort((np.arange(r.size), c, r))
    rp = np.zeros(rows + 1, np.int64)
    np.add.at(rp, np.asarray(r, np.int64) + 1, 1)
    rp = np.cumsum(rp).astype(np.int32)
    return oracle.spmv_f64(rp, np.asarray(c)[order].astype(np.int32), np.asarray(v)[order].astype(np.float32), x, b, alpha, beta)


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


# name -> (env, matrix, check on matrix_info / value_update_info)
CASES = {
    "slices_compact": ({}, lambda: _band(200000, 12, 400), lambda i, u: i["format"] == 0 and i["col_tiles"] == 1 and i["compact_slices"] > 0),
    "slices_wide": ({"HISPMV_FORMAT": "slices"}, lambda: _band(100000, 8, 45000), lambda i, u: i["format"] == 0 and i["compact_slices"] < i["n_slices"]),
    "plan_global": ({"HISPMV_FORMAT": "slices", "HISPMV_PLAN": "global"}, lambda: _band(200000, 12, 400), lambda i, u: i["format"] == 0),
    "tile_stream": ({"HISPMV_FORMAT": "tts"}, lambda: _band(100000, 8, 45000), lambda i, u: i["format"] == 1),
    "column_tiles": ({"HISPMV_FORMAT": "slices", "HISPMV_BAND_TILES": "0", "HISPMV_COL_TILE_BYTES": "65536"}, lambda: _band(100000, 8, 45000),
                     lambda i, u: i["tile_kind"] == 1 and i["col_tiles"] >= 2),
    "band_tiles": ({}, lambda: _band(250000, 20, 30000), lambda i, u: i["tile_kind"] == 2),
    "stray_split": ({"HISPMV_STRAY_SLOTS": "0"}, lambda: _strays(0.03), lambda i, u: i["tile_kind"] == 3),
    "stray_slots": ({}, lambda: _strays(0.03), lambda i, u: i["tile_kind"] == 0 and i["compact_slices"] == i["n_slices"]),
    "batch_layout": ({"HISPMV_BATCH_MIN_SLICES": "1"}, lambda: _band(400000, 12, 400), lambda i, u: i["batch_group_slices"] > 0 and u["written"] > u["map_slots"]),
    "prep_device": ({"HISPMV_PREP": "device"}, lambda: _band(200000, 12, 400), lambda i, u: i["format"] == 0),
    "layout_device": ({"HISPMV_LAYOUT": "device", "HISPMV_FORMAT": "slices"}, lambda: _strays(0.03), lambda i, u: i["format"] == 0),
}


def _runs(torch, h, idx, rows, cols, x, b, xs):
    """y of run_kernel, linear (3 vectors) and spmv_device (on the context's stream) for handle idx."""
    y = np.full(rows, np.nan, np.float32)
    h.select_matrix(idx)
    h.run_kernel(x, b, y, ALPHA, BETA)
    lin = h.linear(idx, xs, b)
    dev = torch.device("cuda", 0)
    dx, db = torch.from_numpy(x).to(dev), torch.from_numpy(b).to(dev)
    dy = torch.full((rows,), float("nan"), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    h.spmv_device(idx, dx.data_ptr(), db.data_ptr(), dy.data_ptr(), ALPHA, BETA)
    h.synchronize()
    return y, lin, dy.cpu().numpy()


@pytest.mark.parametrize("case", sorted(CASES))
def test_updated_handle_gives_the_bits_of_a_fresh_one(torch_mod, monkeypatch, case):
    env, make, check = CASES[case]
    for k, val in env.items():          # (some switches are read at context creation, others at handle creation: set for the whole test)
        monkeypatch.setenv(k, val)
    r, c = _shuffled_with_duplicates(*make())
    rows = cols = int(max(r.max(), c.max())) + 1
    rng = np.random.default_rng(17)
    v1 = rng.random(r.size, dtype=np.float32) - np.float32(0.5)
    v2 = rng.random(r.size, dtype=np.float32) * np.float32(3.0) - np.float32(1.0)
    x = rng.random(cols, dtype=np.float32) - np.float32(0.3)
    b = rng.random(rows, dtype=np.float32)
    xs = rng.random(3 * cols, dtype=np.float32)
    hu, hp = make_handle(updates=True), make_handle()
    try:
        a = hu.create_sparse_handle(r, c, v1, rows, cols)          # updated to v2 below
        n = hu.create_sparse_handle(r, c, v2, rows, cols)          # updatable, never updated
        p = hp.create_sparse_handle(r, c, v2, rows, cols)          # plain
        hu.load_matrices()
        hp.load_matrices()
        ia, ip = hu.matrix_info(a), hp.matrix_info(p)
        ua = hu.value_update_info(a)
        assert ua["updatable"] and ua["n"] == r.size and ua["map_slots"] > 0 and ua["written"] >= ua["map_slots"]
        assert not hp.value_update_info(p)["updatable"]
        for k in ("format", "tile_kind", "col_tiles", "n_slices", "compact_slices", "block_threads", "group_slices", "lds_bytes", "batch_group_slices"):
            assert ia[k] == ip[k], (k, ia[k], ip[k])
        assert check(ia, ua), (case, ia, ua)
        # the map's arena charge: 4 B per map slot + the chunk table
        assert ia["device_bytes"] - ip["device_bytes"] == 4 * ua["map_slots"] + 24 * (ua["map_slots"] // 1024)
        ref = _runs(torch_mod, hp, p, rows, cols, x, b, xs)
        never = _runs(torch_mod, hu, n, rows, cols, x, b, xs)
        for got, want in zip(never, ref):
            assert same_bits(got, want), f"{case}: updatable handle without an update differs from a plain one"
        hu.update_values(a, v2)
        got = _runs(torch_mod, hu, a, rows, cols, x, b, xs)
        for k, (g, w) in enumerate(zip(got, ref)):
            assert same_bits(g, w), f"{case}: path {k} after the update differs from a fresh handle"
        y64, mag = truth(r, c, v2, rows, x, b, ALPHA, BETA)
        assert bwd_err(got[0], y64, mag) < TOL and bwd_err(got[2], y64, mag) < TOL
        for k in range(3):
            yk64, mk = truth(r, c, v2, rows, xs[k * cols:(k + 1) * cols], b, 1.0, 1.0)
            assert bwd_err(got[1][k * rows:(k + 1) * rows], yk64, mk) < TOL
        # and back again, from device memory this time
        dv1 = torch_mod.from_numpy(v1).to("cuda:0")
        torch_mod.cuda.synchronize()
        hu.update_values_device(a, dv1.data_ptr(), r.size)
        hu.synchronize()
        y = np.full(rows, np.nan, np.float32)
        hu.select_matrix(a)
        hu.run_kernel(x, b, y, ALPHA, BETA)
        y64, mag = truth(r, c, v1, rows, x, b, ALPHA, BETA)
        assert bwd_err(y, y64, mag) < TOL
    finally:
        hu.close()
        hp.close()


def test_csr_input_with_unsorted_rows(torch_mod):
    """_from_csr: values come in the order of col_idx BEFORE the per-row sort."""
    rng = np.random.default_rng(3)
    rows, cols, per = 20000, 30000, 24
    rp = np.arange(rows + 1, dtype=np.int32) * per
    ci = rng.integers(0, cols, rows * per).astype(np.int32)          # unsorted within rows, duplicates possible
    v1 = rng.random(ci.size, dtype=np.float32)
    v2 = rng.random(ci.size, dtype=np.float32) - np.float32(0.5)
    x = rng.random(cols, dtype=np.float32)
    b = rng.random(rows, dtype=np.float32)
    hu, hp = make_handle(updates=True), make_handle()
    try:
        a = hu.create_sparse_handle_from_csr(rp, ci, v1, rows, cols)
        p = hp.create_sparse_handle_from_csr(rp, ci, v2, rows, cols)
        hu.load_matrices()
        hp.load_matrices()
        hu.update_values(a, v2)
        ya, yp = np.zeros(rows, np.float32), np.zeros(rows, np.float32)
        hu.select_matrix(a)
        hu.run_kernel(x, b, ya, ALPHA, BETA)
        hp.select_matrix(p)
        hp.run_kernel(x, b, yp, ALPHA, BETA)
        assert same_bits(ya, yp)
        y64, mag = truth(np.repeat(np.arange(rows, dtype=np.int32), per), ci, v2, rows, x, b, ALPHA, BETA)
        assert bwd_err(ya, y64, mag) < TOL
    finally:
        hu.close()
        hp.close()


def test_dense_handles(torch_mod):
    """A dense handle's update is a copy into its row-major values."""
    rng = np.random.default_rng(5)
    rows, cols = 3000, 2048
    W1 = rng.random((rows, cols), dtype=np.float32) - np.float32(0.5)
    W2 = rng.random((rows, cols), dtype=np.float32) - np.float32(0.5)
    x = rng.random(cols, dtype=np.float32)
    b = rng.random(rows, dtype=np.float32)
    xs = rng.random(4 * cols, dtype=np.float32)
    hu, hp = make_handle(updates=True), make_handle()
    try:
        a = hu.create_dense_handle(W1.reshape(-1), rows, cols)
        p = hp.create_dense_handle(W2.reshape(-1), rows, cols)
        hu.load_matrices()
        hp.load_matrices()
        u = hu.value_update_info(a)
        assert u == {"updatable": True, "n": rows * cols, "map_slots": 0, "written": rows * cols}
        assert hu.matrix_info(a)["device_bytes"] == hp.matrix_info(p)["device_bytes"]
        hu.update_values(a, W2)
        ref, got = _runs(torch_mod, hp, p, rows, cols, x, b, xs), _runs(torch_mod, hu, a, rows, cols, x, b, xs)
        for g, w in zip(got, ref):
            assert same_bits(g, w)
        dW1 = torch_mod.from_numpy(W1.reshape(-1)).to("cuda:0")
        torch_mod.cuda.synchronize()
        hu.update_values_device(a, dW1.data_ptr(), rows * cols)
        y = np.zeros(rows, np.float32)
        hu.select_matrix(a)
        hu.run_kernel(x, b, y, 1.0, 1.0)
        assert np.allclose(y, oracle.naive_gemv(W1, x, b, 1.0, 1.0), rtol=1e-4, atol=1e-5)
    finally:
        hu.close()
        hp.close()


def test_update_is_ordered_on_its_stream(torch_mod):
    """update_values_device, then spmv_device on the same non-default stream, no synchronisation in between: the new values."""
    torch = torch_mod
    r, c = _band(400000, 16, 3000)
    rows = cols = 400000
    rng = np.random.default_rng(9)
    v1 = rng.random(r.size, dtype=np.float32)
    v2 = rng.random(r.size, dtype=np.float32) - np.float32(0.5)
    x = rng.random(cols, dtype=np.float32)
    b = rng.random(rows, dtype=np.float32)
    h = make_handle(updates=True)
    try:
        a = h.create_sparse_handle(r, c, v1, rows, cols)
        h.load_matrices()
        dev = torch.device("cuda", 0)
        s = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(s):
            dx, db = torch.from_numpy(x).to(dev), torch.from_numpy(b).to(dev)
            dy = torch.full((rows,), float("nan"), dtype=torch.float32, device=dev)
            dv = torch.from_numpy(v2).to(dev)
            for _ in range(3):         # old, new, old, new ... all queued on s
                h.spmv_device(a, dx.data_ptr(), db.data_ptr(), dy.data_ptr(), ALPHA, BETA, s.cuda_stream)
            h.update_values_device(a, dv.data_ptr(), r.size, s.cuda_stream)
            h.spmv_device(a, dx.data_ptr(), db.data_ptr(), dy.data_ptr(), ALPHA, BETA, s.cuda_stream)
            y = dy.cpu()                # (on s: the copy is ordered behind the launches)
        s.synchronize()
        h.synchronize()
        y64, mag = truth(r, c, v2, rows, x, b, ALPHA, BETA)
        assert bwd_err(y.numpy(), y64, mag) < TOL
    finally:
        h.close()


@pytest.fixture(scope="module")
def set20():
    from hispmv_amd import matrices as M
    mats = [m for m in M.benchmark_set() if "rp" in m]
    assert len(mats) >= 20
    return mats[:20]


def _batch_run(torch, h, idx, mats, batch_state, reps=1):
    dev = torch.device("cuda", 0)
    if batch_state.get("batch") is None:
        dx, db, dy = [], [], []
        for m in mats:
            rng = np.random.default_rng(m["rows"])
            dx.append(torch.from_numpy(rng.random(m["cols"], dtype=np.float32)).to(dev))
            db.append(torch.from_numpy(rng.random(m["rows"], dtype=np.float32)).to(dev))
            dy.append(torch.full((m["rows"],), float("nan"), dtype=torch.float32, device=dev))
        batch_state.update(dx=dx, db=db, dy=dy,
                           batch=h.prepare_batch(idx, [t.data_ptr() for t in dx], [t.data_ptr() for t in db], [t.data_ptr() for t in dy]))
    for _ in range(reps):
        torch.cuda.synchronize()
        h.spmv_device_batch(batch_state["batch"], ALPHA, BETA)
        h.synchronize()
    return [t.cpu().numpy() for t in batch_state["dy"]]


def _new_values(m):
    return (np.random.default_rng(m["nnz"]).random(m["nnz"], dtype=np.float32) - np.float32(0.5))


@pytest.mark.parametrize("graph", ["0", "1"])
def test_batch_keeps_its_plan_across_updates(torch_mod, set20, graph):
    """20 matrices of the benchmark set in one batch call, 6 of them updated, the SAME prepared batch run again: every y equals a
    fresh context built from the new values; by default the step kernel runs the call before and after, under HISPMV_BATCH_GRAPH=1
    (the grids captured into a graph) no graph is instantiated again."""
    env = {"HISPMV_BATCH_GRAPH": graph}
    upd = [0, 3, 7, 11, 15, 19]
    hu, hp = make_handle(env, updates=True), make_handle(env)
    try:
        iu = [hu.create_sparse_handle_from_csr(m["rp"], m["ci"], m["va"], m["rows"], m["cols"]) for m in set20]
        ip = [hp.create_sparse_handle_from_csr(m["rp"], m["ci"], _new_values(m) if k in upd else m["va"], m["rows"], m["cols"])
              for k, m in enumerate(set20)]
        assert min(iu) >= 0 and min(ip) >= 0
        hu.load_matrices()
        hp.load_matrices()
        su, sp = {}, {}
        before = _batch_run(torch_mod, hu, iu, set20, su, reps=2)       # (HISPMV_BATCH_GRAPH=1: the second call is captured)
        assert hu.batch_call_info()["step_kernel"] == (graph == "0")
        inst = hu.batch_graph_stats()["instantiations"]
        assert inst >= (1 if graph == "1" else 0)
        for k in upd:
            hu.update_values(iu[k], _new_values(set20[k]))
        after = _batch_run(torch_mod, hu, iu, set20, su)
        assert hu.batch_call_info()["step_kernel"] == (graph == "0")
        assert hu.batch_graph_stats()["instantiations"] == inst
        ref = _batch_run(torch_mod, hp, ip, set20, sp)
        for k, m in enumerate(set20):
            assert np.all(np.isfinite(after[k])), m["name"]
            assert same_bits(after[k], ref[k]), f'{m["name"]}: batch after the update differs from a fresh handle'
            if k not in upd:
                assert same_bits(before[k], after[k]), m["name"]
    finally:
        hu.close()
        hp.close()


def test_error_contract_and_arena(torch_mod, tmp_path):
    from hispmv_amd import matrices as M
    r, c = _band(50000, 8, 200)
    rows = cols = 50000
    v = np.random.default_rng(1).random(r.size, dtype=np.float32)
    h = make_handle(updates=True)
    try:
        a = h.create_sparse_handle(r, c, v, rows, cols)
        with pytest.raises(AssertionError, match="load"):
            h.update_values(a, v)                                    # not loaded yet (HISPMV_ESTATE)
        h.set_value_updates(False)
        p = h.create_sparse_handle(r, c, v, rows, cols)              # plain again: same bytes as a plain context's
        h.set_value_updates(True)
        h.load_matrices()
        assert not h.value_update_info(p)["updatable"]
        with pytest.raises(AssertionError):
            h.update_values(p, v)                                    # not updatable (HISPMV_ESTATE)
        with pytest.raises(ValueError):
            h.update_values(a, v[:-1])                               # wrong n
        with pytest.raises(IndexError):
            h.update_values(5, v)                                    # bad index
        with pytest.raises(IndexError):
            h.value_update_info(-1)
        with pytest.raises(ValueError):
            h.update_values_device(a, 0, r.size)                     # NULL device pointer
        path = tmp_path / "m.mtx"
        M.write_mtx(path, rows, cols, r[:1000], c[:1000], v[:1000])
        with pytest.raises(ValueError, match="MatrixMarket"):
            h.create_sparse_handle_from_mtx(str(path))
        # arena: the map counts; -1 when only the map no longer fits
        ia, ip = h.matrix_info(a), h.matrix_info(p)
        assert ia["device_bytes"] > ip["device_bytes"]
        assert h.arena_bytes_used() == ia["device_bytes"] + ip["device_bytes"]
    finally:
        h.close()
    h = make_handle(updates=True, arena=ip["device_bytes"])
    try:
        assert h.create_sparse_handle(r, c, v, rows, cols) == -1
        h.set_value_updates(False)
        assert h.create_sparse_handle(r, c, v, rows, cols) == 0
    finally:
        h.close()
    # the experiment geometries of the tile stream are refused at creation
    h = make_handle({"HISPMV_TTS_GEOMETRY": "tall"}, updates=True)
    try:
        with pytest.raises(ValueError, match="experiment"):
            h.create_sparse_handle(r, c, v, rows, cols)
    finally:
        h.close()
