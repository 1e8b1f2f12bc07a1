"""bf16 value storage on the MI355X (hispmv_set_value_storage, hispmv_value_storage_info).

The central check needs no tolerance: a bf16 handle created from values v gives, BIT FOR BIT, the y of an fp32 handle created in a
second context under the same switches from the pre-rounded values R(v) -- same plan, same operands, same order -- for every
format and variant the loader can choose, through run_kernel, linear with 3 and 5 vectors, spmv_device and spmv_device_batch (a
bf16 sparse, an fp32 sparse and a dense handle in one call; step kernel at its default and HISPMV_STEP_KERNEL=0).  R is CPU
torch's v.to(bfloat16).to(float32).  Dense handles (the lane-to-column assignment of the bf16 GeMV differs from the fp32 one): the
1e-5 gate against fp64 of R(W), and linear / the multi-matrix grid bitwise equal to the single launch.  Bookkeeping: device bytes,
arena, the refusal next to value updates.  One timing assertion: where the bytes shrink, the bf16 handle is faster."""
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


def R(v):
    import torch
    v = np.ascontiguousarray(v, np.float32)
    return torch.from_numpy(v).to(torch.bfloat16).to(torch.float32).numpy()


def make_handle(env=None, storage="fp32", arena=64 << 30):
    """An FpgaHandle created under `env` (the switches are read when the context is created) with the given value storage."""
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
    h.set_value_storage(storage)
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


def _mixed(rows=100000):
    """The mixed matrix of tests/test_value_storage_host.py: stray couplings in the first third of the rows only."""
    r, c = _band(rows, 16, 1500)
    far = (np.random.default_rng(5).random(c.size) < 0.2) & (r < rows / 3)
    return r, np.where(far, np.random.default_rng(6).integers(0, rows, c.size), c).astype(np.int32)


def _shuffled_with_duplicates(r, c, seed=1):
    """Input order differs from CSR order, and some coordinates come twice (duplicates are summed, not coalesced)."""
    rng = np.random.default_rng(seed)
    dup = rng.integers(0, r.size, r.size // 50)
    r, c = np.concatenate([r, r[dup]]), np.concatenate([c, c[dup]])
    p = rng.permutation(r.size)
    return r[p], c[p]


# name -> (env, matrix, check on matrix_info, 2-byte slots expected): the table of tests/test_gpu_value_updates.py (its batch_layout
# predicate without the value-map term: these handles are not updatable), plus compact and wide groups in one launch and the look-back carry
CASES = {
    "slices_compact": ({}, lambda: _band(200000, 12, 400), lambda i: i["format"] == 0 and i["col_tiles"] == 1 and i["compact_slices"] > 0),
    "slices_wide": ({"HISPMV_FORMAT": "slices"}, lambda: _band(100000, 8, 45000), lambda i: i["format"] == 0 and i["compact_slices"] < i["n_slices"]),
    "plan_global": ({"HISPMV_FORMAT": "slices", "HISPMV_PLAN": "global"}, lambda: _band(200000, 12, 400), lambda i: i["format"] == 0),
    "tile_stream": ({"HISPMV_FORMAT": "tts"}, lambda: _band(100000, 8, 45000), lambda i: i["format"] == 1),
    "column_tiles": ({"HISPMV_FORMAT": "slices", "HISPMV_BAND_TILES": "0", "HISPMV_COL_TILE_BYTES": "65536"}, lambda: _band(100000, 8, 45000),
                     lambda i: i["tile_kind"] == 1 and i["col_tiles"] >= 2),
    "band_tiles": ({}, lambda: _band(250000, 20, 30000), lambda i: i["tile_kind"] == 2),
    "stray_split": ({"HISPMV_STRAY_SLOTS": "0"}, lambda: _strays(0.03), lambda i: i["tile_kind"] == 3),
    "stray_slots": ({}, lambda: _strays(0.03), lambda i: i["tile_kind"] == 0 and i["compact_slices"] == i["n_slices"]),
    "batch_layout": ({"HISPMV_BATCH_MIN_SLICES": "1"}, lambda: _band(400000, 12, 400), lambda i: i["batch_group_slices"] > 0),
    "prep_device": ({"HISPMV_PREP": "device"}, lambda: _band(200000, 12, 400), lambda i: i["format"] == 0),
    "layout_device": ({"HISPMV_LAYOUT": "device", "HISPMV_FORMAT": "slices"}, lambda: _strays(0.03), lambda i: i["format"] == 0),
    "mixed_groups": ({"HISPMV_STRAY_SPLIT": "0"}, _mixed, lambda i: 0 < i["compact_slices"] < i["n_slices"]),
    "lookback_carry": ({"HISPMV_CARRY": "lookback"}, lambda: _band(200000, 12, 400), lambda i: i["carry_lookback"] == 1 and i["compact_slices"] > 0),
}
NO_HALF = {"tile_stream", "plan_global"}


def _runs(torch, h, idx, rows, cols, x, b, xs3, xs5):
    """y of run_kernel, linear (3 and 5 vectors) and spmv_device (on the context's stream) for handle idx."""
    y = np.full(rows, np.nan, np.float32)
    h.select_matrix(idx)
    h.run_kernel(x, b, y, ALPHA, BETA)
    lin3, lin5 = h.linear(idx, xs3, b), h.linear(idx, xs5, b)
    dev = torch.device("cuda", 0)
    dx, db = torch.from_numpy(x).to(dev), torch.from_numpy(b).to(dev)
    dy = torch.full((rows,), float("nan"), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    h.spmv_device(idx, dx.data_ptr(), db.data_ptr(), dy.data_ptr(), ALPHA, BETA)
    h.synchronize()
    return y, lin3, lin5, dy.cpu().numpy()


def _batch(torch, h, idx, shapes, vecs):
    """One spmv_device_batch call over the handles idx -> their y."""
    dev = torch.device("cuda", 0)
    dx = [torch.from_numpy(x).to(dev) for x, _ in vecs]
    db = [torch.from_numpy(b).to(dev) for _, b in vecs]
    dy = [torch.full((rows,), float("nan"), dtype=torch.float32, device=dev) for rows, _ in shapes]
    batch = h.prepare_batch(idx, [t.data_ptr() for t in dx], [t.data_ptr() for t in db], [t.data_ptr() for t in dy])
    for _ in range(2):                   # (the second call replays the cached plan)
        torch.cuda.synchronize()
        h.spmv_device_batch(batch, ALPHA, BETA)
        h.synchronize()
    return [t.cpu().numpy() for t in dy], h.batch_call_info()


# the companions of the batch call: an fp32 sparse handle and a dense one
def _companions():
    rng = np.random.default_rng(23)
    r2, c2 = _band(60000, 10, 300, seed=4)
    v2 = rng.random(r2.size, dtype=np.float32) - np.float32(0.5)
    W = rng.random((512, 1024), dtype=np.float32) - np.float32(0.5)
    return (r2, c2, v2, 60000), W


@pytest.mark.parametrize("case", sorted(CASES))
def test_bf16_handle_gives_the_bits_of_an_fp32_handle_of_the_rounded_values(torch_mod, monkeypatch, case):
    env, make, check = CASES[case]
    for k, val in env.items():          # (some switches are read at context creation, others at handle creation: set for the whole test)
        monkeypatch.setenv(k, val)
    r, c = _shuffled_with_duplicates(*make())
    rows = cols = int(max(r.max(), c.max())) + 1
    rng = np.random.default_rng(17)
    v = rng.random(r.size, dtype=np.float32) - np.float32(0.5)
    rv = R(v)
    assert not np.array_equal(v, rv)
    x = rng.random(cols, dtype=np.float32) - np.float32(0.3)
    b = rng.random(rows, dtype=np.float32)
    xs3, xs5 = rng.random(3 * cols, dtype=np.float32), rng.random(5 * cols, dtype=np.float32)
    (r2, c2, v2, n2), W = _companions()
    x2, b2 = rng.random(n2, dtype=np.float32), rng.random(n2, dtype=np.float32)
    x3, b3 = rng.random(W.shape[1], dtype=np.float32), rng.random(W.shape[0], dtype=np.float32)
    shapes = [(rows, cols), (n2, n2), W.shape]
    vecs = [(x, b), (x2, b2), (x3, b3)]
    hb, hf, hb0 = make_handle(storage="bf16"), make_handle(), make_handle({"HISPMV_STEP_KERNEL": "0"}, storage="bf16")
    try:
        def fill(h, vals):
            a = h.create_sparse_handle(r, c, vals, rows, cols)
            h.set_value_storage("fp32")             # one context holds both kinds
            q = h.create_sparse_handle(r2, c2, v2, n2, n2)
            d = h.create_dense_handle(W.reshape(-1), *W.shape)
            return [a, q, d]
        ib, i0, i_f = fill(hb, v), fill(hb0, v), fill(hf, rv)
        u = hf.create_sparse_handle(r, c, v, rows, cols)          # fp32 storage of the unrounded values
        assert min(ib + i0 + i_f + [u]) >= 0
        for h in (hb, hf, hb0):
            h.load_matrices()
        a, p = ib[0], i_f[0]
        ia, ip = hb.matrix_info(a), hf.matrix_info(p)
        # same plan, whatever the storage
        for k in ("format", "tile_kind", "col_tiles", "n_slices", "n_elems", "n_split_rows", "compact_slices", "block_threads", "group_slices", "lds_bytes",
                  "batch_group_slices", "carry_lookback", "col_tile_width", "col_tile_base"):
            assert ia[k] == ip[k], (k, ia[k], ip[k])
        assert check(ia), (case, ia)
        sa, sp, sq = hb.value_storage_info(a), hf.value_storage_info(p), hb.value_storage_info(ib[1])
        print(case, ia, sa)
        assert sa["storage"] == "bf16" and sp["storage"] == "fp32" and sq["storage"] == "fp32"
        assert (sa["slots_2byte"] > 0) == (ia["compact_slices"] > 0), (sa, ia["compact_slices"])
        if case in NO_HALF:
            assert sa["slots_2byte"] == 0 and sa["saved_bytes"] == 0
        copies = 2 if ia["batch_group_slices"] > 0 else 1
        assert sa["slots_2byte"] == 1024 * ia["compact_slices"] * copies and sa["saved_bytes"] == 2 * sa["slots_2byte"]
        assert sa["slots_2byte"] + sa["slots_4byte"] == sp["slots_4byte"] and sp["slots_2byte"] == 0 and sp["saved_bytes"] == 0
        assert ia["device_bytes"] == ip["device_bytes"] - sa["saved_bytes"]
        assert hf.arena_bytes_used() - hb.arena_bytes_used() == hf.matrix_info(u)["device_bytes"] + sa["saved_bytes"]

        ref = _runs(torch_mod, hf, p, rows, cols, x, b, xs3, xs5)
        got = _runs(torch_mod, hb, a, rows, cols, x, b, xs3, xs5)
        for k, (g, w) in enumerate(zip(got, ref)):
            assert np.all(np.isfinite(g)), (case, k)
            assert same_bits(g, w), f"{case}: path {k} of the bf16 handle differs from the fp32 handle of the rounded values"
        # the gate against fp64, with the truth computed from R(v)
        y64, mag = truth(r, c, rv, rows, x, b, ALPHA, BETA)
        assert bwd_err(got[0], y64, mag) < TOL and bwd_err(got[3], y64, mag) < TOL
        for xs, lin in ((xs3, got[1]), (xs5, got[2])):
            for k in range(xs.size // cols):
                yk64, mk = truth(r, c, rv, rows, xs[k * cols:(k + 1) * cols], b, 1.0, 1.0)
                assert bwd_err(lin[k * rows:(k + 1) * rows], yk64, mk) < TOL
        # the rounding really happened
        y_unrounded = np.full(rows, np.nan, np.float32)
        hf.select_matrix(u)
        hf.run_kernel(x, b, y_unrounded, ALPHA, BETA)
        assert not same_bits(got[0], y_unrounded)

        # bf16 sparse + fp32 sparse + dense in one batch call
        want, _ = _batch(torch_mod, hf, i_f, shapes, vecs)
        for h, idx, name in ((hb, ib, "step kernel at its default"), (hb0, i0, "HISPMV_STEP_KERNEL=0")):
            out, info = _batch(torch_mod, h, idx, shapes, vecs)
            if ia["compact_slices"] > 0:
                assert not info["step_kernel"], "a call with half groups runs as separate grids"
            for k in range(3):
                assert same_bits(out[k], want[k]), f"{case}: matrix {k} of the batch call ({name}) differs"
        assert bwd_err(want[0], y64, mag) < TOL
    finally:
        for h in (hb, hf, hb0):
            h.close()
    from hispmv_amd._lib import lib
    assert lib.hispmv_free_failures() == 0


def test_a_call_that_qualifies_for_the_step_kernel_runs_as_grids_once_it_holds_half_groups(torch_mod, monkeypatch):
    """Sparse handles only, 1024- and 256-thread plans, HISPMV_BATCH_STREAMS=2 (the shared-chip threshold drops to 0, as in
    tests/test_gpu_step_small.py): the all-fp32 call provably takes the step kernel -- with the batch layouts -- and the same call
    with two bf16 handles in it (one with stray slots and a batch layout, one with a 256-thread plan) must not: the step kernel has
    no body for half groups.  It is planned again from the first layouts and runs as grids on two lanes, the bits of the fp32
    context of R(v)."""
    for k, val in {"HISPMV_BATCH_STREAMS": "2", "HISPMV_BATCH_MIN_SLICES": "1"}.items():
        monkeypatch.setenv(k, val)
    mats = [_strays(0.03), _band(400000, 12, 400), _band(200000, 12, 400)]
    bf16 = [True, False, True]
    rng = np.random.default_rng(29)
    vals = [rng.random(r.size, dtype=np.float32) - np.float32(0.5) for r, _ in mats]
    dims = [int(max(r.max(), c.max())) + 1 for r, c in mats]
    vecs = [(rng.random(n, dtype=np.float32) - np.float32(0.3), rng.random(n, dtype=np.float32)) for n in dims]
    shapes = [(n, n) for n in dims]
    hb, hf = make_handle(), make_handle()
    try:
        ib, i_f = [], []
        for (r, c), v, n, half in zip(mats, vals, dims, bf16):
            hb.set_value_storage("bf16" if half else "fp32")
            ib.append(hb.create_sparse_handle(r, c, v, n, n))
            i_f.append(hf.create_sparse_handle(r, c, R(v) if half else v, n, n))
        assert min(ib + i_f) >= 0
        hb.load_matrices()
        hf.load_matrices()
        infos = [hf.matrix_info(i) for i in i_f]
        assert [i["block_threads"] for i in infos] == [1024, 1024, 256] and all(i["format"] == 0 and i["col_tiles"] == 1 for i in infos), infos
        assert infos[0]["batch_group_slices"] > 0 and infos[0]["compact_slices"] == infos[0]["n_slices"]
        for k, (a, p) in enumerate(zip(ib, i_f)):
            assert (hb.value_storage_info(a)["slots_2byte"] > 0) == bf16[k]
            for key in ("n_slices", "compact_slices", "block_threads", "group_slices", "lds_bytes", "batch_group_slices"):
                assert hb.matrix_info(a)[key] == hf.matrix_info(p)[key], (k, key)
        want, info_f = _batch(torch_mod, hf, i_f, shapes, vecs)
        assert info_f["step_kernel"], ("the all-fp32 call must qualify for the step kernel", info_f)
        got, info_b = _batch(torch_mod, hb, ib, shapes, vecs)
        print("fp32 call", info_f, "call with half groups", info_b)
        assert not info_b["step_kernel"], info_b
        assert info_b["launches"] > info_f["launches"]
        for k, ((r, c), v, n) in enumerate(zip(mats, vals, dims)):
            assert np.all(np.isfinite(got[k])), k
            assert same_bits(got[k], want[k]), f"matrix {k} of the call with half groups differs from the step kernel's fp32 result"
            y64, mag = truth(r, c, R(v) if bf16[k] else v, n, vecs[k][0], vecs[k][1], ALPHA, BETA)
            assert bwd_err(got[k], y64, mag) < TOL
        # the C entry refuses an unknown storage on a live context and keeps the setting
        from hispmv_amd import _lib
        assert _lib.lib.hispmv_set_value_storage(hb._ctx, 7) == _lib.HISPMV_EINVAL
        assert b"storage" in _lib.lib.hispmv_last_error(hb._ctx)
    finally:
        hb.close()
        hf.close()
    from hispmv_amd._lib import lib
    assert lib.hispmv_free_failures() == 0


def _dense_truth(W, x, b, alpha, beta):
    W64, x64 = W.astype(np.float64), x.astype(np.float64)
    return alpha * (W64 @ x64) + beta * b.astype(np.float64), abs(alpha) * (np.abs(W64) @ np.abs(x64)) + np.abs(beta * b.astype(np.float64))


@pytest.mark.parametrize("shape", [(1024, 8192), (1000, 1003), (1000, 1004)])
def test_dense_bf16(torch_mod, shape):
    torch = torch_mod
    rows, cols = shape
    rng = np.random.default_rng(5)
    W = rng.random((rows, cols), dtype=np.float32) - np.float32(0.5)
    W2 = rng.random((300, 520), dtype=np.float32) - np.float32(0.5)
    x = rng.random(cols, dtype=np.float32) - np.float32(0.3)
    b = rng.random(rows, dtype=np.float32)
    h = make_handle(storage="bf16")
    try:
        d = h.create_dense_handle(W.reshape(-1), rows, cols)
        h.set_value_storage("fp32")
        f = h.create_dense_handle(W2.reshape(-1), *W2.shape)          # an fp32 entry for the multi-matrix grid
        h.set_value_storage("bf16")
        e = h.create_dense_handle(W2.reshape(-1), *W2.shape)
        h.load_matrices()
        s = h.value_storage_info(d)
        assert s == {"storage": "bf16", "slots_2byte": rows * cols, "slots_4byte": 0, "saved_bytes": 2 * rows * cols}
        assert h.matrix_info(d)["device_bytes"] == 2 * rows * cols and h.matrix_info(f)["device_bytes"] == 2 * h.matrix_info(e)["device_bytes"]
        assert h.arena_bytes_used() == 2 * rows * cols + 6 * W2.size
        y = np.full(rows, np.nan, np.float32)
        h.select_matrix(d)
        h.run_kernel(x, b, y, ALPHA, BETA)
        y64, mag = _dense_truth(R(W), x, b, ALPHA, BETA)
        assert bwd_err(y, y64, mag) < TOL
        y_fp32 = oracle.naive_gemv(W, x, b, ALPHA, BETA)
        assert not same_bits(y, y_fp32), "the rounding really happened"
        # linear: every vector has the bits of the single launch, however many vectors share a pass over W
        for n in (1, 2, 3, 8, 9):
            xs = np.random.default_rng(100 + n).random(n * cols, dtype=np.float32)
            lin = h.linear(d, xs, b)
            for k in range(n):
                xk = xs[k * cols:(k + 1) * cols]
                yk = np.full(rows, np.nan, np.float32)
                h.run_kernel(xk, b, yk, 1.0, 1.0)
                assert same_bits(lin[k * rows:(k + 1) * rows], yk), (n, k)
                yk64, mk = _dense_truth(R(W), xk, b, 1.0, 1.0)
                assert bwd_err(yk, yk64, mk) < TOL
        # the multi-matrix grid: bf16 and fp32 entries in one launch, each with the bits of its single launch
        dev = torch.device("cuda", 0)
        x2 = rng.random(W2.shape[1], dtype=np.float32)
        b2 = rng.random(W2.shape[0], dtype=np.float32)
        idx = [d, f, e]
        xs_, bs_ = [x, x2, x2], [b, b2, b2]
        dx = [torch.from_numpy(t).to(dev) for t in xs_]
        db = [torch.from_numpy(t).to(dev) for t in bs_]
        dy = [torch.full((t.size,), float("nan"), dtype=torch.float32, device=dev) for t in bs_]
        torch.cuda.synchronize()
        h.spmv_device_batch(h.prepare_batch(idx, [t.data_ptr() for t in dx], [t.data_ptr() for t in db], [t.data_ptr() for t in dy]), ALPHA, BETA)
        h.synchronize()
        for k, i in enumerate(idx):
            yk = np.full(bs_[k].size, np.nan, np.float32)
            h.select_matrix(i)
            h.run_kernel(xs_[k], bs_[k], yk, ALPHA, BETA)
            assert same_bits(dy[k].cpu().numpy(), yk), k
        y64, mag = _dense_truth(R(W2), x2, b2, ALPHA, BETA)
        assert bwd_err(dy[2].cpu().numpy(), y64, mag) < TOL
        y64, mag = _dense_truth(W2, x2, b2, ALPHA, BETA)
        assert bwd_err(dy[1].cpu().numpy(), y64, mag) < TOL
    finally:
        h.close()
    from hispmv_amd._lib import lib
    assert lib.hispmv_free_failures() == 0


def test_bookkeeping_arena_and_the_refusal_next_to_value_updates(torch_mod, tmp_path):
    from hispmv_amd import matrices as M
    r, c = _band(200000, 12, 400)
    rows = cols = 200000
    v = np.random.default_rng(1).random(r.size, dtype=np.float32) + np.float32(0.25)
    nm, km = 8500, 96000                   # a small matrix for the MatrixMarket entry point (its reader drops zeros: none here)
    h = make_handle()
    try:
        with pytest.raises(ValueError):
            h.set_value_storage("fp16")
        f = h.create_sparse_handle(r, c, v, rows, cols)
        used_f = h.arena_bytes_used()
        h.set_value_storage("bf16")
        a = h.create_sparse_handle(r, c, v, rows, cols)
        path = tmp_path / "m.mtx"
        M.write_mtx(path, nm, nm, r[:km], c[:km], v[:km])
        m = h.create_sparse_handle_from_mtx(str(path))          # the MatrixMarket entry point honours the switch too
        sa, sm = h.value_storage_info(a), h.value_storage_info(m)
        assert sa["storage"] == "bf16" and sa["saved_bytes"] > 0 and sm["storage"] == "bf16"
        bytes_f, bytes_a = h.matrix_info(f)["device_bytes"], h.matrix_info(a)["device_bytes"]
        assert bytes_f == used_f and bytes_a == bytes_f - sa["saved_bytes"]
        assert h.arena_bytes_used() == bytes_f + bytes_a + h.matrix_info(m)["device_bytes"]
        with pytest.raises(IndexError):
            h.value_storage_info(7)
        # both switches on: refused with a message that says so, for every entry point; the context stays usable
        h.set_value_updates(True)
        order = np.lexsort((c, r))
        rp = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=rows))]).astype(np.int32)
        for create in (lambda: h.create_sparse_handle(r, c, v, rows, cols),
                       lambda: h.create_sparse_handle_from_csr(rp, c[order], v[order], rows, cols),
                       lambda: h.create_dense_handle(np.ones(64, np.float32), 8, 8)):
            with pytest.raises(ValueError, match="value updates"):
                create()
        assert h.num_matrices() == 3
        h.set_value_updates(False)
        h.load_matrices()
        x, b = np.random.default_rng(2).random(cols, dtype=np.float32), np.zeros(rows, np.float32)
        ya, ym = np.full(rows, np.nan, np.float32), np.full(nm, np.nan, np.float32)
        h.select_matrix(a)
        h.run_kernel(x, b, ya, 1.0, 0.0)
        h.select_matrix(m)
        h.run_kernel(x[:nm], b[:nm], ym, 1.0, 0.0)
        y64, mag = truth(r, c, R(v), rows, x, b, 1.0, 0.0)
        assert bwd_err(ya, y64, mag) < TOL
        y64, mag = truth(r[:km], c[:km], R(v[:km]), nm, x[:nm], b[:nm], 1.0, 0.0)
        assert bwd_err(ym, y64, mag) < TOL
        y64, mag = truth(r[:km], c[:km], v[:km], nm, x[:nm], b[:nm], 1.0, 0.0)
        assert bwd_err(ym, y64, mag) > TOL, "the MatrixMarket handle holds rounded values"
    finally:
        h.close()
    # an arena sized between the two accepts the bf16 handle and is full for the fp32 one
    h = make_handle(arena=(bytes_f + bytes_a) // 2)
    try:
        assert h.create_sparse_handle(r, c, v, rows, cols) == -1
        h.set_value_storage("bf16")
        assert h.create_sparse_handle(r, c, v, rows, cols) == 0
        assert h.arena_bytes_used() == bytes_a
    finally:
        h.close()
    from hispmv_amd._lib import lib
    assert lib.hispmv_free_failures() == 0


def _alternated_medians(torch, h, i_fp32, i_bf16, rows, cols, rounds=7, reps=20):
    dev = torch.device("cuda", 0)
    dx = torch.rand(cols, dtype=torch.float32, device=dev)
    db = torch.rand(rows, dtype=torch.float32, device=dev)
    dy = torch.empty(rows, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    t = {i_fp32: [], i_bf16: []}
    for i in (i_fp32, i_bf16):
        h.time_device(i, dx.data_ptr(), db.data_ptr(), dy.data_ptr(), 1.0, 1.0, 3)       # warm-up
    for _ in range(rounds):
        for i in (i_fp32, i_bf16):
            t[i].append(h.time_device(i, dx.data_ptr(), db.data_ptr(), dy.data_ptr(), 1.0, 1.0, reps))
    return float(np.median(t[i_fp32])), float(np.median(t[i_bf16])), t


def test_bf16_is_faster_where_the_bytes_shrink(torch_mod):
    """Median device time of the bf16 handle < that of the fp32 handle, alternated in one process, on an all-compact band matrix
    whose fp32 stream (>= 512 MiB) does not stay in the last-level cache, and on the 8192 x 4096 dense layer of examples/model_check.py."""
    rows = 6000000
    r, c = _band(rows, 16, 400)
    rng = np.random.default_rng(3)
    v = rng.random(r.size, dtype=np.float32) - np.float32(0.5)
    W = rng.random((8192, 4096), dtype=np.float32) - np.float32(0.5)
    h = make_handle()
    try:
        f = h.create_sparse_handle(r, c, v, rows, rows)
        fd = h.create_dense_handle(W.reshape(-1), *W.shape)
        h.set_value_storage("bf16")
        a = h.create_sparse_handle(r, c, v, rows, rows)
        ad = h.create_dense_handle(W.reshape(-1), *W.shape)
        h.load_matrices()
        i_f, s = h.matrix_info(f), h.value_storage_info(a)
        assert i_f["compact_slices"] == i_f["n_slices"] and i_f["col_tiles"] == 1 and 6144 * i_f["n_slices"] >= 512 << 20, i_f
        assert s["slots_2byte"] == 1024 * i_f["n_slices"] and s["slots_4byte"] == 0
        m_f, m_a, t = _alternated_medians(torch_mod, h, f, a, rows, rows)
        print(f"band {rows} x 16: fp32 {m_f * 1e3:.1f} us, bf16 {m_a * 1e3:.1f} us, ratio {m_a / m_f:.3f} (byte ratio 4/6); rounds {t}")
        d_f, d_a, t = _alternated_medians(torch_mod, h, fd, ad, *W.shape, reps=50)
        print(f"dense 8192 x 4096: fp32 {d_f * 1e3:.1f} us, bf16 {d_a * 1e3:.1f} us, ratio {d_a / d_f:.3f} (byte ratio 1/2); rounds {t}")
        assert m_a < m_f
        assert d_a < d_f
    finally:
        h.close()
