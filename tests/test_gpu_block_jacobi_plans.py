"""The block-Jacobi extraction (include/hispmv.h: hispmv_block_jacobi_extract_device, _setup_device) on every slice plan the header
promises -- compact, half and wide groups under a window, stray slots, 256 and 1024 threads, column tiles, band tiles, both parts of a
stray split, fp32 and bf16 storage -- on dense handles whose n is no multiple of the block size, after value updates, and on the handle
states of set_transposable.  The inputs and the plan each exists for: tests/block_jacobi_plan_cases.py (checked on the host by
tests/test_block_jacobi_plans_host.py, and here again from matrix_info of the loaded handle).

Every comparison is exact against tests/block_jacobi_model.py; there is no tolerance in this module.

  plan        matrix_info, block_jacobi_info and value_storage_info of the loaded handle show the plan the case is named for
  extraction  the block area equals the model's padded blocks of the STORED values by == (NaN where the model holds NaN and nowhere
              else); the flag area and 4096 guard bytes behind the buffer keep their fill; a second call gives the same bits
  setup       blocks and flags bit for bit the model's inversion of the model's blocks; holes_1024: the flagged blocks are the ones
              the case names, each the identity
  apply       block size 8: the front end's multiply bit for bit the model's
  updates     update_values_device with fresh values (a bf16 handle rounds them on the device), then the blocks of the new values
  dense       n = 1, 3, 33, 97, 130, fp32 and bf16
  states      set_transposable(True) on a would-be tile stream, "companion", "keep_format"
"""
import numpy as np
import pytest
import scipy.sparse as sp

import block_jacobi_model as bj
import block_jacobi_plan_cases as P
import step_small_cases as S
from block_jacobi_harness import Ctx, bits
from hispmv_amd import prep

pytestmark = pytest.mark.gpu

f32 = np.float32
GUARD = 4096
FILL = 0xCD


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


# ---- the contexts: one per (switches, storage), with all of its cases loaded once ------------------------------------------------------
def _contexts():
    out = {}
    for name, case in P.CASES.items():
        for storage in case["storages"]:
            key = (tuple(sorted(case["env"].items())), storage)
            out.setdefault(key, []).append(name)
    return out


CONTEXTS = _contexts()
SWEEP = [(key, name, bs) for key in sorted(CONTEXTS) for name in CONTEXTS[key] for bs in bj.SIZES]          # grouped by context


def _id(p):
    key, name, bs = p
    return f"{name}-{key[1]}-bs{bs}"


class Contexts:
    """The context of a key, created when the sweep reaches it and closed when it moves on (the sweep is grouped by key)."""

    def __init__(self, torch):
        self.torch, self.key, self.cx = torch, None, None

    def get(self, key):
        if key != self.key:
            self.close()
            env, storage = dict(key[0]), key[1]
            self.cx = Ctx(self.torch, [P.matrix(name) for name in CONTEXTS[key]], env=env, storage=storage)
            self.key = key
        return self.cx

    def close(self):
        if self.cx is not None:
            self.cx.__exit__()
        self.key, self.cx = None, None


@pytest.fixture(scope="module")
def contexts(torch_mod):
    c = Contexts(torch_mod)
    yield c
    c.close()


# ---- the calls and the comparisons --------------------------------------------------------------------------------------------------------
def run(cx, idx, n, bs, call, status=False):
    """`call` (the extraction or the setup) into a fresh buffer of pre_bytes + GUARD bytes of FILL, told pre_bytes.
    -> (blocks [n_blocks, bs, bs], the flag area up to pre_bytes as bytes, the guard as bytes[, block_jacobi_status of the buffer])"""
    torch = cx.torch
    l = bj.layout(n, bs)
    assert l == prep.block_jacobi(n, bs)
    buf = torch.full((l["pre_bytes"] + GUARD,), FILL, dtype=torch.uint8, device=cx.dev)
    assert buf.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    call(idx, bs, buf.data_ptr(), l["pre_bytes"])
    more = (cx.h.block_jacobi_status(buf.data_ptr(), n, bs),) if status else ()
    cx.h.synchronize()
    torch.cuda.synchronize()
    raw = buf.cpu().numpy()
    words = l["n_blocks"] * bs * bs
    assert 4 * words == l["flags_offset"]
    return (raw[:4 * words].view(f32).reshape(l["n_blocks"], bs, bs), raw[l["flags_offset"]:l["pre_bytes"]], raw[l["pre_bytes"]:]) + more


def flags_of(area, n_blocks):
    return area[:4 * n_blocks].view(np.int32)


def assert_same_blocks(got, want, tag):
    """== everywhere, and NaN exactly where the model holds NaN"""
    assert got.shape == want.shape, tag
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (tag, "NaN words", int(np.isnan(got).sum()), int(nan.sum()))
    bad = ~nan & (got != want)
    assert not bad.any(), (tag, int(bad.sum()), "words differ; blocks", np.unique(np.argwhere(bad)[:, 0])[:8])


def check_extraction(cx, idx, T, bs, tag):
    """Extract-only, twice, of handle idx against the model's blocks of T (the stored values) -> the model's blocks"""
    n = T.shape[0]
    want = bj.extract(T, bs)
    got, flag_area, guard = run(cx, idx, n, bs, cx.h.block_jacobi_extract_device)
    assert_same_blocks(got, want, tag)
    assert (flag_area == FILL).all(), (tag, "the extraction wrote into the flag area")
    assert (guard == FILL).all(), (tag, "the extraction wrote behind the buffer")
    again, flag_area, guard = run(cx, idx, n, bs, cx.h.block_jacobi_extract_device)
    assert np.array_equal(bits(again), bits(got)), (tag, "a second extraction gives other bits")
    assert (flag_area == FILL).all() and (guard == FILL).all(), tag
    return want


def check_plan(cx, idx, name, storage, bs):
    e = P.CASES[name]["expect"]
    info = cx.h.matrix_info(idx)
    tag = (name, storage, info)
    assert info["format"] == 0 and info["tile_kind"] == e.get("tile_kind", 0) and info["col_tiles"] == e.get("parts", 1), tag
    if "threads" in e:
        assert info["block_threads"] == e["threads"], tag
    if "group" in e:
        assert info["group_slices"] == e["group"], tag
    if "window" in e:
        assert (info["lds_bytes"] > 0) == e["window"], tag
    if e["compact"] is not None:
        assert info["compact_slices"] == (info["n_slices"] if e["compact"] == "all" else 0), tag
    bi = cx.h.block_jacobi_info(idx, bs)
    assert bi["accepted"] and bi["n"] == info["rows"] and bi["pre_bytes"] == bj.layout(info["rows"], bs)["pre_bytes"], bi
    assert bi["setup_launches"] == 2 + e.get("parts", 1), (tag, bi)          # the fill, a walk per part that holds slices, the inversion
    vs = cx.h.value_storage_info(idx)
    assert vs["storage"] == storage, vs
    if storage == "bf16":
        assert vs["slots_2byte"] > 0, (tag, vs)


# ---- the sweep ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SWEEP, ids=_id)
def test_plan_extraction_setup_apply(torch_mod, contexts, case):
    from hispmv_amd import solvers
    torch = torch_mod
    key, name, bs = case
    storage = key[1]
    cx = contexts.get(key)
    idx = cx.idx[CONTEXTS[key].index(name)]
    T = P.stored(P.matrix(name), storage)
    n = T.shape[0]
    tag = (name, storage, bs)
    check_plan(cx, idx, name, storage, bs)
    blocks = check_extraction(cx, idx, T, bs, tag)
    # setup
    want, wflags = bj.invert_many(blocks)
    got, flag_area, guard, n_flagged = run(cx, idx, n, bs, cx.h.block_jacobi_setup_device, status=True)
    gflags = flags_of(flag_area, len(want))
    assert (guard == FILL).all(), (tag, "the setup wrote behind the buffer")
    assert np.array_equal(gflags, wflags), (tag, np.flatnonzero(gflags != wflags)[:8])
    bad = np.flatnonzero((bits(got) != bits(want)).any(axis=(1, 2)))
    assert bad.size == 0, (tag, "blocks differ from the model's inverse", bad[:8])
    assert n_flagged == int(wflags.sum()), tag
    if name == "holes_1024":
        flagged = P.holes_flagged(bs)
        assert np.flatnonzero(gflags).tolist() == flagged, (tag, np.flatnonzero(gflags))
        eye = np.eye(bs, dtype=f32)
        for k in flagged:
            assert np.array_equal(bits(got[k]), bits(eye)), (tag, k)
        for k in sorted({k + d for k in flagged for d in (-1, 1)} - set(flagged)):
            if 0 <= k < len(got):          # a neighbour is an ordinary block: inverted, and not the identity
                assert gflags[k] == 0 and not np.array_equal(got[k], eye), (tag, k)
    # apply
    if bs == 8:
        r = np.random.default_rng(n).uniform(-1, 1, n).astype(f32)
        pre = solvers.block_jacobi(cx.h, idx, 8)
        z = pre.apply(torch.from_numpy(r).to(cx.dev))
        torch.cuda.synchronize()
        assert pre.singular_blocks() == int(wflags.sum())
        zm = bj.BlockInverse(want, n, wflags) * r
        assert np.array_equal(bits(z.cpu().numpy()), bits(zm)), (tag, "apply", int((bits(z.cpu().numpy()) != bits(zm)).sum()))


# ---- value updates ------------------------------------------------------------------------------------------------------------------------
UPDATES = (("window_compact_256", "fp32", True), ("half_strays_1024", "bf16", "any_storage"), ("column_tiles_8", "fp32", True))


@pytest.mark.parametrize("name,storage,updates", UPDATES, ids=[u[0] for u in UPDATES])
def test_extraction_after_a_value_update(torch_mod, name, storage, updates):
    torch = torch_mod
    A = P.matrix(name)
    n = A.shape[0]
    v2 = (np.random.default_rng(len(name)).random(A.nnz, dtype=f32) * f32(3.0) - f32(1.0)).astype(f32)
    A2 = sp.coo_matrix((v2, (A.row, A.col)), shape=A.shape)
    if storage == "bf16":
        assert (S.bf16_exact(v2) != v2).mean() > 0.9          # the device has to round them
    with Ctx(torch, [A], env=P.CASES[name]["env"], storage=storage, updates=updates) as cx:
        idx = cx.idx[0]
        assert cx.h.value_update_info(idx)["updatable"] and cx.h.value_update_info(idx)["n"] == A.nnz
        check_plan(cx, idx, name, storage, 8)
        first = {bs: check_extraction(cx, idx, P.stored(A, storage), bs, (name, storage, bs, "before")) for bs in bj.SIZES}
        dv = torch.from_numpy(v2).to(cx.dev)
        torch.cuda.synchronize()
        cx.h.update_values_device(idx, dv.data_ptr(), A.nnz)
        cx.h.synchronize()
        for bs in bj.SIZES:
            second = check_extraction(cx, idx, P.stored(A2, storage), bs, (name, storage, bs, "after"))
            assert (second != first[bs]).any()


# ---- dense handles ------------------------------------------------------------------------------------------------------------------------
DENSE_SIZES = (1, 3, 33, 97, 130)


def _dense(n):
    return np.random.default_rng(500 + n).standard_normal((n, n)).astype(f32)


@pytest.fixture(scope="module", params=["fp32", "bf16"])
def dense_ctx(request, torch_mod):
    with Ctx(torch_mod, [_dense(n) for n in DENSE_SIZES], storage=request.param) as cx:
        cx.storage = request.param
        yield cx


@pytest.mark.parametrize("k", range(len(DENSE_SIZES)), ids=[str(n) for n in DENSE_SIZES])
def test_dense_extraction(dense_ctx, k):
    cx = dense_ctx
    W = cx.mats[k]
    T = W if cx.storage == "fp32" else S.bf16_exact(W)
    assert cx.storage == "fp32" or (T != W).any()
    info = cx.h.matrix_info(cx.idx[k])
    assert info["is_dense"] and cx.h.value_storage_info(cx.idx[k])["storage"] == cx.storage
    for bs in bj.SIZES:
        bi = cx.h.block_jacobi_info(cx.idx[k], bs)
        assert bi["accepted"] and bi["setup_launches"] == 2 and bi["n"] == W.shape[0], bi
        check_extraction(cx, cx.idx[k], T, bs, (W.shape[0], cx.storage, bs))


# ---- handle states ------------------------------------------------------------------------------------------------------------------------
def _tile_stream():
    from test_gpu_block_jacobi import _tile_stream_system
    A = _tile_stream_system().tocoo()
    assert P.most_stored(A) <= 2          # (random positions: a few come twice, which is order-free; none three times)
    return A


def test_transposable_keeps_a_would_be_tile_stream_extractable(torch_mod):
    A = _tile_stream()
    with Ctx(torch_mod, [A], env=S.TTS, transposable=True) as cx:
        assert cx.h.matrix_info(cx.idx[0])["format"] == 0
        for bs in bj.SIZES:
            assert cx.h.block_jacobi_info(cx.idx[0], bs)["accepted"]
            check_extraction(cx, cx.idx[0], A, bs, ("transposable", bs))


def test_a_companion_plays_no_part(torch_mod):
    A = P.matrix("window_compact_256")
    n = A.shape[0]
    with Ctx(torch_mod, [A]) as plain:
        check_plan(plain, plain.idx[0], "window_compact_256", "fp32", 8)
        want = {bs: run(plain, plain.idx[0], n, bs, plain.h.block_jacobi_setup_device) for bs in bj.SIZES}
    with Ctx(torch_mod, [A], transposable="companion") as cx:
        assert cx.h.companion_info(cx.idx[0])["has"]
        check_plan(cx, cx.idx[0], "window_compact_256", "fp32", 8)
        for bs in bj.SIZES:
            check_extraction(cx, cx.idx[0], A, bs, ("companion", bs))
            got = run(cx, cx.idx[0], n, bs, cx.h.block_jacobi_setup_device)
            for g, w in zip(got, want[bs]):
                assert np.array_equal(g, w), ("companion", bs)          # blocks (as bytes would be: no NaN here), flags, guard


def test_keep_format_refuses_a_tile_stream(torch_mod):
    torch = torch_mod
    A = _tile_stream()
    with Ctx(torch, [A], env=S.TTS, transposable="keep_format") as cx:
        assert cx.h.matrix_info(cx.idx[0])["format"] == 1
        buf = torch.full((4 << 20,), FILL, dtype=torch.uint8, device=cx.dev)
        torch.cuda.synchronize()
        for bs in bj.SIZES:
            assert not cx.h.block_jacobi_info(cx.idx[0], bs)["accepted"]
            for call in (cx.h.block_jacobi_extract_device, cx.h.block_jacobi_setup_device):
                with pytest.raises(NotImplementedError):
                    call(cx.idx[0], bs, buf.data_ptr(), buf.numel())
        cx.h.synchronize()
        torch.cuda.synchronize()
        assert bool((buf == FILL).all())          # nothing was launched
