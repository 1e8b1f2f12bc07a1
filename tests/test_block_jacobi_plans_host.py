"""The inputs of tests/test_gpu_block_jacobi_plans.py get the plans they are named for (tests/block_jacobi_plan_cases.py), checked on the
host: the loader's decision at 256 CUs (step_small_cases.host_info) and, for a single-part case, the device layout with its group
words (prep.device_layout_from_coo).  A planner change that turned the sweep back into a row of plans without a window fails here.
Also the batched inversion of the numpy model, which the GPU module uses on its tens of thousands of blocks, against the model's
block-by-block one."""
import numpy as np
import pytest

import block_jacobi_model as bj
import block_jacobi_plan_cases as P
import step_small_cases as S
from hispmv_amd import prep

f32 = np.float32
N_CUS = 256


@pytest.mark.parametrize("name", sorted(P.CASES))
def test_case_gets_its_plan(name):
    case, e = P.CASES[name], P.CASES[name]["expect"]
    A = P.matrix(name)
    n = A.shape[0]
    assert A.shape[0] == A.shape[1] and A.data.dtype == f32
    assert (n % 4 != 0) == e["odd_n"], n
    assert P.most_stored(A) == e.get("stored", 1)
    info = S.host_info(P.as_case(name), case["env"])
    print(f"{name}: n {n}, {A.nnz} entries, {info}")
    assert info["format"] == 0, info
    assert info["tile_kind"] == e.get("tile_kind", 0) and info["col_tiles"] == e.get("parts", 1), info
    if "threads" in e:
        assert info["block_threads"] == e["threads"], info
    if "group" in e:
        assert info["group_slices"] == e["group"], info
    if "window" in e:
        assert (info["lds_bytes"] > 0) == e["window"], info
    if e.get("parts", 1) > 1:
        return
    for storage in case["storages"]:
        with S.environment(case["env"]):
            lay = prep.device_layout_from_coo(A.row, A.col, A.data, n, n, N_CUS, value_storage=storage)
        words = lay["dgroups"][:, 3]
        print(f'  {storage}: threads {lay["threads"]} slices/group {lay["group_slices"]} window {4 * lay["window_floats"]} B (strays {4 * lay["stray_floats"]} B) '
              f'slices {lay["n_slices"]} compact {lay["compact_slices"]} with strays {lay["stray_slices"]} group words {sorted(set(words.tolist()))}')
        assert (lay["threads"], lay["group_slices"]) == (e["threads"], e["group"]), lay["threads"]
        assert (lay["window_floats"] > 0) == e["window"]
        assert lay["n_slices"] > 4 * lay["group_slices"]                                   # more than one workgroup, by far
        assert lay["compact_slices"] == (lay["n_slices"] if e["compact"] == "all" else 0)
        assert lay["stray_slices"] == (lay["n_slices"] if e["strays"] == "all" else 0)
        want = e["words"][storage]
        assert int(np.bitwise_and.reduce(words)) == want and int(np.bitwise_or.reduce(words)) == want, (storage, sorted(set(words.tolist())), want)


def test_holes_are_where_the_case_says():
    A = P.matrix("holes_1024").tocsr()
    n = A.shape[0]
    assert not np.diff(A.indptr)[list(P.HOLE_ROWS)].any() and (np.diff(A.indptr) == 0).sum() == len(P.HOLE_ROWS)
    assert np.isnan(A[P.NAN_AT]) and np.isposinf(A[P.INF_AT]) and (~np.isfinite(A.data)).sum() == 2
    for storage in ("fp32", "bf16"):
        T = P.stored(P.matrix("holes_1024"), storage)
        for bs in bj.SIZES:
            blocks = bj.extract(T, bs)
            zero = [k for k in range(len(blocks)) if not blocks[k].any()]
            assert zero == P.holes_zero_blocks(bs), (bs, zero)
            assert np.isnan(blocks[P.NAN_AT[0] // bs]).sum() == 1 and np.isnan(blocks).sum() == 1
            assert P.NAN_AT[0] // bs != P.INF_AT[0] // bs and P.NAN_AT[0] // bs == P.NAN_AT[1] // bs
            inv, flags = bj.invert_many(blocks)
            assert np.flatnonzero(flags).tolist() == P.holes_flagged(bs), (bs, np.flatnonzero(flags))
            assert len(blocks) * bs > n                                                     # the last block is partial, and flagged: row n - 1 is empty
            assert flags[-1] == 1


def test_bf16_cases_round_something():
    for name, case in P.CASES.items():
        if "bf16" in case["storages"] and case["storages"] != ("bf16",):
            A = P.matrix(name)
            assert (P.stored(A, "bf16").data != A.data).any(), name
        if case["storages"] == ("bf16",):                                                    # given bf16-exact already, as the table says
            A = P.matrix(name)
            assert np.array_equal(P.stored(A, "bf16").data, A.data), name


@pytest.mark.parametrize("bs", bj.SIZES)
def test_batched_inversion_is_the_models_block_by_block(bs):
    rng = np.random.default_rng(40 + bs)
    blocks = np.stack([bj.block_of(bj.KINDS[k % len(bj.KINDS)], bs, rng) for k in range(4 * len(bj.KINDS))]
                      + [(rng.standard_normal((bs, bs)) * 10.0 ** rng.uniform(-3, 3)).astype(f32) for _ in range(40)]
                      + [np.triu(rng.random((bs, bs), dtype=f32) - f32(0.5)) for _ in range(8)])
    blocks[-1][bs // 2] = 0                                                                  # an upper triangle with an empty row
    want, wflags = bj.invert(blocks)
    got, gflags = bj.invert_many(blocks)
    assert 0 < wflags.sum() < len(blocks)
    assert np.array_equal(gflags, wflags), (gflags, wflags)
    assert got.dtype == f32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    none, nflags = bj.invert_many(blocks[:0])
    assert none.shape == (0, bs, bs) and nflags.shape == (0,)
