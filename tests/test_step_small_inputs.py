"""Premises of tests/test_gpu_step_small.py, checked on the host: every generated matrix of its cases gets, from the loader's own
planner at 256 CUs (hispmv_prep_choose_format / the host packer) under the case's switches, the plan the case was written for --
format, thread count, slices per group, window or not, group count and its residue mod 4, part count, cut rows -- and the CPU
model of each matrix is within the 1e-5 gate of the fp64 accumulation for every alpha/beta pair used, so that on the GPU the
gate cannot be what fails.  When a planner threshold moves, this test says which input has to move with it."""
import numpy as np
import pytest

import step_small_cases as S
from conftest import ALPHA, BETA, TOL
from util import bwd_err


def _facts(m, env):
    info = S.host_info(m, env)
    pk = S.packed(m, info)
    S.check_expect(m, info, pk)
    return info, pk


def _model_within_gate(m, info, pk, pairs=S.PAIRS):
    for alpha, beta in pairs:
        ye, y64, mag = S.reference(m, info, pk, alpha, beta)
        assert np.all(np.isfinite(ye)) and bwd_err(ye, y64, mag) < TOL, (m["name"], alpha, beta, bwd_err(ye, y64, mag))


def test_pairs_are_the_projects():
    assert S.PAIRS[0] == (ALPHA, BETA)


def test_case_a_group_counts_cover_every_residue():
    mats = S.case_a()
    res = {True: [], False: []}
    counts = []
    for m in mats:
        info, pk = _facts(m, S.SLICES)
        assert info["block_threads"] == 256 and info["group_slices"] == 4 and info["col_tiles"] == 1
        g = S.groups_of(pk[0].n_slices, 4)
        counts.append(g)
        res[info["lds_bytes"] > 0].append(g % 4)
        _model_within_gate(m, info, pk, S.PAIRS + S.MORE_PAIRS)
    assert {g % 4 for g in counts} == {0, 1, 2, 3} and 1 in counts, counts
    assert sum(r != 0 for r in res[True]) >= 2 and sum(r != 0 for r in res[False]) >= 2, res
    by = dict(zip((m["name"] for m in mats), mats))
    empty = by["uniform_3000x2500_0_s10"]
    assert empty["r"].size == 0 and empty["rows"] == 3000                         # nnz = 0: filler slices only, still one group
    assert by["single_row"]["rows"] == 1 and S.packed(by["single_row"], S.host_info(by["single_row"], S.SLICES))[0].n_slices >= 30
    assert np.unique(by["sparse_rows"]["r"]).size == 50


def test_case_c_holds_every_item_kind():
    kinds = set()
    for m in S.case_c():
        info, pk = _facts(m, S.AUTO)
        kinds.add((info["format"], info["block_threads"] if info["format"] == 0 else 0, info["lds_bytes"] > 0))
        _model_within_gate(m, info, pk)
    assert {(0, 1024, True), (0, 256, True), (0, 256, False), (1, 0, False)} <= kinds, kinds
    info, pk = _facts(S.tile_stream_cut_row(), S.AUTO)
    assert pk.tts["n_carry"] > 0 and pk.tts["fix"].shape[0] > 0


@pytest.mark.parametrize("maker,env", [(S.stray_split_band, S.SLICES), (S.column_tiled, S.COLTILES), (S.two_way_band, S.NOSPLIT),
                                       (S.stray_slot_band, S.SLICES)])
def test_case_d_plans(maker, env):
    m = maker()
    info, pk = _facts(m, env)
    _model_within_gate(m, info, pk)
    if maker is S.column_tiled:
        assert info["col_tile_width"] == 25024 and len(pk) == 8
    if maker is S.two_way_band:
        with S.environment(env):
            strays, compact, n = S.stray_layout(m)
        assert compact == 0 and n == pk[0].n_slices                               # wide elements: a window AND gathers outside it
    if maker is S.stray_slot_band:
        strays, compact, n = S.stray_layout(m)
        assert info["group_slices"] > 16 and strays > 0 and compact == n, (info, strays, compact, n)


def test_case_d_neighbours_keep_their_plans_under_the_other_switches():
    """The small parts of case A that ride next to the case D matrices are planned the same under those contexts' switches."""
    for env in (S.COLTILES, S.NOSPLIT):
        for m in S.case_a()[:8]:
            _facts(m, env)


def test_case_e_inputs():
    mats = S.case_e_sparse()
    facts = [_facts(m, S.SLICES) for m in mats]
    assert len(mats) == 40
    # the planner's order of the parts (thread count, then slices, descending; stable): cut rows on both sides of entry 32
    order = sorted(range(40), key=lambda k: -facts[k][1][0].n_slices)
    cut = [sum(S.cut_rows(*facts[k])) > 0 for k in order]
    assert any(cut[:32]) and any(cut[32:])
    for m, (info, pk) in zip(mats, facts):
        _model_within_gate(m, info, pk)
    tiled = S.case_e_column_tiled()
    assert len(tiled) == 34
    for m in tiled:
        info, pk = _facts(m, S.COLTILES)
        _model_within_gate(m, info, pk)
    streams = S.case_e_tile_streams()
    assert len(streams) == 33
    for m in streams:
        info, pk = _facts(m, S.AUTO)
        assert info["group_slices"] == 28                                          # one geometry: one class of tile grids
        _model_within_gate(m, info, pk)
    dense = S.dense_shapes()
    assert len(dense) == 35
    for m in dense:
        _model_within_gate(m, None, None)
