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


def test_x_in_lds_cases_cover_the_widths_and_both_sides_of_the_boundary():
    """HISPMV_TTS_XLDS=1: the mirror of tts_batch_width on the packer's arrays gives case A four vectors per pass with x in the LDS,
    B two (four through the cache), C one (four through the cache); D (16 384 columns) is the longest x that qualifies, E (16 385) does
    not.  Every case is a standard-geometry tile stream under HISPMV_FORMAT=tts; A and C have a row cut into pieces."""
    cases = S.xlds_cases()
    lds_widths = set()
    for name, m in cases.items():
        for env in (S.TTS_XLDS, S.TTS):
            info, pk = _facts(m, env)                                             # (check_expect: format, geometry, widths, x in the LDS or not)
            assert info["format"] == 1 and info["group_slices"] == 28 and info["col_tiles"] == 1, (name, info)
        assert m["cols"] % 2 == 1 or name == "D"
        lds, cache = S.tts_widths(pk.tts, m["cols"])
        lds_widths.add(lds)
        assert (lds > 0) == (name != "E") and (cache == 4 or name not in "ABC"), (name, lds, cache)
        _model_within_gate(m, info, pk, S.PAIRS + S.MORE_PAIRS)
    assert {4, 2, 1} <= lds_widths and cases["D"]["cols"] == S.TTS_XLDS_MAX and cases["E"]["cols"] == S.TTS_XLDS_MAX + 1, lds_widths
    for name in "AC":
        pk = S.packed(cases[name], S.host_info(cases[name], S.TTS_XLDS))
        assert pk.tts["fix"].shape[0] == 1 and pk.tts["n_carry"] > 0, name
    # a `linear` call of 7 vectors: A takes 4 + 2 + 1 from the LDS, C 4 + 2 through the cache and the last vector from the LDS
    tA, tC = (S.packed(cases[n], S.host_info(cases[n], S.TTS_XLDS)).tts for n in "AC")
    assert S.linear_passes(tA, cases["A"]["cols"], 7, True) == [(4, True), (2, True), (1, True)]
    assert S.linear_passes(tC, cases["C"]["cols"], 7, True) == [(4, False), (2, False), (1, True)]
    assert S.linear_passes(tC, cases["C"]["cols"], 7, False) == [(4, False), (2, False), (1, False)]
    # the size the loader asks of a forced tile stream: the same shape with 60 000 entries stays a slice stream
    assert S.host_info(S.uniform(2000, 2047, 60000, 301, {}, heavy_row=(7, 1.0 / 3)), S.TTS_XLDS)["format"] == 0


def test_neighbours_of_the_x_in_lds_calls_keep_their_plans():
    """Under HISPMV_FORMAT=tts: tile_stream_cut_row is a standard-geometry stream (x far too long for the LDS), tile_stream (60 000
    entries) and the small parts of case A stay 256-thread slice streams."""
    for env in (S.TTS_XLDS, S.TTS):
        info, pk = _facts(S.tile_stream_cut_row(), env)
        assert info["group_slices"] == 28 and not S.x_in_lds(pk.tts, 400000)
        _facts(S.as_slices(S.tile_stream(), threads=256), env)
        for m in S.case_a()[:7]:
            _facts(m, env)


def test_small_geometry_band():
    m = S.small_band()
    info, pk = _facts(m, S.TTS_SMALL)
    assert info["group_slices"] == 13 and 1.3 < pk.tts["lines_per_gather"] < 1.5 and pk.tts["max_slots"] <= 13 * 1024 and pk.tts["max_rows"] <= 4096
    assert S.host_info(m, S.TTS)["group_slices"] == 28                            # without the switch: the standard geometry
    _model_within_gate(m, info, pk, S.PAIRS + S.MORE_PAIRS)
    info, pk = _facts(S.tile_stream_cut_row(), S.TTS_SMALL)                       # its neighbour in the two-class call: 28 K-slot blocks
    assert info["group_slices"] == 28


def test_single_row_long_is_a_long_chain():
    m = S.single_row_long()
    for env in (S.AUTO, S.SLICES):
        info, pk = _facts(m, env)                                                 # (check_expect: one chain of more than 32 slices)
        assert pk[0].fix.shape[0] == 1 and pk[0].fix[0, 2] == pk[0].n_slices - 1 > 32
    _model_within_gate(m, info, pk)
    short = S.single_row()
    assert S.packed(short, S.host_info(short, S.SLICES))[0].fix[0, 2] <= 32       # the older case: a short chain


@pytest.mark.parametrize("geometry", ["tall", "tallgap"])
def test_tall_geometries_of_the_graph_cases(geometry):
    m = S.tall(S.tile_stream_cut_row(), geometry)
    info, pk = _facts(m, S.tall_env(geometry))
    assert len(pk.tts) == 2 and sum(S.cut_rows(info, pk)) > 0
    assert all(bool(t["zero_fill"]) == (geometry == "tall") and (t["flags_hi"] is not None) == (geometry == "tallgap") for t in pk.tts)
    _model_within_gate(m, info, pk)
    _facts(S.case_a()[3], S.tall_env(geometry))                                  # its neighbour stays a 256-thread slice stream


def test_bf16_exact_values_survive_the_bf16_packer():
    """as_bf16: values rounded to bfloat16 once on the host; the packer's own rounding (value_storage="bf16") then changes nothing."""
    from hispmv_amd.prep import prep_from_coo
    m = S.as_bf16(S.case_a()[3])
    assert m["storage"] == "bf16" and not np.array_equal(m["v"], S.case_a()[3]["v"])
    assert np.all(m["v"].view(np.uint32) & 0xFFFF == 0)
    a = prep_from_coo(m["r"], m["c"], m["v"], m["rows"], m["cols"])
    b = prep_from_coo(m["r"], m["c"], m["v"], m["rows"], m["cols"], value_storage="bf16")
    assert np.array_equal(a.values.view(np.uint32), b.values.view(np.uint32)) and np.array_equal(a.words, b.words)
    d = S.as_bf16(S.dense_shapes()[1])
    assert np.all(d["W"].view(np.uint32) & 0xFFFF == 0) and d["W"].shape == (301, 520)
