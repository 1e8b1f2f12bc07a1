"""The step kernel (hispmv_kernels.hip: spmv_step_kernel) and the chunked tails of a batch call (hispmv_batch.cpp), at SMALL shapes.

HISPMV_BATCH_STREAMS=2 sets the size threshold of the shared-chip decision to 0, so a call of tiny matrices takes the step kernel.
Small matrices make the CPU models cheap, and every y of every call is checked, in this order, against
  1. the CPU model of its format, bit for bit (oracle.emu_spmv over the host packer's parts, fix-up carry variant; oracle.emu_tts
     on the packer's tile arrays; oracle.emu_gemv for dense handles) -- y starts as NaN, so an item that was never drawn or a
     sub-block that skipped a real group fails here;
  2. the fp64 accumulation, within the project's 1e-5 backward-error gate;
  3. the same call issued as grids (HISPMV_STEP_KERNEL=0, a second context), bit for bit;
  4. guards: x, bias and y of every matrix live inside larger device tensors; the floats between the y vectors hold a sentinel
     pattern that must survive the call, the floats around x and bias hold NaN (a filler element multiplies its x by 0, and
     0 * NaN is NaN: even a padding read outside [0, cols) shows up in y).
Every call is issued three times back to back on a non-default stream without host synchronisation (the queue rearms itself);
y is copied aside and refilled with NaN on that stream after every repetition, and every repetition is checked.  For every call
the library's own account (batch_call_info: launches, step_kernel, items, streams) is compared with counts computed here from
the host packer and matrix_info.  The inputs and the plans they must get: tests/step_small_cases.py (checked on the host by
tests/test_step_small_inputs.py, and again here from matrix_info -- no case is skipped at run time).
Reference counterpart: none -- the reference runs one matrix at a time (pyhispmv/src/fpga_handle.cpp:286-321)."""
import numpy as np
import pytest

import step_small_cases as S
from conftest import ALPHA, BETA
from step_small_harness import GRIDS, NO_PIN, N_CUS, Ctx, _play, _script, _step_and_grids

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def test_sub_blocks_past_the_last_group(torch_mod):
    """Case A: one call of 256-thread parts whose group counts are 1, 1, 2, 3, 4, 5, 147 (window), 293 (window), 1 (a 1 x 1
    matrix), 8 (one row cut over 30 slices) and 13 (50 live rows of 50 000): every residue mod 4, so the last item of most parts
    hosts one to three sub-blocks past the last group; with and without an LDS window, whose offset depends on the sub-block."""
    mats = S.case_a()
    info, recs = _step_and_grids(torch_mod, S.SLICES, mats, _script([list(range(len(mats)))], S.PAIRS + S.MORE_PAIRS), "case A")
    groups = [S.groups_of(i["n_slices"], i["group_slices"]) for i in info]
    assert all(i["block_threads"] == 256 and i["group_slices"] == 4 and i["batch_group_slices"] == 0 for i in info)
    assert {g % 4 for g in groups} == {0, 1, 2, 3} and 1 in groups, groups
    assert sum(g % 4 != 0 and i["lds_bytes"] > 0 for g, i in zip(groups, info)) >= 2
    assert sum(g % 4 != 0 and i["lds_bytes"] == 0 for g, i in zip(groups, info)) >= 2
    assert recs[0].info["items"] == sum(-(-g // 4) for g in groups) and recs[0].info["launches"] == 2


def test_fewer_items_than_workgroups_and_alternating_calls(torch_mod):
    """Case B: calls of 1, 1, 2 and 8 items (step_workgroups = items < CUs: the exit counter rearms against that grid size), a call
    of more items than CUs in the same context, and the smallest and the largest call alternating on one stream without host
    synchronisation (each has its own cached plan and its own sync words)."""
    a = S.case_a()
    mats = a + [S.big_band(), S.band(4000, 300, 19, a[7]["expect"]), S.band(4000, 300, 20, a[7]["expect"])]
    name = {m["name"]: k for k, m in enumerate(mats)}
    one = [name["one_by_one"]]
    alone = [name["uniform_3000x2500_1024_s11"]]
    two = [name["uniform_3000x2500_0_s10"], name["uniform_3000x2500_4096_s12"]]
    three = [name["uniform_3000x2500_17000_s15"], name["single_row"], name["sparse_rows"]]
    big = [11, 6, 7, 12, 13] + three

    def script(cx):
        recs = _script([one, alone, two, three, big], S.PAIRS)(cx)
        ca, cb = cx.prepare(one), cx.prepare(big)
        for alpha, beta in S.PAIRS:
            for _ in range(2):
                recs += [cx.issue(ca, alpha, beta), cx.issue(cb, alpha, beta)]            # A-B-A-B
        return recs
    _, recs = _step_and_grids(torch_mod, S.SLICES, mats, script, "case B")
    seen = {tuple(r.call.sel): r.info["items"] for r in recs}
    assert [seen[tuple(s)] for s in (one, alone, two, three)] == [1, 1, 2, 8], seen
    assert seen[tuple(big)] > N_CUS, seen


def test_every_item_kind_in_one_small_call(torch_mod):
    """Case C: 1024-thread groups, 256-thread groups with and without a window, tiles of two tile streams (one with a row cut into
    pieces: carry tiles, its fix-up in the tail) in one call, under the three queue orders: the same bits each time."""
    mats = S.case_c()
    first = None
    for order in ("", "lpt", "grid"):
        env = dict(S.AUTO, **({"HISPMV_STEP_ORDER": order} if order else {}))
        label = f"case C (order {order or 'default'})"
        if first is None:
            info, recs = _step_and_grids(torch_mod, env, mats, _script([list(range(len(mats)))], S.PAIRS), label)
            first = [r.snap.cpu().numpy().view(np.int32) for r in recs]
        else:
            bits, info, recs = _play(torch_mod, env, mats, _script([list(range(len(mats)))], S.PAIRS), label, step=True)
            for a, b in zip(first, bits):
                assert np.array_equal(a, b), f"{label}: other bits than under the default order"
        kinds = {(i["format"], i["block_threads"] if i["format"] == 0 else 0, i["lds_bytes"] > 0) for i in info}
        assert {(0, 1024, True), (0, 256, True), (0, 256, False), (1, 0, False)} <= kinds, kinds
        assert info[2]["format"] == 1 and info[2]["n_split_rows"] > 0


def test_calls_the_planner_keeps_on_the_grids(torch_mod):
    """Case C, continued: a call of tile streams only and a call with a dense handle next to sparse parts keep their grids
    (step_kernel False) and pass the same checks."""
    mats = S.case_c() + S.dense_shapes()[:2]
    only_tiles, with_dense = [1, 2], [0, 3, 7, 1, 5, 8]

    def script(cx):
        return _script([only_tiles, with_dense], S.PAIRS)(cx)
    _, _, recs = _play(torch_mod, S.AUTO, mats, script, "case C (grids kept)", step=False)
    assert all(r.info["step_kernel"] is False and r.info["items"] == 0 for r in recs)


def test_stray_split_two_way_gathers_and_stray_slots(torch_mod):
    """Case D: next to plain parts, in step calls -- a stray-split matrix (tile_kind 3: windowed part + strays into a partial vector,
    merged in the tail); 256-thread sub-blocks whose groups have a window AND elements outside it (wide elements, HISPMV_STRAY_SPLIT=0);
    a part with stray slots (the spmv_step_kernel<true> instantiation: a 22 000-row band of 4.6 M entries, 18 slices per group)."""
    a = S.case_a()
    small = [a[0], a[3], a[5], a[6], a[7], a[8]]
    m = S.stray_split_band()
    info, _ = _step_and_grids(torch_mod, S.SLICES, [m] + small, _script([list(range(7))], S.PAIRS), "case D (stray split)")
    assert info[0]["tile_kind"] == 3 and info[0]["col_tiles"] == 2
    m = S.two_way_band()
    info, _ = _step_and_grids(torch_mod, S.NOSPLIT, [m] + small, _script([list(range(7))], S.PAIRS), "case D (two-way gather)")
    g = S.groups_of(info[0]["n_slices"], info[0]["group_slices"])
    assert info[0]["block_threads"] == 256 and info[0]["lds_bytes"] > 0 and info[0]["compact_slices"] == 0 and g % 4 == 1, (info[0], g)
    m = S.stray_slot_band()
    strays, compact, n = S.stray_layout(m)                            # (host-only packer: groups with stray slots under the loader's plan)
    assert strays > 0 and compact == n
    info, _ = _step_and_grids(torch_mod, S.SLICES, [m] + small, _script([list(range(7))], S.PAIRS), "case D (stray slots)")
    assert info[0]["block_threads"] == 1024 and info[0]["group_slices"] > 16 and info[0]["compact_slices"] == info[0]["n_slices"], info[0]


def test_column_parts_pinned_and_queued_singly(torch_mod):
    """Case D: a matrix in eight L2-sized column parts (partial vectors, merge in the tail).  Pinned to XCD subsets it is ONE item
    of eight parts in the grids and keeps the call off the step kernel; with HISPMV_NO_XCD_PIN=1 its parts are queued singly."""
    a = S.case_a()
    mats = [S.column_tiled(), a[0], a[3], a[5], a[6], a[7]]
    script = _script([list(range(6))], S.PAIRS)
    pinned, info, recs = _play(torch_mod, S.COLTILES, mats, script, "case D (column parts, pinned)", step=False, pin=True)
    assert info[0]["tile_kind"] == 1 and info[0]["col_tiles"] == 8 and info[0]["col_tile_width"] == 25024 and info[0]["block_threads"] == 256
    assert all(r.info["step_kernel"] is False for r in recs)
    info, recs = _step_and_grids(torch_mod, dict(S.COLTILES, **NO_PIN), mats, script, "case D (column parts, queued singly)", pin=False)
    assert all(r.info["step_kernel"] is True for r in recs)
    single, _, _ = _play(torch_mod, dict(S.COLTILES, **NO_PIN), mats, script, "case D (column parts, again)", step=True, pin=False)
    for p, s in zip(pinned, single):
        assert np.array_equal(p, s)                                   # pinned or not: the same bits


def test_more_than_32_plain_parts(torch_mod):
    """Case E: 40 small matrices with cut rows: the fused tail is dropped, two fix-up launches; as grids two slice grids of one class."""
    mats = S.case_e_sparse()
    info, recs = _step_and_grids(torch_mod, S.SLICES, mats, _script([list(range(40))], S.PAIRS), "case E (40 plain parts)")
    order = sorted(range(40), key=lambda k: -info[k]["n_slices"])
    assert any(info[k]["n_split_rows"] > 0 for k in order[:32]) and any(info[k]["n_split_rows"] > 0 for k in order[32:])
    assert all(i["block_threads"] == 256 for i in info)
    assert recs[0].info["launches"] == 1 + 2                          # the step launch + two fix-up launches (grids: 2 + 2, in _account)


def test_more_than_32_column_tiled_matrices(torch_mod):
    """Case E: 34 matrices of eight column parts: two merge launches and nine fix-up launches in the tail; 272 parts in the step
    kernel's one table (HISPMV_NO_XCD_PIN=1), pinned eight-part items cut over nine grids without it."""
    mats = S.case_e_column_tiled()
    script = _script([list(range(34))], S.PAIRS)
    info, recs = _step_and_grids(torch_mod, dict(S.COLTILES, **NO_PIN), mats, script, "case E (34 column-tiled, queued singly)", pin=False)
    assert all(i["col_tiles"] == 8 and i["tile_kind"] == 1 for i in info)
    assert recs[0].info["launches"] == 1 + 9 + 2, recs[0].info
    _, _, recs = _play(torch_mod, S.COLTILES, mats, script, "case E (34 column-tiled, pinned)", step=False, pin=True)
    assert recs[0].info["launches"] == 9 + 9 + 2 and not recs[0].info["step_kernel"], recs[0].info


def test_more_than_32_dense_handles(torch_mod):
    """Case E: 35 dense handles next to one sparse matrix: two GeMV grids, no step kernel."""
    mats = S.dense_shapes() + [S.case_a()[7]]
    first, _, recs = _play(torch_mod, S.SLICES, mats, _script([list(range(36))], S.PAIRS), "case E (35 dense)", step=False)
    assert recs[0].info["launches"] == 2 + 1 + 1, recs[0].info         # two GeMV grids, the slice grid, the tail
    again, _, _ = _play(torch_mod, dict(S.SLICES, **GRIDS), mats, _script([list(range(36))], S.PAIRS), "case E (35 dense, step kernel off)", step=False)
    for a, b in zip(first, again):
        assert np.array_equal(a, b)


def test_more_than_32_tile_streams(torch_mod):
    """Case E: 33 tile streams next to slice parts: 33 entries in the step kernel's tile table; as grids two tile grids."""
    a = S.case_a()
    mats = S.case_e_tile_streams() + [a[3], a[6], a[7]]
    info, recs = _step_and_grids(torch_mod, S.AUTO, mats, _script([list(range(36))], S.PAIRS), "case E (33 tile streams)")
    assert sum(i["format"] == 1 for i in info) == 33 and len({i["group_slices"] for i in info if i["format"] == 1}) == 1
    assert recs[0].info["launches"] == 1 + 1, recs[0].info             # (grids: two tile grids + one slice grid + the tail, in _account)


def test_plan_cache_turnover(torch_mod):
    """Case F: 18 distinct call signatures over the same handles, each issued once: the 17th frees all cached plans (step-kernel
    queues and their sync words included); then the first again, rebuilt.  No free is rejected up to and including close()."""
    from hispmv_amd._lib import lib
    before = lib.hispmv_free_failures()
    a = S.case_a()
    mats = [a[3], a[5], a[7], a[9]]

    def script(cx):
        calls = [cx.prepare([0, 1, 2, 3]) for _ in range(18)]
        recs = [cx.issue(c, ALPHA, BETA) for c in calls]
        recs += [cx.issue(calls[0], ALPHA, BETA) for _ in range(3)]
        return recs
    _, _, recs = _play(torch_mod, S.SLICES, mats, script, "case F", step=True)
    assert len(recs) == 21 and len({r.call.Y.data_ptr() for r in recs}) == 18
    assert lib.hispmv_free_failures() == before


def test_two_tile_geometries_in_one_call(torch_mod):
    """HISPMV_TTS_SMALL=1: a narrow band in 13 K-slot blocks next to a stream in the standard 28 K-slot blocks and two 256-thread slice
    parts.  The step kernel takes tiles of both geometries (its LDS is the larger one's); as grids the two streams are two classes:
    two tile grids.  The two streams alone keep their grids."""
    a = S.case_a()
    mats = [S.small_band(), S.tile_stream_cut_row(), a[3], a[6]]
    info, recs = _step_and_grids(torch_mod, S.TTS_SMALL, mats, _script([[0, 1, 2, 3]], S.PAIRS), "two tile geometries")
    assert [i["group_slices"] for i in info[:2]] == [13, 28] and all(i["format"] == 1 for i in info[:2])
    assert recs[0].info["launches"] == 1 + 1, recs[0].info                       # (grids: two tile grids + a slice grid + the tail, in _account)
    _, _, recs = _play(torch_mod, S.TTS_SMALL, mats, _script([[0, 1]], S.PAIRS), "two tile geometries (tiles only)", step=False)
    assert recs[0].info["launches"] == 2 + 1 and recs[0].info["streams"] == 2, recs[0].info


def test_ticket_look_back_back_to_back(torch_mod):
    """HISPMV_CARRY=ticket: the look-back whose groups are handed out in start order, through spmv_device on a 293-group matrix with
    cut rows, three launches per alpha/beta pair on one stream without host synchronisation: launch k draws the tickets
    [k * 293, (k + 1) * 293).  The model is the look-back variant of the slice stream (mode 1)."""
    m = S.case_a()[7]
    with Ctx(torch_mod, dict(S.SLICES, HISPMV_CARRY="ticket"), [m]) as cx:
        assert cx.info[0]["carry_lookback"] == 1 and S.groups_of(cx.info[0]["n_slices"], cx.info[0]["group_slices"]) == 293, cx.info[0]
        call = cx.prepare([0])
        recs = [cx.issue_single(call, alpha, beta) for alpha, beta in S.PAIRS + S.MORE_PAIRS for _ in range(3)]
        for n, r in enumerate(recs):
            cx.check(r, f"ticket look-back, launch {n}", mode=1)
        cx.h.synchronize()                                                        # (a bounded wait that expired would raise here)
