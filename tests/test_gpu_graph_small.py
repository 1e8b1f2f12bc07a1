"""Batch calls replayed as HIP graphs (HISPMV_BATCH_GRAPH=1, HISPMV_BATCH_STREAMS=2; hispmv_batch.cpp: capture, the second executable,
graph_set_alpha through the kernel registry of hispmv_kernels.hip) at SMALL shapes, on the harness of tests/step_small_harness.py.
Every kernel a captured call can hold is patched here at least once: both slice multi kernels, both half-slice multi kernels, the four
tile-stream multi kernels, both GeMV multi kernels, the fused tail, the long-chain fix-up behind it, the fix-up and merge launches.

Per call and per beta (two call signatures) alpha runs through a, a, a, b, b, c, a: plain launches, the capture, a replay, the second
executable instantiated and patched, a replay, and two patches of the executable used longest ago.  Issued on a non-default stream
without host synchronisation, y copied aside after each.  Each of the seven y sets is checked against the CPU model at ITS alpha bit
for bit (a patch that missed a kernel, hit another argument or reached an executable still in flight shows here), against fp64
within the gate, for its guards, and bit for bit against the same sequence under HISPMV_BATCH_GRAPH=0 HISPMV_STEP_KERNEL=0.  After
each signature's sequence the library's counters have moved by exactly two instantiations and three alpha updates: none means the
capture was refused (the library then goes on with plain launches, silently), more means a patch failed and the call was captured again.
Reference counterpart: none -- the reference runs one matrix at a time (pyhispmv/src/fpga_handle.cpp:286-321)."""
import numpy as np
import pytest

import step_small_cases as S
from conftest import ALPHA, BETA
from step_small_harness import Rec, _play

pytestmark = pytest.mark.gpu

GRAPH = {"HISPMV_BATCH_GRAPH": "1"}
PLAIN = {"HISPMV_BATCH_GRAPH": "0", "HISPMV_STEP_KERNEL": "0"}
A, B, C = ALPHA, -1.75, 0.3125
SEQUENCE = (A, A, A, B, B, C, A)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def _sequence(sels, counts, after=None):
    """The script of one context: per call and per beta the alpha sequence; `counts` collects the moves of the library's counters."""
    def run(cx):
        recs = []
        for sel in sels:
            call = cx.prepare(sel)
            for beta in (BETA, 0.0):
                before = cx.h.batch_graph_stats()
                recs += [cx.issue(call, alpha, beta) for alpha in SEQUENCE]
                now = cx.h.batch_graph_stats()
                counts.append((now["instantiations"] - before["instantiations"], now["alpha_updates"] - before["alpha_updates"]))
            if after is not None:
                recs += after(cx, call)
        return recs
    return run


def _replayed_and_plain(torch, env, mats, sels, label, launches, after=None):
    """-> the matrix_info list.  The y checks come first (in _play), then the account of every call, then the counters."""
    counts, none = [], []
    graph, info, recs = _play(torch, dict(env, **GRAPH), mats, _sequence(sels, counts, after), label + " (graphs)", step=False)
    assert all(r.info["streams"] == 2 and r.info["launches"] == launches and not r.info["step_kernel"] for r in recs), [r.info for r in recs[::7]]
    assert counts == [(2, 3)] * (2 * len(sels)), f"{label}: instantiations and alpha updates per call signature {counts}, expected (2, 3) each"
    plain, _, _ = _play(torch, dict(env, **PLAIN), mats, _sequence(sels, none), label + " (plain launches)", step=False)
    assert none == [(0, 0)] * (2 * len(sels)), none
    n = 14 * len(sels)
    assert len(plain) == n and len(graph) >= n
    for k, (p, q) in enumerate(zip(graph[:n], plain)):                            # (behind them: what `after` issued)
        assert np.array_equal(p, q), f"{label}: issue {k} (alpha {SEQUENCE[k % 7]}): the replayed call's y differs from plain launches'"
    return info


def _g1_slices():
    a = S.case_a()
    return [S.big_band(), a[3], a[5], a[6], S.single_row_long()]


def test_g1_every_main_kind_and_a_long_chain_behind_the_fused_tail(torch_mod):
    """A 1024-thread band, three 256-thread parts with and without a window, two tile streams (one with a row cut into pieces), two dense
    handles and one row of 40 000 entries: four main grids on two lanes, the fused tail and, behind it, the long-chain fix-up launch
    (a chain of 39 slices, more than kFixShortMax).  Then the CALLER captures the call into a graph of its own: the library must issue
    plain launches into the capture (its counters do not move) and the replay must write every y."""
    torch = torch_mod
    mats = _g1_slices() + [S.tile_stream(), S.tile_stream_cut_row()] + S.dense_shapes()[:2]

    def caller_capture(cx, call):
        before = cx.h.batch_graph_stats()
        side = torch.cuda.Stream(device=cx.dev)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with S.environment(cx.env), torch.cuda.graph(g, stream=side):
            cx.h.spmv_device_batch(call.with_bias, A, BETA, side.cuda_stream)
        info = cx.h.batch_call_info()
        call.Y.copy_(call.Y0)                                                      # NaN in every y, sentinels between them
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        snap = call.Y.clone()
        call.Y.copy_(call.Y0)
        torch.cuda.synchronize()
        del g
        assert cx.h.batch_graph_stats() == before, (cx.h.batch_graph_stats(), before)
        return [Rec(call, A, BETA, snap, info)]
    info = _replayed_and_plain(torch, S.AUTO, mats, [list(range(len(mats)))], "G1", launches=4 + 1, after=caller_capture)
    assert info[4]["n_split_rows"] == 1 and info[4]["block_threads"] == 256 and info[4]["n_slices"] > 33
    assert [i["format"] for i in info[:7]] == [0, 0, 0, 0, 0, 1, 1]


def test_g2_parts_with_stray_slots(torch_mod):
    """The band whose compact groups keep stray slots next to 256-thread parts: spmv_slices_multi_kernel<true> in a grid of its own."""
    a = S.case_a()
    info = _replayed_and_plain(torch_mod, S.SLICES, [S.stray_slot_band(), a[3], a[6]], [[0, 1, 2]], "G2", launches=2 + 1)
    assert info[0]["block_threads"] == 1024 and info[0]["group_slices"] > 16


def test_g3_bf16_value_storage(torch_mod):
    """G1's slice matrices and G2's band stored as bf16 (their values are bf16-exact, so the CPU models apply unchanged), a bf16 and an
    fp32 dense handle: both half-slice multi kernels (with and without stray slots) and the mixed GeMV kernel."""
    d = S.dense_shapes()
    mats = [S.as_bf16(m) for m in _g1_slices() + [S.stray_slot_band(), d[1]]] + [d[0]]
    seen = []

    def storage(cx, call):
        seen.extend(cx.h.value_storage_info(i) for i in cx.idx)
        return []
    _replayed_and_plain(torch_mod, S.SLICES, mats, [list(range(len(mats)))], "G3", launches=4 + 1, after=storage)
    assert [v["storage"] for v in seen[:8]] == ["bf16"] * 7 + ["fp32"], seen[:8]
    assert seen[0]["slots_2byte"] > 0 and seen[5]["slots_2byte"] > 0 and seen[6]["slots_2byte"] == 301 * 520, seen[:8]      # half slots in both bands


def test_g4_more_than_32_cut_parts(torch_mod):
    """40 small matrices with cut rows: two slice grids of one class, the fused tail is dropped -- two spmv_fixup_multi_kernel launches."""
    _replayed_and_plain(torch_mod, S.SLICES, S.case_e_sparse(), [list(range(40))], "G4", launches=2 + 2)


def test_g5_column_parts_merged_in_the_tail(torch_mod):
    """A matrix in eight pinned L2-sized column parts, 256-thread parts and a dense handle (the second main grid): the merge half of the
    fused tail; with HISPMV_NO_FUSED_TAIL=1 spmv_fixup_multi_kernel and spmv_merge_multi_kernel as launches of their own."""
    a = S.case_a()
    mats = [S.column_tiled(), a[0], a[3], a[5], a[6], a[7], S.dense_shapes()[1]]
    info = _replayed_and_plain(torch_mod, S.COLTILES, mats, [list(range(7))], "G5", launches=2 + 1)
    assert info[0]["tile_kind"] == 1 and info[0]["col_tiles"] == 8
    _replayed_and_plain(torch_mod, dict(S.COLTILES, HISPMV_NO_FUSED_TAIL="1"), mats, [list(range(7))], "G5 (no fused tail)", launches=2 + 1 + 1)


@pytest.mark.parametrize("geometry", ["tall", "tallgap", "xlds"])
def test_g6_the_other_tile_stream_kernels(torch_mod, geometry):
    """spmv_tts_multi_kernel<true, false, false> (tall: zero-filled staging), <false, false, true> (tallgap: gap-coded row ends) and
    <false, true, false> (x in the LDS), each next to a 256-thread slice part."""
    part = S.case_a()[3]
    if geometry == "xlds":
        mats, env = [S.xlds_cases()["A"], part], S.TTS_XLDS
    else:
        mats, env = [S.tall(S.tile_stream_cut_row(), geometry), part], S.tall_env(geometry)
    info = _replayed_and_plain(torch_mod, env, mats, [[0, 1]], f"G6 ({geometry})", launches=2 + 1)
    assert info[0]["format"] == 1 and info[0]["col_tiles"] == (1 if geometry == "xlds" else 2)
