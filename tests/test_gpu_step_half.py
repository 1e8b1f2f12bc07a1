"""Batch calls with bf16 handles through the step kernel (hispmv_kernels.hip: spmv_step_kernel<., HALF = 1>; opt-in: HISPMV_STEP_HALF=1 /
hispmv_set_step_half), at SMALL shapes.

Every case goes through the harness of tests/test_gpu_step_small.py (tests/step_small_harness.py) with HISPMV_STEP_HALF=1 added to the
case's switches, so every y of every call gets that module's four checks: the CPU model of its format bit for bit (the values are
bf16-exact, S.as_bf16: the models apply unchanged), the fp64 accumulation within the 1e-5 gate, the same bits as the grids in a second
context (HISPMV_STEP_KERNEL=0, which still wins), and the guards around y, x and bias.  Every call is issued three times back to back on
a non-default stream, and the library's account of it (launches, step_kernel True, items, streams) is compared with the harness's own
count.  Without the new kernel and its routing a call with half groups runs as grids: the account says step_kernel False and the cases
fail there.  The inputs, and which of their parts have HALF groups: tests/step_half_cases.py, checked on the host by
tests/test_step_half_host.py.  Reference counterpart: none -- the reference stores fp32 values and runs one matrix at a time."""
import numpy as np
import pytest

import step_half_cases as H
import step_small_cases as S
from step_small_harness import N_CUS, Ctx, _account, _play, _script, _step_and_grids

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def _with_storage_info(script, out):
    """The script, with value_storage_info of every handle noted first (the contexts are closed when the harness returns)."""
    def run(cx):
        out.append([cx.h.value_storage_info(i) for i in cx.idx])
        return script(cx)
    return run


def _half_as_marked(mats, storage):
    """value_storage_info against the marks of the case: 2-byte slots exactly in the matrices with a part the case calls half."""
    for m, s in zip(mats, storage):
        assert s["storage"] == m.get("storage", "fp32"), (m["name"], s)
        assert (s["slots_2byte"] > 0) == bool(m["half"] and any(m["half"])), (m["name"], s, m["half"])


def test_half_sub_blocks_past_the_last_group(torch_mod):
    """H-A: case A with every matrix bf16.  The two windowed 256-thread parts have half groups, 147 and 293 of them: their last items
    hold one and three sub-blocks past the last group of a HALF part; the window-less parts are 32-bit slots with bf16-exact values
    through the half kernel's wide body."""
    mats = H.case_ha()
    storage = []
    script = _with_storage_info(_script([list(range(len(mats)))], S.PAIRS + S.MORE_PAIRS), storage)
    info, recs = _step_and_grids(torch_mod, H.half_env(S.SLICES), mats, script, "case H-A")
    _half_as_marked(mats, storage[0])
    assert [k for k, s in enumerate(storage[0]) if s["slots_2byte"] > 0] == [6, 7] == [k for k, i in enumerate(info) if i["lds_bytes"] > 0]
    groups = [S.groups_of(i["n_slices"], i["group_slices"]) for i in info]
    assert all(i["block_threads"] == 256 and i["group_slices"] == 4 and i["batch_group_slices"] == 0 for i in info)
    assert (groups[6], groups[7]) == (147, 293) and {groups[6] % 4, groups[7] % 4} == {3, 1}
    assert recs[0].info["items"] == sum(-(-g // 4) for g in groups) and recs[0].info["launches"] == 2 and recs[0].info["step_kernel"] is True


def test_three_bodies_and_tiles_in_one_queue(torch_mod):
    """H-C: 1024-thread half groups read from a batch layout, 256-thread half groups, compact fp32 groups, wide groups and the tiles of two
    tile streams (one of them bf16: 32-bit slots all the same) in one queue, under the three queue orders: the same bits each time."""
    mats = H.case_hc()
    first = None
    for order in ("", "lpt", "grid"):
        env = dict(H.half_env(S.AUTO), **({"HISPMV_STEP_ORDER": order} if order else {}))
        label = f"case H-C (order {order or 'default'})"
        storage = []
        script = _with_storage_info(_script([list(range(len(mats)))], S.PAIRS), storage)
        if first is None:
            info, recs = _step_and_grids(torch_mod, env, mats, script, label)
            first = [r.snap.cpu().numpy().view(np.int32) for r in recs]
        else:
            bits, info, recs = _play(torch_mod, env, mats, script, label, step=True)
            for a, b in zip(first, bits):
                assert np.array_equal(a, b), f"{label}: other bits than under the default order"
        _half_as_marked(mats, storage[0])
        assert info[0]["block_threads"] == 1024 and info[0]["batch_group_slices"] > info[0]["group_slices"], info[0]      # the half batch layout is what ran
        assert info[1]["format"] == 1 and info[2]["format"] == 1 and info[2]["n_split_rows"] > 0
        assert info[5]["compact_slices"] > 0 and storage[0][5]["slots_2byte"] == 0                                       # compact fp32 groups in the same queue
        assert all(r.info["step_kernel"] is True for r in recs)


def test_stray_slots_and_a_stray_split_next_to_half_groups(torch_mod):
    """H-D: a bf16 part whose half groups have stray slots (spmv_step_kernel<true, 1>: the stray fetch next to half slices) with
    neighbours of both storages; and a bf16 stray split -- a half windowed part, a wide stray part into a partial vector, merged in the tail."""
    for maker, label in ((H.case_hd_stray_slots, "case H-D (stray slots)"), (H.case_hd_stray_split, "case H-D (stray split)")):
        mats = maker()
        storage = []
        script = _with_storage_info(_script([list(range(len(mats)))], S.PAIRS), storage)
        info, recs = _step_and_grids(torch_mod, H.half_env(S.SLICES), mats, script, label)
        _half_as_marked(mats, storage[0])
        if maker is H.case_hd_stray_slots:
            assert info[0]["block_threads"] == 1024 and info[0]["group_slices"] > 16 and info[0]["compact_slices"] == info[0]["n_slices"], info[0]
        else:
            assert info[0]["tile_kind"] == 3 and info[0]["col_tiles"] == 2, info[0]
        assert all(r.info["step_kernel"] is True for r in recs)


def test_few_items_and_alternating_kernels(torch_mod):
    """H-B: the smallest windowed bf16 input alone (32 items < CUs: the exit counter rearms against that grid size), a half call of more
    items than CUs and an all-fp32 call (spmv_step_kernel<., 0> as ever) in one context, then a-b-c-a-b-c on one stream without host
    synchronisation: each cached plan has its own sync words, and the two kernels alternate."""
    mats, one, big, fp32 = H.case_hb()

    def script(cx):
        recs = _script([one, big, fp32], S.PAIRS)(cx)
        calls = [cx.prepare(sel) for sel in (one, big, fp32)]
        for alpha, beta in S.PAIRS:
            for _ in range(2):
                recs += [cx.issue(c, alpha, beta) for c in calls]
        return recs
    info, recs = _step_and_grids(torch_mod, H.half_env(S.SLICES), mats, script, "case H-B")
    seen = {tuple(r.call.sel): r.info["items"] for r in recs}
    assert seen[tuple(one)] == 32 and seen[tuple(big)] > N_CUS and 0 < seen[tuple(fp32)] < N_CUS, seen
    assert all(mats[k].get("storage", "fp32") == "fp32" for k in fp32) and info[one[0]]["lds_bytes"] > 0


def test_the_switch(torch_mod):
    """H-S: a context created WITHOUT the environment variable runs the H-C call as grids (today's behaviour); after set_step_half(True)
    the same call signature runs as the step kernel, after set_step_half(False) as grids again -- the same bits every time.  A value
    other than 0 or 1 is refused and changes nothing."""
    from hispmv_amd import _lib
    mats = H.case_hc()
    sel = list(range(len(mats)))
    with Ctx(torch_mod, S.AUTO, mats) as cx:
        call = cx.prepare(sel)
        runs = []
        for state, step in ((None, False), (True, True), (False, False), (True, True)):
            if state is not None:
                cx.h.set_step_half(state)
            assert _lib.lib.hispmv_set_step_half(cx.h._ctx, 2) == _lib.HISPMV_EINVAL
            assert _lib.lib.hispmv_set_step_half(cx.h._ctx, -1) == _lib.HISPMV_EINVAL
            runs.append((step, [cx.issue(call, alpha, beta) for alpha, beta in S.PAIRS for _ in range(3)]))
        first = None
        for n, (step, recs) in enumerate(runs):
            label = f"case H-S (state {n}: step kernel {step})"
            wrong = [msg for msg in (_account(cx, r, step, label) for r in recs) if msg]
            assert not wrong, wrong[0]
            assert all(r.info["step_kernel"] is step for r in recs)
            bits = [cx.check(r, label) for r in recs]
            if first is None:
                first = bits
            for a, b in zip(first, bits):
                assert np.array_equal(a, b), f"{label}: other bits than the first state's"
        fp32_only = cx.prepare([3, 4, 5])                                 # no half group in the call: the step kernel in either state
        cx.h.set_step_half(False)
        off = [cx.issue(fp32_only, *S.PAIRS[0])]
        cx.h.set_step_half(True)
        on = [cx.issue(fp32_only, *S.PAIRS[0])]
        for r in off + on:
            assert _account(cx, r, True, "case H-S (fp32 call)") is None and r.info["step_kernel"] is True, r.info
        assert np.array_equal(cx.check(off[0], "case H-S (fp32 call, off)"), cx.check(on[0], "case H-S (fp32 call, on)"))


def test_updates_reach_the_half_batch_layout(torch_mod):
    """H-U: an updatable bf16 handle with a batch layout (the H-C band) in a step call; update_values_device with values that are not
    bf16-exact (the device rounds them, into the first layout AND into the half slices of the batch layout, which only the step call
    reads); the step call again.  Every y equals, bit for bit, the CPU model of the rounded new values, the grids of the same context
    (set_step_half(False)) and the step call of a fresh bf16 context created from the rounded new values -- and differs from the y
    before the update."""
    c = H.case_hc()
    mats = [c[0], c[6], c[3]]                                            # the band, a 256-thread half part, a wide fp32 part
    v1, r1 = H.new_values(mats[0])
    after_mats = [H.updated(mats[0], r1)] + mats[1:]
    env = H.half_env(S.AUTO)
    sel = [0, 1, 2]
    with H.UpdatableCtx(torch_mod, env, mats) as cx:
        up = cx.h.value_update_info(cx.idx[0])
        assert up["updatable"] and up["n"] == v1.size and up["written"] > up["map_slots"], up            # the second destination exists
        assert cx.info[0]["batch_group_slices"] > cx.info[0]["group_slices"] and cx.h.value_storage_info(cx.idx[0])["slots_2byte"] > 0
        call = cx.prepare(sel)
        before = [cx.issue(call, alpha, beta) for alpha, beta in S.PAIRS]
        bits_before = [cx.check(r, "case H-U (before the update)") for r in before]
        assert all(_account(cx, r, True, "case H-U (before)") is None for r in before), [r.info for r in before]
        dv = torch_mod.from_numpy(v1).to(cx.dev)
        torch_mod.cuda.synchronize()
        cx.h.update_values_device(cx.idx[0], dv.data_ptr(), dv.numel(), cx.stream.cuda_stream)          # ordered on the calls' stream
        cx.mats = after_mats                                              # from here on the models are those of the new values
        cx.pk[0] = S.packed(after_mats[0], cx.info[0])
        step = [cx.issue(call, alpha, beta) for alpha, beta in S.PAIRS]
        cx.h.set_step_half(False)
        grids = [cx.issue(call, alpha, beta) for alpha, beta in S.PAIRS]
        bits_step = [cx.check(r, "case H-U (step kernel after the update)") for r in step]
        bits_grids = [cx.check(r, "case H-U (grids after the update)") for r in grids]
        for r in step:
            assert _account(cx, r, True, "case H-U (step)") is None, r.info
        for r in grids:
            assert _account(cx, r, False, "case H-U (grids)") is None, r.info
        for a, b, old in zip(bits_step, bits_grids, bits_before):
            assert np.array_equal(a, b), "case H-U: the step call after the update differs from the grids of the same context"
            assert not np.array_equal(a, old), "case H-U: the update changed nothing"
    fresh, _, recs = _play(torch_mod, env, after_mats, _script([sel], S.PAIRS, reps=1), "case H-U (fresh handles)", step=True)
    for a, b in zip(bits_step, fresh):
        assert np.array_equal(a, b), "case H-U: the step call after the update differs from a fresh handle's"
