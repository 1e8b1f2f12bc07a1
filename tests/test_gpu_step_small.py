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
from collections import namedtuple

import numpy as np
import pytest

import step_small_cases as S
from conftest import ALPHA, BETA, TOL
from util import bwd_err

pytestmark = pytest.mark.gpu

HW = ("tests.xclbin", 0, 24, 1, 1, 2, 5, True, False, True)
SHARED = {"HISPMV_BATCH_STREAMS": "2"}
GRIDS = {"HISPMV_STEP_KERNEL": "0"}
NO_PIN = {"HISPMV_NO_XCD_PIN": "1"}
GUARD = 64                         # floats: 256 bytes, so every vector keeps the 16-byte alignment of an allocation of its own
SENTINEL = 0x5EA15EA1
N_CUS = 256
MULTI_MAX = 32                     # kMultiMax (hispmv_kernels.h): entries of one grid / fix-up / merge launch
FIX_SHORT_MAX = 32                 # chains of more slices take a launch of their own and keep a cut matrix off the fused tail
TAIL_MAX_PARTS = 9

Rec = namedtuple("Rec", "call alpha beta snap info")
Call = namedtuple("Call", "sel off_x off_b off_y X B Y Y0 guard with_bias no_bias")

_PACKED = {}
_REFS = {}


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def _layout(sizes):
    off, cur = [], 0
    for n in sizes:
        cur += GUARD
        off.append(cur)
        cur = -(-(cur + n) // GUARD) * GUARD
    return off, cur + GUARD


class Ctx:
    """One context created under the case's switches with the matrices loaded; calls over subsets of them."""

    def __init__(self, torch, env, mats):
        import pyhispmv
        self.torch, self.env, self.mats = torch, dict(SHARED, **env), mats
        self.dev = torch.device("cuda", 0)
        with S.environment(self.env):
            self.h = pyhispmv.FpgaHandle(*HW)          # (the switches are read when the context is created)
        try:
            with S.environment(self.env):
                self.idx = []
                for m in mats:
                    if m.get("dense"):
                        self.idx.append(self.h.create_dense_handle(m["W"].flatten(), m["rows"], m["cols"]))
                    else:
                        self.idx.append(self.h.create_sparse_handle(m["r"], m["c"], m["v"], m["rows"], m["cols"]))
                    assert self.idx[-1] >= 0
                self.h.load_matrices()
            self.info = [self.h.matrix_info(i) for i in self.idx]
            self.pk = []
            for m, info in zip(mats, self.info):
                if m.get("dense"):
                    self.pk.append(None)
                    continue
                key = (m["name"], info["format"], info["col_tiles"], info["tile_kind"], info["col_tile_width"], info["col_tile_base"], info["group_slices"])
                if key not in _PACKED:
                    _PACKED[key] = S.packed(m, info)
                self.pk.append(_PACKED[key])
                S.check_expect(m, info, self.pk[-1])                 # the plan the case was written for, or the test fails
                assert (info["n_split_rows"] > 0) == (sum(S.cut_rows(info, self.pk[-1])) > 0), (m["name"], info)
            self.stream = torch.cuda.Stream(device=self.dev)
        except BaseException:
            self.h.close()
            raise

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.torch.cuda.synchronize()
        self.h.close()

    def prepare(self, sel):
        torch = self.torch
        ms = [self.mats[k] for k in sel]
        off_x, nx = _layout([m["cols"] for m in ms])
        off_b, nb = _layout([m["rows"] for m in ms])
        off_y, ny = _layout([m["rows"] for m in ms])
        X, B = np.full(nx, np.nan, np.float32), np.full(nb, np.nan, np.float32)
        Y0 = np.full(ny, SENTINEL, np.int32)
        guard = np.ones(ny, bool)
        for m, ox, ob, oy in zip(ms, off_x, off_b, off_y):
            X[ox:ox + m["cols"]] = m["x"]
            B[ob:ob + m["rows"]] = m["b"]
            Y0[oy:oy + m["rows"]] = np.float32(np.nan).view(np.int32)
            guard[oy:oy + m["rows"]] = False
        dX, dB, dY0 = (torch.from_numpy(a).to(self.dev) for a in (X, B, Y0.view(np.float32)))
        dY = dY0.clone()
        px = [dX.data_ptr() + 4 * o for o in off_x]
        pb = [dB.data_ptr() + 4 * o for o in off_b]
        py = [dY.data_ptr() + 4 * o for o in off_y]
        assert all(p % 16 == 0 for p in px + pb + py)
        idx = [self.idx[k] for k in sel]
        torch.cuda.synchronize()
        return Call(list(sel), off_x, off_b, off_y, dX, dB, dY, dY0, guard, self.h.prepare_batch(idx, px, pb, py), self.h.prepare_batch(idx, px, None, py))

    def issue(self, call, alpha, beta):
        """The call on the context's test stream, y copied aside and refilled with NaN behind it on the same stream; no host
        synchronisation.  -> Rec with the device-side copy and the library's account of the call."""
        with S.environment(self.env), self.torch.cuda.stream(self.stream):        # (HISPMV_NO_XCD_PIN is read when a plan is built)
            self.h.spmv_device_batch(call.with_bias if beta != 0.0 else call.no_bias, alpha, beta, self.stream.cuda_stream)
            snap = call.Y.clone()
            call.Y.copy_(call.Y0)
        return Rec(call, alpha, beta, snap, self.h.batch_call_info())

    def reference(self, k, alpha, beta):
        m, info = self.mats[k], self.info[k]
        key = (m["name"], alpha, beta) if m.get("dense") else (m["name"], alpha, beta, info["format"], info["col_tiles"], info["tile_kind"], info["col_tile_width"],
                                                                info["col_tile_base"], info["group_slices"])
        if key not in _REFS:
            _REFS[key] = S.reference(m, info, self.pk[k], alpha, beta)
        return _REFS[key]

    def check(self, rec, label):
        """Checks 1, 2 and 4 on one repetition of one call.  -> the bits of the whole y tensor (for check 3)."""
        self.torch.cuda.synchronize()
        bits = rec.snap.cpu().numpy().view(np.int32)
        out = bits.view(np.float32)
        call = rec.call
        for k, oy in zip(call.sel, call.off_y):
            m = self.mats[k]
            tag = f'{label}: {m["name"]} alpha={rec.alpha} beta={rec.beta}'
            y = out[oy:oy + m["rows"]]
            ye, y64, mag = self.reference(k, rec.alpha, rec.beta)
            bad = np.flatnonzero(y.view(np.uint32) != ye.view(np.uint32))
            assert bad.size == 0, (f"{tag}: {bad.size} of {m['rows']} rows differ from the CPU model (rows {bad[:6]} .. {bad[-3:]}), "
                                   f"{int(np.isnan(y).sum())} NaN (never written, or a read outside x)")
            err = bwd_err(y, y64, mag)
            assert err < TOL, f"{tag}: backward error {err}"
        hit = np.flatnonzero(bits[call.guard] != SENTINEL)
        assert hit.size == 0, f"{label}: {hit.size} guard words around the y vectors were overwritten (first at float {np.flatnonzero(call.guard)[hit[0]]}, vectors at {call.off_y})"
        return bits

    # ---- what the call should look like, counted from the host packer and matrix_info ------------------------------------------
    def items(self, sel):
        return sum(S.queue_items(self.info[k], self.pk[k]) for k in sel)

    def planned(self, sel, step, pin=True):
        """-> dict(launches, streams, items): the chunking of hispmv_batch.cpp applied to the parts of the call -- grids of at
        most 32 entries per class, one step launch instead of the slice and tile grids, a fused tail when at most 32 plain parts
        and 32 cut matrices (all of them fusable) are in the call, else fix-up and merge launches in chunks of 32."""
        dense = [k for k in sel if self.mats[k].get("dense")]
        tts = [k for k in sel if not self.mats[k].get("dense") and self.info[k]["format"] == 1]
        sl = [k for k in sel if not self.mats[k].get("dense") and self.info[k]["format"] == 0]
        Part = namedtuple("Part", "k threads strays slices fix single")
        queue = []                                                     # items of the slice grids: lists of parts
        for k in sl:
            info, pk, e = self.info[k], self.pk[k], self.mats[k]["expect"]
            parts = [Part(k, th, bool(e.get("stray_slots")), P.n_slices, int(P.fix.shape[0]), len(pk) == 1)
                     for P, (th, _) in zip(pk, S.part_plans(info, pk, shared_chip=step))]
            if e.get("l2_tiles") and pin:
                queue.append(parts)                                    # one XCD-pinned item of all its parts
            else:
                queue += [[p] for p in parts]
        queue.sort(key=lambda it: (-it[0].threads, it[0].strays, -sum(p.slices for p in it)))         # (stable, as the planner's)
        refs = [p for it in queue for p in it]
        mains = -(-len(dense) // MULTI_MAX)
        if step:
            assert not dense
            mains += 1
        else:
            mains += -(-len(tts) // MULTI_MAX)
            q = 0
            while q < len(queue):
                cls, n = (queue[q][0].threads, queue[q][0].strays), 0
                while q < len(queue) and (queue[q][0].threads, queue[q][0].strays) == cls and n + len(queue[q]) <= MULTI_MAX:
                    n += len(queue[q])
                    q += 1
                mains += 1
        fix = [p.fix > 0 for p in refs] + [True for k in tts if self.pk[k].tts["fix"].shape[0] > 0]
        plain = [p.fix > 0 for p in refs if p.single] + [True for k in tts if self.pk[k].tts["fix"].shape[0] > 0]
        tiled = [k for k in sl if len(self.pk[k]) > 1]
        fusable = all(len(self.pk[k]) <= TAIL_MAX_PARTS and all(int(P.fix[:, 2].max(initial=0)) <= FIX_SHORT_MAX for P in self.pk[k]) for k in tiled)
        if fusable and len(plain) <= MULTI_MAX and len(tiled) <= MULTI_MAX:
            tail = 1 if (tiled or any(plain)) else 0
        else:
            tail = sum(any(fix[q:q + MULTI_MAX]) for q in range(0, len(fix), MULTI_MAX)) + -(-len(tiled) // MULTI_MAX)
        return dict(launches=mains + tail, streams=min(2, mains), items=self.items(sel) if step else 0, step_kernel=step)


def _account(cx, rec, step, label, pin=True):
    """-> None, or what is wrong with the library's account of the call."""
    want = cx.planned(rec.call.sel, step, pin)
    return None if rec.info == want else f"{label}: the library issued the call as {rec.info}, the parts of the call imply {want}"


def _play(torch, env, mats, script, label, step=None, pin=True):
    """One context; `script(cx)` issues calls and returns their Recs; every Rec is checked (1, 2, 4) and, where `step` says how
    the calls must have been issued, accounted for.  -> the y bits of every Rec, the context's matrix_info list."""
    with Ctx(torch, env, mats) as cx:
        recs = script(cx)
        wrong = [msg for msg in (_account(cx, r, step, label, pin) for r in recs)  if msg] if step is not None else []
        try:
            bits = [cx.check(r, label) for r in recs]
        except AssertionError as e:                                    # (the first check that fails, and the account next to it)
            raise AssertionError(f"{e}" + (f"\nALSO: {wrong[0]}" if wrong else "")) from None
        assert not wrong, wrong[0]
        _report(cx, recs, label)
        return bits, cx.info, recs


def _report(cx, recs, label):
    """The facts that show what the case ran (pytest -rA prints them): per matrix its plan, per distinct call the library's account."""
    print(f"[{label}]")
    for m, i in zip(cx.mats, cx.info):
        if not m.get("dense"):
            g = S.groups_of(i["n_slices"], i["group_slices"]) if i["format"] == 0 and i["col_tiles"] == 1 else None
            print(f'  {m["name"]}: format {i["format"]} threads {i["block_threads"]} slices/group {i["group_slices"]} (batch layout {i["batch_group_slices"]}) lds_bytes {i["lds_bytes"]} '
                  f'parts {i["col_tiles"]} tile_kind {i["tile_kind"]} slices {i["n_slices"]} groups {g} (mod 4: {None if g is None else g % 4}) cut rows {i["n_split_rows"]}')
    seen = set()
    for r in recs:
        key = (tuple(r.call.sel), r.beta != 0.0)
        if key not in seen:
            seen.add(key)
            print(f'  call of {len(r.call.sel)} matrices, beta {r.beta}: {r.info}')


def _script(sels, pairs, reps=3):
    def run(cx):
        recs = []
        for sel in sels:
            call = cx.prepare(sel)
            for alpha, beta in pairs:
                recs += [cx.issue(call, alpha, beta) for _ in range(reps)]          # back to back: the queue rearms itself
        return recs
    return run


def _step_and_grids(torch, env, mats, script, label, pin=True):
    """The script under the step kernel (checks 1, 2, 4 + the account of every call), then as grids in a second context (the
    same checks), then check 3: the same bits, guards included."""
    step, info, recs = _play(torch, env, mats, script, label + " (step kernel)", step=True, pin=pin)
    grids, _, _ = _play(torch, dict(env, **GRIDS), mats, script, label + " (grids)", step=False, pin=pin)
    assert len(step) == len(grids)
    for n, (a, b) in enumerate(zip(step, grids)):
        assert np.array_equal(a, b), f"{label}: call {n}: the step kernel's y differs from the grids'"
    return info, recs


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
