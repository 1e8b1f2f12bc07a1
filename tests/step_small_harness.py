"""The harness of the small-shape GPU modules (tests/test_gpu_step_small.py, test_gpu_xlds.py, test_gpu_graph_small.py): one context
per case with the matrices of tests/step_small_cases.py loaded, batch calls over subsets of them issued without host synchronisation,
and the four checks of every y (CPU model bit for bit, fp64 within the gate, guards, the library's account of the call against counts
made here).  The checks are described in tests/test_gpu_step_small.py.  No product code; not a test module and not a conftest."""
from collections import namedtuple

import numpy as np

import step_small_cases as S
from conftest import TOL
from util import bwd_err

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
                    self.h.set_value_storage(m.get("storage", "fp32"))          # ("bf16": S.as_bf16 -- the values are bf16-exact already)
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

    def issue_single(self, call, alpha, beta):
        """The one matrix of `call` through spmv_device (its own kernels, not the batch machinery) on the test stream, from the same
        guarded tensors; beta = 0 passes no bias.  -> Rec without an account."""
        (k,), (ox,), (ob,), (oy,) = call.sel, call.off_x, call.off_b, call.off_y
        with S.environment(self.env), self.torch.cuda.stream(self.stream):
            self.h.spmv_device(self.idx[k], call.X.data_ptr() + 4 * ox, call.B.data_ptr() + 4 * ob if beta != 0.0 else 0, call.Y.data_ptr() + 4 * oy,
                               alpha, beta, self.stream.cuda_stream)
            snap = call.Y.clone()
            call.Y.copy_(call.Y0)
        return Rec(call, alpha, beta, snap, None)

    def reference(self, k, alpha, beta, mode=0):
        m, info = self.mats[k], self.info[k]
        key = (m["name"], alpha, beta) if m.get("dense") else (m["name"], alpha, beta, info["format"], info["col_tiles"], info["tile_kind"], info["col_tile_width"],
                                                                info["col_tile_base"], info["group_slices"])
        if mode != 0:
            key += (mode,)
        if key not in _REFS:
            _REFS[key] = S.reference(m, info, self.pk[k], alpha, beta, mode)
        return _REFS[key]

    def check(self, rec, label, mode=0):
        """Checks 1, 2 and 4 on one repetition of one call (mode: the carry variant of the slice model; a batch call takes 0, the
        fix-up variant).  -> the bits of the whole y tensor (for check 3)."""
        self.torch.cuda.synchronize()
        bits = rec.snap.cpu().numpy().view(np.int32)
        out = bits.view(np.float32)
        call = rec.call
        for k, oy in zip(call.sel, call.off_y):
            m = self.mats[k]
            tag = f'{label}: {m["name"]} alpha={rec.alpha} beta={rec.beta}'
            y = out[oy:oy + m["rows"]]
            ye, y64, mag = self.reference(k, rec.alpha, rec.beta, mode)
            bad = np.flatnonzero(y.view(np.uint32) != ye.view(np.uint32))
            assert bad.size == 0, (f"{tag}: {bad.size} of {m['rows']} rows differ from the CPU model (rows {bad[:6]} .. {bad[-3:]}), "
                                   f"{int(np.isnan(y).sum())} NaN (never written, or a read outside x)")
            err = bwd_err(y, y64, mag)
            assert err < TOL, f"{tag}: backward error {err}"
        hit = np.flatnonzero(bits[call.guard] != SENTINEL)
        assert hit.size == 0, f"{label}: {hit.size} guard words around the y vectors were overwritten (first at float {np.flatnonzero(call.guard)[hit[0]]}, vectors at {call.off_y})"
        return bits

    # ---- what the call should look like, counted from the host packer and matrix_info ------------------------------------------
    def x_in_lds(self, k):
        """The tile stream gathers x from the LDS: the context was created with the switch and the mirror of tts_x_in_lds agrees."""
        return "HISPMV_TTS_XLDS" in self.env and S.x_in_lds(self.pk[k].tts, self.mats[k]["cols"])

    def items(self, sel):
        return sum(S.queue_items(self.info[k], self.pk[k]) for k in sel)

    def planned(self, sel, step, pin=True):
        """-> dict(launches, streams, items): the chunking of hispmv_batch.cpp applied to the parts of the call -- grids of at
        most 32 entries per class (slice parts: thread count, stray slots; tile streams: geometry, x in the LDS -- tts_class), one step
        launch instead of the slice and tile grids, a fused tail when at most 32 plain parts and 32 cut matrices (all of them fusable)
        are in the call, else fix-up and merge launches in chunks of 32."""
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
            classes = {}                                               # the column parts of a tall-geometry stream are entries of their own
            for k in tts:
                classes.setdefault((self.info[k]["group_slices"], self.x_in_lds(k)), []).append(self.info[k]["col_tiles"])
            for entries in classes.values():
                n = 0
                for e in entries:
                    if n + e > MULTI_MAX:
                        mains, n = mains + 1, 0
                    n += e
                mains += 1
            q = 0
            while q < len(queue):
                cls, n = (queue[q][0].threads, queue[q][0].strays), 0
                while q < len(queue) and (queue[q][0].threads, queue[q][0].strays) == cls and n + len(queue[q]) <= MULTI_MAX:
                    n += len(queue[q])
                    q += 1
                mains += 1
        tts_cut = {k: S.cut_rows(self.info[k], self.pk[k]) for k in tts}            # per part of a tile stream: rows cut into pieces
        fix = [p.fix > 0 for p in refs] + [True for k in tts for n in tts_cut[k] if n > 0]
        plain = [p.fix > 0 for p in refs if p.single] + [True for k in tts if len(tts_cut[k]) == 1 and tts_cut[k][0] > 0]
        tiled = [k for k in sl if len(self.pk[k]) > 1]
        fusable = all(len(self.pk[k]) <= TAIL_MAX_PARTS and all(int(P.fix[:, 2].max(initial=0)) <= FIX_SHORT_MAX for P in self.pk[k]) for k in tiled)
        tiled += [k for k in tts if len(tts_cut[k]) > 1]                             # (two column parts: merged in the tail, always fusable)
        if fusable and len(plain) <= MULTI_MAX and len(tiled) <= MULTI_MAX and "HISPMV_NO_FUSED_TAIL" not in self.env:
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
