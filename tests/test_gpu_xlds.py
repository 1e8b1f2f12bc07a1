"""Tile streams whose x the kernels keep in the LDS (HISPMV_TTS_XLDS=1 with HISPMV_FORMAT=tts; hispmv_kernels.hip: the XLDS branches of
tts_tile_body, spmv_tts_nv_kernel<., 1 | 2 | 4, true>, spmv_tts_multi_kernel<false, true, false>), on the harness of
tests/step_small_harness.py.  The cases (tests/step_small_cases.py: xlds_cases, checked on the host by tests/test_step_small_inputs.py):
A takes four vectors per pass with x in the LDS, B two, C one; D has the longest x that qualifies (16 384 columns), E (16 385) does not.
Every case runs in a context with the switch and in one without it; every y is checked against oracle.emu_tts on the packer's arrays
bit for bit, against the fp64 accumulation within the 1e-5 gate, for its guards (x and bias inside NaN, y between sentinels), and the
two contexts against each other bit for bit: where x is gathered from changes no bit.
Reference counterpart: none -- the reference streams x from HBM into on-chip buffers per column tile (common/src/spmv-helper.cpp:242-263)."""
import numpy as np
import pytest

import oracle
import step_small_cases as S
from step_small_harness import GRIDS, Ctx, _play, _script

pytestmark = pytest.mark.gpu

CASES = S.xlds_cases()


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def _seven_vectors(x):
    """Distinct vectors, as in tests/test_gpu_tts.py."""
    return [x, (x * np.float32(0.5)).astype(np.float32), x[::-1].copy(), (x + np.float32(0.25)).astype(np.float32),
            (x * np.float32(-1.5)).astype(np.float32), np.roll(x, 17), (x * x).astype(np.float32)]


@pytest.mark.parametrize("name", list(CASES))
def test_single_launches_and_seven_vectors(torch_mod, name):
    """spmv_device for every alpha/beta pair, twice each (both HAS_BETA instantiations), then `linear` with 7 vectors: passes of
    4, 2 and 1 vectors (A: all with x in the LDS; B: 2 + 2 + 2 + 1; C and D: 4 and 2 through the cache, the last vector from the LDS),
    each vector with the bits of its model and of its own one-vector call."""
    m = CASES[name]
    bits, lin = {}, {}
    for label, env in (("x in the LDS", S.TTS_XLDS), ("x through the cache", S.TTS)):
        with Ctx(torch_mod, env, [m]) as cx:
            assert cx.x_in_lds(0) == (env is S.TTS_XLDS and name != "E")
            tts = cx.pk[0].tts
            passes = S.linear_passes(tts, m["cols"], 7, env is S.TTS_XLDS)
            print(f'[{name}, {label}] tiles {tts["n_tiles"]} max_rows {tts["max_rows"]} max_slots {tts["max_slots"]} cut rows {tts["fix"].shape[0]} '
                  f'widths (LDS, cache) {S.tts_widths(tts, m["cols"])} passes of 7 vectors {passes}')
            call = cx.prepare([0])
            recs = [cx.issue_single(call, alpha, beta) for alpha, beta in S.PAIRS + S.MORE_PAIRS for _ in range(2)]
            bits[label] = [cx.check(r, f"{name}, {label}, spmv_device") for r in recs]
            cx.h.synchronize()                                                     # (raises when a kernel has set the context's error word)
            xs = _seven_vectors(m["x"])
            out = cx.h.linear(cx.idx[0], np.concatenate(xs), m["b"])
            for k, xk in enumerate(xs):
                yk = out[k * m["rows"]:(k + 1) * m["rows"]]
                ye = oracle.emu_tts(tts, xk, m["b"], 1.0, 1.0, m["rows"])
                assert np.array_equal(yk.view(np.uint32), ye.view(np.uint32)), f"{name}, {label}: vector {k} of 7 differs from its model (passes {passes})"
                one = cx.h.linear(cx.idx[0], xk, m["b"])
                assert np.array_equal(yk.view(np.uint32), one.view(np.uint32)), f"{name}, {label}: vector {k} of 7 differs from its one-vector call"
            lin[label] = out
    a, b = bits.values()
    assert len(a) == len(b) == 8
    for n, (p, q) in enumerate(zip(a, b)):
        assert np.array_equal(p, q), f"{name}: launch {n}: x from the LDS and x through the cache give different bits"
    assert np.array_equal(*(v.view(np.uint32) for v in lin.values()))


def _batch_mats():
    a = S.case_a()
    return [CASES["A"], CASES["B"], CASES["D"], S.tile_stream_cut_row(), S.as_slices(S.tile_stream(), threads=256), a[3],
            S.dense_shapes()[1], CASES["E"]]


def test_two_tile_stream_classes_in_one_batch_call(torch_mod):
    """A, B and D (x in the LDS) next to a standard-geometry stream whose x is far too long for it, two 256-thread slice parts and a
    dense handle: two tile grids (tts_class), a slice grid, a GeMV grid, the tail (A and the long-x stream have a row cut into
    pieces).  Then E in the place of A and D: E rides in the OTHER class.  beta != 0 and beta = 0, three repetitions back to back;
    with HISPMV_STEP_KERNEL at its default and at 0 the step kernel must refuse the call (an x-in-LDS matrix is in it)."""
    mats = _batch_mats()
    first, with_e = list(range(7)), [7, 1, 3, 5]
    script = _script([first, with_e], S.PAIRS)
    runs = {}
    for label, env in (("default", S.TTS_XLDS), ("step kernel off", dict(S.TTS_XLDS, **GRIDS)), ("x through the cache", S.TTS)):
        # (without the switch and without a dense handle the second call is one the step kernel takes)
        step = None if env is S.TTS else False
        runs[label], info, recs = _play(torch_mod, env, mats, script, f"x in the LDS, batch ({label})", step=step)
        if env is S.TTS:
            assert [r.info["step_kernel"] for r in recs[::6]] == [False, True], [r.info for r in recs[::6]]
            continue
        assert all(r.info["step_kernel"] is False and r.info["items"] == 0 and r.info["streams"] == 2 for r in recs)
        assert [r.info["launches"] for r in recs[::6]] == [2 + 1 + 1 + 1, 2 + 1 + 1], [r.info for r in recs[::6]]
    for label in ("step kernel off", "x through the cache"):
        assert len(runs[label]) == len(runs["default"]) == 12
        for n, (p, q) in enumerate(zip(runs["default"], runs[label])):
            assert np.array_equal(p, q), f"call {n}: other bits under '{label}'"
