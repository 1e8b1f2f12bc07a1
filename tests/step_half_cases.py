"""Inputs of tests/test_gpu_step_half.py (batch calls with bf16 handles through the step kernel, hispmv_set_step_half /
HISPMV_STEP_HALF=1), in one place: which matrices of tests/step_small_cases.py are created under bf16 value storage in each case, which
of their parts must come out with HALF groups and which must stay wide, and two helpers of the harness (a context whose handles are
updatable, the half groups of a part from the host packer).  tests/test_step_half_host.py checks the premises on the host (no GPU).
No product code; not a test module and not a conftest."""
from __future__ import annotations

import numpy as np

import step_small_cases as S
from step_small_harness import Ctx

HALF = {"HISPMV_STEP_HALF": "1"}
GROUP_COMPACT, GROUP_STRAYS, GROUP_HALF = 1, 2, 4        # bits of groups[].w (hispmv_format.h)


def half_env(env):
    return dict(env, **HALF)


def part_entries(m, info):
    """The COO entries of every slice part of the matrix: one part, or the two parts of a stray split (tests/util.py: prepared_tiles)."""
    r, c, v = m["r"], m["c"], m["v"]
    if info["col_tiles"] <= 1:
        return [(r, c, v)]
    assert info["tile_kind"] == 3 and info["col_tiles"] == 2, info
    from hispmv_amd.prep import window_membership
    inside, order = window_membership(r, c, v, m["rows"], m["cols"], 256)
    keep = np.zeros(r.size, dtype=bool)
    keep[order] = inside.astype(bool)
    return [(r[keep], c[keep], v[keep]), (r[~keep], c[~keep], v[~keep])]


def group_kinds(m, info, env, storage="bf16"):
    """Per slice part of the matrix, from the host packer under the case's switches (prep.device_layout_from_coo, every part planned on
    its own at 256 CUs): dict(half=, compact=, strays=, groups=) -- the groups whose w has the half bit, the compact ones that are not half,
    the ones with stray slots, all groups."""
    from hispmv_amd import prep
    out = []
    with S.environment(env):
        for r, c, v in part_entries(m, info):
            lay = prep.device_layout_from_coo(r, c, v, m["rows"], m["cols"], value_storage=storage)
            w = lay["dgroups"][:, 3] if lay["dgroups"].size else np.zeros(0, np.int32)
            out.append(dict(half=int(((w & GROUP_HALF) != 0).sum()), compact=int((((w & GROUP_COMPACT) != 0) & ((w & GROUP_HALF) == 0)).sum()),
                            strays=int(((w & GROUP_STRAYS) != 0).sum()), groups=int(w.size), threads=lay["threads"], group_slices=lay["group_slices"]))
    return out


def mark(mats, bf16, half):
    """The matrices at the indices `bf16` through S.as_bf16; m["half"] = per slice part, whether the case calls it half (True), wide
    (False: a bf16 or fp32 part without a half group); tile streams carry no mark."""
    out = []
    for k, m in enumerate(mats):
        m = S.as_bf16(m) if k in bf16 else dict(m)
        m["half"] = half.get(k, (False,) * m["expect"].get("parts", 1)) if m["expect"]["format"] == 0 else None
        out.append(m)
    return out


# ---- H-A: half sub-blocks past the last group ---------------------------------------------------------------------------------------
def case_ha():
    """S.case_a(), every matrix bf16: the two windowed 256-thread parts (147 and 293 groups: residues 3 and 1 mod 4) get half groups, the
    window-less parts stay wide (32-bit slots that hold bf16-exact values, read by the half kernel's wide body)."""
    mats = S.case_a()
    return mark(mats, set(range(len(mats))), {6: (True,), 7: (True,)})


# ---- H-C: three bodies and tiles in one queue -----------------------------------------------------------------------------------------
def case_hc():
    """S.case_c(): big_band (1024-thread groups; its batch layout is what a step call reads) and the 293-group windowed 256-thread band as
    bf16; the 147-group windowed part stays fp32 (compact fp32 groups next to half groups); tile_stream is bf16 (32-bit slots all the
    same), tts_cut_row fp32; the two window-less parts stay fp32 and wide."""
    return mark(S.case_c(), {0, 1, 6}, {0: (True,), 6: (True,)})


# ---- H-D: stray slots, a stray split ----------------------------------------------------------------------------------------------------
def _neighbours():
    a = S.case_a()
    return [a[0], a[3], a[5], a[6], a[7], a[8]]


def case_hd_stray_slots():
    """S.stray_slot_band() as bf16 (half groups WITH stray slots: spmv_step_kernel<true, 1>) next to the small neighbours of case D: the
    9000-entry window-less part and the 147-group windowed part as bf16, the others fp32."""
    return mark([S.stray_slot_band()] + _neighbours(), {0, 2, 4}, {0: (True,), 4: (True,)})


def case_hd_stray_split():
    """S.stray_split_band() as bf16: a half windowed part and a wide stray part into a partial vector; the 293-group band as bf16 too."""
    return mark([S.stray_split_band()] + _neighbours(), {0, 5}, {0: (True, False), 5: (True,)})


# ---- H-B: few items, alternating kernels --------------------------------------------------------------------------------------------------
def small_windowed():
    """The smallest windowed input the planner gives: a stream of fewer than 512 slices never gets a window (hispmv_plan.cpp: make_plan),
    and this one has exactly 512 -- 128 groups of a 256-thread plan, 32 queue items (the same matrix with 522 000 entries: 510 slices,
    no window)."""
    return S.uniform(3000, 2500, 524000, 21, dict(format=0, threads=256, window=True, groups=128))


def case_hb():
    """-> (mats, one, big, fp32): case H-A's matrices, the small windowed input and big_band as bf16, two fp32 bands; the call of the
    small input alone, a call of more items than CUs with half parts, and an all-fp32 call."""
    mats = case_ha()
    n = len(mats)
    e = S.case_a()[7]["expect"]
    mats += mark([small_windowed(), S.big_band(), S.band(4000, 300, 19, e), S.band(4000, 300, 20, e)], {0, 1}, {0: (True,), 1: (True,), 2: (False,), 3: (False,)})
    return mats, [n], [n + 1, 6, 7, n + 2, n + 3, 5, 9, 10], [n + 2, n + 3]


# ---- H-U: updates reach the half batch layout -----------------------------------------------------------------------------------------------
def new_values(m, seed=77):
    """Values that are NOT bf16-exact (the device rounds them), and the same rounded once on the host: what a fresh bf16 handle stores."""
    rng = np.random.default_rng(seed)
    v1 = rng.random(m["v"].size, dtype=np.float32) * np.float32(3.0) - np.float32(1.0)
    assert np.any(v1.view(np.uint32) & 0xFFFF != 0)
    return v1, S.bf16_exact(v1)


def updated(m, v):
    """The matrix with other values under another name (the harness caches packed streams and references by name)."""
    return dict(m, name=m["name"] + "_updated", v=v)


class UpdatableCtx(Ctx):
    """The harness's context with every handle created under set_value_updates("any_storage").  The harness creates its context itself and has
    no hook between creation and the first handle, so for the duration of Ctx.__init__ the module attribute pyhispmv.FpgaHandle is replaced
    by a factory that sets the switch (restored in a finally).  This relies on the harness calling `pyhispmv.FpgaHandle(...)` through the
    module: should it ever import the class another way, the handles come out not updatable and the H-U test says so at its first assertion
    (value_update_info()["updatable"])."""

    def __init__(self, torch, env, mats):
        import pyhispmv
        real = pyhispmv.FpgaHandle

        def make(*args):
            h = real(*args)
            h.set_value_updates("any_storage")
            return h
        pyhispmv.FpgaHandle = make
        try:
            super().__init__(torch, env, mats)
        finally:
            pyhispmv.FpgaHandle = real
