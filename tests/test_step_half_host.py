"""Batch calls with bf16 handles through the step kernel (hispmv_set_step_half), the parts that need no device: the entry point's
argument check, and the premises of every case of tests/test_gpu_step_half.py in the manner of tests/test_step_small_inputs.py --
every input gets, from the loader's own planner at 256 CUs under the case's switches, the plan the case needs (threads, window, group
count and its residue mod 4, parts, stray slots, a batch layout where the case reads one); the host packer under bf16 value storage
gives HALF groups (groups[].w & 4) in every part the case calls half and none in the parts it calls wide; and the CPU model of each
matrix is within the 1e-5 gate for every alpha/beta pair used.  When a planner threshold moves, this test says which input of
tests/step_half_cases.py has to move with it."""
import numpy as np
import pytest

import step_half_cases as H
import step_small_cases as S
from conftest import TOL
from util import bwd_err


def test_the_entry_point_checks_its_arguments_before_any_device_call():
    from hispmv_amd import _lib
    from hispmv_amd.fpga_handle import FpgaHandle
    assert _lib.lib.hispmv_set_step_half(None, 1) == _lib.HISPMV_EINVAL
    assert _lib.lib.hispmv_set_step_half(None, 0) == _lib.HISPMV_EINVAL
    assert callable(FpgaHandle.set_step_half)


def _premises(m, env, pairs):
    """-> (info, pk, kinds): the plan (check_expect), the half / wide parts, the model within the gate."""
    info = S.host_info(m, env)
    pk = S.packed(m, info)
    S.check_expect(m, info, pk)
    kinds = None
    if info["format"] == 0:
        kinds = H.group_kinds(m, info, env, m.get("storage", "fp32"))
        assert len(kinds) == len(m["half"]) == info["col_tiles"], (m["name"], kinds, m["half"])
        for t, (k, want) in enumerate(zip(kinds, m["half"])):
            tag = (m["name"], t, k, info)
            if want:
                # (a bf16 part has no compact group that is not half; its thread count is the part's own plan)
                assert m.get("storage") == "bf16" and k["half"] > 0 and k["compact"] == 0, tag
                assert k["threads"] == info["block_threads"] and info["lds_bytes"] > 0, tag
            else:
                assert k["half"] == 0, tag
    else:
        assert m["half"] is None
    for alpha, beta in pairs:
        ye, y64, mag = S.reference(m, info, pk, alpha, beta)
        assert np.all(np.isfinite(ye)) and bwd_err(ye, y64, mag) < TOL, (m["name"], alpha, beta, bwd_err(ye, y64, mag))
    if m.get("storage") == "bf16" and not m.get("dense"):
        assert np.all(m["v"].view(np.uint32) & 0xFFFF == 0), m["name"]             # bf16-exact: the CPU models apply unchanged
    return info, pk, kinds


def _batch_layout(m, env):
    """Host-only: the number of batch layouts of the handle the loader would make under bf16 storage, slots written, map slots."""
    from hispmv_amd import prep
    with S.environment(env):
        d = prep.value_layouts_from_coo(m["r"], m["c"], m["v"], m["rows"], m["cols"], value_storage="bf16")
    return d["batch_layouts"], d["written"], d["map_slots"]


def test_case_ha_half_groups_in_the_windowed_parts_only():
    mats = H.case_ha()
    assert all(m["storage"] == "bf16" for m in mats)
    half = {}
    for k, m in enumerate(mats):
        info, pk, kinds = _premises(m, S.SLICES, S.PAIRS + S.MORE_PAIRS)
        assert info["block_threads"] == 256 and info["group_slices"] == 4 and info["col_tiles"] == 1
        if kinds[0]["half"]:
            assert kinds[0]["half"] == kinds[0]["groups"] == S.groups_of(pk[0].n_slices, 4)
            half[k] = kinds[0]["groups"]
        assert (info["lds_bytes"] > 0) == bool(kinds[0]["half"]), (m["name"], info, kinds)
    assert half == {6: 147, 7: 293} and 147 % 4 == 3 and 293 % 4 == 1, half        # last items: one and three sub-blocks past a HALF part's last group


def test_case_hc_three_bodies_tiles_and_a_batch_layout():
    mats = H.case_hc()
    seen = set()
    for k, m in enumerate(mats):
        info, pk, kinds = _premises(m, S.AUTO, S.PAIRS)
        if info["format"] == 0:
            seen.add((info["block_threads"], "half" if kinds[0]["half"] else "compact" if kinds[0]["compact"] else "wide"))
    assert {(1024, "half"), (256, "half"), (256, "compact"), (256, "wide")} <= seen, seen
    assert [m.get("storage", "fp32") for m in mats[1:3]] == ["bf16", "fp32"]         # one of the two tile streams is bf16
    assert all(S.host_info(m, S.AUTO)["format"] == 1 for m in mats[1:3])
    n, written, slots = _batch_layout(mats[0], S.AUTO)
    assert n > 0 and written > slots, (n, written, slots)                           # big_band: a second destination for every value


@pytest.mark.parametrize("maker", [H.case_hd_stray_slots, H.case_hd_stray_split])
def test_case_hd_stray_slots_and_stray_split(maker):
    mats = maker()
    for k, m in enumerate(mats):
        info, pk, kinds = _premises(m, S.SLICES, S.PAIRS)
        if k == 0 and maker is H.case_hd_stray_slots:
            assert info["block_threads"] == 1024 and info["group_slices"] > 16 and kinds[0]["strays"] > 0 and kinds[0]["half"] == kinds[0]["groups"], (info, kinds)
        if k == 0 and maker is H.case_hd_stray_split:
            assert info["tile_kind"] == 3 and info["col_tiles"] == 2 and kinds[1]["groups"] > 0, (info, kinds)
    assert {m.get("storage", "fp32") for m in mats[1:]} == {"bf16", "fp32"}          # neighbours of both storages


def test_case_hb_calls():
    mats, one, big, fp32 = H.case_hb()
    facts = {k: _premises(mats[k], S.SLICES, S.PAIRS) for k in sorted(set(one + big + fp32))}
    items = {k: S.queue_items(info, pk, shared_chip=False) for k, (info, pk, _) in facts.items()}
    (kb,) = [k for k in big if mats[k]["name"] == S.as_bf16(S.big_band())["name"]]
    (k1,) = one
    assert facts[k1][0]["lds_bytes"] > 0 and facts[k1][1][0].n_slices == 512 and items[k1] == 32 and facts[k1][2][0]["half"] == 128
    nearly = S.uniform(3000, 2500, 522000, 21, dict(format=0, threads=256, window=False))
    info = S.host_info(nearly, S.SLICES)
    S.check_expect(nearly, info, S.packed(nearly, info))                            # 510 slices: no window -- 512 is the smallest
    # (big_band's batch layout has groups up to four times as long: a quarter of its items as the lower bound)
    assert any(facts[k][2][0]["half"] for k in big) and sum(items[k] // 4 if k == kb else items[k] for k in big) > 256
    assert all(mats[k].get("storage", "fp32") == "fp32" and facts[k][2][0]["compact"] > 0 for k in fp32)


def test_case_hu_new_values_are_not_bf16_exact():
    m = H.case_hc()[0]
    v1, r1 = H.new_values(m)
    assert not np.array_equal(v1.view(np.uint32), r1.view(np.uint32)) and np.all(r1.view(np.uint32) & 0xFFFF == 0)
    assert not np.array_equal(r1, m["v"])
    u = H.updated(m, r1)
    info, pk, kinds = _premises(u, S.AUTO, S.PAIRS)
    assert kinds[0]["half"] == kinds[0]["groups"] and u["name"] != m["name"]
