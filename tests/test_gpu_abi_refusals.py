"""Every refusal of the device-pointer entries -- return code and hispmv_last_error text -- is what it was before the entries were put
on one preamble (hispmv_ctx.h: find_handle, adopt_stream, LAUNCH_TRY; hispmv_spmm_abi.cpp: spmm_target, check_spmm).

tests/abi_refusal_cases.py lists the cases and collects [return code, text] for each from the loaded library;
tests/golden/abi_refusals.json holds what the library of the commit before that change answered.  A case the entry accepts is in the
list too, as [0, ""]: its arguments are real device buffers of the right size, so a refusal that went missing shows as a changed
answer, not as a fault.  After every case hispmv_synchronize must return OK (asserted while collecting)."""
import json

import pytest

import abi_refusal_cases as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def answers():
    import torch
    assert torch.cuda.is_available()
    return R.collect(torch)


@pytest.fixture(scope="module")
def golden_answers():
    return json.loads((GOLDEN / "abi_refusals.json").read_text())


def test_the_case_list_is_the_recorded_one(answers, golden_answers):
    assert sorted(answers) == sorted(golden_answers)
    refused = [k for k, v in golden_answers.items() if v[0] != 0]
    print(f"{len(golden_answers)} cases, {len(refused)} of them refusals")
    assert refused


@pytest.mark.parametrize("entry", R.ENTRIES)
def test_refusals_are_unchanged(answers, golden_answers, entry):
    mine = {k: v for k, v in answers.items() if k.split("/")[1] == entry}
    assert mine, entry
    wrong = {k: (v, golden_answers.get(k)) for k, v in mine.items() if golden_answers.get(k) != v}
    assert not wrong, wrong


def test_no_free_was_rejected():
    from hispmv_amd._lib import lib
    assert lib.hispmv_free_failures() == 0
