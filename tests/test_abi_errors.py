"""CPU test: the order and wording of the C ABI's argument and state checks that run before a
device is needed.  tests/abi_error_cases.py holds the calls; tests/golden/abi_errors.json holds what
the library answered before its host runtime was split into one file per entry family
(tests/golden/make_golden.py abi_errors).  Code and text are compared exactly."""
import json
import os

import pytest

import abi_error_cases as ac
from conftest import GOLDEN


def golden():
    with open(os.path.join(GOLDEN, "abi_errors.json")) as f:
        return {(r["entry"], r["case"]): r for r in json.load(f)}


def check(rt, cases):
    want = golden()
    got = ac.run(rt, cases)
    assert [(r["entry"], r["case"]) for r in got] == [(e, c) for e, c, _ in cases]
    for r in got:
        assert r == want[(r["entry"], r["case"])], r


def test_golden_lists_every_case():
    assert sorted(golden()) == sorted((e, c) for e, c, _ in ac.CASES + ac.CASES_NO_DEVICE)


def test_argument_checks_answer_as_recorded(rt):
    check(rt, ac.CASES)


def test_valid_calls_without_gpu_answer_as_recorded(rt):
    if rt.device_count() > 0:
        pytest.skip("a GPU is present")
    check(rt, ac.CASES_NO_DEVICE)
    codes = {r["code"] for r in golden().values() if r["case"] == "valid call, no device"}
    assert codes == {rt.RT_ERR_NODEV}
