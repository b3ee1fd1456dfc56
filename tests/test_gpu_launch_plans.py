"""The host's launch plan for every shape of tests/launch_plan_cases.py against the record
tests/golden/launch_plans.json (tools/record_launch_plans.py, run once on the commit before
the kernel choice in csrc/nestmc.hip was gathered into one function): waves, chain blocks,
persistent, chains per block, mode, kernel, variate source, split members and batch, key for
key.  Contexts are created and destroyed; no step kernel is launched."""

import json
import os

import pytest

import launch_plan_cases as lp

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_plans.json")


def test_launch_plans_match_the_record(gpu_lib, monkeypatch):
    for k in [k for k in os.environ if k.startswith("NMC_")]:
        monkeypatch.delenv(k)
    with open(FIXTURE) as f:
        want = json.load(f)["plans"]
    assert sorted(want) == sorted(lp.BY_NAME)
    wrong = {}
    for case in lp.CASES:
        got = lp.plan(case)
        print(case.name, got)
        assert sorted(got) == sorted(want[case.name]), case.name
        diff = {k: (want[case.name][k], got[k]) for k in got if got[k] != want[case.name][k]}
        if diff:
            wrong[case.name] = diff
    assert not wrong, wrong
