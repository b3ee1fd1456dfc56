"""tests/golden/launch_plans.json without a GPU: it covers the table of
tests/launch_plan_cases.py, every case took the path it is in the table for, and the table
holds the shapes it is meant to (the thresholds between two kernels)."""

import json
import os
import re

import launch_plan_cases as lp

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_plans.json")
KEYS = ["chain_blocks", "chain_blocks_per_launch", "chains_per_block", "kernel", "mode",
        "persistent", "split_members", "waves_per_group", "zin"]


def _record():
    with open(FIXTURE) as f:
        return json.load(f)


def test_record_covers_the_table():
    rec = _record()
    assert re.fullmatch(r"[0-9a-f]{40}", rec["commit"]), rec["commit"]
    assert sorted(rec["plans"]) == sorted(lp.BY_NAME)
    for name, plan in rec["plans"].items():
        assert sorted(plan) == KEYS, name


def test_recorded_cases_took_their_path():
    plans = _record()["plans"]
    wrong = {c.name: lp.off_path(c, plans[c.name]) for c in lp.CASES
             if lp.off_path(c, plans[c.name])}
    assert not wrong, wrong


def test_table_shapes():
    by = lp.BY_NAME
    assert {len(c.sizes) for c in lp.CASES if c.name.startswith("gibbs-G")} == {
        2, 64, 65, 120, 129, 512, 513}
    assert len(set(by["ragged"].sizes)) > 1 and 0 in by["ragged"].sizes
    for c in lp.CASES:
        fam = lp.family(c)
        assert fam.n_fields == c.nf and fam.obs().shape == (sum(c.sizes), c.nf), c.name
        assert not fam.obs().any(), c.name   # (zeros: nmc_create never evaluates them)
    plans = _record()["plans"]
    # the sweep and its Gibbs kernel, whole grid and resident batches
    assert plans["cfg4-shard"]["kernel"] == lp.SWEEP_CFG4
    assert plans["cfg4-whole"]["chain_blocks_per_launch"] < plans["cfg4-whole"]["chain_blocks"]
