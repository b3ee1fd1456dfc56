#!/usr/bin/env python
"""Record what the host decides for every shape of tests/launch_plan_cases.py:

    python tools/record_launch_plans.py [--commit SHA] [--out FILE]

builds an Engine per case with no NMC_* variable set, reads launch_config() (waves, chain
blocks, persistent, chains per block, mode, kernel, zin, split members and batch), closes
it, and writes tests/golden/launch_plans.json with the commit it ran at.  No step kernel is
launched.  The file is the net under a change of the host's kernel choice: record it on the
commit BEFORE the change and never from the branch that makes it;
tests/test_gpu_launch_plans.py compares the branch with it key for key.
"""

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mcmc-for-nested-data_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", help="the commit of the library (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "launch_plans.json"))
    a = ap.parse_args()
    import launch_plan_cases as lp
    commit = a.commit or subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"],
                                                 text=True).strip()
    plans, wrong = {}, {}
    for case in lp.CASES:
        plans[case.name] = lp.plan(case)
        print(case.name, json.dumps(plans[case.name], sort_keys=True), flush=True)
        if lp.off_path(case, plans[case.name]):
            wrong[case.name] = lp.off_path(case, plans[case.name])
    if wrong:
        sys.exit("cases off their stated path (fix the case): %s" % wrong)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"commit": commit, "plans": plans}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s (%d cases, commit %s)" % (a.out, len(plans), commit))


if __name__ == "__main__":
    main()
