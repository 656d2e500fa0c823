#!/usr/bin/env python3
"""Print the table of DESIGN section 2 for the reference runs off the defaults (tests/golden/params/): per fixture the
cars compared teacher-forced, oracle against reference, the shares of bit-equal v and x values, the largest distance in
ulp and the cars beyond conftest's float bound (tests/test_oracle_params.py states the bars and asserts them); then the
same columns for the runs from loaded ring states (tests/golden/states/, tests/test_oracle_states.py) and the tallies of
the branches the reference took in each of them.  CPU only.

Usage:  python tools/params_fixture_table.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "traffic-env_amd"), ROOT):
    sys.path.insert(0, p)

import test_oracle_states as states  # noqa: E402
from test_oracle_params import fixture, param_names, teacher_forced  # noqa: E402


def main():
    for name in param_names():
        tally = teacher_forced(fixture(name))
        print(tally.row())
        for car in tally.beyond:
            print("   tick %d: v %.7g -> reference %.7g, oracle %.7g: %d ulp, |dv| %.3g, bound %.3g" % car)
    for name in states.SCENARIOS:
        states.print_tally(states.teacher_forced(states.fixture(name)))
    for name in states.SCENARIOS:
        print("%-30s %s" % (name, "  ".join("%s %d" % (k, states.fixture(name).tally(k)) for k in states.TALLIES)))


if __name__ == "__main__":
    main()
