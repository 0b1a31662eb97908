"""Writes tests/golden/lifetime_floor.json and tests/golden/lifetime_hooks_floor.json: per FP64 case of tests/lifetime_script.py
and per checkpoint of its script (make_script) and of its second script (make_hooks_script), the largest relative difference
of the four fields between the mirror run through the numpy oracle and through the plain-C port
(tests/test_lifetime_oracle.py measure_floor, measure_hooks_floor).  Numbers only.  `hooks` as the one argument writes the
second file alone."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests.test_lifetime_oracle import FLOOR_FILE, FP64, HOOKS_FLOOR_FILE, measure_floor, measure_hooks_floor  # noqa: E402

if __name__ == "__main__":
    jobs = [(FLOOR_FILE, measure_floor), (HOOKS_FLOOR_FILE, measure_hooks_floor)]
    for path, measure in jobs[1:] if sys.argv[1:] == ["hooks"] else jobs:
        floor = {}
        for case in FP64:
            floor[case.name] = [float("%.3e" % v) for v in measure(case)]
            print(os.path.basename(path), case.name, "%.2e .. %.2e" % (min(floor[case.name]), max(floor[case.name])))
        with open(path, "w") as f:
            json.dump(floor, f, indent=0, sort_keys=True)
            f.write("\n")
