"""Writes tests/golden/lifetime_floor.json: per FP64 case of tests/lifetime_script.py and per checkpoint of its script, the
largest relative difference of the four fields between the mirror run through the numpy oracle and through the plain-C port
(tests/test_lifetime_oracle.py measure_floor).  Numbers only."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests.test_lifetime_oracle import FLOOR_FILE, FP64, measure_floor  # noqa: E402

if __name__ == "__main__":
    floor = {}
    for case in FP64:
        floor[case.name] = [float("%.3e" % v) for v in measure_floor(case)]
        print(case.name, "%.2e .. %.2e" % (min(floor[case.name]), max(floor[case.name])))
    with open(FLOOR_FILE, "w") as f:
        json.dump(floor, f, indent=0, sort_keys=True)
        f.write("\n")
