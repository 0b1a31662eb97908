"""What the gauges (sg_set_gauges, kernels_gauge.hip) cost beside the velocity receivers (sg_set_receivers, kernels_recv.hip),
measured on one GPU in one job; the numbers of DESIGN.md "Gauges" and profiles/r15/gauges.txt.

  python tools/gauge_cost.py [--only c3|2d] [--points 1000] [--steps 40]

Config 3's block (64^3 x 6, P4, FP64, symmetric storage) and the 2-D N = 256 P4 mesh: the step time (sg_last_step_ms of one
sg_step(steps), per step) on one handle with nothing armed, with 1000 velocity receivers (what = 1), with 1000 gauges of kind 0
(gradient) and with 1000 gauges of kind 3 (strain rate) at the same random points, a sample after every step, alternating run
by run, median of 5.  A receiver reads nd values per component through one thread that walks them; a gauge reads nd * dim
values through one wave whose lanes load them side by side: the expectation is that the gauges add no more than the receivers.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.spectra_cost import CONFIGS, make_block  # noqa: E402

SETTINGS = ("off", "receivers", "gauges kind 0", "gauges kind 3")


def arm(blk, setting, pts, steps):
    dim = blk.dim
    blk.set_receivers(pts if setting == "receivers" else np.zeros((0, dim)), 1, 1, steps)
    if setting.startswith("gauges"):
        blk.set_gauges(pts, int(setting[-1]), 1, steps)
    else:
        blk.set_gauges(np.zeros((0, dim)))


def armed_against_unarmed(config, steps, npoints):
    dim, degree, n = CONFIGS[config]
    blk = make_block(config, 1)
    pts = np.random.default_rng(15).uniform(0.02, 0.98, (npoints, dim))
    blk.step(steps)
    ms = {s: [] for s in SETTINGS}
    for _ in range(5):
        for s in SETTINGS:
            arm(blk, s, pts, steps)
            blk.step(steps)
            ms[s].append(blk.last_step_ms() / steps)
            if s == "receivers":
                assert blk.get_receivers().shape[0] == steps
            if s.startswith("gauges"):
                assert blk.get_gauges().shape[0] == steps
    name = blk.stage_kernel_name(0)
    arm(blk, "off", pts, steps)
    blk.close()
    x = float(np.median(ms["off"]))
    print("%s %r P%d (%s, nd = %d): step with nothing armed %.4f ms, runs %s"
          % (config, n, degree, name, blk.nd, x, ["%.4f" % v for v in ms["off"]]))
    added = {}
    for s in SETTINGS[1:]:
        y = float(np.median(ms[s]))
        added[s] = 1e3 * (y - x)
        weights = blk.nd * (1 if s == "receivers" else dim)
        print("%s %d %s, a sample every step: %.4f ms: %+.1f us (%+.2f %%); %d nodal values and %d weights a point and sample; runs %s"
              % (config, npoints, s, y, added[s], 100 * (y / x - 1), blk.nd * dim, weights, ["%.4f" % v for v in ms[s]]))
    for s in SETTINGS[2:]:
        print("%s %s against the receivers: %+.1f us against %+.1f us: the expectation %s"
              % (config, s, added[s], added["receivers"], "held" if added[s] <= added["receivers"] else "did not hold"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=tuple(CONFIGS), default=None)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--points", type=int, default=1000)
    args = ap.parse_args()
    for config in CONFIGS:
        if args.only not in (None, config):
            continue
        armed_against_unarmed(config, args.steps, args.points)
        sys.stdout.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
