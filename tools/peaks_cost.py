"""What the peak maps (sg_set_peaks, kernels_peak.hip) cost, measured on one GPU in one job; the numbers of DESIGN.md "Peak
maps" and profiles/r13/peaks.txt.

  python tools/peaks_cost.py [--only c3|2d]

  - config 3's block (64^3 x 6, P4, FP64, symmetric storage) and the 2-D N = 256 P4 mesh: the step time (sg_last_step_ms of
    one sg_step(steps), per step) with the maps off, of the velocity only, and of both fields, a sample after every step,
    on one handle, alternating run by run, median of 5;
  - beside it the byte model: per node and selected field the lines the kernel reads (dim, or the stress's dim^2 - the
    i <= j ones in symmetric storage), one read of val, and - only where the node exceeded - one write of val and a read and
    a write of idx (half a word each): lines + 1 words at least, lines + 3 at most, against the step's 90 words per node;
    and the time of both ends of the model at the rate the spectra pass reached (profiles/r10/spectra.txt).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.spectra_cost import CONFIGS, make_block  # noqa: E402

SPECTRA_RATE = 5.1e12        # B/s: (1 + 4 nfreq) x 8 B x words / added time of profiles/r10/spectra.txt, 5.08 .. 5.24 TB/s
WHATS = ((0, "off"), (1, "velocity"), (3, "velocity and stress"))


def armed_against_unarmed(config, steps):
    dim, degree, _ = CONFIGS[config]
    blk = make_block(config, 1)
    sym = blk.is_sym()
    lines = {1: dim, 3: dim + (dim * (dim + 1) // 2 if sym else dim * dim)}       # field words read per node
    fields = {1: 1, 3: 2}
    nodes = blk.ncells * blk.nd
    blk.step(steps)
    ms = {what: [] for what, _ in WHATS}
    for _ in range(5):
        for what, _ in WHATS:
            blk.set_peaks(what, 1, steps)
            blk.step(steps)
            ms[what].append(blk.last_step_ms() / steps)
            assert blk.peaks_samples() == (steps if what else 0)
    name = blk.stage_kernel_name(0)
    blk.set_peaks(0)
    blk.close()
    x = float(np.median(ms[0]))
    print("%s %r P%d (%s, %s storage, %.3e nodes): step with the maps off %.4f ms, runs %s"
          % (config, CONFIGS[config][2], degree, name, "symmetric" if sym else "full", nodes, x, ["%.4f" % v for v in ms[0]]))
    for what, tag in WHATS[1:]:
        y = float(np.median(ms[what]))
        lo, hi = 8.0 * nodes * (lines[what] + fields[what]), 8.0 * nodes * (lines[what] + 3 * fields[what])
        added = 1e-3 * (y - x)
        print("%s maps of the %s, a sample every step: %.4f ms: %+.1f us (%+.1f %%); model %d .. %d words per node against the step's 90: "
              "%.1f .. %.1f us at %.1f TB/s; (model bytes) / added time = %.2f .. %.2f TB/s; runs %s"
              % (config, tag, y, 1e3 * (y - x), 100 * (y / x - 1), lines[what] + fields[what], lines[what] + 3 * fields[what],
                 1e6 * lo / SPECTRA_RATE, 1e6 * hi / SPECTRA_RATE, SPECTRA_RATE / 1e12,
                 lo / added / 1e12 if added > 0 else float("nan"), hi / added / 1e12 if added > 0 else float("nan"),
                 ["%.4f" % v for v in ms[what]]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=tuple(CONFIGS), default=None)
    ap.add_argument("--steps", type=int, default=40)
    args = ap.parse_args()
    for config in CONFIGS:
        if args.only not in (None, config):
            continue
        armed_against_unarmed(config, args.steps)
        sys.stdout.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
