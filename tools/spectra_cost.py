"""What the spectra (sg_set_spectra, kernels_spectra.hip) cost, measured on one GPU in one job; the numbers of DESIGN.md
"Spectra" and profiles/r10/spectra.txt.

  python tools/spectra_cost.py [--parent-lib PATH] [--only c3|2d]

  - config 3's block (64^3 x 6, P4, FP64, symmetric storage) and the 2-D N = 256 P4 mesh: the step time (sg_last_step_ms of
    one sg_step(steps), per step) with 1 and with 4 frequencies of both fields armed and a sample after every step, against
    the same handle with nothing armed, alternating run by run, median of 5; and the effective rate of the added time,
    (1 + 4 nfreq) x 8 B x accumulated words / added time;
  - with --parent-lib: the step time of this library with nothing armed and of the parent commit's, alternating child
    processes, median of 5.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"c3": (3, 4, (64, 64, 64)), "2d": (2, 4, (256, 256))}
NEW_SYMBOLS = ("sg_set_spectra", "sg_get_spectrum", "sg_spectra_samples", "sg_correlate_spectra", "sg_spectra_clock", "sg_spectra_lines")
NFREQS = (1, 4)


def make_block(config, seed):
    from seigen_amd import _lib
    from seigen_amd.backend import HipBlock
    dim, degree, n = CONFIGS[config]
    h = [1.0 / k for k in n]
    blk = HipBlock(dim, degree, n, h, [0.0] * dim)
    blk.set_params(1.0, 0.05 * min(h) / degree ** 2, 0.5, 0.25)
    # smooth-sized non-zero values, one chunk of cells repeated over the block (the cost does not depend on the values)
    rng = np.random.default_rng(seed)
    chunk = 12288
    u = rng.uniform(-1, 1, (chunk, blk.nd, dim))
    s = rng.uniform(-1, 1, (chunk, blk.nd, dim, dim))
    s = 0.5 * (s + np.swapaxes(s, -1, -2))
    for c0 in range(0, blk.ncells, chunk):
        m = min(chunk, blk.ncells - c0)
        blk.set_field_range(_lib.FIELD_U, c0, u[:m])
        blk.set_field_range(_lib.FIELD_S, c0, s[:m])
    return blk


def armed_against_unarmed(config, steps):
    dim, degree, _ = CONFIGS[config]
    blk = make_block(config, 1)
    lines = dim * (dim + 1) // 2 if blk.is_sym() else dim * dim       # stress lines accumulated per node
    words = blk.ncells * blk.nd * (dim + lines)
    blk.step(steps)
    ms = {0: []}
    ms.update({nf: [] for nf in NFREQS})
    for _ in range(5):
        for nf in (0,) + NFREQS:
            if nf == 0:
                blk.set_spectra(None, None)
            else:
                w = np.zeros((steps, nf, 2))
                w[..., 0], w[..., 1] = 1e-3, -1e-3
                blk.set_spectra(w, w, 1)
            blk.step(steps)
            ms[nf].append(blk.last_step_ms() / steps)
            if nf:
                assert blk.spectra_samples() == steps
    name = blk.stage_kernel_name(0)
    blk.set_spectra(None, None)
    blk.close()
    x = float(np.median(ms[0]))
    print("%s %r P%d (%s, %s storage, %.3e accumulated words): step with nothing armed %.4f ms, runs %s"
          % (config, CONFIGS[config][2], degree, name, "symmetric" if lines < dim * dim else "full", words, x, ["%.4f" % v for v in ms[0]]))
    for nf in NFREQS:
        y = float(np.median(ms[nf]))
        rate = (1 + 4 * nf) * 8.0 * words / (1e-3 * (y - x)) / 1e12 if y > x else float("nan")
        print("%s nfreq = %d, both fields, a sample every step: %.4f ms: %+.1f us (%+.1f %%), (1 + 4 nfreq) x 8 B x words / added time = "
              "%.2f TB/s; runs %s" % (config, nf, y, 1e3 * (y - x), 100 * (y / x - 1), rate, ["%.4f" % v for v in ms[nf]]))


def child_step(config, steps, parent):
    if parent:      # the parent commit's library has no spectra: bind what it exports
        from seigen_amd import _lib
        for name in NEW_SYMBOLS:
            _lib.SYMBOLS.pop(name)
    blk = make_block(config, 1)
    blk.step(steps)
    ms = []
    for _ in range(3):
        blk.step(steps)
        ms.append(blk.last_step_ms() / steps)
    print(json.dumps({"ms_per_step": float(np.median(ms))}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--only", choices=tuple(CONFIGS), default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-parent", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--steps", type=int, default=40)
    args = ap.parse_args()
    if args.child:
        return child_step(args.child, args.steps, args.child_parent)
    for config in CONFIGS:
        if args.only not in (None, config):
            continue
        armed_against_unarmed(config, args.steps)
        sys.stdout.flush()
        if not args.parent_lib:
            continue
        res = {"this": [], "parent": []}
        for _ in range(5):
            for name, lib in (("this", None), ("parent", args.parent_lib)):
                env = dict(os.environ)
                if lib:
                    env["SEIGEN_HIP_LIB"] = lib
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", config, "--steps", str(args.steps)] +
                                   (["--child-parent"] if lib else []),
                                   env=env, capture_output=True, text=True, timeout=300)
                if r.returncode != 0:
                    print("child failed (%s): %s" % (name, r.stderr[-800:]))
                    return 1
                res[name].append(json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step"])
        x, y = np.median(res["this"]), np.median(res["parent"])
        print("%s step, nothing armed: this %.4f ms, parent %.4f ms (%+.2f %%); runs this %s parent %s; spread this %.2f %% parent %.2f %%"
              % (config, x, y, 100 * (x / y - 1), ["%.4f" % v for v in res["this"]], ["%.4f" % v for v in res["parent"]],
                 100 * (max(res["this"]) - min(res["this"])) / x, 100 * (max(res["parent"]) - min(res["parent"])) / y))
        sys.stdout.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
