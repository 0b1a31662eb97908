"""What the point injectors (sg_set_injectors, kernels_inject.hip) cost, measured on one GPU in one job; the numbers of
DESIGN.md "Injectors" and profiles/r09/injectors.txt.

  python tools/inject_cost.py [--parent-lib PATH] [--only c3|2d]

  - config 3's block (64^3 x 6, P4, FP64, symmetric storage) and the 2-D N = 256 P4 mesh: the step time (sg_last_step_ms of
    one sg_step(steps), per step) with 1000 velocity injectors at random points adding an entry at every step, against the
    same handle with nothing armed, alternating run by run, median of 5;
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
NEW_SYMBOLS = ("sg_injector_weights", "sg_inject", "sg_set_injectors")
NPOINTS = 1000


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
    dim = CONFIGS[config][0]
    blk = make_block(config, 1)
    rng = np.random.default_rng(2)
    pts = rng.uniform(0.0, 1.0, (NPOINTS, dim))
    series = 1e-6 * rng.uniform(-1.0, 1.0, (steps, NPOINTS, dim))
    blk.step(steps)
    ms = {"unarmed": [], "armed": []}
    for _ in range(5):
        blk.set_injectors(pts, None)
        blk.step(steps)
        ms["unarmed"].append(blk.last_step_ms() / steps)
        assert blk.set_injectors(pts, series, 1).all()
        blk.step(steps)
        ms["armed"].append(blk.last_step_ms() / steps)
    name = blk.stage_kernel_name(0)
    blk.close()
    x, y = float(np.median(ms["unarmed"])), float(np.median(ms["armed"]))
    print("%s %r P%d (%s): step with nothing armed %.4f ms, with %d velocity injectors adding an entry every step %.4f ms: %+.1f us "
          "(%+.2f %%); runs unarmed %s armed %s" % (config, CONFIGS[config][2], CONFIGS[config][1], name, x, NPOINTS, y, 1e3 * (y - x),
                                                    100 * (y / x - 1), ["%.4f" % v for v in ms["unarmed"]], ["%.4f" % v for v in ms["armed"]]))


def child_step(config, steps, parent):
    if parent:      # the parent commit's library has no injectors: bind what it exports
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
    return 0


if __name__ == "__main__":
    sys.exit(main())
