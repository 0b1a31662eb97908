"""What the monitor (sg_measure / sg_set_monitor, kernels_measure.hip) costs, measured on one GPU in one job; the numbers
of DESIGN.md "Monitor" and profiles/r07/monitor.txt.

  python tools/monitor_cost.py [--parent-lib PATH] [--hbm PATH]

  - one sg_measure of config 3's block (64^3 x 6, P4, FP64, symmetric storage) from an event pair on the handle's stream,
    beside the time in which tools/ubench_hbm's read-only loop streams the same bytes (its best rate, scaled), and the ratio;
  - the step time (sg_last_step_ms, median of 5 alternating runs) unarmed / every = 10 / every = 1 on that block and on the
    reference's 2-D N = 256 P4 mesh;
  - with --parent-lib: the unarmed step time of this library and of the parent commit's, alternating child processes.
Pass 2 alone: run `--only measure` under `rocprofv3 --kernel-trace --stats` and read the two kernels' rows.
"""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"c3": (3, 4, (64, 64, 64)), "2d": (2, 4, (256, 256))}


def make_block(key):
    from seigen_amd import _lib
    from seigen_amd.backend import HipBlock
    dim, degree, n = CONFIGS[key]
    h = [1.0 / k for k in n]
    blk = HipBlock(dim, degree, n, h, [0.0] * dim)
    blk.set_params(1.0, 0.05 * min(h) / degree ** 2, 0.5, 0.25)
    # smooth-sized values, one chunk of cells repeated over the block (the cost does not depend on the values)
    rng = np.random.default_rng(1)
    chunk = 12288
    u = rng.uniform(-1, 1, (chunk, blk.nd, dim))
    s = rng.uniform(-1, 1, (chunk, blk.nd, dim, dim))
    s = 0.5 * (s + np.swapaxes(s, -1, -2))
    for c0 in range(0, blk.ncells, chunk):
        m = min(chunk, blk.ncells - c0)
        blk.set_field_range(_lib.FIELD_U, c0, u[:m])
        blk.set_field_range(_lib.FIELD_S, c0, s[:m])
    assert blk.is_sym() or dim < 2
    return blk


def field_bytes(blk):
    d = blk.dim
    ncomp = d + (d * (d + 1) // 2 if blk.is_sym() else d * d)
    return blk.ncells * blk.nd * ncomp * 8


def time_measure(blk, reps=20):
    """one sg_measure between two HIP events on the handle's stream (the runtime's own calls, bound with ctypes)"""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    stream = C.c_void_p(blk.stream_ptr())
    w = np.array([0.5, 1.0, -0.25])

    def ok(rc):
        if rc != 0:
            raise RuntimeError("HIP runtime error %d" % rc)

    e0, e1 = C.c_void_p(), C.c_void_p()
    ok(hip.hipEventCreate(C.byref(e0)))
    ok(hip.hipEventCreate(C.byref(e1)))
    blk.measure(w)
    ms = []
    for _ in range(reps):
        ok(hip.hipEventRecord(e0, stream))
        blk.measure(w)
        ok(hip.hipEventRecord(e1, stream))
        ok(hip.hipEventSynchronize(e1))
        t = C.c_float()
        ok(hip.hipEventElapsedTime(C.byref(t), e0, e1))
        ms.append(t.value)
    ok(hip.hipEventDestroy(e0))
    ok(hip.hipEventDestroy(e1))
    return float(np.median(ms)), float(np.min(ms))


def step_ms(blk, every, steps):
    w = np.array([0.5, 1.0, -0.25])
    blk.set_monitor(every, steps // every if every else 0, w if every else None)
    blk.step(steps)
    return blk.last_step_ms() / steps


def hbm_read_rate(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300).stdout
    rates = [float(m.group(1)) for m in re.finditer(r"reads=\s*\d+ writes=\s*0 .*?, (\d+) GB/s", out)]
    return max(rates), out


def child_unarmed(key, steps, parent):
    if parent:      # the parent commit's library has no monitor: bind what it exports
        from seigen_amd import _lib
        for name in ("sg_measure", "sg_set_monitor", "sg_get_monitor"):
            _lib.SYMBOLS.pop(name)
    blk = make_block(key)
    blk.step(steps)
    ms = []
    for _ in range(3):
        blk.step(steps)
        ms.append(blk.last_step_ms() / steps)
    print(json.dumps({"ms_per_step": float(np.median(ms))}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--hbm", default=os.path.join(ROOT, "build_tools", "ubench_hbm"))
    ap.add_argument("--only", choices=("measure", "steps", "parent"), default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-parent", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--steps", type=int, default=40)
    args = ap.parse_args()
    if args.child:
        return child_unarmed(args.child, args.steps, args.child_parent)
    if args.only in (None, "measure"):
        blk = make_block("c3")
        med, best = time_measure(blk)
        nbytes = field_bytes(blk)
        print("config 3 block: sg_measure %.3f ms median, %.3f ms best of 20 (event pair); %.3f GB of u and s -> %.0f GB/s"
              % (med, best, nbytes / 1e9, nbytes / med / 1e6))
        if os.path.exists(args.hbm):
            rate, raw = hbm_read_rate(args.hbm)
            t = nbytes / rate / 1e6
            print("ubench_hbm read-only loop, best rate %.0f GB/s: the same bytes in %.3f ms; sg_measure / stream = %.2f"
                  % (rate, t, med / t))
        blk.close()
    if args.only in (None, "steps"):
        for key in ("c3", "2d"):
            blk = make_block(key)
            steps = args.steps if key == "c3" else 10 * args.steps
            blk.step(steps)
            runs = {0: [], 10: [], 1: []}
            for _ in range(5):
                for every in (0, 10, 1):
                    runs[every].append(step_ms(blk, every, steps))
            blk.set_monitor(0, 0)
            med = {k: float(np.median(v)) for k, v in runs.items()}
            print("%s %r P%d: step %.4f ms unarmed, %.4f ms every = 10 (%+.2f %%), %.4f ms every = 1 (%+.2f %%); runs %s"
                  % (key, CONFIGS[key][2], CONFIGS[key][1], med[0], med[10], 100 * (med[10] / med[0] - 1), med[1],
                     100 * (med[1] / med[0] - 1), {k: ["%.4f" % x for x in v] for k, v in runs.items()}))
            blk.close()
    if args.only in (None, "parent") and args.parent_lib:
        res = {"this": [], "parent": []}
        for _ in range(5):
            for name, lib in (("this", None), ("parent", args.parent_lib)):
                env = dict(os.environ)
                if lib:
                    env["SEIGEN_HIP_LIB"] = lib
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "c3", "--steps", str(args.steps)] +
                                   (["--child-parent"] if lib else []),
                                   env=env, capture_output=True, text=True, timeout=300)
                if r.returncode != 0:
                    print("child failed (%s): %s" % (name, r.stderr[-800:]))
                    return 1
                res[name].append(json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step"])
        a, b = np.median(res["this"]), np.median(res["parent"])
        print("config 3 unarmed step: this %.4f ms, parent %.4f ms (%+.2f %%); runs this %s parent %s; spread this %.2f %% parent %.2f %%"
              % (a, b, 100 * (a / b - 1), ["%.4f" % x for x in res["this"]], ["%.4f" % x for x in res["parent"]],
                 100 * (max(res["this"]) - min(res["this"])) / a, 100 * (max(res["parent"]) - min(res["parent"])) / b))
    return 0


if __name__ == "__main__":
    sys.exit(main())
