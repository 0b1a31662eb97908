"""What the correlation (sg_correlate, kernels_xcorr.hip) costs, measured on one GPU in one job; the numbers of DESIGN.md
"Correlation" and profiles/r08/correlate.txt.

  python tools/correlate_cost.py [--parent-lib PATH] [--hbm PATH]

  - one sg_correlate of two handles on config 3's block (64^3 x 6, P4, FP64, symmetric storage) from an event pair on the
    first handle's stream, for the matrix-pipe form and for the LDS-staged one (SEIGEN_HIP_XCORR=lds), alternating call by
    call: handle a correlates against b in one form, b against a in the other, so both read the same bytes; beside the
    time in which tools/ubench_hbm's read-only loop streams those bytes (its best rate, scaled), and the ratios;
  - with --parent-lib: the step time of this library (no correlation) and of the parent commit's, alternating child
    processes, median of 5.
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

CONFIG3 = (3, 4, (64, 64, 64))
NEW_SYMBOLS = ("sg_correlate", "sg_get_correlation", "sg_reset_correlation")


def make_block(seed, n=None):
    from seigen_amd import _lib
    from seigen_amd.backend import HipBlock
    dim, degree, n3 = CONFIG3
    n = n or n3
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
    assert blk.is_sym()
    return blk


def field_bytes(blk):
    d = blk.dim
    ncomp = d + (d * (d + 1) // 2 if blk.is_sym() else d * d)
    return blk.ncells * blk.nd * ncomp * 8


def time_forms(a, b, reps=20):
    """{form: (median ms, best ms)}: a against b in the matrix-pipe form, b against a in the LDS-staged one, one call of each
    in turn between two HIP events (the runtime's own calls, bound with ctypes)"""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")

    def ok(rc):
        if rc != 0:
            raise RuntimeError("HIP runtime error %d" % rc)

    e0, e1 = C.c_void_p(), C.c_void_p()
    ok(hip.hipEventCreate(C.byref(e0)))
    ok(hip.hipEventCreate(C.byref(e1)))
    w = np.array([0.5, 1.0, -0.25])
    # the form is chosen when a handle's tables are built, at its first call
    os.environ.pop("SEIGEN_HIP_XCORR", None)
    a.correlate(b, w)
    os.environ["SEIGEN_HIP_XCORR"] = "lds"
    b.correlate(a, w)
    os.environ.pop("SEIGEN_HIP_XCORR", None)
    a.sync()
    b.sync()
    ms = {"mfma": [], "lds": []}
    for _ in range(reps):
        for form, x, y in (("mfma", a, b), ("lds", b, a)):
            stream = C.c_void_p(x.stream_ptr())
            ok(hip.hipEventRecord(e0, stream))
            x.correlate(y, w)
            ok(hip.hipEventRecord(e1, stream))
            ok(hip.hipEventSynchronize(e1))
            t = C.c_float()
            ok(hip.hipEventElapsedTime(C.byref(t), e0, e1))
            ms[form].append(t.value)
            y.sync()
    ok(hip.hipEventDestroy(e0))
    ok(hip.hipEventDestroy(e1))
    # the two forms computed the same thing (w and the operands' roles are symmetric here: B(a, b) = B(b, a))
    ca, cb = a.get_correlation(), b.get_correlation()
    dev = float(np.max(np.abs(ca - cb)) / np.max(np.abs(ca)))
    return {k: (float(np.median(v)), float(np.min(v))) for k, v in ms.items()}, dev


def hbm_read_rate(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300).stdout
    rates = [float(m.group(1)) for m in re.finditer(r"reads=\s*\d+ writes=\s*0 .*?, (\d+) GB/s", out)]
    return max(rates), out


def child_step(steps, parent):
    if parent:      # the parent commit's library has no correlation: bind what it exports
        from seigen_amd import _lib
        for name in NEW_SYMBOLS:
            _lib.SYMBOLS.pop(name)
    blk = make_block(1)
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
    ap.add_argument("--only", choices=("correlate", "parent"), default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--child-parent", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--n", type=int, nargs=3, default=None, help="cubes per axis instead of config 3's 64 64 64")
    args = ap.parse_args()
    if args.child:
        return child_step(args.steps, args.child_parent)
    if args.only in (None, "correlate"):
        a, b = make_block(1, args.n), make_block(2, args.n)
        forms, dev = time_forms(a, b)
        nbytes = 2 * field_bytes(a)
        print("block %r P4: two handles, %.3f GB of u and s each; the two forms' accumulators differ by %.1e of the largest entry"
              % (tuple(args.n or CONFIG3[2]), nbytes / 2e9, dev))
        for form in ("mfma", "lds"):
            med, best = forms[form]
            print("sg_correlate, %s form: %.3f ms median, %.3f ms best of 20 (event pair) -> %.0f GB/s"
                  % (form, med, best, nbytes / med / 1e6))
        if os.path.exists(args.hbm):
            rate, raw = hbm_read_rate(args.hbm)
            t = nbytes / rate / 1e6
            print("ubench_hbm read-only loop, best rate %.0f GB/s: the same bytes in %.3f ms; mfma form / stream = %.2f, lds form / stream = %.2f"
                  % (rate, t, forms["mfma"][0] / t, forms["lds"][0] / t))
        a.close()
        b.close()
    if args.only in (None, "parent") and args.parent_lib:
        res = {"this": [], "parent": []}
        for _ in range(5):
            for name, lib in (("this", None), ("parent", args.parent_lib)):
                env = dict(os.environ)
                if lib:
                    env["SEIGEN_HIP_LIB"] = lib
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--steps", str(args.steps)] +
                                   (["--child-parent"] if lib else []),
                                   env=env, capture_output=True, text=True, timeout=300)
                if r.returncode != 0:
                    print("child failed (%s): %s" % (name, r.stderr[-800:]))
                    return 1
                res[name].append(json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step"])
        x, y = np.median(res["this"]), np.median(res["parent"])
        print("config 3 step, no correlation: this %.4f ms, parent %.4f ms (%+.2f %%); runs this %s parent %s; spread this %.2f %% parent %.2f %%"
              % (x, y, 100 * (x / y - 1), ["%.4f" % v for v in res["this"]], ["%.4f" % v for v in res["parent"]],
                 100 * (max(res["this"]) - min(res["this"])) / x, 100 * (max(res["parent"]) - min(res["parent"])) / y))
    return 0


if __name__ == "__main__":
    sys.exit(main())
