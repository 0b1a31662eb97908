"""What a gradient (sg_get_gradient_dev, kernels_grad.hip) costs, measured on one GPU in one job; the numbers of DESIGN.md
"Gradient" and profiles/r14/gradient.txt.

  python tools/grad_cost.py [--only CASE]        one JSON line per figure, then the table

  Cases: config 3's block (3-D P4 tetrahedra 64^3, gw = 16), the 2-D N = 256 P4 triangles (tile family, gw = 16), hexahedra
  DQ_4 32^3 (gw = 16: the values of an item go through LDS in twelve slices).
  Per call: the time of one call between hipEvents on the handle's stream around REPS queued calls, median of 5 runs that
  alternate with the yardstick beside it: sg_get_field_dev of the stress of the same block into a buffer of the same type - it
  writes the same dim^2 words per node as kind 0 and was there before the gradient.  Kinds 0 (gradient) and 1 (divergence),
  double and float buffers.  Bytes: the algorithmic traffic, dim words read and ncomp written per node (12 for kind 0 in 3-D),
  and the rate it amounts to.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (dim, degree, cubes, diagonal)
CASES = {
    "c3": (3, 4, (64, 64, 64), "left"),
    "2d": (2, 4, (256, 256), "left"),
    "dq4": (3, 4, (32, 32, 32), "quadrilateral"),
}
REPS = 5


def measure(case):
    import torch
    from seigen_amd import _lib
    from seigen_amd.backend import HipBlock, gradient_plan
    dim, degree, n, diagonal = CASES[case]
    os.environ.pop("SEIGEN_HIP_PATH", None)
    ts = torch.cuda.Stream()
    h = [1.0 / k for k in n]
    blk = HipBlock(dim, degree, n, h, [0.0] * dim, diagonal, stream=int(ts.cuda_stream))
    blk.set_params(1.0, 0.05 * min(h) / degree ** 2, 0.5, 0.25)
    gw = 16          # the three cases run on the matrix-pipe families (MFMA, tile, hexm)
    assert "generic" not in blk.stage_kernel_name(_lib.STAGE_UH1) and "lane" not in blk.stage_kernel_name(_lib.STAGE_UH1)
    out = []
    with torch.cuda.stream(ts):
        for f in (_lib.FIELD_U, _lib.FIELD_S):
            src = torch.rand(blk.field_shape(f), dtype=torch.float64, device="cuda")
            if f == _lib.FIELD_S:
                src = 0.5 * (src + src.transpose(-1, -2)).contiguous()
            blk.set_field_dev(f, src)
            del src
        nodes = blk.ncells * blk.nd
        for tdt, word in ((torch.float64, 8), (torch.float32, 4)):
            stress = torch.empty(blk.field_shape(_lib.FIELD_S), dtype=tdt, device="cuda")
            for kind, kname in ((0, "grad"), (1, "div")):
                ncomp = dim * dim if kind == 0 else 1
                buf = torch.empty(blk.gradient_shape(kind), dtype=tdt, device="cuda")
                plan = gradient_plan(gw, blk.ncls, blk.nd, dim, ncomp, 8, word, 0, blk.ncells)

                def timed(fn):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    fn()
                    e0.record(ts)
                    for _ in range(REPS):
                        fn()
                    e1.record(ts)
                    e1.synchronize()
                    return e0.elapsed_time(e1) / REPS

                what = [("gradient", lambda: blk.get_gradient_dev(_lib.FIELD_U, kind, out=buf)),
                        ("stress_dev", lambda: blk.get_field_dev(_lib.FIELD_S, out=stress))]
                runs = {}
                for _ in range(5):
                    for name, fn in what:
                        runs.setdefault(name, []).append(timed(fn))
                rec = dict(case=case, kind=kname, buffer="double" if word == 8 else "float", nodes=nodes, slices=plan["slices"],
                           lds_bytes=plan["lds_bytes"], bytes=nodes * (dim * 8 + ncomp * word),
                           stress_bytes=nodes * dim * dim * (8 + word))
                for name, ms in runs.items():
                    rec[name + "_ms"] = float(np.median(ms))
                    rec[name + "_runs_ms"] = [round(v, 4) for v in ms]
                out.append(rec)
                print(json.dumps(rec))
                sys.stdout.flush()
                del buf
            del stress
    ts.synchronize()
    blk.close()
    return out


def table(recs):
    print("%-4s %-5s %-7s %10s %6s %7s | %9s %8s %8s | %9s %8s | %6s %s" % (
        "case", "kind", "buffer", "nodes", "slices", "LDS", "grad ms", "MB", "GB/s", "stress ms", "GB/s", "ratio", "spread"))
    for r in recs:
        g, s = r["gradient_ms"], r["stress_dev_ms"]
        lo, hi = min(r["gradient_runs_ms"]), max(r["gradient_runs_ms"])
        print("%-4s %-5s %-7s %10d %6d %7d | %9.4f %8.1f %8.1f | %9.4f %8.1f | %6.2f %.0f%%" % (
            r["case"], r["kind"], r["buffer"], r["nodes"], r["slices"], r["lds_bytes"], g, 1e-6 * r["bytes"], 1e-6 * r["bytes"] / g,
            s, 1e-6 * r["stress_bytes"] / s, g / s, 100 * (hi - lo) / g))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=tuple(CASES), default=None)
    args = ap.parse_args()
    recs = []
    for case in CASES:
        if args.only in (None, case):
            recs += measure(case)
    table(recs)
    return 0


if __name__ == "__main__":
    sys.exit(main())
