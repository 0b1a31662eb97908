"""What a frame (sg_get_frame_dev, kernels_frame.hip) costs, measured on one GPU in one job; the numbers of DESIGN.md "Frames"
and profiles/r12/frames.txt.

  python tools/frame_cost.py [--only CASE]        one JSON line per figure, then the table

  Cases: config 3's block (3-D P4 64^3, gw = 16): a z slice with m = 4 and m = 8 of u and s, and the (2, 2, 2) volume of u;
  the 2-D N = 256 P4 mesh (gw = 16): m = 2, u and s.
  Per frame: the time of one frame between hipEvents on the handle's stream around REPS queued frames (double image), median
  of 5 runs that alternate with the yardsticks:
  (a) a hipMemcpyAsync device-to-device that moves the bytes the frame must read plus write - the nodal lines of the listed
      (group, class) items whose class holds a pixel, plus the image; a copy of B bytes reads B and writes B, so it copies
      half that sum.  The floor.
  (b) the receivers (sg_set_receivers) armed with the same pixel centres, one sample: REPS queued sg_end_step.
  (c) sg_get_field_dev of the whole field.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (dim, degree, cubes, diagonal, frames = [(label, field, m, slice)])
CASES = {
    "c3": (3, 4, (64, 64, 64), "left", [
        ("z slice m=4 u", "u", (4, 4, 1), {2: 0.3}), ("z slice m=4 s", "s", (4, 4, 1), {2: 0.3}),
        ("z slice m=8 u", "u", (8, 8, 1), {2: 0.3}), ("z slice m=8 s", "s", (8, 8, 1), {2: 0.3}),
        ("volume (2,2,2) u", "u", (2, 2, 2), None)]),
    "2d": (2, 4, (256, 256), "left", [("m=2 u", "u", (2, 2), None), ("m=2 s", "s", (2, 2), None)]),
}
REPS = 5
CAPACITY = 40      # receiver samples: 5 runs of 1 + REPS


def pixel_centres(cfg, m, slice):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from tests import frame_cases as fc
    return fc.pixels(cfg, m, slice)


def measure(case):
    import torch
    from seigen_amd import _lib
    from seigen_amd.backend import HipBlock, frame_weights
    from tests import frame_cases as fc
    dim, degree, n, diagonal, frames = CASES[case]
    os.environ.pop("SEIGEN_HIP_PATH", None)
    ts = torch.cuda.Stream()
    h = [1.0 / k for k in n]
    blk = HipBlock(dim, degree, n, h, [0.0] * dim, diagonal, stream=int(ts.cuda_stream))
    blk.set_params(1.0, 0.05 * min(h) / degree ** 2, 0.5, 0.25)
    cfg = fc.block_cfg(dim, degree, n, diagonal)
    out = []
    with torch.cuda.stream(ts):
        for f in (_lib.FIELD_U, _lib.FIELD_S):
            src = torch.rand(blk.field_shape(f), dtype=torch.float64, device="cuda")
            if f == _lib.FIELD_S:
                src = 0.5 * (src + src.transpose(-1, -2)).contiguous()
            blk.set_field_dev(f, src)
            del src
        for label, fname, m, slice in frames:
            f = _lib.FIELD_U if fname == "u" else _lib.FIELD_S
            ncomp = dim if fname == "u" else dim * dim
            px = pixel_centres(cfg, m, slice)
            plan = px["plan"]
            cls, _, _ = frame_weights(cfg, degree, px["frame"], blk.nd)
            image = torch.empty(blk.frame_shape(f, m, slice), dtype=torch.float64, device="cuda")
            read = plan["ngroups"] * len(set(cls)) * blk.nd * ncomp * plan["gw"] * 8
            written = image.numel() * 8
            half = torch.empty((read + written) // 16, dtype=torch.float64, device="cuda")
            half2 = torch.empty_like(half)
            whole = torch.empty(blk.field_shape(f), dtype=torch.float64, device="cuda")
            owned = blk.set_receivers(px["centre"], 1 if fname == "u" else 2, 1, CAPACITY)
            assert owned.all()

            def timed(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                fn()
                e0.record(ts)
                for _ in range(REPS):
                    fn()
                e1.record(ts)
                e1.synchronize()
                return e0.elapsed_time(e1) / REPS

            what = [("frame", lambda: blk.get_frame_dev(f, m=m, slice=slice, out=image)),
                    ("a_memcpy", lambda: half2.copy_(half)),
                    ("b_receivers", lambda: blk.end_step()),
                    ("c_field_dev", lambda: blk.get_field_dev(f, out=whole))]
            runs = {}
            for _ in range(5):
                for name, fn in what:
                    runs.setdefault(name, []).append(timed(fn))
            blk.set_receivers(np.zeros((0, dim)), 1, 1, 1)
            rec = dict(case=case, frame=label, pixels=int(np.prod(px["P"])), Q=plan["Q"], groups=plan["ngroups"], bytes_read=read,
                       bytes_written=written)
            for name, ms in runs.items():
                rec[name + "_ms"] = float(np.median(ms))
                rec[name + "_runs_ms"] = [round(v, 4) for v in ms]
            out.append(rec)
            print(json.dumps(rec))
            sys.stdout.flush()
            del image, half, half2, whole
    ts.synchronize()
    blk.close()
    return out


def table(recs):
    print("%-4s %-18s %9s %9s | %9s %9s %9s %9s | %7s %7s %7s %s" % ("case", "frame", "pixels", "MB r+w", "frame ms", "(a) ms", "(b) ms",
                                                                      "(c) ms", "x (a)", "(b)/fr", "(c)/fr", "spread"))
    for r in recs:
        fr = r["frame_ms"]
        lo, hi = min(r["frame_runs_ms"]), max(r["frame_runs_ms"])
        print("%-4s %-18s %9d %9.1f | %9.4f %9.4f %9.4f %9.4f | %7.2f %7.1f %7.1f %.0f%%  %s" % (
            r["case"], r["frame"], r["pixels"], 1e-6 * (r["bytes_read"] + r["bytes_written"]), fr, r["a_memcpy_ms"], r["b_receivers_ms"],
            r["c_field_dev_ms"], fr / r["a_memcpy_ms"], r["b_receivers_ms"] / fr, r["c_field_dev_ms"] / fr, 100 * (hi - lo) / fr,
            "not slower than (b)" if fr <= r["b_receivers_ms"] else "SLOWER than (b)"))


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
