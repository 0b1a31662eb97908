"""What the device transfers (sg_get_field_dev / sg_set_field_dev, kernels_xfer.hip) cost, measured on one GPU in one job; the
numbers of DESIGN.md "Device transfers" and profiles/r11/device_transfer.txt.

  python tools/xfer_cost.py [--only CASE]                      the transfers and yardstick (a), one JSON line per figure
  python tools/xfer_cost.py --host-path CASE get|set           what yardstick (b) profiles: the host transfers of the same block
  python tools/xfer_cost.py --summarise RAW STATS_DIR          the ratios to (a) and (b) from the raw lines and the profiles

  Cases: config 3's block (3-D P4 64^3, gw = 16), the 2-D N = 256 P4 mesh (gw = 16), a lane-family block (2-D P2 1024^2,
  gw = 64), and the hexahedral DQ_2 64^3 block on the lane family, whose stress item is moved in slices.
  Per case, field (u, s), direction (get, set) and buffer type (double, float): the time of one transfer between hipEvents
  on the handle's stream around REPS queued transfers, median of 5 runs that alternate with the yardstick, and bytes moved
  (read + written) divided by that time.
  (a) a hipMemcpyAsync device-to-device of the field's bytes (it moves twice that) in the same runs: the stream-rate floor.
  (b) the kernel time of sg::layout_kernel<double> per field word in sg_get_field_range / sg_set_field_range of the same
      block, from `rocprofv3 --kernel-trace --stats -- python tools/xfer_cost.py --host-path CASE DIR` (no counters in that
      run); the host transfers keep that kernel, so the profile of this commit's library is the parent commit's.
"""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (dim, degree, cubes, diagonal, SEIGEN_HIP_PATH, gw)
CASES = {
    "c3": (3, 4, (64, 64, 64), "left", None, 16),
    "2d": (2, 4, (256, 256), "left", None, 16),
    "lane": (2, 2, (1024, 1024), "left", "lane", 64),
    "hexlane": (3, 2, (64, 64, 64), "quadrilateral", "lane", 64),
}
REPS = 5
HOST_WORDS = 1 << 27       # the host transfers of yardstick (b) move at most this many words of a field (1 GB)


def make_block(case, stream=None):
    from seigen_amd.backend import HipBlock
    dim, degree, n, diagonal, path, gw = CASES[case]
    if path:
        os.environ["SEIGEN_HIP_PATH"] = path
    else:
        os.environ.pop("SEIGEN_HIP_PATH", None)
    h = [1.0 / k for k in n]
    blk = HipBlock(dim, degree, n, h, [0.0] * dim, diagonal, stream=stream)
    blk.set_params(1.0, 0.05 * min(h) / degree ** 2, 0.5, 0.25)
    return blk


def measure(case):
    import torch
    from seigen_amd import _lib
    ts = torch.cuda.Stream()
    blk = make_block(case, int(ts.cuda_stream))
    gw = CASES[case][5]
    out = []
    with torch.cuda.stream(ts):
        for fname, f in (("u", _lib.FIELD_U), ("s", _lib.FIELD_S)):
            shape = blk.field_shape(f)
            words = int(np.prod(shape))
            # a symmetric stress of modest size (the cost does not depend on the values)
            src = torch.rand(shape, dtype=torch.float64, device="cuda")
            if f == _lib.FIELD_S:
                src = 0.5 * (src + src.transpose(-1, -2)).contiguous()
            bufs = {"double": src, "float": src.to(torch.float32)}
            blk.set_field_dev(f, src)
            other = torch.empty_like(src)
            runs = {}

            def timed(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                fn()
                e0.record(ts)
                for _ in range(REPS):
                    fn()
                e1.record(ts)
                e1.synchronize()
                return e0.elapsed_time(e1) / REPS

            what = [("memcpy", None, lambda: other.copy_(src))]
            for tname in ("double", "float"):
                what.append(("get", tname, lambda t=bufs[tname]: blk.get_field_dev(f, out=t)))
                what.append(("set", tname, lambda t=bufs[tname]: blk.set_field_dev(f, t)))
            for _ in range(5):
                for d, tname, fn in what:
                    runs.setdefault((d, tname), []).append(timed(fn))
            assert blk.is_sym() == (gw != 1)
            for (d, tname), ms in runs.items():
                med = float(np.median(ms))
                moved = words * (16 if d == "memcpy" else 8 + (8 if tname == "double" else 4))
                out.append(dict(case=case, gw=gw, field=fname, op=d, buffer=tname, words=words, ms=med, bytes_moved=moved,
                                GBps=moved / (1e-3 * med) / 1e9, ns_per_word=1e6 * med / words, runs_ms=[round(v, 4) for v in ms]))
                print(json.dumps(out[-1]))
                sys.stdout.flush()
            del src, bufs, other
    ts.synchronize()
    blk.close()
    return out


def host_path(case, direction):
    """sg_get_field_range / sg_set_field_range of u and s of the case's block: the launches of sg::layout_kernel<double>"""
    from seigen_amd import _lib
    blk = make_block(case)
    words = 0
    for f in (_lib.FIELD_U, _lib.FIELD_S):
        shape = blk.field_shape(f)
        per_cell = int(np.prod(shape[1:]))
        cells = min(blk.ncells, HOST_WORDS // per_cell)
        host = np.zeros((cells,) + shape[1:])
        if direction == "get":
            blk.get_field_range(f, 0, cells, out=host)
        else:
            blk.set_field_range(f, 0, host)
        words += cells * per_cell
    blk.sync()
    blk.close()
    print(json.dumps(dict(case=case, op=direction, host_path_words=words)))


def summarise(raw, stats_dir):
    lines = [json.loads(l) for l in open(raw) if l.startswith("{")]
    new = [l for l in lines if "ms" in l]
    host = {(l["case"], l["op"]): l["host_path_words"] for l in lines if "host_path_words" in l}
    layout = {}     # (case, op) -> ns per word of layout_kernel<double>
    for (case, op), words in host.items():
        ns = 0
        for path in glob.glob(os.path.join(stats_dir, "%s_%s" % (case, op), "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                if "sg::layout_kernel<double>" in row["Name"]:
                    ns += int(row["TotalDurationNs"])
        if ns:
            layout[(case, op)] = ns / words
            print("(b) %s %s: sg::layout_kernel<double> %.3f ms for %d words of u and s: %.4f ns per word" % (case, op, 1e-6 * ns, words, ns / words))
    memcpy = {(l["case"], l["field"]): l for l in new if l["op"] == "memcpy"}
    for l in new:
        if l["op"] == "memcpy":
            print("(a) %s %s: hipMemcpyAsync device-to-device of %d words: %.4f ms, %.1f GB/s moved" % (l["case"], l["field"], l["words"], l["ms"], l["GBps"]))
            continue
        a = memcpy[(l["case"], l["field"])]
        print("%s %s %s %s: %.4f ms, %.1f GB/s moved, %.2f of (a)'s rate" % (l["case"], l["field"], l["op"], l["buffer"], l["ms"], l["GBps"], l["GBps"] / a["GBps"]))
    for case in CASES:
        for op in ("get", "set"):
            mine = [l for l in new if l["case"] == case and l["op"] == op and l["buffer"] == "double"]
            if len(mine) != 2 or (case, op) not in layout:
                continue
            t = sum(1e6 * l["ms"] for l in mine) / sum(l["words"] for l in mine)
            b = layout[(case, op)]
            print("against (b) %s %s, u and s, double buffers: %.4f ns per word against %.4f of sg::layout_kernel<double>: %.2f x the time (%s)"
                  % (case, op, t, b, t / b, "not slower" if t <= b else "SLOWER"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=tuple(CASES), default=None)
    ap.add_argument("--host-path", nargs=2, metavar=("CASE", "DIR"), default=None)
    ap.add_argument("--summarise", nargs=2, metavar=("RAW", "STATS_DIR"), default=None)
    args = ap.parse_args()
    if args.summarise:
        return summarise(*args.summarise)
    if args.host_path:
        return host_path(*args.host_path)
    for case in CASES:
        if args.only in (None, case):
            measure(case)
    return 0


if __name__ == "__main__":
    sys.exit(main())
