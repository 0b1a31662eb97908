"""Memory / MFMA / wait instructions of the kernels in a hipcc -S listing: one kernel's compressed trace, or a table of
static counts per kernel.

usage: python tools/isa_ops.py file.s mangled_kernel_name [last_n]      the trace of one kernel
       python tools/isa_ops.py --counts file.s [name_filter]             one line of counts per kernel whose name has the filter

--counts, per kernel: FP64 vector instructions (v_*_f64 without the matrix ones and the conversions), FP32 ones, 64-bit vector
address adds (v_lshl_add_u64; gfx950 has no other form), global loads and stores, scratch accesses, scalar branches, and VGPRs /
AGPRs / SGPRs / scratch bytes / LDS bytes / waves per SIMD from the resource comments that follow the kernel.  The counts are
of the WHOLE kernel text - set-up, every code path - not of one item: compare the same kernel in two listings; what one item
executes follows from the difference where the change touches the item body alone.
"""
import re
import sys


def trace(path, name, last=None):
    s = open(path).read()
    i = s.index(name + ":")
    j = s.index(".Lfunc_end", i)
    ops = []
    for l in s[i:j].splitlines():
        t = l.strip().split()
        if not t:
            continue
        o = t[0]
        if o.startswith(("global_store", "scratch_", "global_load", "s_waitcnt", "v_mfma", "s_cbranch", "s_barrier", "ds_read", "buffer_")):
            ops.append(o if not o.startswith("s_waitcnt") else o + " " + " ".join(t[1:3]))
    out, prev, cnt = [], None, 0
    for o in ops:
        if o == prev:
            cnt += 1
        else:
            if prev:
                out.append("%s x%d" % (prev, cnt))
            prev, cnt = o, 1
    out.append("%s x%d" % (prev, cnt))
    print("\n".join(out[-(last or len(out)):]))


def kernels(text):
    for m in re.finditer(r"^(_Z\w+):\s*; @\1\n", text, re.M):
        end = text.index(".Lfunc_end", m.end())
        yield m.group(1), text[m.end():end], text[end:end + 3000]      # name, body, the resource comments after it


def count(body, pred):
    n = 0
    for line in body.splitlines():
        t = line.split()
        if t and not t[0].startswith((";", ".")) and pred(t[0]):
            n += 1
    return n


def field(tail, key):
    m = re.search(r"%s[ :]+(\d+)" % re.escape(key), tail)
    return int(m.group(1)) if m else -1


def counts(path, flt="mfma_stage_"):
    text = open(path).read()
    print("%-22s %6s %6s %6s %6s %6s %6s %6s %5s %5s %5s %6s %7s %4s" %
          ("kernel", "f64", "f32", "add64", "gload", "gstore", "scrtch", "sbr", "vgpr", "agpr", "sgpr", "scr_B", "lds_B", "occ"))
    fp = lambda o, w: o.startswith("v_") and w in o and not o.startswith("v_mfma") and "cvt" not in o      # noqa: E731
    for name, body, tail in kernels(text):
        if flt not in name:
            continue
        print("%-22s %6d %6d %6d %6d %6d %6d %6d %5d %5d %5d %6d %7d %4d" % (
            name.replace("_ZN2sg12mfma_stage_", "").replace("EEvNS_9StageArgsE", ""),
            count(body, lambda o: fp(o, "_f64")), count(body, lambda o: fp(o, "_f32")),
            count(body, lambda o: o.startswith("v_lshl_add_u64")),
            count(body, lambda o: o.startswith("global_load")), count(body, lambda o: o.startswith("global_store")),
            count(body, lambda o: o.startswith("scratch_")), count(body, lambda o: o.startswith("s_cbranch")),
            field(tail, "; NumVgprs"), field(tail, "; NumAgprs"), field(tail, "; TotalNumSgprs"), field(tail, "; ScratchSize"),
            field(tail, "; LDSByteSize"), field(tail, "; Occupancy")))


def main():
    if sys.argv[1] == "--counts":
        counts(*sys.argv[2:4])
    else:
        trace(sys.argv[1], sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else None)


if __name__ == "__main__":
    main()
