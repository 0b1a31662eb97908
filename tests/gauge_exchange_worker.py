"""Worker of tests/test_gauges_gpu.py: one rank of a block grid driving the C-ABI directly with the exchange inside the
library (sg_comm_init over tests/fake_rccl, as tests/receiver_exchange_worker.py does) and gauges armed on every rank: each
block records the gauges it owns inside ONE sg_step(n), and probes the same points once behind it.  The case is
native_exchange_worker.py's (setup_block), in one, two or three dimensions.

argv: out dir, world, rank, grid gx[,gy[,gz]], mesh nx[,ny[,nz]], degree, steps, cell, SEIGEN_HIP_PATH or -, every, kind,
points file (.npy)."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    import faulthandler
    faulthandler.dump_traceback_later(200, exit=True)
    from native_exchange_worker import setup_block
    from seigen_amd import _lib
    from seigen_amd.backend import HipBlock, comm_unique_id
    from seigen_amd.mesh import Partition
    out, world, rank = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    grid = tuple(int(x) for x in sys.argv[4].split(","))
    n = tuple(int(x) for x in sys.argv[5].split(","))
    degree, steps, cell, path = int(sys.argv[6]), int(sys.argv[7]), sys.argv[8], sys.argv[9]
    every, kind = int(sys.argv[10]), int(sys.argv[11])
    pts = np.load(sys.argv[12])
    if path != "-":
        os.environ["SEIGEN_HIP_PATH"] = path
    dim = len(n)
    part = Partition(n, rank, world, grid)
    peers = [part.neighbour(s) for s in range(2 * dim)] + [None] * (6 - 2 * dim)
    blk = HipBlock(dim, degree, part.n, [1.0 / n[a] for a in range(dim)], [0.0] * dim, cell, part.nbr_mask, cube0=list(part.start))
    setup_block(blk, n, degree, "plain")
    idfile = os.path.join(out, "unique_id.bin")
    if rank == 0:
        with open(idfile + ".tmp", "wb") as f:
            f.write(comm_unique_id())
        os.replace(idfile + ".tmp", idfile)
    t0 = time.time()
    while not os.path.exists(idfile):
        if time.time() - t0 > 120:
            raise RuntimeError("no unique id from rank 0")
        time.sleep(0.01)
    blk.comm_check(rank, world, peers)
    blk.comm_init(open(idfile, "rb").read(), rank, world, peers)
    assert blk.comm_selftest() == 0
    owned = blk.set_gauges(pts, kind, every, steps // every)
    blk.step(steps)              # ONE C-ABI call: stages, exchanges and the gauges of every step
    blk.sync()
    probe, powned = blk.probe_gradient(_lib.FIELD_U, kind, pts)
    np.savez(os.path.join(out, "rank%d.npz" % rank), owned=owned, traces=blk.get_gauges(), probe=probe, powned=powned,
             steps=blk.counters()["steps"])
    blk.comm_finalize()
    blk.close()


if __name__ == "__main__":
    main()
