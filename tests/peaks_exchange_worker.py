"""Worker of tests/test_peaks_gpu.py: one rank of a block grid driving the C-ABI directly with the exchange inside the
library (sg_comm_init over tests/fake_rccl, as tests/spectra_exchange_worker.py does) and peak maps armed on every rank: each
block keeps the maxima of its own cells inside ONE sg_step(n).  The case is native_exchange_worker.py's (setup_block: a
source and a sponge); the rank saves its maps with the cells' indices in the whole mesh.

argv: out dir, world, rank, grid gx,gy,gz, mesh nx,ny,nz, degree, steps."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

EVERY = 2


def peaks_of(blk):
    """{"uv", "us": value and sample of the velocity, "sv", "ss": of the stress}"""
    (uv, us), (sv, ss) = blk.get_peaks(0), blk.get_peaks(1)
    return {"uv": uv, "us": us, "sv": sv, "ss": ss}


def main():
    import faulthandler
    faulthandler.dump_traceback_later(200, exit=True)
    from native_exchange_worker import setup_block
    from seigen_amd.backend import HipBlock, comm_unique_id
    from seigen_amd.mesh import Partition
    out, world, rank = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    grid = tuple(int(x) for x in sys.argv[4].split(","))
    n = tuple(int(x) for x in sys.argv[5].split(","))
    degree, steps = int(sys.argv[6]), int(sys.argv[7])
    part = Partition(n, rank, world, grid)
    peers = [part.neighbour(s) for s in range(6)]
    blk = HipBlock(3, degree, part.n, [1.0 / n[a] for a in range(3)], [0.0] * 3, "left", part.nbr_mask, cube0=list(part.start))
    setup_block(blk, n, degree, "source")
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
    blk.set_peaks(3, EVERY, steps // EVERY)
    blk.step(steps)              # ONE C-ABI call: stages, exchanges and the samples of every second step
    blk.sync()
    ax = [np.arange(part.start[a], part.start[a] + part.n[a]) for a in range(3)]
    cube = (ax[0][None, None, :] + n[0] * (ax[1][None, :, None] + n[1] * ax[2][:, None, None])).reshape(-1)
    cells = (cube[:, None] * 6 + np.arange(6)[None, :]).reshape(-1)          # cell of the whole mesh of every local cell
    np.savez(os.path.join(out, "rank%d.npz" % rank), cells=cells, steps=blk.counters()["steps"], samples=blk.peaks_samples(),
             **peaks_of(blk))
    blk.comm_finalize()
    blk.close()


if __name__ == "__main__":
    main()
