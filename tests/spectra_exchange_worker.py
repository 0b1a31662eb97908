"""Worker of tests/test_spectra_gpu.py: one rank of a block grid driving the C-ABI directly with the exchange inside the
library (sg_comm_init over tests/fake_rccl, as tests/injector_exchange_worker.py does) and spectra armed on every rank: each
block accumulates the transforms of its own cells inside ONE sg_step(n).  The case is native_exchange_worker.py's
(setup_block: a source and a sponge); the rank saves its spectra with the cells' indices in the whole mesh.

argv: out dir, world, rank, grid gx,gy,gz, mesh nx,ny,nz, degree, steps."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

FREQS = (0.0, 3.0, 11.0)
EVERY = 2


def weights_of(dt, steps):
    """(wu, ws): three frequencies, f = 0 among them, a sample after every second step"""
    from seigen_amd.elastic import spectra_weights
    n = steps // EVERY
    return spectra_weights(FREQS, dt, EVERY, n), spectra_weights(FREQS, dt, EVERY, n, stagger=0.5 * dt)


def spectra_of(blk):
    """{"u": [nfreq, ...] complex, "s": likewise}"""
    return {"u": np.array([blk.get_spectrum(0, f) for f in range(len(FREQS))]),
            "s": np.array([blk.get_spectrum(1, f) for f in range(len(FREQS))])}


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
    dt = setup_block(blk, n, degree, "source")
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
    wu, ws = weights_of(dt, steps)
    blk.set_spectra(wu, ws, EVERY)
    blk.step(steps)              # ONE C-ABI call: stages, exchanges and the samples of every second step
    blk.sync()
    ax = [np.arange(part.start[a], part.start[a] + part.n[a]) for a in range(3)]
    cube = (ax[0][None, None, :] + n[0] * (ax[1][None, :, None] + n[1] * ax[2][:, None, None])).reshape(-1)
    cells = (cube[:, None] * 6 + np.arange(6)[None, :]).reshape(-1)          # cell of the whole mesh of every local cell
    sp = spectra_of(blk)
    np.savez(os.path.join(out, "rank%d.npz" % rank), cells=cells, u=sp["u"], s=sp["s"], steps=blk.counters()["steps"],
             samples=blk.spectra_samples())
    blk.comm_finalize()
    blk.close()


if __name__ == "__main__":
    main()
