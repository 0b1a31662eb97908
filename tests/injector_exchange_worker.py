"""Worker of tests/test_injectors_gpu.py: one rank of a block grid driving the C-ABI directly with the exchange inside the
library (sg_comm_init over tests/fake_rccl, as tests/receiver_exchange_worker.py does) and injectors armed on every rank:
every block is handed all points and adds the ones it owns inside ONE sg_step(n).  The case is native_exchange_worker.py's
(setup_block); the rank saves its fields with the cells' indices in the whole mesh.

argv: out dir, world, rank, grid gx,gy[,gz], mesh nx,ny[,nz] (2-D or 3-D), degree, steps - and, optionally, the cell type
(left | right | quadrilateral; default left)."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

# for the mesh (16, 4, 4) cut at z = 0.5: in a cell touching the cut from below, on the cut plane itself (the lower block's),
# in a cell touching it from above, in the interior of the upper block
POINTS = np.array([[0.35, 0.6, 0.45], [0.71, 0.23, 0.5], [0.2, 0.4, 0.55], [0.6, 0.8, 0.9]])
# for the 2-D mesh (9, 6) cut at y = 0.5, likewise: below the cut, on the cut line (an edge of cells of both blocks), above
# it, in the interior of the upper block
POINTS_2D = np.array([[0.35, 0.45], [0.71, 0.5], [0.2, 0.55], [0.6, 0.87]])


def points_of(dim):
    return {2: POINTS_2D, 3: POINTS}[dim]


def series_of(steps, dim=3):
    """[steps - 2][npts][dim + dim * dim]: velocity and (symmetric) stress entries; the series runs out two steps before
    the end"""
    rng = np.random.default_rng(77)
    npts = len(points_of(dim))
    au = rng.uniform(-1.0, 1.0, (steps - 2, npts, dim))
    a = rng.uniform(-1.0, 1.0, (steps - 2, npts, dim, dim))
    a = np.triu(a) + np.swapaxes(np.triu(a, 1), -1, -2)
    return np.concatenate([au, a.reshape(steps - 2, npts, dim * dim)], axis=-1)


def main():
    import faulthandler
    faulthandler.dump_traceback_later(200, exit=True)
    from native_exchange_worker import block_cells, setup_block
    from seigen_amd import _lib
    from seigen_amd.backend import HipBlock, comm_unique_id
    from seigen_amd.mesh import Partition
    out, world, rank = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    grid = tuple(int(x) for x in sys.argv[4].split(","))
    n = tuple(int(x) for x in sys.argv[5].split(","))
    degree, steps = int(sys.argv[6]), int(sys.argv[7])
    cell = sys.argv[8] if len(sys.argv) > 8 else "left"
    dim = len(n)
    part = Partition(n, rank, world, grid)
    peers = [part.neighbour(s) for s in range(2 * dim)] + [None] * (6 - 2 * dim)
    blk = HipBlock(dim, degree, part.n, [1.0 / n[a] for a in range(dim)], [0.0] * dim, cell, part.nbr_mask, cube0=list(part.start))
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
    owned = blk.set_injectors(points_of(dim), series_of(steps, dim), 3)
    blk.step(steps)              # ONE C-ABI call: stages, exchanges and the injections of every step
    blk.sync()
    cells = block_cells(n, part.start, part.n, cell)          # cell of the whole mesh of every local cell
    st = blk.comm_stats()
    np.savez(os.path.join(out, "rank%d.npz" % rank), owned=owned, cells=cells, u=blk.get_field(_lib.FIELD_U),
             s=blk.get_field(_lib.FIELD_S), steps=blk.counters()["steps"], exchanges=st["exchanges"],
             kernels=np.array([blk.stage_kernel_name(k) for k in range(6)]))
    blk.comm_finalize()
    blk.close()


if __name__ == "__main__":
    main()
