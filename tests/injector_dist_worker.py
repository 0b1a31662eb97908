"""Worker of tests/test_injectors_gpu.py: one rank of tests/dist_worker.py's case (launched by torch.distributed.run, gloo
process group) with a stress series on the solver class - ElasticLF4.set_injectors before run().  With
SEIGEN_HALO_NATIVE=0 the halo exchange runs from the host stage by stage (seigen_amd/parallel.py HaloExchanger: sg_end_step
ends every step, and the traces of s1 travel again after a step that added a stress entry).  Every rank saves its fields
with the cells' indices in the whole mesh.

argv: out dir, degree, steps, mesh nx,ny,nz, grid gx,gy,gz."""
import os
import sys
from contextlib import contextmanager

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

# for a mesh cut at z = 0.5: in a cell touching the cut from below, on the cut plane itself (the lower block's), in a cell
# touching it from above, in the interior of the upper block
POINTS = np.array([[0.35, 0.6, 0.45], [0.71, 0.23, 0.5], [0.2, 0.4, 0.55], [0.6, 0.8, 0.9]])


def stress_series(steps):
    """[steps - 1][npts][3][3], symmetric: the series runs out two steps before the end of the run"""
    a = np.random.default_rng(78).uniform(-1.0, 1.0, (steps - 1, len(POINTS), 3, 3))
    return np.triu(a) + np.swapaxes(np.triu(a, 1), -1, -2)


@contextmanager
def injectors_on_create(points, series):
    """ElasticLF4.create hands back a solver with the series armed: dist_worker.run_case builds and runs its case in one
    call (the entry before step 1 goes into the zero fields of the new solver and is overwritten with them)"""
    from seigen_amd import ElasticLF4
    create = ElasticLF4.create

    def with_injectors(*args, **kwargs):
        el = create(*args, **kwargs)
        el.set_injectors(points, series, what="stress")
        return el
    ElasticLF4.create = staticmethod(with_injectors)
    try:
        yield
    finally:
        ElasticLF4.create = staticmethod(create)


def main():
    import faulthandler
    faulthandler.dump_traceback_later(200, exit=True)
    out, degree, nsteps = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    n = tuple(int(x) for x in sys.argv[4].split(","))
    grid = tuple(int(x) for x in sys.argv[5].split(","))
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(int(os.environ.get("SEIGEN_HIP_DEVICE", "0")))
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    from dist_worker import run_case
    from seigen_amd.mesh import Partition
    part = Partition(n, rank, world, grid)
    with injectors_on_create(POINTS, stress_series(nsteps)):
        el, u, s = run_case(n, degree, nsteps, part, True)
    ax = [np.arange(part.start[a], part.start[a] + part.n[a]) for a in range(3)]
    cube = (ax[0][None, None, :] + n[0] * (ax[1][None, :, None] + n[1] * ax[2][:, None, None])).reshape(-1)
    cells = (cube[:, None] * 6 + np.arange(6)[None, :]).reshape(-1)          # cell of the whole mesh of every local cell
    np.savez(os.path.join(out, "rank%d.npz" % rank), cells=cells, u=u, s=s, native=int(getattr(el._exchanger, "native", False)))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
