"""Worker of tests/test_receivers_gpu.py: one rank of tests/dist_worker.py's case (launched by torch.distributed.run, gloo
process group) with receivers on the solver class - ElasticLF4.set_receivers before run(), receiver_traces() after it.
The halo exchange runs inside the library (SEIGEN_HALO_NATIVE=force, over tests/fake_rccl) or from the host stage by
stage (SEIGEN_HALO_NATIVE=0: sg_end_step ends every step).  Rank 0 saves the traces of all receivers.

argv: out dir, degree, steps, mesh nx,ny,nz, grid gx,gy,gz, every."""
import os
import sys
from contextlib import contextmanager

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

# on block faces, edges and the centre corner of a (1, 2, 2) grid of the unit cube, in the interior, on the mesh boundary
POINTS = np.array([[0.5, 0.5, 0.5], [0.3, 0.5, 0.7], [0.3, 0.7, 0.5], [0.71, 0.5, 0.5], [0.2, 0.3, 0.3],
                   [0.66, 0.8, 0.2], [0.0, 0.5, 0.25], [1.0, 1.0, 1.0], [0.4375, 0.25, 0.75]])


@contextmanager
def receivers_on_create(points, every):
    """ElasticLF4.create hands back a solver with receivers set: dist_worker.run_case builds and runs its case in one call"""
    from seigen_amd import ElasticLF4
    create = ElasticLF4.create

    def with_receivers(*args, **kwargs):
        el = create(*args, **kwargs)
        el.set_receivers(points, every=every, fields=("velocity", "stress"))
        return el
    ElasticLF4.create = staticmethod(with_receivers)
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
    every = int(sys.argv[6])
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(int(os.environ.get("SEIGEN_HIP_DEVICE", "0")))
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    from dist_worker import run_case
    from seigen_amd.mesh import Partition
    with receivers_on_create(POINTS, every):
        el, _, _ = run_case(n, degree, nsteps, Partition(n, rank, world, grid), True)
    times, tr = el.receiver_traces()
    if rank == 0:
        np.savez(os.path.join(out, "traces.npz"), times=times, velocity=tr["velocity"], stress=tr["stress"],
                 native=int(getattr(el._exchanger, "native", False)))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
