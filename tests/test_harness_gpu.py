"""GPU tests through the solver-class API (seigen_amd.ElasticLF4) against the oracle:
sponge + source (explosive source set-up), eigenmode (BASELINE config 1), per-cell
material, multi-block halo exchange on one device."""
import math
import os

import numpy as np
import pytest

from oracle import harness as oh
from oracle import mesh as omesh
from oracle.lf4 import OracleLF4
from tests.util import rel_err, seeded

pytestmark = pytest.mark.gpu


def test_eigenmode_2d_config1(gpu):
    """BASELINE config 1: 40x40 squares (3200 triangles), P1, dt=0.0125, T=5 (400 steps).
    Error functional of eigenmode_2d.py:40-65; HIP path vs oracle within 1e-9 (north star: 1e-6)."""
    from seigen_amd.harness.eigenmode import Eigenmode2DLF4
    N, P = 40, 1
    dt = 0.5 * (1.0 / N) / (2.0 ** (P - 1))
    em = Eigenmode2DLF4(N, P, dt, output=False)
    u1, s1 = em.eigenmode2d(T=5.0)
    u_err, s_err = em.eigenmode_error(u1, s1)
    ref = oh.Eigenmode2D(N, P, dt)
    ou, os_ = ref.run(5.0)
    assert ref.elastic.nsteps == 400
    e = ref.errors(ou, os_)
    assert abs(u_err - e["u_error"]) < 1e-9 and abs(s_err - e["s_error"]) < 1e-9
    assert rel_err(u1.dat.data_cells, ou) < 1e-9
    assert rel_err(s1.dat.data_cells, os_) < 1e-9
    # the values the survey's throw-away restatement found, plain L2
    assert abs(e["u_l2"] - 7.9664e-3) < 2e-6 and abs(e["s_l2"] - 3.9453e-2) < 2e-6


@pytest.mark.parametrize("P,N", [(2, 4), (4, 2)])
def test_eigenmode_3d_short(gpu, P, N):
    from seigen_amd.harness.eigenmode import Eigenmode3DLF4
    dt = 0.5 * (1.0 / N) / (2.0 ** (P - 1))
    T = 10 * dt
    em = Eigenmode3DLF4(N, P, dt, output=False)
    u1, s1 = em.eigenmode3d(T=T)
    ref = oh.Eigenmode3D(N, P, dt)
    ou, os_ = ref.run(T)
    assert rel_err(u1.dat.data_cells, ou) < 1e-10
    assert rel_err(s1.dat.data_cells, os_) < 1e-10
    u_err, s_err = em.eigenmode_error(u1, s1)
    e = ref.errors(ou, os_, Pproj=3)
    assert abs(u_err - e["u_error"]) < 1e-10 and abs(s_err - e["s_error"]) < 1e-10


def test_explosive_source_sponge_and_source(gpu):
    """explosive_source_lf4.py set-up (DG4 sponge, box-Ricker stress source) on a reduced
    domain, 60 steps of dt=1e-3 around the source peak, HIP vs oracle."""
    from seigen_amd.harness.explosive_source import ExplosiveSourceLF4
    Lx, Ly, h = 100.0, 50.0, 2.5
    ex = ExplosiveSourceLF4()
    el = ex.setup(Lx=Lx, Ly=Ly, h=h, dt=1e-3, source_x=45.0)
    nsteps = 60
    T = nsteps * 1e-3
    u1, s1 = el.run(T)

    ref = oh.ExplosiveSource(Lx=Lx, Ly=Ly, h=h, src=(45.0, None))
    ref.elastic.dt = 1e-3
    ou, os_ = ref.elastic.run(T)
    assert ref.elastic.nsteps == len(el.step_times(T))
    scale = np.abs(os_).max()
    assert scale > 0
    assert np.abs(s1.dat.data_cells - os_).max() / scale < 1e-9
    assert np.abs(u1.dat.data_cells - ou).max() / max(np.abs(ou).max(), 1e-300) < 1e-9


def test_time_windowed_and_static_sources(gpu):
    """Sources the reference would simply re-interpolate every step (elastic.py:285-288): one that is
    non-zero during four steps only - zero at t = 0, at the last step and at any coarse sampling of the
    run - and one without time dependence (uploaded as a single slice, sg_set_source nsteps = -1)."""
    from seigen_amd import ElasticLF4, Expression, Function, RectangleMesh
    nx, ny, P, dt, nsteps = 12, 8, 2, 1e-3, 40
    box = "x[0] >= 2.5 && x[0] <= 6.0 && x[1] >= 3.0 && x[1] <= 5.5"
    for kind in ("window", "static"):
        mesh = RectangleMesh(nx, ny, 12.0, 8.0)
        el = ElasticLF4.create(mesh, "DG", P, dimension=2, solver="explicit", output=False)
        el.density, el.mu, el.l, el.dt = 1.0, 3.0, 2.0, dt
        if kind == "window":
            code = "%s && t >= 0.0165 && t <= 0.0205 ? 50.0*x[0] : 0.0" % box       # steps 17..20
            el.source_expression = Expression(((code, "0.0"), ("0.0", code)), t=0)
        else:
            code = "%s ? 2.0 + x[1] : 0.0" % box
            el.source_expression = Expression(((code, "0.0"), ("0.0", code)))
        el.source_function = Function(el.S)
        el.source = el.source_expression
        u1, s1 = el.run(nsteps * dt * (1 + 1e-9))

        m = omesh.RectangleMesh(nx, ny, 12.0, 8.0)
        orc = OracleLF4(m, P)
        orc.density, orc.mu, orc.l, orc.dt = 1.0, 3.0, 2.0, dt
        X = m.node_coords(P)
        inbox = (X[..., 0] >= 2.5) & (X[..., 0] <= 6.0) & (X[..., 1] >= 3.0) & (X[..., 1] <= 5.5)
        pat = np.zeros(X.shape[:-1] + (2, 2))
        if kind == "window":
            pat[inbox, 0, 0] = pat[inbox, 1, 1] = 50.0 * X[inbox][:, 0]
            orc.source = lambda t: pat if 0.0165 <= t <= 0.0205 else None
        else:
            pat[inbox, 0, 0] = pat[inbox, 1, 1] = 2.0 + X[inbox][:, 1]
            orc.source = lambda t: pat
        orc.run(nsteps * dt * (1 + 1e-9))
        assert orc.nsteps == nsteps and np.abs(orc.s1).max() > 1e-3
        assert rel_err(u1.dat.data_cells, orc.u1) < 1e-10, kind
        assert rel_err(s1.dat.data_cells, orc.s1) < 1e-10, kind


def test_per_cell_material(gpu):
    """Build-defined heterogeneous extension: each cell scales its own g by its own (lambda, mu)."""
    from seigen_amd import _lib
    from seigen_amd.backend import HipBlock
    for dim, degree, n, L in ((2, 3, (4, 3), (1.0, 1.0)), (3, 4, (2, 2, 2), (1.0, 1.0, 1.0))):
        h = [L[a] / n[a] for a in range(dim)]
        blk = HipBlock(dim, degree, n, h, [0.0] * dim)
        m = omesh.structured(dim, n, L)
        orc = OracleLF4(m, degree)
        rng = np.random.default_rng(7)
        lam = rng.uniform(0.4, 0.9, m.ncells)
        mu = rng.uniform(0.2, 0.5, m.ncells)
        orc.dt, orc.l, orc.mu, orc.density = 1e-3, lam, mu, 1.0
        orc.u0 = seeded(blk.field_shape(_lib.FIELD_U), 8)
        orc.s0 = seeded(blk.field_shape(_lib.FIELD_S), 9)
        blk.set_params(1.0, orc.dt, lam, mu)
        blk.set_field(_lib.FIELD_U, orc.u0)
        blk.set_field(_lib.FIELD_S, orc.s0)
        blk.step(2)
        orc.step(orc.dt)
        orc.step(2 * orc.dt)
        assert rel_err(blk.get_field(_lib.FIELD_U), orc.u1) < 1e-10
        assert rel_err(blk.get_field(_lib.FIELD_S), orc.s1) < 1e-10


# ------------------------------------------------------------------------------------------------
#  halo layer on ONE device: split the mesh into blocks, exchange packed traces by device copies,
#  and require the result to equal the single-block run BITWISE (SURVEY 8e determinism check)
# ------------------------------------------------------------------------------------------------
class _LocalExchange(object):
    """Same call sequence as seigen_amd.parallel.HaloExchanger.step, with the point-to-point
    transport replaced by device-to-device copies between blocks living on one GPU.

    host_sync=False: every block launches on the caller's stream `stream` (a torch.cuda.Stream), the copies run on that
    stream too, and the host never waits between pack, copy and stage: the stream alone orders them (and the blocks'
    second streams against it, sg_run_stage)."""

    def __init__(self, blocks, parts, host_sync=True, stream=None):
        import torch
        from seigen_amd import _lib
        self.torch, self.lib = torch, _lib
        self.blocks, self.parts = blocks, parts
        self.host_sync, self.stream = host_sync, stream
        assert host_sync or stream is not None, "without host synchronisation the copies need the blocks' stream"
        self.send, self.recv = [], []
        for b, p in zip(blocks, parts):
            snd, rcv = {}, {}
            for kind, field in (("u", _lib.FIELD_U), ("s", _lib.FIELD_S)):
                for s in range(2 * p.dim):
                    if p.neighbour(s) is None:
                        continue
                    n = b.halo_bytes(field, s)          # raw bytes: the library knows what the buffers hold
                    snd[(kind, s)] = torch.zeros(n, dtype=torch.uint8, device="cuda")
                    rcv[(kind, s)] = torch.zeros(n, dtype=torch.uint8, device="cuda")
            for field in range(4):
                kind = "s" if field in (_lib.FIELD_S, _lib.FIELD_SH) else "u"
                for s in range(2 * p.dim):
                    if p.neighbour(s) is not None:
                        b.halo_attach(field, s, rcv[(kind, s)].data_ptr())
            self.send.append(snd)
            self.recv.append(rcv)
        # the zero fills above run on torch's current stream, the blocks' packs on their own non-blocking streams:
        # no fill may land after the first pack (seigen_amd/parallel.py HaloExchanger does the same).  Without this a
        # multi-block test failed once in a long session (torch's caching allocator hands out blocks without a
        # synchronising hipMalloc, so the fills really are asynchronous), never in a fresh process.
        torch.cuda.synchronize()

    def _exchange(self, field):
        lib = self.lib
        kind = "s" if field in (lib.FIELD_S, lib.FIELD_SH) else "u"
        for r, (b, p) in enumerate(zip(self.blocks, self.parts)):
            for s in range(2 * p.dim):
                if p.neighbour(s) is not None:
                    b.halo_pack(field, s, self.send[r][(kind, s)].data_ptr())
        if self.host_sync:
            for b in self.blocks:
                b.sync()
        with self.torch.cuda.stream(self.stream):      # (None: torch's current stream, as ever)
            for r, p in enumerate(self.parts):
                for s in range(2 * p.dim):
                    nb = p.neighbour(s)
                    if nb is not None:
                        self.recv[r][(kind, s)].copy_(self.send[nb][(kind, s ^ 1)])
        if self.host_sync:
            self.torch.cuda.synchronize()

    def step(self, nsteps, pipelined=True):
        from seigen_amd.parallel import STAGE_INPUT, STAGE_OUTPUT
        lib = self.lib
        if pipelined:
            self._exchange(STAGE_INPUT[0])
        for _ in range(nsteps):
            for stage in range(6):
                if pipelined:      # HaloExchanger.step: FIRST, traces of the output, SECOND
                    for b in self.blocks:
                        b.run_stage(stage, lib.REGION_FIRST)
                    self._exchange(STAGE_OUTPUT[stage])
                    for b in self.blocks:
                        b.run_stage(stage, lib.REGION_SECOND)
                else:              # HaloExchanger.step_unpipelined: traces of the input, interior, shell
                    for b in self.blocks:
                        b.run_stage(stage, lib.REGION_INTERIOR)
                    self._exchange(STAGE_INPUT[stage])
                    for b in self.blocks:
                        b.run_stage(stage, lib.REGION_BOUNDARY)
                if self.host_sync:
                    for b in self.blocks:
                        b.sync()
            for b in self.blocks:
                b.end_step()


def _multiblock_case(dim, degree, n, grid, pipelined, extras=False, dtype="f64", separable=False, diagonal="left",
                     sym=False, stream=None, host_sync=True):
    """Steps the mesh as one block and as the blocks of `grid` and asserts the two agree bitwise.  sym: a symmetric
    initial stress (the blocks stay in symmetric-stress mode).  stream: a torch.cuda.Stream that every block made here
    launches on (sg_config::stream), None: each block's own; host_sync: _LocalExchange.  Returns the single block's inputs
    and results (u0, s0, dt, sigma, src_nodes, src_steps - the source values of each step -, u, s), the stage kernels the
    split blocks name and their (stream, second stream) pointers."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no GPU")
    from seigen_amd import _lib
    from seigen_amd.backend import HipBlock
    from seigen_amd.mesh import Partition
    L = tuple(1.0 for _ in range(dim))
    h = [L[a] / n[a] for a in range(dim)]
    sptr = None if stream is None else stream.cuda_stream
    single = HipBlock(dim, degree, n, h, [0.0] * dim, diagonal, stream=sptr, dtype=dtype)
    u0 = seeded(single.field_shape(_lib.FIELD_U), 11)
    s0 = seeded(single.field_shape(_lib.FIELD_S), 12)
    if sym:
        s0 = 0.5 * (s0 + np.swapaxes(s0, -1, -2))
    dt = 0.02 * min(h) / degree ** 2
    single.set_params(1.0, dt, 0.5, 0.25)
    single.set_field(_lib.FIELD_U, u0)
    single.set_field(_lib.FIELD_S, s0)
    nd = single.nd
    sigma = src_nodes = src_steps = None
    if extras:      # a sponge and a time-dependent source scattered over the mesh (shell cells included)
        r3 = np.random.default_rng(77)
        nq = 5 ** dim if diagonal == "quadrilateral" else {1: 5, 2: 15, 3: 35}[dim]
        sigma = np.where(r3.uniform(size=(single.ncells, nq)) > 0.6, 3.0, 0.0)
        sigma[::4] = 3.0          # every fourth cell: one value on all nodes (applied without a matrix where a family can)
        src_nodes = np.unique(r3.integers(0, single.ncells * nd, size=min(40, single.ncells * nd)))
        sv = r3.uniform(-1, 1, size=(3, len(src_nodes), dim, dim))
        src_vals = 0.5 * (sv + np.swapaxes(sv, -1, -2))
        src_w = np.array([0.7, -1.3, 0.4])
        single.set_absorption(sigma, 4)
        if separable:       # one slice and a weight per step (sg_set_source_separable)
            single.set_source_separable(src_nodes, src_vals[0], src_w)
            src_steps = src_w[:, None, None, None] * src_vals[0]
        else:
            single.set_source(src_nodes, src_vals)
            src_steps = src_vals
    single.step(3)
    uref, sref = single.get_field(_lib.FIELD_U), single.get_field(_lib.FIELD_S)

    world = int(np.prod(grid))
    parts = [Partition(n, r, world, grid) for r in range(world)]
    ncls = 1 if diagonal == "quadrilateral" else {1: 1, 2: 2, 3: 6}[dim]

    def cells_of(p):
        """global cell indices of a block, in the block's own cell order"""
        ax = [np.arange(p.start[a], p.start[a] + p.n[a]) for a in range(dim)]
        if dim == 1:
            cube = ax[0]
        elif dim == 2:
            cube = (ax[0][None, :] + n[0] * ax[1][:, None]).reshape(-1)
        else:
            cube = (ax[0][None, None, :] + n[0] * (ax[1][None, :, None] + n[1] * ax[2][:, None, None])).reshape(-1)
        return (cube[:, None] * ncls + np.arange(ncls)[None, :]).reshape(-1)

    blocks = []
    for p in parts:
        origin = [p.start[a] * h[a] for a in range(dim)]
        b = HipBlock(dim, degree, p.n, h, origin, diagonal, p.nbr_mask, stream=sptr, dtype=dtype)
        sel = cells_of(p)
        b.set_params(1.0, dt, 0.5, 0.25)
        b.set_field(_lib.FIELD_U, u0[sel])
        b.set_field(_lib.FIELD_S, s0[sel])
        if extras:
            b.set_absorption(sigma[sel], 4)
            local = {int(c): i for i, c in enumerate(sel)}        # global cell -> cell of this block
            mine = [j for j, g in enumerate(src_nodes) if int(g) // nd in local]
            mynodes = np.array([local[int(src_nodes[j]) // nd] * nd + int(src_nodes[j]) % nd for j in mine], dtype=np.int64)
            if separable and mine:
                b.set_source_separable(mynodes, src_vals[0][mine], src_w)
            else:
                b.set_source(mynodes, src_vals[:, mine] if mine else None)
        blocks.append(b)
    ex = _LocalExchange(blocks, parts, host_sync=host_sync, stream=stream)
    names = sorted({b.stage_kernel_name(st) for b in blocks for st in range(6)})     # halo buffers attached: as they run
    ex.step(3, pipelined)
    for b, p in zip(blocks, parts):
        sel = cells_of(p)
        assert np.array_equal(b.get_field(_lib.FIELD_U), uref[sel]), "velocity differs from the single-block run"
        assert np.array_equal(b.get_field(_lib.FIELD_S), sref[sel]), "stress differs from the single-block run"
    return dict(u0=u0, s0=s0, dt=dt, sigma=sigma, src_nodes=src_nodes, src_steps=src_steps, u=uref, s=sref, names=names,
                streams=[(b.stream_ptr(), b.stream2_ptr()) for b in blocks] + [(single.stream_ptr(), single.stream2_ptr())])


@pytest.mark.parametrize("dim,degree,n,grid", [
    (2, 2, (6, 4), (2, 2)),
    (2, 3, (5, 4), (1, 2)),
    (3, 2, (4, 4, 2), (2, 2, 1)),
    (3, 4, (4, 2, 4), (2, 1, 2)),
    (3, 4, (2, 4, 4), (1, 2, 2)),
    (3, 3, (4, 3, 2), (2, 1, 1)),
    # 27 blocks: the centre block has neighbours on all six sides, so its FIRST region is seven
    # boxes (half an interior + six slabs): MFMA kernels (P3) and generic kernels (P1)
    (3, 3, (9, 9, 9), (3, 3, 3)),
    (3, 1, (7, 8, 9), (3, 3, 3)),
    # block sides normal to x on the interleaved layouts (16 cubes of an x-row per item): the shell next to an x side is
    # a whole layout group thick (csrc/handle.hpp shell_width_x), so blocks must be wider than 32 cubes for the launch
    # that overlaps the exchange to have anything to do; 40 and 36 cubes per block also make groups straddle rows
    (3, 3, (80, 3, 4), (2, 1, 2)),
    (3, 4, (120, 2, 2), (3, 1, 1)),
    (2, 3, (72, 6), (2, 2)),
])
@pytest.mark.parametrize("pipelined", [True, False])
def test_multiblock_equals_single_block(gpu, dim, degree, n, grid, pipelined):
    _multiblock_case(dim, degree, n, grid, pipelined)


@pytest.mark.parametrize("dim,degree,n,grid", [(3, 3, (40, 3, 4), (2, 1, 2)), (2, 2, (40, 6), (2, 2))])
def test_multiblock_separable_source(gpu, dim, degree, n, grid):
    """A separable source (one slice + a weight per step) in blocks with neighbours: the source of a split stage is
    added part by part (FIRST, then SECOND) with this step's weight; bitwise equal to the single block (and the single
    block with a separable source equals the one with the table of products: test_separable_source)."""
    _multiblock_case(dim, degree, n, grid, True, extras=True, separable=True)


def test_two_blocks_across_x_at_production_width(gpu):
    """Two 64 x 32 x 32-cube P4 blocks side by side along x (the 2 x 2 x 2 grid's kind of neighbour) on the
    MFMA kernels with everything the production path switches on at that size - group-thick x shell, item lists of the
    FIRST / SECOND regions, chunked item order, per-item neighbour table with remote-trace slots - bitwise equal to
    the single 128 x 32 x 32 block, both schedules."""
    for pipelined in (True, False):
        _multiblock_case(3, 4, (128, 32, 32), (2, 1, 1), pipelined)


@pytest.mark.parametrize("dim,degree,n,grid", [(3, 4, (4, 2, 4), (2, 1, 2)), (2, 3, (10, 9), (1, 3))])
def test_multiblock_single_stream(gpu, monkeypatch, dim, degree, n, grid):
    """SEIGEN_HIP_OVERLAP=0: both halves of a split stage on the main stream (the default launches the second
    half on its own stream beside the first); same bitwise result."""
    monkeypatch.setenv("SEIGEN_HIP_OVERLAP", "0")
    _multiblock_case(dim, degree, n, grid, True, extras=True)


@pytest.mark.parametrize("seed", range(int(os.environ.get("SEIGEN_TEST_RANDOM_CASES", "8"))))
def test_multiblock_random_grids(gpu, seed):
    """Random block grids, x splits and one-cube-thin blocks included (the shell then covers the whole
    block and the halves of the pipelined schedule are empty): bitwise equal to the single block."""
    rng = np.random.default_rng(500 + seed)
    dim = int(rng.integers(1, 4))
    degree = int(rng.integers(1, 5))
    grid = tuple(int(g) for g in rng.integers(1, 4, size=dim))
    if int(np.prod(grid)) == 1:
        grid = grid[:-1] + (2,)
    n = tuple(int(g * rng.integers(1, 4) + rng.integers(0, 2)) for g in grid)
    # every fourth case on tensor-product cells (quadrilaterals, hexahedra)
    diagonal = "quadrilateral" if (dim >= 2 and seed % 4 == 3) else "left"
    # every fifth case in the float mode, where an MFMA kernel family runs the blocks
    f32_ok = ((dim == 3 and degree >= 2) or dim == 2) and not (dim == 3 and diagonal == "quadrilateral")
    dtype = "f32" if (seed % 5 == 4 and f32_ok) else "f64"
    _multiblock_case(dim, degree, n, grid, bool(seed % 2 == 0), extras=(seed % 3 != 1), diagonal=diagonal, dtype=dtype)


def test_receiver_traces_full_run_vs_oracle(gpu):
    """The whole explosive-source run of the reference (explosive_source_lf4.py, dt = 0.001 of
    uy.py:25, T = 2.5: 2500 steps = 15 000 fused launches) on the GPU, receivers sampled every 5th
    step as uy.py does, against the oracle's committed traces - with the reference's nodally interpolated
    source and with the unit-moment projected source of the REF-C convergence study (what these traces say
    about REF-C1..3 is asserted on the oracle side, tests/test_oracle_pins.py)."""
    import os
    from seigen_amd.harness.explosive_source import ExplosiveSourceLF4
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    for mode, fixture in (("interpolate", "explosive_oracle.npz"), ("project", "explosive_oracle_project.npz")):
        d = np.load(os.path.join(gold, fixture))
        ex = ExplosiveSourceLF4()
        ex.setup(dt=1e-3, source_mode=mode)
        t, tr = ex.record_receivers(2.5)
        np.testing.assert_allclose(t, d["times"], atol=1e-9)
        scale = np.abs(d["traces"]).max()
        assert np.abs(tr - d["traces"]).max() < 1e-9 * scale, mode
        if mode == "project":
            assert abs(ex.source_integral - 1.0) < 1e-12
            # the committed HIP traces of the convergence study (tools/refc_convergence.py) are this run
            h = np.load(os.path.join(gold, "refc_convergence_hip.npz"))
            assert np.abs(tr - h["project_h2.5_P2"]).max() < 1e-12 * scale


def test_fullspace_analytic_on_the_gpu(gpu):
    """HIP path against the exact 2-D full-space solution of an explosive line source (oracle/analytic.py):
    explosive-source set-up with the source in the interior, unit-moment projected source, h = 1.25 / P3 and
    h = 0.625 / P4, receivers inside cells 30-45 m away, before any reflection arrives.  Amplitude within 1 %
    (0.5 %), relative L2 misfit below 2 % (0.7 %): the normalisation of the stress source (elastic.py:217-218)
    and the P-wave speed are right (tests/checks/fullspace_check.py, profiles/r03/fullspace_check.txt)."""
    from oracle.analytic import explosive_line_source_2d
    from seigen_amd.harness.explosive_source import ExplosiveSourceLF4
    src = (150.0, 75.0)
    recv = ((194.3, 75.4), (180.3, 105.4), (150.4, 109.3))
    for h, P, dt, tol_a, tol_m in ((1.25, 3, 0.0005, 0.01, 0.02), (0.625, 4, 0.00025, 0.005, 0.007)):
        ex = ExplosiveSourceLF4()
        ex.setup(h=h, degree=P, dt=dt, source_mode="project", source_x=src[0], source_y=src[1])
        t, tr = ex.record_receivers(1.1, receivers=recv, every=int(round(0.005 / dt)))
        for i, (x, y) in enumerate(recv):
            dx, dy = x - src[0], y - src[1]
            r = float(np.hypot(dx, dy))
            vr = explosive_line_source_2d(r, t, ex.Vp)
            ours = tr[:, i, 0] * dx / r + tr[:, i, 1] * dy / r
            a = np.dot(ours, vr) / np.dot(vr, vr)
            m = np.linalg.norm(ours - vr) / np.linalg.norm(vr)
            assert abs(a - 1.0) < tol_a and m < tol_m, (h, P, x, y, a, m)


def test_halfspace_analytic_on_the_gpu(gpu):
    """HIP path against the EXACT solution of the reference's explosive-source problem - an explosive line source 1 m
    below the free surface of a half space (Garvin's problem with buried receivers; oracle/analytic.py
    explosive_line_source_halfspace: direct P in closed form, reflected P, converted SV and the Rayleigh wave by the
    discrete wavenumber method).  The source sits 300 m from the nearest sponge: in the reference's own domain it is
    25 m from the left one, whose abrupt onset (sigma 0 -> 1000, explosive_source_lf4.py:45) reflects P waves into the
    receivers' windows.  Against the point-source solution integrated over the 1 m source box: both components, two
    distances and depths (h = 0.625, P4), amplitude within 0.05 %, relative L2 misfit below 0.1 % over the whole wave train
    (tests/checks/halfspace_check.py, profiles/r03/halfspace_check.txt: 1.0000 / 2e-5 .. 2e-4; 3e-4 .. 5e-3 at h = 1.25, P3)."""
    from oracle.analytic import explosive_box_source_halfspace
    from seigen_amd.harness.explosive_source import ExplosiveSourceLF4
    sx = 300.0
    recv = ((sx + 45.3, 149.0), (sx + 95.3, 147.7))
    ex = ExplosiveSourceLF4()
    ex.setup(Lx=700.0, h=0.625, degree=4, dt=0.00025, source_mode="project", source_x=sx)
    t, tr = ex.record_receivers(2.5, receivers=recv, every=20)
    for i, (x, y) in enumerate(recv):
        vx, vz = explosive_box_source_halfspace(x - sx, 150.0 - y, 1.0, t, ex.Vp, ex.Vs, period=2000.0)
        w = (t > 0.3) & (t < (x - sx) / (0.9194 * ex.Vs) + 0.75)          # up to the end of the Rayleigh wave train
        for ours, exact in ((tr[:, i, 0], vx), (-tr[:, i, 1], vz)):
            a = np.dot(ours[w], exact[w]) / np.dot(exact[w], exact[w])
            m = np.linalg.norm(ours[w] - exact[w]) / np.linalg.norm(exact[w])
            assert abs(a - 1.0) < 5e-4 and m < 1e-3, (x, y, a, m)


def test_fullspace_3d_analytic_on_the_gpu(gpu):
    """3-D MFMA path against the exact full-space solution of an explosive source (oracle/analytic.py
    explosive_point_source_3d, integrated over the source box): the ingredients of BASELINE config 4 - the explosive
    test's material, a Ricker stress source (elastic.py:217-218, :285-288) in the 2 x 2 x 2 cubes at the centre of a
    48^3-cube P3 mesh - at three receivers 25 m away in different directions, before any reflection from the outer
    boundary arrives.  Amplitude within 0.1 %, relative L2 misfit below 0.1 %, no transverse motion
    (tests/checks/fullspace3d_check.py, profiles/r03/fullspace3d_check.txt: 1.0000 / 1e-4 at P3 and P4)."""
    import importlib.util
    from oracle.analytic import explosive_point_source_3d
    spec = importlib.util.spec_from_file_location(
        "fullspace3d_check", os.path.join(os.path.dirname(os.path.abspath(__file__)), "checks", "fullspace3d_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    t, tr, rel, vp, vol = mod.run(n=48, P=3)
    gx, gw = np.polynomial.legendre.leggauss(4)
    a = vol ** (1.0 / 3.0)
    for i in range(len(rel)):
        r = float(np.linalg.norm(rel[i]))
        vbox = np.zeros((len(t), 3))
        for p0, w0 in zip(gx, gw):
            for p1, w1 in zip(gx, gw):
                for p2, w2 in zip(gx, gw):
                    dvec = rel[i] - 0.5 * a * np.array([p0, p1, p2])
                    rr = float(np.linalg.norm(dvec))
                    vbox += (w0 * w1 * w2 / 8.0) * explosive_point_source_3d(rr, t, vp, volume=vol)[:, None] * (dvec / rr)[None, :]
        scale = np.abs(vbox).max()
        assert scale > 0 and np.abs(tr[:, i, :] - vbox).max() < 2e-3 * scale, (i, np.abs(tr[:, i, :] - vbox).max() / scale)
        vr, ours = vbox @ (rel[i] / r), tr[:, i, :] @ (rel[i] / r)
        assert abs(np.dot(ours, vr) / np.dot(vr, vr) - 1.0) < 1e-3
        assert np.linalg.norm(ours - vr) / np.linalg.norm(vr) < 1e-3


def test_pulse_1d(gpu):
    """tests/pulse/pulse_1d_lf4.py (1-D DG1, Gaussian pulse, DG1 sponge at both ends, T = 2: 800 steps)."""
    from seigen_amd.harness.pulse import pulse_1d_lf4
    el, u1, s1 = pulse_1d_lf4(T=2.0)
    m = omesh.IntervalMesh(400, 4.0)
    orc = OracleLF4(m, 1)
    orc.density, orc.dt, orc.mu, orc.l = 1.0, 0.0025, 0.25, 0.5
    X = m.node_coords(1)
    orc.E.set_absorption(np.where((X[..., 0] >= 3.5) | (X[..., 0] <= 0.5), 100.0, 0.0), 1)
    g = np.exp(-50 * (X[..., 0] - 1) ** 2)
    orc.u0 = g[..., None].copy()
    orc.s0 = -g[..., None, None].copy()
    ou, os_ = orc.run(2.0)
    assert orc.nsteps == 800
    assert rel_err(u1.dat.data_cells, ou) < 1e-9
    assert rel_err(s1.dat.data_cells, os_) < 1e-9
    # a right-going pulse (u = -s) travels at Vp = 1: from x = 1 to x = 3 in T = 2
    k = np.unravel_index(np.abs(ou).argmax(), ou.shape)
    assert abs(X[k[0], k[1], 0] - 3.0) < 0.05 and abs(np.abs(ou).max() - 1.0) < 0.02


@pytest.mark.parametrize("degree,n", [(4, (5, 3, 2)), (3, (4, 2, 3)), (2, (3, 3, 2))])
def test_3d_source_and_sponge(gpu, degree, n):
    """The ingredients of BASELINE config 4 (3-D explosive source: a time-dependent diagonal stress
    source in a box, elastic.py:217-218 / :285-288, and a DG4 sponge, :207-208) through the 3-D
    kernels (MFMA for P3/P4, generic for P2), HIP vs oracle over 6 steps."""
    from seigen_amd import _lib
    from seigen_amd.backend import HipBlock
    L = (1.0, 0.6, 0.4)
    h = [L[a] / n[a] for a in range(3)]
    blk = HipBlock(3, degree, n, h, [0.0] * 3)
    m = omesh.structured(3, n, L)
    orc = OracleLF4(m, degree)
    dt = 0.02 * min(h) / degree ** 2
    orc.dt, orc.l, orc.mu, orc.density = dt, 0.5, 0.25, 1.0
    blk.set_params(1.0, dt, 0.5, 0.25)
    # sponge: sigma = 40 for x >= 0.7, interpolated into DG4 (explosive_source_lf4.py:43-45)
    Xs = m.node_coords(4)
    sig = np.where(Xs[..., 0] >= 0.7, 40.0, 0.0)
    orc.E.set_absorption(sig, 4)
    blk.set_absorption(sig, 4)
    # source: indicator of a box times a Ricker-like pulse, on the diagonal
    X = m.node_coords(degree)
    mask = (np.abs(X[..., 0] - 0.3) <= 0.2) & (np.abs(X[..., 1] - 0.3) <= 0.2) & (np.abs(X[..., 2] - 0.2) <= 0.15)
    assert mask.any()
    pattern = np.zeros(X.shape[:-1] + (3, 3))
    for i in range(3):
        pattern[mask, i, i] = 1.0 + 0.5 * i

    def pulse(t):
        a = 4000.0
        return (-1.0 + 2.0 * a * (t - 2.5 * dt) ** 2) * np.exp(-a * (t - 2.5 * dt) ** 2)

    orc.source = lambda t: pulse(t) * pattern
    nsteps = 6
    nodes = np.nonzero(mask.ravel())[0]
    vals = np.stack([pulse((k + 1) * dt) * pattern.reshape(-1, 3, 3)[nodes] for k in range(nsteps)])
    blk.set_source(nodes, vals)
    orc.u0 = seeded(blk.field_shape(_lib.FIELD_U), 21)
    s0 = seeded(blk.field_shape(_lib.FIELD_S), 22)
    orc.s0 = 0.5 * (s0 + np.swapaxes(s0, -1, -2))
    blk.set_field(_lib.FIELD_U, orc.u0)
    blk.set_field(_lib.FIELD_S, orc.s0)
    blk.step(nsteps)
    for k in range(nsteps):
        orc.step((k + 1) * dt)
    assert rel_err(blk.get_field(_lib.FIELD_U), orc.u1) < 1e-10
    assert rel_err(blk.get_field(_lib.FIELD_S), orc.s1) < 1e-10
    # both ingredients must matter: without them the result is different
    plain = HipBlock(3, degree, n, h, [0.0] * 3)
    plain.set_params(1.0, dt, 0.5, 0.25)
    plain.set_field(_lib.FIELD_U, seeded(blk.field_shape(_lib.FIELD_U), 21))
    plain.set_field(_lib.FIELD_S, 0.5 * (s0 + np.swapaxes(s0, -1, -2)))
    plain.step(nsteps)
    assert rel_err(plain.get_field(_lib.FIELD_U), orc.u1) > 1e-6


def test_output_streams(gpu, tmp_path, monkeypatch):
    """output=True (the reference's default, seigen/elastic.py:28): velocity_<k>.vtu / stress_<k>.vtu
    after the initial state and after every step, with point data VelocityNew / StressNew that a
    probe like tests/explosive_source/uy.py:36-43 reads."""
    from seigen_amd import ElasticLF4, UnitSquareMesh, Function, Expression
    from seigen_amd.vtu import read_vtu, vertex_nodes
    monkeypatch.chdir(tmp_path)
    el = ElasticLF4.create(UnitSquareMesh(4, 4), "DG", 2, dimension=2, solver="explicit", output=True)
    el.density, el.dt, el.mu, el.l = 1.0, 0.01, 0.25, 0.5
    el.u0.assign(Function(el.U).interpolate(Expression(("sin(3*x[0])", "cos(2*x[1])"))))
    el.s0.assign(Function(el.S).interpolate(Expression((("x[0]", "0.0"), ("0.0", "x[1]")))))
    u1, s1 = el.run(0.03)                      # 3 steps
    files = sorted(f for f in os.listdir(".") if f.startswith("velocity_"))
    assert files == ["velocity_%d.vtu" % k for k in range(4)]          # initial state + 3 steps
    assert os.path.exists("velocity.pvd") and os.path.exists("stress.pvd")
    pts, data = read_vtu("velocity_3.vtu")
    vn = vertex_nodes(2, 2)
    np.testing.assert_allclose(data["VelocityNew"][:, :2], u1.dat.data_cells[:, vn].reshape(-1, 2), rtol=0, atol=1e-15)
    _, sd = read_vtu("stress_3.vtu")
    np.testing.assert_allclose(sd["StressNew"].reshape(-1, 3, 3)[:, :2, :2], s1.dat.data_cells[:, vn].reshape(-1, 2, 2), atol=1e-15)


def test_eigenmode_bench_record(gpu, tmp_path):
    """The pybench-style record of tests/eigenmode/eigenmode_bench.py:19-57: series, timers, metadata."""
    import json
    from seigen_amd.harness.eigenmode_bench import eigenmode_record
    path = tmp_path / "EigenmodeLF4.json"
    # T = 5: the error functional of the reference compares with the analytic fields at t = 5
    # (eigenmode_2d.py:49-63), whatever T the run had
    rec = eigenmode_record(dim=2, N=8, degree=2, dt=-1.0, T=5.0, path=str(path))
    assert rec["series"] == {"np": 1, "dim": 2, "size": 8, "T": 5.0, "solver": "explicit", "opt": 2, "degree": 2,
                             "dt": 0.5 / 8 / 2}
    assert rec["meta"]["dofs"] == 8 * 8 * 2 * 6 * 4                      # S dofs as elastic.py:85-86
    assert 0 < rec["meta"]["u_error"] < 1e-2 and 0 < rec["meta"]["s_error"] < 1e-2
    for task in ("timestepping", "solver setup", "compute_error"):
        assert rec["timings"][task] > 0
    assert json.loads(path.read_text())["meta"]["dofs"] == rec["meta"]["dofs"]


def test_explosive_source_bench_record(gpu, tmp_path):
    """The pybench-style record of tests/explosive_source/explosive_source_bench.py:15-24: series h, T, explicit; the
    run's named timers."""
    import json
    import seigen_amd
    import seigen_amd.helpers as helpers
    import seigen_amd.harness.explosive_source as hx
    helpers.log = seigen_amd.elastic.log = hx.log = lambda s: None
    from seigen_amd.harness.explosive_source_bench import explosive_source_record
    path = tmp_path / "ExplosiveSourceLF4.json"
    rec = explosive_source_record(T=0.01, h=2.5, explicit=True, path=str(path), dt=0.001)
    assert rec["series"] == {"np": 1, "h": 2.5, "T": 0.01, "explicit": True}
    assert rec["meta"] == {"dofs": 120 * 60 * 2 * 6 * 4, "steps": 10}
    for task in ("mesh generation", "timestepping", "solver setup", "elastic-run"):
        assert rec["timings"][task] > 0, (task, rec["timings"])
    assert json.loads(path.read_text())["series"] == rec["series"]
    rec2 = explosive_source_record(T=0.005, explicit=False, dt=0.001)       # the implicit class runs too
    assert rec2["series"]["explicit"] is False and rec2["meta"]["steps"] == 5


def test_separable_source(gpu):
    """sg_set_source_separable (one slice + a weight per step) against sg_set_source with the table of the products:
    bitwise equal, on the fused-source 2-D tile path and on the launch path (3-D); through the solver class an
    Expression source whose table would not fit is factorised after testing it, a source that does not factorise
    still raises."""
    from seigen_amd import ElasticLF4, Expression, Function, RectangleMesh, _lib
    from seigen_amd.backend import HipBlock
    rng = np.random.default_rng(4)
    for dim, degree, n in ((2, 3, (20, 9)), (3, 4, (3, 2, 2)), (3, 2, (2, 2, 3))):
        res = []
        for mode in ("table", "separable"):
            blk = HipBlock(dim, degree, n, [1.0 / v for v in n], [0.0] * dim)
            blk.set_params(1.0, 1e-3, 0.5, 0.25)
            r2 = np.random.default_rng(5)
            blk.set_field(_lib.FIELD_U, r2.uniform(-1, 1, blk.field_shape(_lib.FIELD_U)))
            nodes = np.sort(r2.choice(blk.ncells * blk.nd, 9, replace=False))
            pat = r2.uniform(-1, 1, (9, dim, dim))
            pat = pat + np.swapaxes(pat, 1, 2)
            w = r2.uniform(-2, 2, 5)
            if mode == "table":
                blk.set_source(nodes, w[:, None, None, None] * pat[None])
            else:
                blk.set_source_separable(nodes, pat, w)
            blk.step(7)                                  # two steps beyond the source's five
            res.append((blk.get_field(_lib.FIELD_U), blk.get_field(_lib.FIELD_S)))
            blk.close()
        assert np.abs(res[0][1]).max() > 0
        assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]), (dim, degree)
    # solver class: the same box x Ricker source as a table and, with the table "too large", factorised
    out = []
    for cap in (None, 0):
        mesh = RectangleMesh(16, 8, 16.0, 8.0)
        el = ElasticLF4.create(mesh, "DG", 2, dimension=2, solver="explicit", output=False)
        el.density, el.mu, el.l, el.dt = 1.0, 3.0, 2.0, 1e-3
        code = "x[0] >= 4.0 && x[0] <= 9.0 && x[1] >= 2.0 && x[1] <= 5.0 ? (1.0 + x[0]) * sin(40.0 * t) : 0.0"
        el.source_expression = Expression(((code, "0.0"), ("0.0", code)), t=0)
        el.source_function = Function(el.S)
        el.source = el.source_expression
        if cap is not None:
            el.SOURCE_TABLE_MAX_BYTES = cap
        u1, s1 = el.run(30 * el.dt * (1 + 1e-9))
        out.append((u1.dat.data_cells.copy(), s1.dat.data_cells.copy()))
    scale = np.abs(out[0][1]).max()
    assert scale > 0 and np.abs(out[0][1] - out[1][1]).max() < 1e-13 * scale
    assert np.abs(out[0][0] - out[1][0]).max() < 1e-13 * max(np.abs(out[0][0]).max(), 1e-300)
    # not separable: the box moves with t
    mesh = RectangleMesh(16, 8, 16.0, 8.0)
    el = ElasticLF4.create(mesh, "DG", 2, dimension=2, solver="explicit", output=False)
    el.density, el.mu, el.l, el.dt = 1.0, 3.0, 2.0, 1e-3
    code = "x[0] >= 4.0 + 100.0 * t && x[0] <= 9.0 + 100.0 * t ? 1.0 : 0.0"
    el.source_expression = Expression(((code, "0.0"), ("0.0", code)), t=0)
    el.source_function = Function(el.S)
    el.source = el.source_expression
    el.SOURCE_TABLE_MAX_BYTES = 0
    with pytest.raises(MemoryError):
        el.run(30 * el.dt)


@pytest.mark.parametrize("case", ["tri", "quad", "tet"])
def test_box_ricker_source_from_its_parameters(gpu, case):
    """sg_set_source_box_ricker (the reference's source, explosive_source_lf4.py:36-40, from box and wavelet parameters)
    against the same source handed over as nodes + Expression values by the host layer: same node set, weights equal
    to the last bit or two of exp(), fields to 1e-13; boxes that contain no node / reach outside the block."""
    import math
    from seigen_amd import _lib
    from seigen_amd.backend import HipBlock
    a, t0 = 159.42, 0.03
    if case == "tet":
        dim, P, n, h, diag = 3, 3, (6, 5, 4), [2.5, 2.5, 2.5], "left"
        lo, hi = (4.5, 4.5, 4.5), (8.0, 8.0, 8.0)
    else:
        dim, P, n, h, diag = 2, 2, (24, 10), [2.5, 2.5], "quadrilateral" if case == "quad" else "left"
        lo, hi = (14.5, 18.5), (15.5, 19.5)          # the reference's 1 m box: a node on the box line counts (closed box)
    dt, nsteps = 1e-3, 40
    res = []
    for mode in ("host", "abi"):
        blk = HipBlock(dim, P, n, h, [0.0] * dim, diag)
        blk.set_params(1.0, dt, 3599.3664, 3600.0)
        if mode == "host":
            X = blk.node_coords().reshape(-1, dim)
            inside = np.all((X >= np.asarray(lo)) & (X <= np.asarray(hi)), axis=1)
            nodes = np.nonzero(inside)[0]
            assert len(nodes) > 0
            pat = np.zeros((len(nodes), dim, dim))
            for i in range(dim):
                pat[:, i, i] = 1.0
            w = np.array([(-1.0 + 2 * a * (dt * (k + 1) - t0) ** 2) * math.exp(-a * (dt * (k + 1) - t0) ** 2) for k in range(nsteps)])
            blk.set_source_separable(nodes, pat, w)
        else:
            blk.set_source_box_ricker(lo, hi, a, t0, dt, dt, nsteps)
        blk.step(nsteps + 3)
        res.append((blk.get_field(_lib.FIELD_U), blk.get_field(_lib.FIELD_S)))
        blk.close()
    scale = np.abs(res[0][1]).max()
    assert scale > 0
    assert np.abs(res[0][1] - res[1][1]).max() < 1e-13 * scale
    assert np.abs(res[0][0] - res[1][0]).max() < 1e-13 * np.abs(res[0][0]).max()
    # a box between the nodes: no source; a box that sticks out of the block: clipped; lo > hi: an error
    blk = HipBlock(dim, P, n, h, [0.0] * dim, diag)
    blk.set_params(1.0, dt, 0.5, 0.25)
    blk.set_source_box_ricker([0.3] * dim, [0.4] * dim, a, t0, dt, dt, nsteps)
    blk.step(3)
    assert np.abs(blk.get_field(_lib.FIELD_S)).max() == 0.0
    blk.set_source_box_ricker([-50.0] * dim, [1.0] * dim, a, t0, dt, dt, nsteps)
    blk.step(3)
    assert np.abs(blk.get_field(_lib.FIELD_S)).max() > 0.0
    with pytest.raises(_lib.SeigenHipError):
        blk.set_source_box_ricker([1.0] * dim, [0.5] * dim, a, t0, dt, dt, nsteps)


@pytest.mark.parametrize("quad", [0, 1])
def test_plain_c_host_through_the_c_abi(gpu, tmp_path, quad):
    """examples/explosive_source_c_abi.c: the explosive-source set-up (sponge, box-Ricker source, run, download) from a
    C99 program that links libseigen_hip.so and nothing else - the drop-in boundary without the Python host layer.
    Its final velocity field equals the same run through HipBlock bit for bit."""
    import subprocess
    from seigen_amd import _lib
    from seigen_amd.backend import HipBlock
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "explosive_source_c_abi")
    libdir = os.path.join(root, "seigen_amd")
    cc = subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I" + os.path.join(root, "include"),
                         os.path.join(root, "examples", "explosive_source_c_abi.c"), "-o", exe,
                         "-L" + libdir, "-lseigen_hip", "-Wl,-rpath," + libdir, "-lm"], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    nx, ny, P, nsteps = 40, 24, 2, 60
    out = str(tmp_path / "u.bin")
    run = subprocess.run([exe, str(nx), str(ny), str(P), str(nsteps), str(quad), out], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "device_ms_per_step" in run.stdout
    u_c = np.fromfile(out)
    blk = HipBlock(2, P, (nx, ny), [2.5, 2.5], [0.0, 0.0], "quadrilateral" if quad else "left")
    blk.set_params(1.0, 1e-3, 3599.3664, 3600.0)
    X = blk.node_coords(4)
    Lx, Ly = nx * 2.5, ny * 2.5
    blk.set_absorption(np.where((X[..., 0] <= 20.0) | (X[..., 0] >= Lx - 20.0) | (X[..., 1] <= 20.0), 1000.0, 0.0), 4)
    blk.set_source_box_ricker((44.5, Ly - 1.5), (45.5, Ly - 0.5), 159.42, 0.03, 1e-3, 1e-3, nsteps)
    blk.step(nsteps)
    u_py = blk.get_field(_lib.FIELD_U)
    assert np.abs(u_py).max() > 0
    assert np.array_equal(u_c, u_py.ravel())


@pytest.mark.parametrize("seed", range(int(os.environ.get("SEIGEN_TEST_SOLVER_FUZZ", "6"))))
def test_solver_class_random_setups_against_the_oracle(gpu, seed):
    """Host-layer fuzz: the public solver class with a random mesh (interval / triangles / quadrilaterals /
    tetrahedra), degree, material and density (floats or per-cell arrays, either density convention), Expression
    initial conditions, an Expression sponge in a DG space of random degree, an Expression source `box ? f(t) : 0`
    (table or factorised upload), run(T) with the reference's step rule - against the oracle fed with the same
    Expressions evaluated at its own nodes."""
    import seigen_amd
    import seigen_amd.helpers as helpers
    from seigen_amd import (BoxMesh, ElasticLF4, Expression, Function, FunctionSpace, IntervalMesh, RectangleMesh)
    from tests.util import oracle_mesh
    helpers.log = seigen_amd.elastic.log = lambda s: None
    rng = np.random.default_rng(13000 + seed)
    dim = int(rng.integers(1, 4))
    P = int(rng.integers(1, 5))
    n = tuple(int(x) for x in rng.integers(2, {1: 14, 2: 8, 3: 4}[dim], size=dim))
    L = tuple(float(x) for x in rng.uniform(0.8, 2.2, size=dim))
    quad = bool(dim == 2 and rng.integers(0, 2))
    diagonal = "right" if (dim == 2 and not quad and rng.integers(0, 2)) else "left"
    if dim == 1:
        mesh, om = IntervalMesh(n[0], L[0]), oracle_mesh(1, n, L)
    elif dim == 2:
        mesh = RectangleMesh(n[0], n[1], L[0], L[1], diagonal=diagonal, quadrilateral=quad)
        om = oracle_mesh(2, n, L, "quadrilateral" if quad else diagonal)
    else:
        mesh, om = BoxMesh(n[0], n[1], n[2], L[0], L[1], L[2]), oracle_mesh(3, n, L)
    solver = ("explicit", "implicit", "tiling")[int(rng.integers(0, 3))]
    el = ElasticLF4.create(mesh, "DG", P, dimension=dim, solver=solver, output=False)
    orc = OracleLF4(om, P)
    nc = om.ncells
    assert el.U.ncells == nc
    per_cell = bool(rng.integers(0, 2))
    el.l = orc.l = rng.uniform(0.4, 0.9, nc) if per_cell else float(rng.uniform(0.4, 0.9))
    el.mu = orc.mu = rng.uniform(0.2, 0.5, nc) if per_cell else float(rng.uniform(0.2, 0.5))
    el.density = orc.density = rng.uniform(0.7, 1.5, nc) if rng.integers(0, 2) else float(rng.uniform(0.7, 1.5))
    if solver == "implicit":
        orc.density_physical = True                       # the implicit forms' convention (elastic.py:175-178)
    elif rng.integers(0, 2):
        el.density_physical = orc.density_physical = True
    h = min(L[a] / n[a] for a in range(dim))
    el.dt = orc.dt = 0.03 * h / P ** 2
    nsteps = int(rng.integers(1, 6))
    # initial conditions
    k1, k2 = float(rng.uniform(1, 4)), float(rng.uniform(1, 4))
    ucode = tuple("sin(%r*x[%d]) + 0.3*cos(%r*x[0])" % (k1 + i, i, k2) for i in range(dim))
    scode = tuple(tuple("0.2*sin(%r*x[%d])*cos(%r*x[%d])" % (k1 + i + j, i, k2, j) for j in range(dim)) for i in range(dim))
    uex, sex = Expression(ucode if dim > 1 else ucode[0]), Expression(scode if dim > 1 else scode[0][0])
    if dim == 1:
        uex, sex = Expression((ucode[0],)), Expression(((scode[0][0],),))
    el.u0.assign(Function(el.U).interpolate(uex))
    el.s0.assign(Function(el.S).interpolate(sex))
    Xo = om.node_coords(P)
    orc.u0 = uex.evaluate(Xo).reshape(nc, -1, dim)
    orc.s0 = sex.evaluate(Xo).reshape(nc, -1, dim, dim)
    # sponge
    if rng.integers(0, 2):
        q = int(rng.integers(1, 5))
        cut = float(rng.uniform(0.2, 0.8)) * L[0]
        aex = Expression("x[0] <= %r ? %r : 0.0" % (cut, float(rng.uniform(2.0, 30.0))))
        el.absorption_function = Function(FunctionSpace(mesh, "DG", q))
        el.absorption = aex
        orc.E.set_absorption(aex.evaluate(om.node_coords(q)).reshape(nc, -1), q)
    # source: indicator of a box (edges away from every node) times a function of t
    if rng.integers(0, 2):
        lo = [float(rng.uniform(0.1, 0.4)) * L[a] + 1.2345e-3 for a in range(dim)]
        hi = [float(rng.uniform(0.6, 0.9)) * L[a] + 2.3456e-3 for a in range(dim)]
        box = " && ".join("x[%d] >= %r && x[%d] <= %r" % (a, lo[a], a, hi[a]) for a in range(dim))
        ft = "(1.0 + 0.5*x[0])*sin(%r*t)" % float(rng.uniform(20.0, 200.0))
        code = "%s ? %s : 0.0" % (box, ft)
        rows = tuple(tuple(code if i == j else "0.0" for j in range(dim)) for i in range(dim))
        sx = Expression(rows, t=0)
        el.source_expression = sx
        el.source_function = Function(el.S)
        el.source = el.source_expression
        if rng.integers(0, 2):
            el.SOURCE_TABLE_MAX_BYTES = 0                 # force the factorised (separable) upload

        def osource(t, sx=sx):
            sx.t = t
            return sx.evaluate(Xo).reshape(nc, -1, dim, dim)
        orc.source = osource
    u1, s1 = el.run(nsteps * el.dt * (1 + 1e-9))
    assert el.block.counters()["steps"] == nsteps
    for k in range(nsteps):
        orc.step((k + 1) * orc.dt)
    tol = 1e-9
    assert rel_err(u1.dat.data_cells, orc.u1) < tol, (seed, dim, P, n, quad, solver)
    assert rel_err(s1.dat.data_cells, orc.s1) < tol, (seed, dim, P, n, quad, solver)
