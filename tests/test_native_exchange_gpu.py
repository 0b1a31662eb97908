"""The native in-library halo exchange (csrc/comm.cpp) with 2, 3, 4 and 8 REAL ranks - on the test box's one GPU, through a
test-double transport.

Real RCCL refuses two ranks on one device, and no multi-GPU node is available to the tests, so until now comm.cpp had
only ever run with a single rank that is its own neighbour.  Here every rank is a thread of control of its own (fresh
worker processes; the 8-rank case runs two ranks per process to stay inside the box's limit of GPU processes) that drives
the C-ABI directly - sg_comm_check, sg_comm_init, sg_comm_selftest, one sg_step(n) - while `SEIGEN_RCCL_LIB` binds the
library's nine RCCL entry points to tests/fake_rccl (shared memory + host staging, RCCL's pairing and ordering rules;
checked on its own in tests/test_fake_rccl.py).  What runs for the first time between DIFFERENT ranks: ncclCommInitRank
across processes, peers on all three axes, the facing-side order of the receives, the statistics - and the result must
equal the single-block run BITWISE (the reference's exchange: seigen/elastic.py:404-436, ParLoopHaloEnd in
tests/tiling/utils.py:143-144).  The double has two modes: blocking (every call completes its transfers before it
returns: any number of ranks per process) and ASYNC (the transfers are work on the library's stream - copies and host
functions - and the calls return at once, as RCCL's do: the two-stream schedule of a split stage then runs concurrently
with the exchange instead of being serialised by the transport).

The first test runs 3-D tetrahedral blocks (mfma_stage_F / G, and the generic kernels on small blocks).  The second, test_native_
exchange_of_every_family_and_dimension_bitwise, runs everything else comm.cpp's loop over 2 * dim sides is meant to be blind
to: 1-D and 2-D blocks (two and four sides), triangles of either diagonal, quadrilaterals and hexahedra, FP64 and FP32,
symmetric and full-tensor stress, and each remaining stage family - tile2d_stage, hexm_stage, hex_stage, lane_stage in 1-D,
2-D and 3-D, the generic stage_kernel - every row pinned to its family by the kernel names the split blocks report, and
one row per new dimension and cell class held against OracleLF4 as well.

The second half runs the host-side agreement of seigen_amd/parallel.py::NativeExchanger
through the solver class (gloo process group, SEIGEN_HALO_NATIVE=force): a failure injected into ONE rank - argument
check, communicator, self-test - must put EVERY rank on the host-driven exchanger, within a timeout, with the same
bitwise result; and, without a fault, the 2-D explosive source on 2 and 4 ranks and the reference's own multi-rank protocol -
the 2-D eigenmode on the unit square - on four."""
import json
import math
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


@pytest.fixture(scope="module")
def fake():
    from fake_rccl.build import build
    return build()


def _env(fake, tmp_path, **extra):
    env = dict(os.environ, SEIGEN_RCCL_LIB=fake, FAKE_RCCL_TIMEOUT_S="60", FAKE_RCCL_LOG=str(tmp_path / "fake"),
               HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2")
    env.pop("FAKE_RCCL_HOST", None)
    env.update(extra)
    return env


def _spawn_workers(fake, tmp_path, world, layout, grid, n, degree, steps, dtype, scenario, more=(), **extra_env):
    """The worker processes of one case (`more`: the worker's optional arguments - cell type, SEIGEN_HIP_PATH, initial
    stress).  Every worker writes into a file of its own - a pipe that nobody reads while an earlier worker is waited for
    fills up, and the worker behind it then blocks in a print until the double's timeout - and all share one deadline.
    Nothing is retried: a worker that fails or is killed at the deadline is reported with the tail of its file."""
    procs, logs, first = [], [], 0
    for k in layout:
        logs.append(tmp_path / ("worker%d.log" % first))
        with open(logs[-1], "w") as log:
            procs.append(subprocess.Popen(
                [sys.executable, os.path.join(ROOT, "tests", "native_exchange_worker.py"), str(tmp_path), str(world), str(first),
                 str(k), ",".join(map(str, grid)), ",".join(map(str, n)), str(degree), str(steps), dtype, scenario] + list(more),
                cwd=ROOT, env=_env(fake, tmp_path, **extra_env), stdin=subprocess.DEVNULL, stdout=log, stderr=subprocess.STDOUT))
        first += k
    assert first == world
    deadline = time.time() + 400
    errs = []
    for p, log in zip(procs, logs):
        killed = ""
        try:
            p.wait(timeout=max(1.0, deadline - time.time()))
        except subprocess.TimeoutExpired:
            p.kill()
            p.wait()
            killed = "\n[killed at the deadline]"
        if p.returncode != 0:
            errs.append("%s: exit %r\n%s%s" % (log.name, p.returncode, open(log, errors="replace").read()[-4500:], killed))
    assert not errs, "\n-----\n".join(errs)


def _single_block(n, degree, steps, dtype, scenario, cell="left", nonsym=False):
    """The whole mesh as one block, set up by the worker's setup_block and stepped here; with its fields: the inputs an
    oracle needs (node coordinates, initial fields, time step)."""
    from seigen_amd import _lib
    from seigen_amd.backend import HipBlock
    from native_exchange_worker import setup_block
    dim = len(n)
    blk = HipBlock(dim, degree, n, [1.0 / n[a] for a in range(dim)], [0.0] * dim, cell, 0, dtype=dtype)
    dt = setup_block(blk, n, degree, scenario, nonsym)
    out = {"dt": dt, "X": blk.node_coords(), "X4": blk.node_coords(4), "u0": blk.get_field(_lib.FIELD_U),
           "s0": blk.get_field(_lib.FIELD_S), "kernels": [blk.stage_kernel_name(st) for st in range(6)], "is_sym": blk.is_sym()}
    blk.step(steps)
    blk.sync()
    out.update({"u": blk.get_field(_lib.FIELD_U), "s": blk.get_field(_lib.FIELD_S), "uh": blk.get_field(_lib.FIELD_UH)})
    blk.close()
    return out


def _block_cells(n, start, bn, cell="left"):
    """cells of the mesh `n` in a block, in the block's order: 1-D, 2-D or 3-D; one cell per square / cube for
    "quadrilateral" (quadrilaterals and hexahedra), 2 triangles / 6 tetrahedra otherwise"""
    from native_exchange_worker import block_cells
    return block_cells(n, start, bn, cell)


@pytest.mark.parametrize("world,layout,grid,n,degree,dtype,scenario,mode", [
    (2, [1, 1], (1, 1, 2), (16, 4, 4), 4, "f64", "plain", "blocking"),         # slab, the headline element
    (2, [1, 1], (2, 1, 1), (32, 2, 2), 4, "f64", "source", "blocking"),        # x split: shells of whole layout groups
    (4, [1, 1, 1, 1], (2, 2, 1), (32, 4, 2), 4, "f64", "source", "blocking"),  # 2 x 2 x 1, P4, source + sponge across the blocks
    (4, [1, 1, 1, 1], (1, 2, 2), (16, 4, 4), 2, "f64", "source", "blocking"),  # P2
    (4, [2, 2], (1, 1, 4), (16, 2, 8), 3, "f32", "plain", "blocking"),         # inner blocks with two neighbours on one axis, FP32
    (8, [2, 2, 2, 2], (2, 2, 2), (32, 4, 4), 4, "f64", "source", "blocking"),  # config 4's grid: 2 x 2 x 2, peers on three axes
    (8, [2, 2, 2, 2], (2, 2, 2), (8, 4, 4), 2, "f64", "source", "blocking"),   # P2, generic-kernel sized blocks
    # the double's ASYNC mode (one rank per process): the transfers are stream-ordered work and the calls return at once, as
    # RCCL's do - the SECOND launches on the second stream and the next stage's FIRST really run beside / behind them
    (2, [1, 1], (1, 1, 2), (16, 4, 4), 4, "f64", "source", "async"),
    (4, [1, 1, 1, 1], (2, 2, 1), (32, 4, 2), 4, "f64", "source", "async"),
    (4, [1, 1, 1, 1], (1, 2, 2), (32, 8, 8), 3, "f64", "plain", "async"),       # larger blocks: launches long enough to overlap
    (4, [1, 1, 1, 1], (1, 1, 4), (16, 2, 8), 2, "f32", "source", "async"),
])
def test_native_exchange_between_ranks_bitwise(gpu, fake, tmp_path, world, layout, grid, n, degree, dtype, scenario, mode):
    steps = 3
    extra = {"FAKE_RCCL_ASYNC": "1", "FAKE_RCCL_SLOT_BYTES": "1048576"} if mode == "async" else {}
    _spawn_workers(fake, tmp_path, world, layout, grid, n, degree, steps, dtype, scenario, **extra)
    single = _single_block(n, degree, steps, dtype, scenario)
    assert np.isfinite(single["u"]).all() and np.abs(single["u"]).max() > 0
    for rank in range(world):
        d = np.load(tmp_path / ("rank%d.npz" % rank))
        assert int(d["selftest"]) == 0 and int(d["nsides"]) >= 1 and int(d["version"]) // 10000 == 2
        idx = _block_cells(n, d["start"], d["n"])
        for key in ("u", "s", "uh"):
            assert np.array_equal(d[key], single[key][idx]), "%s differs from the single-block run (rank %d)" % (key, rank)
        # the double really carried it: one message per side and exchange (+ the two self-test exchanges)
        log = json.loads(open(str(tmp_path / "fake") + ".rank%d" % rank).read().splitlines()[-1])
        nex = int(d["exchanges"]) + 2
        assert log["host_mode"] == 0 and log["sends"] == log["recvs"] == nex * int(d["nsides"]) and log["groups"] == nex
        assert log["async"] == (1 if mode == "async" else 0)
        assert log["bytes_sent"] >= int(d["bytes_sent"]) > 0


_Q = "quadrilateral"
_TILE, _LANE, _GEN, _HEXM, _HEX = "sg::tile2d_stage<", "sg::lane_stage<", "sg::stage_kernel<", "sg::hexm_stage<", "sg::hex_stage<"
# Every other kernel family and dimension through comm_step: world, ranks per worker process, cell, degree, dtype,
# SEIGEN_HIP_PATH (None: the library's own choice), mesh, block grid, scenario, the double's mode, non-symmetric initial
# stress, the family every stage kernel of every rank must belong to, oracle anchor.  The shapes are those of the
# host-driven split rows that pin these families (SPLITS of tests/test_tile2d_family_gpu.py and tests/
# test_lane_generic_family_gpu.py, tests/test_hex_gpu.py): x cuts with shells a whole layout group thick (gw = 16: 36 and
# 40 squares per block; gw = 64: 145 cubes and 65 hexahedra per block), blocks narrower than two groups (nothing left to
# the launch beside the exchange), an inner 1-D block (two neighbours on its one axis, two sides in all), corners on the
# (2, 2), (4, 2) and (2, 2, 2) grids.  The hexahedral DQ_2 row names SEIGEN_HIP_PATH=lane, as tests/test_hex_gpu.py does:
# below SG_HEX_LANE_MIN_CELLS cubes the library's own choice is the generic family (hostapi.cpp choose_kernel_path).
FAMILY_ROWS = [
    ("tile-tri-P3-x", 2, [1, 1], "left", 3, "f64", None, (72, 6), (2, 1), "source", "blocking", False, _TILE, False),
    ("tile-right-P3-2x2", 4, [1, 1, 1, 1], "right", 3, "f64", None, (9, 6), (2, 2), "source", "async", False, _TILE, True),
    ("tile-tri-P4-full", 4, [1, 1, 1, 1], "left", 4, "f64", None, (72, 6), (2, 2), "source", "async", True, _TILE, False),
    ("tile-quad-DQ3", 4, [2, 2], _Q, 3, "f64", None, (72, 6), (2, 2), "source", "blocking", False, _TILE, False),
    ("tile-tri-P1-f32", 2, [1, 1], "left", 1, "f32", None, (80, 5), (2, 1), "plain", "async", False, _TILE, False),
    ("tile-quad-DQ4-f32", 4, [2, 2], _Q, 4, "f32", None, (7, 4), (2, 2), "source", "blocking", False, _TILE, False),
    ("tile-tri-P2-4x2", 8, [2, 2, 2, 2], "left", 2, "f64", None, (72, 8), (4, 2), "source", "blocking", False, _TILE, False),
    ("lane-tri-P2-y", 2, [1, 1], "left", 2, "f64", "lane", (6, 7), (1, 2), "source", "blocking", False, _LANE, False),
    ("generic-tri-P3-x", 2, [1, 1], "left", 3, "f64", "generic", (34, 4), (2, 1), "source", "blocking", False, _GEN, False),
    ("lane-1d-P3-three", 3, [1, 1, 1], "left", 3, "f64", "lane", (9,), (3,), "source", "blocking", False, _LANE, True),
    ("generic-1d-P1", 2, [1, 1], "left", 1, "f64", "generic", (70,), (2,), "plain", "async", False, _GEN, False),
    ("lane-tet-P1-x", 2, [1, 1], "left", 1, "f64", "lane", (290, 2, 2), (2, 1, 1), "source", "blocking", False, _LANE, False),
    ("hexm-DQ3-full", 4, [1, 1, 1, 1], _Q, 3, "f64", None, (36, 4, 2), (2, 2, 1), "source", "async", True, _HEXM, True),
    ("hexm-DQ4-2x2x2", 8, [2, 2, 2, 2], _Q, 4, "f64", None, (6, 4, 4), (2, 2, 2), "source", "blocking", False, _HEXM, False),
    ("hex-DQ2-x", 2, [1, 1], _Q, 2, "f64", "lane", (130, 6, 2), (2, 1, 1), "source", "blocking", False, _HEX, False),
    ("generic-hex-DQ1", 8, [2, 2, 2, 2], _Q, 1, "f64", "generic", (4, 4, 4), (2, 2, 2), "plain", "blocking", False, _GEN, False),
]


def _oracle_fields(single, n, cell, degree, steps, scenario):
    """(u, s) of OracleLF4 after `steps` steps from the single block's inputs: the same mesh, material, initial fields, and
    - scenario "source" - the sponge of sigma_at at the DG4 nodes and the box-Ricker source of setup_block, handed over as
    the values of each step on the nodes inside the closed box (sg_set_source_box_ricker: the identity pattern times the
    wavelet at t = (k + 1) dt)"""
    from native_exchange_worker import SOURCE_A, sigma_at, source_box
    from oracle.lf4 import OracleLF4
    from tests.util import oracle_mesh
    dim, dt, X = len(n), single["dt"], single["X"]
    orc = OracleLF4(oracle_mesh(dim, n, (1.0,) * dim, cell), degree)
    orc.dt, orc.l, orc.mu, orc.density = dt, 0.5, 0.25, 1.0
    orc.u0, orc.s0 = single["u0"].copy(), single["s0"].copy()
    inside = np.zeros(X.shape[:2], dtype=bool)
    if scenario == "source":
        orc.E.set_absorption(sigma_at(single["X4"]), 4)
        lo, hi = source_box(dim)
        inside = np.all((X >= np.asarray(lo)) & (X <= np.asarray(hi)), axis=-1)
        assert 0 < inside.sum() < inside.size
    for k in range(steps):
        t = (k + 1) * dt - 2.5 * dt
        S = np.zeros(X.shape[:2] + (dim, dim))
        S[inside] = (-1.0 + 2 * SOURCE_A * t ** 2) * math.exp(-SOURCE_A * t ** 2) * np.eye(dim)
        orc.source = lambda tt, S=S: S
        orc.step((k + 1) * dt)
    return orc.u1, orc.s1


@pytest.mark.parametrize("row", FAMILY_ROWS, ids=[r[0] for r in FAMILY_ROWS])
def test_native_exchange_of_every_family_and_dimension_bitwise(gpu, fake, tmp_path, monkeypatch, row):
    """comm_step on 1-D, 2-D and hexahedral blocks and on the lane and generic families: sg_comm_check / sg_comm_init with
    two and four sides, the byte counts of sg_halo_bytes, the self-test, the facing-side receives, the tile family's fused
    source on a split stage, the hexahedral families' sponge pre-pass under the SECOND region, group-thick x shells and the
    two-stream schedule around stage kernels of microseconds.  Every rank's fields equal the single block's bit for bit, the
    kernels the split blocks name belong to the family the row claims, and three rows - one per new dimension and cell class
    - are assembled and held against the oracle, within the suite's bound for whole steps (10 tol_of, tests/
    test_parity_gpu.py): bitwise agreement alone would not notice both runs being wrong together."""
    from native_exchange_worker import check_family, check_rank_fields
    from tests.test_parity_gpu import tol_of
    from tests.util import rel_err
    name, world, layout, cell, degree, dtype, path, n, grid, scenario, mode, nonsym, family, anchored = row
    assert len(layout) <= 4 and (mode != "async" or set(layout) == {1})      # the box's process limit; the double's rule
    steps = 3
    for var in ("SEIGEN_HIP_SYM", "SEIGEN_HIP_SOURCE_LAUNCH", "SEIGEN_HIP_TILE_GRID", "SEIGEN_HIP_GRAPH", "SEIGEN_HIP_SPONGE_AFFINE"):
        monkeypatch.delenv(var, raising=False)      # nothing but the row picks an instantiation, a grid or a source path
    if path is None:
        monkeypatch.delenv("SEIGEN_HIP_PATH", raising=False)
    else:
        monkeypatch.setenv("SEIGEN_HIP_PATH", path)      # the single block of this process; the workers inherit it too
    extra = {"FAKE_RCCL_ASYNC": "1", "FAKE_RCCL_SLOT_BYTES": "1048576"} if mode == "async" else {}
    _spawn_workers(fake, tmp_path, world, layout, grid, n, degree, steps, dtype, scenario,
                   more=[cell, path or "-", "nonsym" if nonsym else "sym"], **extra)
    single = _single_block(n, degree, steps, dtype, scenario, cell, nonsym)
    assert np.isfinite(single["u"]).all() and np.abs(single["u"]).max() > 0 and np.abs(single["s0"]).max() > 0
    number_type = {"f64": "double", "f32": "float"}[dtype] if family == _TILE else None
    check_family(single["kernels"], family, number_type)
    # (the generic kernels have no symmetric-stress storage: tests/test_lane_generic_family_gpu.py reports_sym)
    sym = not nonsym and family != _GEN
    assert single["is_sym"] == sym
    ranks = [np.load(tmp_path / ("rank%d.npz" % rank)) for rank in range(world)]
    sides = 0
    for rank, d in enumerate(ranks):
        assert int(d["selftest"]) == 0 and int(d["nsides"]) >= 1 and int(d["version"]) // 10000 == 2
        check_family(d["kernels"], family, number_type)
        assert bool(d["is_sym"]) == sym
        check_rank_fields(d, single, n, cell, rank)
        # the double really carried it: one message per side and exchange (+ the two self-test exchanges)
        log = json.loads(open(str(tmp_path / "fake") + ".rank%d" % rank).read().splitlines()[-1])
        nex = int(d["exchanges"]) + 2
        assert log["host_mode"] == 0 and log["sends"] == log["recvs"] == nex * int(d["nsides"]) and log["groups"] == nex
        assert log["async"] == (1 if mode == "async" else 0)
        assert log["bytes_sent"] >= int(d["bytes_sent"]) > 0
        sides += int(d["nsides"])
    # every cut of the grid is one side of each of its two blocks
    assert sides == 2 * sum((grid[a] - 1) * int(np.prod(grid)) // grid[a] for a in range(len(grid)))
    if anchored:
        assert dtype == "f64"
        got = {key: np.full_like(single[key], np.nan) for key in ("u", "s")}
        for d in ranks:
            idx = _block_cells(n, d["start"], d["n"], cell)
            for key in got:
                got[key][idx] = d[key]
        u, s = _oracle_fields(single, n, cell, degree, steps, scenario)
        eu, es, bound = rel_err(got["u"], u), rel_err(got["s"], s), 10 * tol_of(degree, cell)
        print("ORACLE %s: rel_err u %.3e s %.3e, bound %.1e" % (name, eu, es, bound))
        assert rel_err(u, single["u0"]) > 1e-4, "three steps must move the velocity"
        assert eu < bound and es < bound, (name, eu, es, bound)


def test_config3_golden_through_the_native_exchange_on_eight_ranks(gpu, fake, tmp_path):
    """Config 4's partition at production block widths, oracle-backed, through the exchange INSIDE the library: BASELINE
    config 3's input (64^3 cubes x 6 tets, P4, the eigenmode) on the 2 x 2 x 2 grid of eight 32^3 blocks - eight ranks (two
    per worker process), each with three neighbours, group-thick x shells, `T.n` ghost records on three sides - stepped by
    one sg_step per rank over the transport double, against the ORACLE's golden of the unsplit mesh (tests/golden/
    fullsize_c3.npz: sampled cells and slab sums of every field).  tests/test_multigpu_gpu.py checks the same partition
    with device copies between blocks of one process; this is the path the first 8-GPU job takes."""
    from tests import fullsize_cases as fc
    c = fc.C3
    N, world = c["n"], 8
    _spawn_workers(fake, tmp_path, world, [2, 2, 2, 2], (2, 2, 2), (N, N, N), c["P"], c["steps"], "f64", "c3golden")
    gold = np.load(os.path.join(ROOT, "tests", "golden", "fullsize_c3.npz"))
    ranks = [np.load(tmp_path / ("rank%d.npz" % r)) for r in range(world)]
    assert all(int(d["selftest"]) == 0 and int(d["nsides"]) == 3 for d in ranks)
    tol = dict(u=1e-10, s=1e-10, sh=1e-9, uh=1e-7)
    seen = np.zeros(len(gold["cells"]), dtype=int)
    for d in ranks:
        seen[d["g_which"]] += 1
    assert (seen == 1).all(), "every sampled cell of the golden lies in exactly one block"
    for name in ("u", "s", "uh", "sh"):
        want, want_layers = gold[name], gold[name + "_layers"]
        scale, lscale = np.abs(want).max(), np.abs(want_layers).max()
        if name == "uh":      # the UH buffer holds w = dt u1 + dt^3/24 utemp (csrc/stages.cpp; tests/test_fullsize_oracle_gpu.py _compare)
            dt, c3 = c["dt"], c["dt"] ** 3 / 24.0
            scale = lscale = (dt * tol["u"] * np.abs(gold["u"]).max() + c3 * tol["uh"] * np.abs(gold["uh"]).max()) / tol["uh"]
            want, want_layers = dt * gold["u"] + c3 * gold["uh"], dt * gold["u_layers"] + c3 * gold["uh_layers"]
        got = np.empty_like(want)
        layers = np.zeros_like(want_layers)
        for d in ranks:
            got[d["g_which"]] = d["g_" + name]
            z0, nz = int(d["start"][2]), int(d["n"][2])
            layers[z0:z0 + nz] += d["g_" + name + "_layers"].reshape(nz, -1)
        assert np.isfinite(got).all() and scale > 0
        err = np.abs(got - want).max() / scale
        lerr = np.abs(layers - want_layers).max() / max(lscale, scale)
        assert err < tol[name] and lerr < 30 * tol[name], (name, err, lerr)


def test_two_faces_between_one_pair_of_ranks_pair_by_facing_side(gpu, fake, tmp_path):
    """Two blocks around a wrapped z axis: each rank's z- and z+ sides both lead to the other rank.  RCCL pairs the two
    messages of such a pair in posting order; side s must get what the peer sent from its side s ^ 1 (comm.cpp posts the
    receives in the order of the facing sides) - the mirror image would arrive otherwise, silently."""
    _spawn_workers(fake, tmp_path, 2, [1, 1], (1, 1, 2), (16, 4, 4), 3, 2, "f64", "wrap")
    d = [np.load(tmp_path / ("rank%d.npz" % r)) for r in range(2)]
    for r in range(2):
        assert int(d[r]["selftest"]) == 0 and np.isfinite(d[r]["u"]).all()
        for kind in (0, 1):
            for s in (4, 5):
                got, want = d[r]["recv_%d_%d" % (kind, s)], d[1 - r]["send_%d_%d" % (kind, s ^ 1)]
                assert want.any() and np.array_equal(got, want), "rank %d side %d did not receive the peer's facing side" % (r, s)
            assert not np.array_equal(d[r]["recv_%d_4" % kind], d[r]["recv_%d_5" % kind])


# ---- the host-side agreement (seigen_amd/parallel.py::NativeExchanger) through the solver class ---------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.parametrize("fault,native", [
    (None, True),                 # no fault: every rank runs the exchange inside the library
    ("check", False),             # rank 1's peers do not match its neighbour mask: refused locally (sg_comm_check)
    ("init", False),              # rank 2's ncclCommInitRank fails alone
    ("selftest", False),          # rank 3 receives corrupted traces: its self-test counts mismatches
])
def test_ranks_agree_on_the_exchanger(gpu, fake, tmp_path, fault, native):
    world, grid, n, degree = 4, (1, 2, 2), (16, 4, 4), 4
    extra = {"SEIGEN_DIST_BACKEND": "gloo", "SEIGEN_HIP_DEVICE": "0", "SEIGEN_HALO_NATIVE": "force", "SEIGEN_TEST_HANG_DUMP": "200",
             "FAKE_RCCL_TIMEOUT_S": "30"}
    if fault == "init":
        extra["FAKE_RCCL_FAIL_INIT"] = "2"
    if fault == "selftest":
        extra["FAKE_RCCL_CORRUPT_RECV"] = "3"
    if fault == "check":
        extra["SEIGEN_TEST_BAD_PEERS_RANK"] = "1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "dist_worker.py"), str(tmp_path),
           str(degree), "3", ",".join(map(str, n)), ",".join(map(str, grid)), "source"]
    r = subprocess.run(cmd, cwd=ROOT, env=_env(fake, tmp_path, **extra), capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    from dist_worker import run_case
    _, us, ss = run_case(n, degree, 3, None, True)
    for rank in range(world):
        d = np.load(tmp_path / ("rank%d.npz" % rank))
        # every rank ended up on the SAME exchanger: the native one, or - after a failure on one rank - the host-driven one
        assert int(d["native"]) == int(native), "rank %d: native = %d" % (rank, int(d["native"]))
        assert int(d["staged"]) == (0 if native else 1) and int(d["bytes_sent"]) > 0
        idx = _block_cells(n, d["start"], d["n"])
        assert np.array_equal(d["u"], us[idx]) and np.array_equal(d["s"], ss[idx]), "rank %d differs from the single block" % rank
        if native:
            assert os.path.basename(str(d["library"])) == "libfake_rccl.so"


def _solver_class_ranks(fake, tmp_path, world, degree, steps, n, grid, *more):
    """tests/dist_worker.py on `world` ranks under torch.distributed.run: a gloo group, the exchange forced into the library
    and carried by the double, as in the no-fault case above; returns the ranks' files after the checks every case shares"""
    extra = {"SEIGEN_DIST_BACKEND": "gloo", "SEIGEN_HIP_DEVICE": "0", "SEIGEN_HALO_NATIVE": "force", "SEIGEN_TEST_HANG_DUMP": "200",
             "FAKE_RCCL_TIMEOUT_S": "30"}
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "dist_worker.py"), str(tmp_path),
           str(degree), str(steps), ",".join(map(str, n)), ",".join(map(str, grid))] + list(more)
    env = _env(fake, tmp_path, **extra)
    for var in ("SEIGEN_HIP_PATH", "SEIGEN_HIP_SYM", "SEIGEN_HALO_SCHEDULE"):
        env.pop(var, None)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    ranks = [np.load(tmp_path / ("rank%d.npz" % rank)) for rank in range(world)]
    for rank, d in enumerate(ranks):
        assert int(d["native"]) == 1 and int(d["staged"]) == 0 and int(d["bytes_sent"]) > 0, "rank %d is not on the native exchange" % rank
        assert os.path.basename(str(d["library"])) == "libfake_rccl.so"
    return ranks


@pytest.mark.parametrize("world,grid,n,degree,quad", [
    (2, (2, 1), (40, 6), 4, False),      # triangles P4: an x cut, blocks of a whole layout group and a ragged one per row
    (4, (2, 2), (40, 6), 4, False),      # ... and the 2 x 2 grid: blocks that meet at a corner
    (4, (2, 2), (18, 6), 2, True),       # quadrilaterals DQ_2, blocks narrower than a group
], ids=["tri-P4-2x1", "tri-P4-2x2", "quad-DQ2-2x2"])
def test_solver_class_2d_source_and_sponge_through_the_native_exchange(gpu, fake, tmp_path, monkeypatch, world, grid, n, degree, quad):
    """The 2-D explosive source (box-Ricker stress source, DG4 sponge, both across the cuts) through ElasticLF4 on 2 and 4
    ranks with the exchange inside the library: seigen_amd/parallel.py::NativeExchanger hands comm.cpp four sides, not six.
    Every rank is on the native exchange over the double, and its fields equal the single rank's bit for bit."""
    for var in ("SEIGEN_HIP_PATH", "SEIGEN_HIP_SYM"):
        monkeypatch.delenv(var, raising=False)
    steps = 3
    ranks = _solver_class_ranks(fake, tmp_path, world, degree, steps, n, grid, "source", "quadrilateral" if quad else "triangle")
    from dist_worker import run_case
    _, us, ss = run_case(n, degree, steps, None, True, quad)
    assert np.isfinite(us).all() and np.abs(us).max() > 0
    cell = _Q if quad else "left"
    for rank, d in enumerate(ranks):
        idx = _block_cells(n, d["start"], d["n"], cell)
        assert np.array_equal(d["u"], us[idx]) and np.array_equal(d["s"], ss[idx]), "rank %d differs from the single block" % rank


def test_solver_class_2d_eigenmode_of_the_reference_on_four_ranks(gpu, fake, tmp_path, monkeypatch):
    """The one multi-rank protocol the reference publishes (tests/eigenmode/eigenmode_2d.py: the unit square, P2, N = 8, dt =
    0.5 (1/N) / 2^(P-1), run(T = 5) - 160 steps), on four ranks (2, 2) through seigen_amd.harness.Eigenmode2DLF4 with the
    exchange inside the library: each rank starts from the analytic fields at its own block's nodes.  The assembled fields
    equal the single rank's bit for bit, and the single rank's error functional is the oracle's committed one
    (tests/golden/eigenmode_errors.json, to 1e-9 as in tests/test_sweeps_gpu.py)."""
    for var in ("SEIGEN_HIP_PATH", "SEIGEN_HIP_SYM"):
        monkeypatch.delenv(var, raising=False)
    N, P, T, world, grid = 8, 2, 5.0, 4, (2, 2)
    ranks = _solver_class_ranks(fake, tmp_path, world, P, int(T), (N, N), grid, "eigenmode")
    from dist_worker import run_eigenmode
    em, el, us, ss, (u1, s1) = run_eigenmode(N, P, T, None)
    assert el.block.counters()["steps"] == 160 and el.dt == 0.5 * (1.0 / N) / 2.0 ** (P - 1)
    gold = [r for r in json.load(open(os.path.join(ROOT, "tests", "golden", "eigenmode_errors.json")))["2d"] if (r["P"], r["N"]) == (P, N)]
    assert len(gold) == 1 and gold[0]["dt"] == el.dt
    u_error, s_error = em.eigenmode_error(u1, s1)
    print("eigenmode P%d N%d: u_error %r (golden %r), s_error %r (golden %r)" % (P, N, u_error, gold[0]["u_error"], s_error, gold[0]["s_error"]))
    assert abs(u_error - gold[0]["u_error"]) < 1e-9 and abs(s_error - gold[0]["s_error"]) < 1e-9
    got_u, got_s = np.full_like(us, np.nan), np.full_like(ss, np.nan)
    for rank, d in enumerate(ranks):
        assert int(d["steps"]) == 160
        idx = _block_cells((N, N), d["start"], d["n"])
        got_u[idx], got_s[idx] = d["u"], d["s"]
    assert np.array_equal(got_u, us) and np.array_equal(got_s, ss), "the four ranks' fields differ from the single rank's"


@pytest.mark.parametrize("args,cells,scaling", [
    (["--gpus", "4", "--steps", "3", "--warmup", "1", "--cubes", "16"], 4 * 6 * 16 ** 3, "weak"),
    (["--gpus", "4", "--workload", "c4", "--c4-cubes", "32", "--steps", "3", "--warmup", "1"], 6 * 32 ** 3, "strong"),
])
def test_bench_reports_the_native_exchange(gpu, fake, tmp_path, args, cells, scaling):
    """bench.py as the driver launches it for N > 1, with the exchange INSIDE the library (the default of every RCCL run)
    carried by the transport double in its async mode: the line's halo block - driver, transport, which RCCL, payload per
    step against the closed form, waits, the grid sweep of the weak-scaling workload - has only ever been filled by the
    host-driven exchanger before (tests/test_dist_gpu.py); the first 8-GPU job goes through exactly this code."""
    extra = {"SEIGEN_DIST_BACKEND": "gloo", "SEIGEN_HIP_DEVICE": "0", "SEIGEN_HALO_NATIVE": "force", "FAKE_RCCL_ASYNC": "1",
             "FAKE_RCCL_SLOT_BYTES": "1048576", "FAKE_RCCL_TIMEOUT_S": "60"}
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "4", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py")] + args
    r = subprocess.run(cmd, cwd=ROOT, env=_env(fake, tmp_path, **extra), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "rank 0 prints exactly one JSON line"
    out = json.loads(lines[0])
    assert out["n_gpus"] == 4 and out["scaling"] == scaling and out["value"] > 0 and out["config"]["cells"] == cells
    h = out["halo"]
    assert h["driver"] == "native" and h["transport"] == "nccl"
    assert os.path.basename(h["rccl_library"]) == "libfake_rccl.so" and h["rccl_version"] // 10000 == 2
    steps = out["steps"]
    assert h["exchanges_per_step"] == (6 * steps + 1) / steps          # + the exchange of the first stage's input per sg_step call
    for key in ("pack_ms_per_step", "bytes_sent_per_step", "exposed_wait_ms_per_step", "kernel_ms_per_step"):
        assert len(h[key]) == 4 and all(v >= 0 for v in h[key]), (key, h[key])
    assert all(v > 0 for v in h["bytes_sent_per_step"]) and all(v == 0 for v in h["host_blocked_ms_per_step"])
    if scaling == "weak":
        # 1 x 2 x 2 grid of 16^3 blocks, P4: two sides of 16 * 16 * 2 facets * 15 nodes * 3 components each
        face = 16 * 16 * 2 * 15 * 3 * 8
        assert out["config"]["block_grid"] == [1, 2, 2]
        assert all(v == 2 * face * (6 * steps + 1) / steps for v in h["bytes_sent_per_step"]), h["bytes_sent_per_step"]
        sw = h["grid_blocks_sweep_ms_per_step"]
        assert sorted(sw) == ["448", "480", "496", "512"] and all(v > 0 for v in sw.values())
    assert len(out["rank_ms_per_step"]["per_rank"]) == 4
