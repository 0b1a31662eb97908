"""Every instantiation of the 2-D tile family (kernels_tile2d.hip, sg::tile2d_stage) against the FP64 oracle.

TILE2D_KERNELS lists what launch_stage_tile2d can dispatch; test_host_logic.py holds it equal to the kernel objects the
built library exports, so a new template argument cannot join the family without a row here.  Each row of ROWS - (dtype,
degree, cell, symmetric stress, block, SEIGEN_HIP_TILE_GRID, further switches) - first pins the six stage kernels it runs by
the names the library reports, then checks one application of F and G against ElasticOperators and three whole LF4 steps
with every extra at once against OracleLF4: per-cell material, a density (scalar, per cell, per cell physical in turn), a
nodal source with a node listed twice and nodes in the last, partly filled group, and a DG4 sponge with cells of all three
kinds the kernel distinguishes (none, one value per cell, varying) side by side in every 16-cell item; full-tensor rows
start from a non-symmetric stress and add non-symmetric source values.  The blocks are the ones where the item arithmetic
changes: one square, one group per row, groups that straddle rows, rows narrower than a group, nine ragged groups per
row, and (37, 23) on a grid of 8 blocks - 108 items (54 of quadrilaterals) on 32 waves, so a wave works several items and
the last XCD range is short.  SPLITS run every (dtype, degree, triangle / quadrilateral, symmetry) as blocks with neighbours
(GHOST = 1) against the single block, bitwise, and the single block against the oracle.
test_rows_name_every_stage_kernel checks that rows and splits together reach every instantiation.

Tolerances are the suite's own: FP64 tol_of() per application and 10 tol_of() for the steps (test_parity_gpu.py,
test_tile2d_gpu.py), FP32 2e-5 and 5e-5 (test_fp32_gpu.py).  Every figure is printed before it is asserted (pytest -s)."""
import numpy as np
import pytest

from oracle.lf4 import OracleLF4
from tests.test_parity_gpu import tol_of
from tests.util import oracle_mesh, rel_err

pytestmark = pytest.mark.gpu

_TYPES = {"f64": "double", "f32": "float"}
CELLS = ("left", "right", "quadrilateral")


def _name(dtype, P, kind, mode, sym, ghost, cell):
    return "sg::tile2d_stage<%d, %d, %d, %d, %d, %d, %s>" % (P, kind, mode, int(sym), ghost, int(cell == "quadrilateral"),
                                                             _TYPES[dtype])


# tile2d_stage<P, KIND, MODE, SYM, GHOST, TP, R> as launch_stage_tile2d / launch_t2p / launch_t2r / launch_t2 dispatch them:
# P the degree 1..4; KIND 0 = F in three modes (0: UH1 / apply_F, 1: U1, 2: UTEMP), KIND 1 = G in two (0: STEMP, SH1 /
# apply_G, 1: S1); SYM 1 = symmetric-stress storage; GHOST 1 = a block with neighbours (packed remote traces); TP 1 =
# quadrilaterals (DQ_P), 0 = triangles of either diagonal; R the number type.
_KIND_MODES = ((0, 0), (0, 1), (0, 2), (1, 0), (1, 1))
TILE2D_KERNELS = frozenset(
    _name(t, P, kind, mode, sym, ghost, cell) for t in _TYPES for P in (1, 2, 3, 4) for kind, mode in _KIND_MODES
    for sym in (0, 1) for ghost in (0, 1) for cell in ("left", "quadrilateral"))

# dtype, degree, cell, symmetric stress, block, SEIGEN_HIP_TILE_GRID (None: the library's own grid), further switches.
# Every (dtype, triangle / quadrilateral) meets every block shape at some degree, and every (degree, symmetry) once:
#   (1, 1)   one square, 15 padding lanes            (16, k)  exactly one group per row
#   (17, 3)  groups straddle rows, the last holds 3   (1, 40), (3, 11)  rows narrower than a group (gpr, the g0 = 0 clamp,
#   (129, 3) nine groups per row, ragged                       y neighbours inside the own group)
#   (37, 23) with a grid of 8 blocks: 108 / 54 items on 32 waves, XCD label 7 gets items 98-107 only; the switch sets the
#            grid of the F stages with a sponge too, so every stage loops
_Q = "quadrilateral"
ROWS = [
    ("f64", 1, "left", True, (1, 1), None, {}),
    ("f64", 1, "right", False, (16, 2), None, {}),
    ("f64", 2, "left", True, (17, 3), None, {}),
    ("f64", 2, "right", False, (1, 40), None, {}),
    ("f64", 3, "left", True, (3, 11), None, {}),
    ("f64", 3, "right", False, (129, 3), None, {}),
    ("f64", 4, "left", True, (37, 23), 8, {}),
    ("f64", 4, "right", False, (16, 3), None, {}),
    ("f64", 1, _Q, True, (1, 40), None, {}),
    ("f64", 1, _Q, False, (3, 11), None, {}),
    ("f64", 2, _Q, True, (129, 3), None, {}),
    ("f64", 2, _Q, False, (37, 23), 8, {}),
    ("f64", 3, _Q, True, (16, 3), None, {}),
    ("f64", 3, _Q, False, (1, 1), None, {}),
    ("f64", 4, _Q, True, (16, 2), None, {}),
    ("f64", 4, _Q, False, (17, 3), None, {}),
    ("f32", 1, "right", True, (129, 3), None, {}),
    ("f32", 1, "left", False, (37, 23), 8, {}),
    ("f32", 2, "right", True, (16, 3), None, {}),
    ("f32", 2, "left", False, (1, 1), None, {}),
    ("f32", 3, "right", True, (16, 2), None, {}),
    ("f32", 3, "left", False, (17, 3), None, {}),
    ("f32", 4, "right", True, (1, 40), None, {}),
    ("f32", 4, "left", False, (3, 11), None, {}),
    ("f32", 1, _Q, True, (37, 23), 8, {}),
    ("f32", 1, _Q, False, (16, 3), None, {}),
    ("f32", 2, _Q, True, (1, 1), None, {}),
    ("f32", 2, _Q, False, (16, 2), None, {}),
    ("f32", 3, _Q, True, (17, 3), None, {}),
    ("f32", 3, _Q, False, (1, 40), None, {}),
    ("f32", 4, _Q, True, (3, 11), None, {}),
    ("f32", 4, _Q, False, (129, 3), None, {}),
    # the two source paths of the G kernels: the step the host names (no graph replay; the rows above replay a graph and read
    # the device-side step counter), and the source as a launch of its own after every G stage
    ("f64", 3, "right", False, (37, 23), 8, {"SEIGEN_HIP_GRAPH": "0"}),
    ("f32", 2, _Q, True, (17, 3), None, {"SEIGEN_HIP_SOURCE_LAUNCH": "1"}),
    ("f32", 3, "left", True, (37, 23), 8, {"SEIGEN_HIP_GRAPH": "0"}),
    ("f64", 2, "left", False, (17, 3), None, {"SEIGEN_HIP_SOURCE_LAUNCH": "1"}),
]

# GHOST = 1, one split per (dtype, degree, triangle / quadrilateral, symmetry): dtype, degree, cell, symmetric stress, mesh,
# block grid, schedules (True: pipelined - regions FIRST / SECOND; False: un-pipelined - INTERIOR / BOUNDARY, the
# BOUNDARY launch deals its items with StageArgs::spread = 1), SEIGEN_HIP_TILE_GRID.  72 and 80 squares wide in two
# blocks: 36 and 40 per block, wider than two groups and no multiple of 16.  Grid 8 on (72, 24) and (80, 40): blocks of 108
# (triangles) and 100 (quadrilaterals) items, whose FIRST / SECOND lists are longer than the grid's 32 waves.
SPLITS = [
    ("f64", 1, "left", True, (72, 5), (2, 1), (True, False), None),
    ("f64", 1, "right", False, (6, 7), (1, 2), (True,), None),
    ("f64", 2, "left", True, (72, 24), (2, 1), (True,), 8),
    ("f64", 2, "right", False, (34, 4), (2, 1), (False,), None),
    ("f64", 3, "left", True, (5, 8), (1, 2), (False,), None),
    ("f64", 3, "right", False, (9, 6), (2, 2), (True,), None),
    ("f64", 4, "left", True, (7, 4), (2, 2), (True,), None),
    ("f64", 4, "right", False, (5, 6), (1, 2), (True,), None),
    ("f64", 1, _Q, True, (9, 6), (2, 2), (True,), None),
    ("f64", 1, _Q, False, (80, 40), (2, 1), (True,), 8),
    ("f64", 2, _Q, True, (80, 3), (2, 1), (True, False), None),
    ("f64", 2, _Q, False, (5, 6), (1, 2), (False,), None),
    ("f64", 3, _Q, True, (6, 7), (1, 2), (True,), None),
    ("f64", 3, _Q, False, (34, 4), (2, 1), (True,), None),
    ("f64", 4, _Q, True, (5, 8), (1, 2), (True,), None),
    ("f64", 4, _Q, False, (7, 4), (2, 2), (False,), None),
    ("f32", 1, "right", True, (9, 6), (2, 2), (True,), None),
    ("f32", 1, "left", False, (80, 5), (2, 1), (True, False), None),
    ("f32", 2, "right", True, (5, 6), (1, 2), (False,), None),
    ("f32", 2, "left", False, (72, 24), (2, 1), (True,), 8),
    ("f32", 3, "right", True, (34, 4), (2, 1), (True,), None),
    ("f32", 3, "left", False, (6, 7), (1, 2), (True,), None),
    ("f32", 4, "right", True, (7, 4), (2, 2), (False,), None),
    ("f32", 4, "left", False, (5, 8), (1, 2), (True,), None),
    ("f32", 1, _Q, True, (80, 40), (2, 1), (True,), 8),
    ("f32", 1, _Q, False, (5, 8), (1, 2), (False,), None),
    ("f32", 2, _Q, True, (7, 4), (2, 2), (True,), None),
    ("f32", 2, _Q, False, (72, 5), (2, 1), (True, False), None),
    ("f32", 3, _Q, True, (5, 6), (1, 2), (True,), None),
    ("f32", 3, _Q, False, (9, 6), (2, 2), (True,), None),
    ("f32", 4, _Q, True, (34, 4), (2, 1), (False,), None),
    ("f32", 4, _Q, False, (6, 7), (1, 2), (True,), None),
]

SHAPES = {(1, 1), (16, 2), (16, 3), (17, 3), (1, 40), (3, 11), (129, 3), (37, 23)}
_SWITCHES = ("SEIGEN_HIP_SYM", "SEIGEN_HIP_SOURCE_LAUNCH", "SEIGEN_HIP_TILE_GRID", "SEIGEN_HIP_GRAPH")


def _stage_names(dtype, P, cell, sym, ghost=0):
    """the instantiation each of the six stages launches (hostlogic.hpp lf4_stage)"""
    f = lambda mode: _name(dtype, P, 0, mode, sym, ghost, cell)
    g = lambda mode: _name(dtype, P, 1, mode, sym, ghost, cell)
    return [f(0), g(0), f(1), g(0), f(2), g(1)]


def _row_id(r):
    dtype, P, cell, sym, n, tile_grid, switches = r
    return "%s-P%d-%s-%s-%s%s%s" % (dtype, P, cell, "sym" if sym else "full", "x".join(map(str, n)),
                                    "" if tile_grid is None else "-grid%d" % tile_grid,
                                    "".join("-%s=%s" % (k[len("SEIGEN_HIP_"):].lower(), v) for k, v in sorted(switches.items())))


def _split_id(s):
    dtype, P, cell, sym, n, grid, schedules, tile_grid = s
    return "%s-on-%s-%s" % (_row_id((dtype, P, cell, sym, n, tile_grid, {})), "x".join(map(str, grid)),
                            "+".join("pipelined" if p else "unpipelined" for p in schedules))


def _environment(monkeypatch, tile_grid=None, switches=None):
    """a row's switches, and nothing else that picks an instantiation, a grid or a source path"""
    for var in _SWITCHES:
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("SEIGEN_HIP_PATH", "tile")
    if tile_grid is not None:
        monkeypatch.setenv("SEIGEN_HIP_TILE_GRID", str(tile_grid))
    for var, val in (switches or {}).items():
        monkeypatch.setenv(var, val)


def _block(dtype, P, cell, n, L):
    from seigen_amd.backend import HipBlock
    return HipBlock(2, P, n, [L[a] / n[a] for a in range(2)], [0.0, 0.0], cell, dtype=dtype)


def _stress(shape, rng, sym):
    s = rng.uniform(-1, 1, shape)
    return 0.5 * (s + np.swapaxes(s, -1, -2)) if sym else s


def _sponge(m, ncls, rng):
    """DG4 nodal sigma on 2-D cells (ncls cells per square, cell = ncls square + class; an item is the 16 cells of one class
    of 16 consecutive squares): cells without a sponge, with one value on all nodes (sigma u at the node, no matrix) and
    with a varying sigma (a matrix of their own) in turn within every item, and consecutive varying cells of a class in
    pairs with the same sigma (one matrix, two cells of an item)"""
    nq = m.node_coords(4).shape[1]
    cell = np.arange(m.ncells)
    kind = (cell // ncls + cell % ncls) % 3
    sigma = np.zeros((m.ncells, nq))
    c, v = kind == 1, np.flatnonzero(kind == 2)
    sigma[c] = rng.uniform(2.0, 30.0, size=(c.sum(), 1))
    sigma[v] = rng.uniform(0.0, 30.0, size=(len(v), nq))
    for k in range(ncls):
        vk = v[v % ncls == k]
        twin = vk[1::2]
        sigma[twin] = sigma[vk[0::2][:len(twin)]]
    return sigma


def _source_nodes(nc, nd, rng):
    """scattered nodes, nodes of the last cells (the last, partly filled group), one node twice"""
    nodes = rng.integers(0, nc * nd, size=10)
    last = np.array([nc - 1, max(nc - 2, 0)]) * nd + rng.integers(0, nd, size=2)
    nodes = np.concatenate([nodes, last, nodes[:1]])
    assert len(np.unique(nodes)) < len(nodes)
    return nodes


def _oracle_source(nc, nd, dim, nodes, vals):
    S = np.zeros((nc * nd, dim, dim))
    np.add.at(S, nodes, vals)
    return S.reshape(nc, nd, dim, dim)


def _tolerances(dtype, P, cell):
    return (tol_of(P, cell), 10 * tol_of(P, cell)) if dtype == "f64" else (2e-5, 5e-5)


def _err(what, family, dtype, got, want):
    """the figure, printed before anything is asserted on it"""
    e = rel_err(got, want)
    print("ERR %s %s %s %.3e" % (family, dtype, what, e))
    return e


def check_block(family, make_block, m, hmin, P, cell, dtype, sym, names, density, sponge, seed, reports_sym=None):
    """One application of F and G, then three steps with every extra, against the oracle on mesh m (also the rows of
    tests/test_hex_family_gpu.py and tests/test_lane_generic_family_gpu.py).  make_block() builds the block under test;
    hmin: its smallest cell width; names: the six kernels it must report; sponge: None for a run without one; reports_sym:
    what is_sym() must say where that is not `sym` (the generic kernels have no symmetric-stress storage)."""
    from seigen_amd import _lib
    dim = m.dim
    tol1, tol3 = _tolerances(dtype, P, cell)
    rng = np.random.default_rng(seed)
    orc = OracleLF4(m, P)
    nc = m.ncells
    lam, mu = rng.uniform(0.4, 0.8, nc), rng.uniform(0.2, 0.4, nc)
    reports_sym = sym if reports_sym is None else reports_sym

    # the instantiations, before anything runs
    blk = make_block()
    nd = blk.nd
    T = _stress(blk.field_shape(_lib.FIELD_S), rng, sym)
    u = rng.uniform(-1, 1, blk.field_shape(_lib.FIELD_U))
    blk.set_params(1.0, 0.01, lam, mu)
    blk.set_field(_lib.FIELD_S, T)
    blk.set_field(_lib.FIELD_U, u)
    assert blk.is_sym() == reports_sym
    assert [blk.stage_kernel_name(st) for st in range(6)] == names

    # one application of each operator (the MODE 0 kernels)
    blk.apply_F(_lib.FIELD_S, _lib.FIELD_U, _lib.FIELD_UH)
    assert _err("application", family, dtype, blk.get_field(_lib.FIELD_UH), orc.E.apply_F(T, u)) < tol1
    blk.apply_G(_lib.FIELD_U, _lib.FIELD_SH)
    assert _err("application", family, dtype, blk.get_field(_lib.FIELD_SH), orc.E.apply_G(u, lam, mu)) < tol1
    blk.close()

    # three whole steps
    blk = make_block()
    orc.dt, orc.l, orc.mu = 0.04 * hmin / P ** 2, lam, mu
    orc.u0 = rng.uniform(-1, 1, blk.field_shape(_lib.FIELD_U))
    orc.s0 = _stress(blk.field_shape(_lib.FIELD_S), rng, sym)
    u_start = orc.u0
    if density == "scalar":                 # the explicit reference's u1 = rho u0 + ...
        orc.density = 1.1
        blk.set_params(orc.density, orc.dt, lam, mu)
    else:
        orc.density = rng.uniform(0.9, 1.1, nc) if density == "cell" else rng.uniform(0.8, 1.5, nc)
        orc.density_physical = density == "physical"
        blk.set_params(1.0, orc.dt, lam, mu)
        blk.set_density(orc.density, physical=orc.density_physical)
    if sponge is not None:
        sigma = sponge(m, rng)
        orc.E.set_absorption(sigma, 4)
        blk.set_absorption(sigma, 4)
    nodes = _source_nodes(nc, nd, rng)
    vals = _stress((3, len(nodes), dim, dim), rng, sym)
    blk.set_source(nodes, vals)
    blk.set_field(_lib.FIELD_U, orc.u0)
    blk.set_field(_lib.FIELD_S, orc.s0)
    assert blk.is_sym() == reports_sym
    assert [blk.stage_kernel_name(st) for st in range(6)] == names
    blk.step(3)
    for k in range(3):
        orc.source = lambda t, k=k: _oracle_source(nc, nd, dim, nodes, vals[k])
        orc.step((k + 1) * orc.dt)
    errs = [_err("steps", family, dtype, blk.get_field(_lib.FIELD_U), orc.u1),
            _err("steps", family, dtype, blk.get_field(_lib.FIELD_S), orc.s1),
            # what the last step left behind: w = dt u1 + dt^3/24 utemp (UTEMP, MODE 2) and sh1 = G(u1) + S (SH1)
            _err("steps", family, dtype, blk.get_field(_lib.FIELD_UH), orc.dt * orc.u1 + orc.dt ** 3 / 24.0 * orc.last["utemp"]),
            _err("steps", family, dtype, blk.get_field(_lib.FIELD_SH), orc.last["sh1"])]
    blk.close()
    assert max(errs) < tol3, errs
    assert rel_err(orc.u1, u_start) > 1e-4


def _size(n):
    return (0.4 * n[0], 0.3 * n[1])


@pytest.mark.parametrize("row", ROWS, ids=_row_id)
def test_row_against_the_oracle(gpu, monkeypatch, row):
    dtype, P, cell, sym, n, tile_grid, switches = row
    _environment(monkeypatch, tile_grid, switches)
    L = _size(n)
    ncls = 1 if cell == _Q else 2
    check_block("tile2d", lambda: _block(dtype, P, cell, n, L), oracle_mesh(2, n, L, cell), 0.3, P, cell, dtype, sym,
                _stage_names(dtype, P, cell, sym), ("scalar", "cell", "physical")[ROWS.index(row) % 3],
                lambda m, rng: _sponge(m, ncls, rng), 1000 * P + 10 * n[0] + n[1] + (0 if dtype == "f64" else 7))


@pytest.mark.parametrize("split", SPLITS, ids=_split_id)
def test_split_row_is_bitwise_the_single_block(gpu, monkeypatch, split):
    """GHOST = 1: blocks with neighbours through the host-driven exchange (test_harness_gpu._LocalExchange), bitwise equal
    to the single block under every schedule listed, and the single block against the oracle"""
    from tests.test_harness_gpu import _multiblock_case
    dtype, P, cell, sym, n, grid, schedules, tile_grid = split
    _environment(monkeypatch, tile_grid)
    for pipelined in schedules:
        res = _multiblock_case(2, P, n, grid, pipelined, extras=True, dtype=dtype, diagonal=cell, sym=sym)
        assert res["names"] == sorted(set(_stage_names(dtype, P, cell, sym, ghost=1))), res["names"]
    m = oracle_mesh(2, n, (1.0, 1.0), cell)
    orc = OracleLF4(m, P)
    nc, nd = m.ncells, orc.E.nd
    orc.dt, orc.l, orc.mu, orc.density = res["dt"], 0.5, 0.25, 1.0
    orc.E.set_absorption(res["sigma"], 4)
    orc.u0, orc.s0 = res["u0"].copy(), res["s0"].copy()
    for k in range(3):
        orc.source = lambda t, k=k: _oracle_source(nc, nd, 2, res["src_nodes"], res["src_steps"][k])
        orc.step((k + 1) * orc.dt)
    tol3 = _tolerances(dtype, P, cell)[1]
    errs = [_err("steps", "tile2d", dtype, res["u"], orc.u1), _err("steps", "tile2d", dtype, res["s"], orc.s1)]
    assert max(errs) < tol3, errs


def test_the_lists_cover_what_they_claim():
    """every (dtype, degree, triangle / quadrilateral, symmetry) has a row and exactly one split; every (dtype, triangle /
    quadrilateral) meets every block shape, the looping grid and both schedules; both diagonals in both number types"""
    kinds = {(t, P, tp, sym) for t in _TYPES for P in (1, 2, 3, 4) for tp in (False, True) for sym in (False, True)}
    assert {(r[0], r[1], r[2] == _Q, r[3]) for r in ROWS} == kinds
    assert sorted((s[0], s[1], s[2] == _Q, s[3]) for s in SPLITS) == sorted(kinds)
    for t in _TYPES:
        assert {r[2] for r in ROWS if r[0] == t} == set(CELLS)
        for tp in (False, True):
            mine = [r for r in ROWS if r[0] == t and (r[2] == _Q) == tp]
            assert {r[4] for r in mine} == SHAPES
            assert any(r[4] == (37, 23) and r[5] == 8 for r in mine)
            assert any(set(s[6]) == {True, False} for s in SPLITS if s[0] == t and (s[2] == _Q) == tp)
        assert any(s[5] == (2, 1) and s[4][0] // 2 > 32 and (s[4][0] // 2) % 16 for s in SPLITS if s[0] == t)
    assert {s[5] for s in SPLITS} == {(2, 1), (1, 2), (2, 2)}
    assert sum(s[7] == 8 for s in SPLITS) >= 2
    assert any(r[6].get("SEIGEN_HIP_GRAPH") == "0" for r in ROWS) and any(r[6].get("SEIGEN_HIP_SOURCE_LAUNCH") == "1" for r in ROWS)


def test_rows_name_every_stage_kernel(gpu, monkeypatch):
    """ROWS and SPLITS together launch every tile2d_stage instantiation and nothing else.  Each row's block (the blocks of
    the grid with zero halo buffers attached for a split) is set up as its test sets it up and asked for its six kernels."""
    torch = pytest.importorskip("torch")
    from seigen_amd.backend import HipBlock
    from seigen_amd.mesh import Partition
    seen = set()
    for dtype, P, cell, sym, n, tile_grid, switches in ROWS:
        _environment(monkeypatch, tile_grid, switches)
        blk = _block(dtype, P, cell, n, _size(n))
        blk.set_params(1.0, 0.01, 0.5, 0.25)
        if not sym:
            blk.leave_sym()
        names = [blk.stage_kernel_name(st) for st in range(6)]
        assert names == _stage_names(dtype, P, cell, sym), names
        seen.update(names)
        blk.close()
    for dtype, P, cell, sym, n, grid, schedules, tile_grid in SPLITS:
        _environment(monkeypatch, tile_grid)
        world = grid[0] * grid[1]
        bufs = []
        for p in (Partition(n, r, world, grid) for r in range(world)):
            b = HipBlock(2, P, p.n, [1.0 / k for k in n], [p.start[a] / n[a] for a in range(2)], cell, p.nbr_mask,
                         dtype=dtype)
            b.set_params(1.0, 0.01, 0.5, 0.25)
            if not sym:
                b.leave_sym()
            for field in range(4):
                for s in range(4):
                    if p.neighbour(s) is not None:
                        bufs.append(torch.zeros(b.halo_bytes(field, s), dtype=torch.uint8, device="cuda"))
                        b.halo_attach(field, s, bufs[-1].data_ptr())
            names = [b.stage_kernel_name(st) for st in range(6)]
            assert names == _stage_names(dtype, P, cell, sym, ghost=1), names
            seen.update(names)
            b.close()
    assert len(TILE2D_KERNELS) == 320
    assert TILE2D_KERNELS <= seen, sorted(TILE2D_KERNELS - seen)
    assert seen <= TILE2D_KERNELS, sorted(seen - TILE2D_KERNELS)
