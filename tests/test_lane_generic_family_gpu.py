"""Every instantiation of the lane-per-cell family (kernels_lane.hip, sg::lane_stage - the default of large 1-D blocks,
elsewhere through SEIGEN_HIP_PATH=lane) and of the generic family (kernels.hip, sg::stage_kernel - the default of small
1-D blocks, of small 3-D P1 and DQ_1 / DQ_2 blocks, and the second reference of many GPU tests, through
SEIGEN_HIP_PATH=generic) against the FP64 oracle.

LANE_KERNELS and GENERIC_KERNELS list what launch_stage_lane / launch_lane_d / launch_lane_dp and launch_stage / launch_d /
launch_quad / launch_dp can dispatch; test_host_logic.py holds them equal to the kernel objects the built library exports.
Each row - (dimension, degree, cell, symmetric stress, block, further switches) - pins its six stage kernels by name, then
runs the checks of tests/test_tile2d_family_gpu.py (check_block): one application of F and G, and three whole LF4 steps
with per-cell material, a density (scalar, per cell, per cell physical in turn), a nodal source with a node listed twice and
nodes in the last cells, and a DG4 sponge with cells of four kinds (none, constant, general nodal, affine) side by side in
every item; full-tensor rows start from a non-symmetric stress and add non-symmetric source values.

Neither family has a MODE 2 object, a GHOST argument or a grid switch:
  * stage UTEMP runs the F MODE 1 lane object with c_self = 0; stage_kernel has neither MODE nor SYM, so its six stages name
    F, G, F, G, F, G, and a generic block never enters symmetric-stress mode: is_sym() is False whatever the stress
    (api.cpp: only the interleaved families set sg_handle::sym);
  * a 1-D stress is one number and cannot be non-symmetric, so the SYM = 0 lane objects of 1-D run under SEIGEN_HIP_SYM=0;
  * blocks with neighbours take a run-time branch of the same objects: SPLITS run every (family, dimension, degree, cell)
    as blocks against the single block, bitwise, symmetric and not, and one split per (family, dimension, cell) compares its
    single block with the oracle;
  * the persistent loops run a second time only on big blocks: LOOP_ROWS, degree 1, one per code shape.

What the blocks are for.  lane_stage works on items = (group of 64 consecutive cubes, class); the launch has at most 2048
workgroups of 4 waves, eight contiguous item ranges (one per XCD label), a wave stepping through its range by 4 blocks_here:
  (1..)      one cube, 63 padded lanes             (37 / 5x7 / 3x4x5)   fewer than 64 cubes
  64 cubes   exactly one group                     65 cubes             a second group of one cube
  n[0] = 7, 37 with more than 64 cubes: the y / z neighbour lies in another group at a lane offset that is not 0
  n[0] = 64, 128: the x neighbour of lane 63 is lane 0 of the next group
  19237 / 161x120 / 27x27x18: 301 / 302 / 206 groups, so every XCD range and several waves of it hold work
stage_kernel gives a 256-thread workgroup a batch of EB = min(32, 256 / nd) consecutive cells (GENERIC_EB) on a grid of at
most 2048 workgroups: one cube; a cell count that is no multiple of EB (the last batch partly filled); an exact multiple; a
block thin in x (n[0] <= 3), so the cubes of a batch straddle rows and layers.

LOOP_ROWS: generic blocks of more than 2048 EB = 65 536 cells (a second, ragged pass of the batch loop), lane blocks of more
than 8192 items (ipx > 4 blocks_here: a second pass in every XCD range, the last range short), and one DQ_1 block of the
hexahedral lane family's hex_stage, whose grid has the same cap and whose loop no other test visits.  They carry the sponge in
1-D and 2-D; in 3-D the oracle's DG4 sponge set-up (35 / 125 quadrature nodes per cell on some 70 000 to 530 000 cells) would
dominate the module, so the 3-D looping rows run without one.

Tolerances are the suite's own: tol_of() per application, 10 tol_of() for the steps (test_parity_gpu.py); splits bitwise.
Every figure is printed before it is asserted (pytest -s)."""
import numpy as np
import pytest

from oracle.lf4 import OracleLF4
from tests.test_parity_gpu import tol_of
from tests.test_tile2d_family_gpu import _err, _oracle_source, check_block
from tests.util import oracle_mesh

pytestmark = pytest.mark.gpu

_Q = "quadrilateral"
_S = "left"                      # simplices: intervals, triangles, tetrahedra
LANE_KINDS = [(1, P) for P in (1, 2, 3, 4)] + [(2, P) for P in (1, 2, 3, 4)] + [(3, 1), (3, 2)]      # (DIM, P) of lane_stage
# (DIM, P, cell) of stage_kernel: TP 0 simplices of every dimension, TP 1 quadrilaterals, TP 2 hexahedra
GENERIC_KINDS = [(d, P, _S) for d in (1, 2, 3) for P in (1, 2, 3, 4)] + [(d, P, _Q) for d in (2, 3) for P in (1, 2, 3, 4)]

# lane_stage<DIM, P, KIND, MODE, SYM>: KIND 0 = F, 1 = G; MODE 0 the plain application (UH1, STEMP, SH1, apply_F / apply_G),
# MODE 1 the fused combine (U1, UTEMP with c_self = 0, S1); SYM 1 = symmetric-stress storage
LANE_KERNELS = frozenset("sg::lane_stage<%d, %d, %d, %d, %d>" % (d, P, kind, mode, sym) for d, P in LANE_KINDS
                         for kind in (0, 1) for mode in (0, 1) for sym in (0, 1))
# stage_kernel<DIM, P, KIND, TP>
GENERIC_KERNELS = frozenset("sg::stage_kernel<%d, %d, %d, %d>" % (d, P, kind, (0 if cell == _S else d - 1))
                            for d, P, cell in GENERIC_KINDS for kind in (0, 1))

# cells per workgroup of stage_kernel, degrees 1..4 (kernels.hip Geo::EB = min(32, 256 / nd)), by (DIM, cell)
GENERIC_EB = {
    (1, _S): (32, 32, 32, 32),       # nd 2, 3, 4, 5
    (2, _S): (32, 32, 25, 17),       # nd 3, 6, 10, 15
    (3, _S): (32, 25, 12, 7),        # nd 4, 10, 20, 35
    (2, _Q): (32, 28, 16, 10),       # nd 4, 9, 16, 25
    (3, _Q): (32, 9, 4, 2),          # nd 8, 27, 64, 125
}

_AFFINE = {"SEIGEN_HIP_SPONGE_AFFINE": "1"}      # the lane kernels' affine cells through sponge_pre_affine_kernel<double, DIM>
_EAGER = {"SEIGEN_HIP_GRAPH": "0"}               # no graph replay: the host names the source's step

# dimension, degree, cell, symmetric stress, block, further switches
LANE_ROWS = [
    (1, 1, _S, True, (1,), {}),
    (1, 1, _S, False, (19237,), {}),
    (1, 2, _S, True, (65,), _AFFINE),
    (1, 2, _S, False, (64,), {}),
    (1, 3, _S, True, (128,), {}),
    (1, 3, _S, False, (37,), {}),
    (1, 4, _S, True, (19237,), _AFFINE),
    (1, 4, _S, False, (65,), {}),
    (2, 1, _S, True, (161, 120), {}),
    (2, 1, _S, False, (1, 1), {}),
    (2, 2, _S, True, (13, 5), {}),
    (2, 2, _S, False, (64, 3), {}),
    (2, 3, _S, True, (37, 5), {}),
    (2, 3, _S, False, (8, 8), {}),
    (2, 4, _S, True, (128, 2), {}),
    (2, 4, _S, False, (5, 7), {}),
    (2, 2, _S, False, (37, 5), _AFFINE),
    (2, 3, _S, True, (13, 5), _EAGER),
    (3, 1, _S, True, (27, 27, 18), {}),
    (3, 1, _S, False, (1, 1, 1), {}),
    (3, 1, _S, True, (4, 4, 4), {}),
    (3, 1, _S, False, (7, 5, 3), {}),
    (3, 2, _S, True, (13, 5, 1), {}),
    (3, 2, _S, False, (64, 2, 1), {}),
    (3, 2, _S, True, (3, 4, 5), {}),
    (3, 2, _S, False, (128, 1, 2), {}),
    (3, 2, _S, True, (7, 5, 3), _AFFINE),
]

GENERIC_ROWS = [
    (1, 1, _S, True, (1,), {}),
    (1, 1, _S, False, (64,), {}),
    (1, 2, _S, True, (45,), {}),
    (1, 2, _S, False, (1,), {}),
    (1, 3, _S, True, (64,), {}),
    (1, 3, _S, False, (45,), {}),
    (1, 4, _S, True, (33,), {}),
    (1, 4, _S, False, (96,), _EAGER),
    (2, 1, _S, True, (1, 1), {}),
    (2, 1, _S, False, (8, 4), {}),
    (2, 2, _S, True, (2, 9), {}),
    (2, 2, _S, False, (16, 3), {}),
    (2, 3, _S, True, (5, 5), {}),
    (2, 3, _S, False, (3, 7), {}),
    (2, 4, _S, True, (17, 2), {}),
    (2, 4, _S, False, (2, 5), {}),
    (3, 1, _S, True, (1, 1, 1), {}),
    (3, 1, _S, False, (4, 4, 2), {}),
    (3, 2, _S, True, (2, 3, 4), {}),
    (3, 2, _S, False, (5, 5, 1), {}),
    (3, 3, _S, True, (2, 2, 2), {}),
    (3, 3, _S, False, (1, 3, 3), {}),
    (3, 4, _S, True, (7, 1, 1), {}),
    (3, 4, _S, False, (2, 2, 1), {}),
    (2, 1, _Q, True, (1, 1), {}),
    (2, 1, _Q, False, (8, 8), {}),
    (2, 2, _Q, True, (2, 15), {}),
    (2, 2, _Q, False, (7, 8), {}),
    (2, 3, _Q, True, (8, 4), {}),
    (2, 3, _Q, False, (3, 11), {}),
    (2, 4, _Q, True, (5, 4), {}),
    (2, 4, _Q, False, (3, 7), {}),
    (3, 1, _Q, True, (1, 1, 1), {}),
    (3, 1, _Q, False, (4, 4, 4), {}),
    (3, 2, _Q, True, (2, 3, 5), {}),
    (3, 2, _Q, False, (3, 3, 3), {}),
    (3, 3, _Q, True, (2, 2, 4), {}),
    (3, 3, _Q, False, (3, 3, 3), {}),
    (3, 4, _Q, True, (2, 2, 2), {}),
    (3, 4, _Q, False, (3, 3, 3), {}),
]

# family, dimension, cell, block (degree 1, symmetric stress unless 3-D).  generic: 70 001, 69 938, 69 828, 68 906 and 68 921
# cells - 2188, 2186, 2183, 2154 and 2154 batches of 32 on 2048 workgroups, the last batch partly filled.  lane: 8492, 8500
# and 8316 items on 8192 waves - ipx = 1062, 1063 and 1040 against 4 blocks_here = 1024, and the last XCD range shorter.
LOOP_ROWS = [
    ("generic", 1, _S, (70001,)),
    ("generic", 2, _S, (187, 187)),
    ("generic", 3, _S, (23, 23, 22)),
    ("generic", 2, _Q, (263, 262)),
    ("generic", 3, _Q, (41, 41, 41)),
    ("lane", 1, _S, (543461,)),
    ("lane", 2, _S, (521, 522)),
    ("lane", 3, _S, (47, 46, 41)),
    # sg::hex_stage (tests/test_hex_family_gpu.py) has the lane kernels' grid and the same cap, SG_HEX_BLOCKS: 531 200 cubes of
    # DQ_1 are 8300 items, ipx = 1038
    ("hex_lane", 3, _Q, (83, 80, 80)),
]

# family, dimension, degree, cell, mesh, block grid, schedules (True: pipelined - regions FIRST / SECOND; False: un-pipelined -
# INTERIOR / BOUNDARY, the BOUNDARY launch of the lane kernels deals its items with StageArgs::spread = 1), compare the single
# block with the oracle.  Lane, one split per dimension along x with blocks of 150 / 150 / 145 cubes: wider than two groups
# and no multiple of 64, so the FIRST / INTERIOR lists hold whole groups and groups that the x shell cuts.
SPLITS = [
    ("lane", 1, 1, _S, (300,), (2,), (True, False), False),
    ("lane", 1, 2, _S, (10,), (2,), (False,), True),
    ("lane", 1, 3, _S, (9,), (3,), (True,), False),
    ("lane", 1, 4, _S, (140,), (2,), (True,), False),
    ("lane", 2, 1, _S, (300, 3), (2, 1), (True, False), False),
    ("lane", 2, 2, _S, (6, 7), (1, 2), (True,), True),
    ("lane", 2, 3, _S, (9, 6), (2, 2), (False,), False),
    ("lane", 2, 4, _S, (5, 6), (1, 2), (True,), False),
    ("lane", 3, 1, _S, (290, 2, 2), (2, 1, 1), (True, False), False),
    ("lane", 3, 2, _S, (4, 4, 4), (2, 2, 2), (True,), True),
    ("generic", 1, 1, _S, (70,), (2,), (True, False), False),
    ("generic", 1, 2, _S, (9,), (3,), (False,), True),
    ("generic", 1, 3, _S, (10,), (2,), (True,), False),
    ("generic", 1, 4, _S, (8,), (2,), (False,), False),
    ("generic", 2, 1, _S, (6, 7), (1, 2), (True,), True),
    ("generic", 2, 2, _S, (9, 6), (2, 2), (False,), False),
    ("generic", 2, 3, _S, (34, 4), (2, 1), (True,), False),
    ("generic", 2, 4, _S, (5, 6), (1, 2), (True, False), False),
    ("generic", 3, 1, _S, (4, 3, 4), (1, 1, 2), (True,), True),
    ("generic", 3, 2, _S, (4, 4, 4), (2, 2, 2), (False,), False),
    ("generic", 3, 3, _S, (4, 3, 2), (2, 1, 1), (True,), False),
    ("generic", 3, 4, _S, (2, 4, 2), (1, 2, 1), (True, False), False),
    ("generic", 2, 1, _Q, (9, 6), (2, 2), (True,), True),
    ("generic", 2, 2, _Q, (5, 6), (1, 2), (False,), False),
    ("generic", 2, 3, _Q, (6, 7), (2, 1), (True,), False),
    ("generic", 2, 4, _Q, (7, 4), (2, 2), (False,), False),
    ("generic", 3, 1, _Q, (4, 4, 4), (2, 2, 2), (False,), True),
    ("generic", 3, 2, _Q, (6, 3, 4), (3, 1, 2), (True,), False),
    ("generic", 3, 3, _Q, (4, 2, 3), (2, 1, 3), (False,), False),
    ("generic", 3, 4, _Q, (2, 4, 2), (1, 2, 2), (True,), False),
]

_SWITCHES = ("SEIGEN_HIP_SPONGE_AFFINE", "SEIGEN_HIP_SYM", "SEIGEN_HIP_PATH", "SEIGEN_HIP_SOURCE_LAUNCH", "SEIGEN_HIP_GRAPH")


def _ncls(dim, cell):
    return 1 if cell == _Q else {1: 1, 2: 2, 3: 6}[dim]


def _ncells(dim, cell, n):
    return int(np.prod(n)) * _ncls(dim, cell)


def _stage_names(family, dim, P, cell, sym):
    """the instantiation each of the six stages launches (hostlogic.hpp lf4_stage)"""
    if family == "hex_lane":
        from tests.test_hex_family_gpu import _stage_names as hex_stage_names
        return hex_stage_names(P, sym)
    if family == "lane":
        fmt = "sg::lane_stage<%d, %d, %%d, %%d, %d>" % (dim, P, int(sym))
        return [fmt % km for km in ((0, 0), (1, 0), (0, 1), (1, 0), (0, 1), (1, 1))]
    fmt = "sg::stage_kernel<%d, %d, %%d, %d>" % (dim, P, 0 if cell == _S else dim - 1)
    return [fmt % kind for kind in (0, 1, 0, 1, 0, 1)]


def _reports_sym(family, sym):
    """what is_sym() says: the generic family has no symmetric-stress storage and never enters the mode"""
    return sym and family != "generic"


def _cell_id(dim, P, cell):
    return "%dd-%s%d" % (dim, "DQ" if cell == _Q else "P", P)


def _row_id(family):
    def ident(r):
        dim, P, cell, sym, n, switches = r
        return "%s-%s-%s-%s%s" % (family, _cell_id(dim, P, cell), "sym" if sym else "full", "x".join(map(str, n)),
                                  "".join("-%s=%s" % (k[len("SEIGEN_HIP_"):].lower(), v) for k, v in sorted(switches.items())))
    return ident


def _loop_id(r):
    return "%s-%s-%s" % (r[0], _cell_id(r[1], 1, r[2]), "x".join(map(str, r[3])))


def _split_id(s):
    family, dim, P, cell, n, grid, schedules, oracle = s
    return "%s-%s-%s-on-%s-%s" % (family, _cell_id(dim, P, cell), "x".join(map(str, n)), "x".join(map(str, grid)),
                                  "+".join("pipelined" if p else "unpipelined" for p in schedules))


def _environment(monkeypatch, family, dim, sym, switches=None):
    """the family under test and a row's switches, and nothing else that picks an instantiation, the sponge's form or a
    source path; a 1-D full-tensor row never enters symmetric-stress mode (its 1 x 1 stress cannot make the library leave)"""
    for var in _SWITCHES:
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("SEIGEN_HIP_PATH", "lane" if family == "hex_lane" else family)
    if dim == 1 and not sym:
        monkeypatch.setenv("SEIGEN_HIP_SYM", "0")
    for var, val in (switches or {}).items():
        monkeypatch.setenv(var, val)


_WIDTHS = (0.4, 0.3, 0.35)
# The oracle takes a cell's Jacobian from the differences of its vertex coordinates i h (oracle/mesh.py), so its own relative
# error grows like n[0] eps where i h is rounded: 2e-12 on the 19 237 intervals of the rows above, but 6e-11 on 543 461
# intervals of width 0.4 (measured: F off by 5.6e-11 against the lane kernel, which takes h as given, 5.3e-12 on the generic
# kernel's 70 001).  The looping rows therefore use widths that are powers of two: every vertex coordinate and every
# difference is exact, and tol_of() holds unchanged.
_LOOP_WIDTHS = (0.5, 0.25, 0.5)


def _size(n, widths=_WIDTHS):
    return tuple(w * k for w, k in zip(widths, n))


def _block(dim, P, cell, n, widths=_WIDTHS):
    from seigen_amd.backend import HipBlock
    L = _size(n, widths)
    return HipBlock(dim, P, n, [L[a] / n[a] for a in range(dim)], [0.0] * dim, cell)


def _sponge(m, ncls, rng):
    """DG4 nodal sigma in any dimension, the four kinds of test_mfma_family_gpu._sponge - none, one value (sigma u at the
    node where a family can), general nodal (a matrix of its own), affine in x with a gradient of its own (dim + 1
    coefficients under SEIGEN_HIP_SPONGE_AFFINE=1, a matrix otherwise) - in turn along the cubes of every class, so every
    item of 64 cubes of a class and every batch of the generic kernel holds all four"""
    Xq = m.node_coords(4)
    cell = np.arange(m.ncells)
    kind = (cell // ncls + cell % ncls) % 4
    sigma = np.zeros(Xq.shape[:2])
    c, g, a = kind == 1, kind == 2, kind == 3
    sigma[c] = rng.uniform(2.0, 30.0, size=(c.sum(), 1))
    sigma[g] = rng.uniform(0.0, 30.0, size=(g.sum(), Xq.shape[1]))
    grad = rng.uniform(-20.0, 20.0, size=(a.sum(), 1, Xq.shape[2]))
    sigma[a] = rng.uniform(5.0, 30.0, size=(a.sum(), 1)) + (grad * (Xq[a] - Xq[a][:, :1])).sum(axis=-1)
    return sigma


def _check(family, dim, P, cell, sym, n, density, sponge, seed, widths=_WIDTHS):
    ncls = _ncls(dim, cell)
    check_block(family, lambda: _block(dim, P, cell, n, widths), oracle_mesh(dim, n, _size(n, widths), cell), min(widths[:dim]), P,
                cell, "f64", sym, _stage_names(family, dim, P, cell, sym), density,
                (lambda m, rng: _sponge(m, ncls, rng)) if sponge else None, seed, reports_sym=_reports_sym(family, sym))


@pytest.mark.parametrize("row", LANE_ROWS, ids=_row_id("lane"))
def test_lane_row_against_the_oracle(gpu, monkeypatch, row):
    dim, P, cell, sym, n, switches = row
    _environment(monkeypatch, "lane", dim, sym, switches)
    _check("lane", dim, P, cell, sym, n, ("scalar", "cell", "physical")[LANE_ROWS.index(row) % 3], True,
           3000 * P + 100 * dim + 10 * n[0] + n[-1])


@pytest.mark.parametrize("row", GENERIC_ROWS, ids=_row_id("generic"))
def test_generic_row_against_the_oracle(gpu, monkeypatch, row):
    dim, P, cell, sym, n, switches = row
    _environment(monkeypatch, "generic", dim, sym, switches)
    _check("generic", dim, P, cell, sym, n, ("scalar", "cell", "physical")[GENERIC_ROWS.index(row) % 3], True,
           4000 * P + 100 * dim + 10 * n[0] + n[-1] + (0 if cell == _S else 5))


@pytest.mark.parametrize("row", LOOP_ROWS, ids=_loop_id)
def test_looping_row_against_the_oracle(gpu, monkeypatch, row):
    """degree 1 on blocks where the fixed grids loop: more than 2048 batches (generic), more than 8192 items (lane, and
    hex_stage of the hexahedral lane family)"""
    family, dim, cell, n = row
    sym = dim < 3
    _environment(monkeypatch, family, dim, sym)
    if family == "generic":
        assert _ncells(dim, cell, n) > 2048 * GENERIC_EB[(dim, cell)][0] and _ncells(dim, cell, n) % GENERIC_EB[(dim, cell)][0]
    else:
        items = -(-int(np.prod(n)) // 64) * _ncls(dim, cell)
        assert items > 8192 and -(-items // 8) > 4 * (2048 // 8) and items % 8
    _check(family, dim, 1, cell, sym, n, ("cell", "physical", "scalar")[LOOP_ROWS.index(row) % 3], dim < 3, 5000 + 10 * dim + n[0],
           _LOOP_WIDTHS)


@pytest.mark.parametrize("split", SPLITS, ids=_split_id)
def test_split_is_bitwise_the_single_block(gpu, monkeypatch, split):
    """blocks with neighbours through the host-driven exchange (test_harness_gpu._LocalExchange), sponge and source
    included, bitwise equal to the single block from a symmetric and from a non-symmetric stress under every schedule
    listed; the kernels they name are the six of the rows of their kind; where asked, the single block against the oracle"""
    from tests.test_harness_gpu import _multiblock_case
    family, dim, P, cell, n, grid, schedules, oracle = split
    for sym in (True, False):
        _environment(monkeypatch, family, dim, sym)
        for pipelined in schedules:
            res = _multiblock_case(dim, P, n, grid, pipelined, extras=True, diagonal=cell, sym=sym)
            assert res["names"] == sorted(set(_stage_names(family, dim, P, cell, sym))), res["names"]
    if not oracle:
        return
    m = oracle_mesh(dim, n, (1.0,) * dim, cell)
    orc = OracleLF4(m, P)
    nc, nd = m.ncells, orc.E.nd
    orc.dt, orc.l, orc.mu, orc.density = res["dt"], 0.5, 0.25, 1.0
    orc.E.set_absorption(res["sigma"], 4)
    orc.u0, orc.s0 = res["u0"].copy(), res["s0"].copy()
    for k in range(3):
        orc.source = lambda t, k=k: _oracle_source(nc, nd, dim, res["src_nodes"], res["src_steps"][k])
        orc.step((k + 1) * orc.dt)
    errs = [_err("steps", family, "f64", res["u"], orc.u1), _err("steps", family, "f64", res["s"], orc.s1)]
    assert max(errs) < 10 * tol_of(P, cell), errs


def test_the_lists_cover_what_they_claim():
    """every kind has its rows and exactly one split; every dimension / code shape meets every block kind, the looping
    grid, both schedules and every cut; the switches are where the module says"""
    # ---- lane
    kinds = {(d, P, sym) for d, P in LANE_KINDS for sym in (False, True)}
    assert len(kinds) == 20 and {(r[0], r[1], r[3]) for r in LANE_ROWS} == kinds
    assert all(r[2] == _S for r in LANE_ROWS)
    for dim in (1, 2, 3):
        blocks = [r[4] for r in LANE_ROWS if r[0] == dim]
        cubes = [int(np.prod(b)) for b in blocks]
        assert 1 in cubes and any(1 < c < 64 for c in cubes) and 64 in cubes and 65 in cubes
        assert any(b[0] == 64 and c > 64 for b, c in zip(blocks, cubes)) or dim == 1      # (1-D: (128,) below)
        assert any(b[0] == 128 for b in blocks)
        assert any(c >= 200 * 64 and c % 64 for c in cubes)
        if dim > 1:
            assert any(b[0] in (7, 37) and c > 64 for b, c in zip(blocks, cubes))
        assert any(r[5] == _AFFINE for r in LANE_ROWS if r[0] == dim)
    assert [r[:2] for r in LANE_ROWS if r[5] == _EAGER] == [(2, 3)]
    # ---- generic
    gkinds = {(d, P, cell, sym) for d, P, cell in GENERIC_KINDS for sym in (False, True)}
    assert len(gkinds) == 40 and sorted((r[0], r[1], r[2], r[3]) for r in GENERIC_ROWS) == sorted(gkinds)
    for dim, cell in GENERIC_EB:
        mine = [(r[4], _ncells(dim, cell, r[4]), GENERIC_EB[(dim, cell)][r[1] - 1]) for r in GENERIC_ROWS if r[0] == dim and r[2] == cell]
        assert any(int(np.prod(b)) == 1 for b, nc, eb in mine)
        assert any(nc > eb and nc % eb for b, nc, eb in mine) and any(nc >= eb and nc % eb == 0 for b, nc, eb in mine)
        if dim > 1:
            assert any(b[0] <= 3 and nc > eb and int(np.prod(b)) > b[0] for b, nc, eb in mine)
    assert all(int(np.prod(r[4])) <= 70 for r in GENERIC_ROWS if r[2] == _Q and r[0] == 3 and r[1] == 4)
    assert sum(r[5] == _EAGER for r in GENERIC_ROWS) == 1
    # ---- the looping rows: one per code shape
    assert sorted(r[:3] for r in LOOP_ROWS) == sorted([("generic", d, c) for d, c in GENERIC_EB] + [("lane", d, _S) for d in (1, 2, 3)] +
                                                 [("hex_lane", 3, _Q)])
    # ---- splits
    assert sorted(s[:4] for s in SPLITS) == sorted([("lane", d, P, _S) for d, P in LANE_KINDS] + [("generic",) + k for k in GENERIC_KINDS])
    for family in ("lane", "generic"):
        mine = [s for s in SPLITS if s[0] == family]
        assert any(set(s[6]) == {True, False} for s in mine) and any(s[6] == (True,) for s in mine) and any(s[6] == (False,) for s in mine)
        for dim in (1, 2, 3):
            assert any(s[7] for s in mine if s[1] == dim)
            assert any(set(s[6]) == {True, False} for s in mine if s[1] == dim)
        cuts = {tuple(g > 1 for g in s[5]) for s in mine}
        assert {(True,), (True, False), (False, True), (True, True), (True, True, True)} <= cuts
        assert any(c[0] and not c[1] and not c[2] for c in cuts if len(c) == 3) and any(c[2] for c in cuts if len(c) == 3)
    assert {(False, False, True), (False, True, False)} <= {tuple(g > 1 for g in s[5]) for s in SPLITS}
    for dim in (1, 2, 3):      # lane: along x, blocks wider than 128 cubes and no multiple of 64, under both schedules
        assert any(s[5][0] == 2 and all(g == 1 for g in s[5][1:]) and s[4][0] // 2 > 128 and (s[4][0] // 2) % 64 and
                   set(s[6]) == {True, False} for s in SPLITS if s[0] == "lane" and s[1] == dim)
    for cell, d in ((_Q, 3),):  # hexahedra DQ_3 / DQ_4 with ghosts
        assert {s[2] for s in SPLITS if s[0] == "generic" and s[1] == d and s[3] == cell} == {1, 2, 3, 4}


def test_rows_name_every_stage_kernel(gpu, monkeypatch):
    """The rows launch every lane_stage and stage_kernel instantiation and nothing else, and the blocks of the splits (zero
    halo buffers attached) name the same objects: each block is set up as its test sets it up and asked for its six
    kernels.  GENERIC_EB is what the elements' node counts give."""
    torch = pytest.importorskip("torch")
    from seigen_amd.backend import HipBlock
    from seigen_amd.mesh import Partition
    seen = {"lane": set(), "generic": set()}
    for family, rows in (("lane", LANE_ROWS), ("generic", GENERIC_ROWS)):
        for dim, P, cell, sym, n, switches in rows:
            _environment(monkeypatch, family, dim, sym, switches)
            blk = _block(dim, P, cell, n)
            blk.set_params(1.0, 0.01, 0.5, 0.25)
            if not sym:
                blk.leave_sym()
            assert blk.is_sym() == _reports_sym(family, sym)
            names = [blk.stage_kernel_name(st) for st in range(6)]
            assert names == _stage_names(family, dim, P, cell, sym), names
            seen[family].update(names)
            if family == "generic":
                assert GENERIC_EB[(dim, cell)][P - 1] == min(32, 256 // blk.nd), (dim, P, cell, blk.nd)
            blk.close()
    split_names = set()
    for family, dim, P, cell, n, grid, schedules, oracle in SPLITS:
        for sym in (True, False):
            _environment(monkeypatch, family, dim, sym)
            world = int(np.prod(grid))
            bufs = []
            for p in (Partition(n, r, world, grid) for r in range(world)):
                b = HipBlock(dim, P, p.n, [1.0 / k for k in n], [p.start[a] / n[a] for a in range(dim)], cell, p.nbr_mask)
                b.set_params(1.0, 0.01, 0.5, 0.25)
                if not sym:
                    b.leave_sym()
                for field in range(4):
                    for s in range(2 * dim):
                        if p.neighbour(s) is not None:
                            bufs.append(torch.zeros(b.halo_bytes(field, s), dtype=torch.uint8, device="cuda"))
                            b.halo_attach(field, s, bufs[-1].data_ptr())
                names = [b.stage_kernel_name(st) for st in range(6)]
                assert set(names) == set(_stage_names(family, dim, P, cell, sym)), names
                split_names.update(names)
                b.close()
    assert len(LANE_KERNELS) == 80 and len(GENERIC_KERNELS) == 40
    assert seen["lane"] == LANE_KERNELS, sorted(seen["lane"] ^ LANE_KERNELS)
    assert seen["generic"] == GENERIC_KERNELS, sorted(seen["generic"] ^ GENERIC_KERNELS)
    assert split_names == LANE_KERNELS | GENERIC_KERNELS, sorted(split_names ^ (LANE_KERNELS | GENERIC_KERNELS))
