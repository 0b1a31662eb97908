"""Every fused LF4 stage alone, each of its terms at full weight, on every row of the four family modules.

Whole steps at a stable dt weigh what makes a stage *fused* - the epilogue c_self out + c_aux aux + c_new rhs, the density
factors, the sponge operand of a fused F stage, the source coefficient of S1 - at 1e-4 and less of the result
(tests/test_stage_cases_oracle.py has the table), so the rows of the family modules, which compare steps, cannot see an
error there.  Here sg_run_stage runs one stage at dt = 1.9 on operands that tests/stage_cases.py draws and scales from the
oracle's terms until every term is at least 0.05 of the result, and the output is compared with the stage restated on the
oracle's operators.

ROWS takes its rows from the family modules - ROWS of test_mfma_family_gpu.py (blocks that several rows share through one
SharedOracle), ROWS of test_tile2d_family_gpu.py and test_hex_family_gpu.py, LANE_ROWS and GENERIC_ROWS of
test_lane_generic_family_gpu.py - each with its module's block builder, environment switches, sponge, source nodes and
(dtype, degree, storage, cell), so a new row there is a new row here.  Per row:

  1. per-cell lam, mu; the density convention by the row's index (scalar, per cell, per cell physical); the row's sponge,
     scaled; a nodal source with a node listed twice, scaled; is_sym() and the six stage_kernel_names as the family module
     pins them;
  2. for each of the six stages: all four fields uploaded - the operands, and a sentinel in every field that is no operand
     (NaN; a symmetric 1e30 in the stresses of a block in symmetric storage, which a NaN would make it leave) - one
     run_stage, the output against the restated stage at the row's per-application tolerance (tol_of() in FP64, 2e-5 in
     FP32: one stage is one application and an axpy of balanced terms), and the three other fields read back bitwise as
     uploaded: a stage writes its output and nothing else;
  3. stage U1 again in the same handle after new U and SH only: the sponge pre-pass (hostlogic.hpp PrePass) across uploads;
  4. stage UTEMP again after sg_set_field_range of U on one sponge cell: the pre-pass must be redone.

GRID_ROWS: the persistent-grid kernels (mfma_stage_F / mfma_stage_G, hexm_stage: tests/test_item_loop_gpu.py) under
SEIGEN_HIP_GRID_BLOCKS=8 on blocks with more items than the 32 waves of that grid; the six single-stage outputs must be
bitwise those of the library's own grid.  The GHOST = 1 objects are not launched here: their bitwise equality with the single
block (the SPLITS of the family modules, the native-exchange rows) carries this check over to them.

Every figure is printed before it is asserted (pytest -s): ERR stage-alone <family> <dtype> <row> <stage> <figure>.
Largest figures measured on an MI355X, all rows and stages: FP64 mfma 7.8e-13, tile2d 5.1e-13, hexm 6.1e-13, hex_lane 2.9e-14,
lane 1.3e-12, generic 5.6e-13 (tolerance 1e-11, DQ_4 5e-11); FP32 mfma 2.5e-7, tile2d 1.8e-7 (tolerance 2e-5, unmoved).

Shown to bite, once, with a library built aside that held three mistakes: stage UTEMP's c_new = 0.999 dt^3/24 and stage
S1's source coefficient dt (hostapi.cpp lf4_stage), and the per-cell density factor left off the c_new term of
mfma_stage_F (physical density on the dt term only).  Every row here failed: UTEMP on all 141 (3.6e-4 and more), S1 on all
141 (0.08 and more), U1 on the eight mfma rows with a physical density (0.12 to 0.26).  Of the whole-step rows of
test_mfma_family_gpu.py and test_tile2d_family_gpu.py every FP64 row failed, and 24 of the 28 FP32 rows passed - all but the
four mfma rows with a physical density."""
import collections
import functools
import zlib

import numpy as np
import pytest

from oracle import mesh as omesh
from oracle.lf4 import OracleLF4
from tests import stage_cases as sc
from tests import test_hex_family_gpu as hexf
from tests import test_lane_generic_family_gpu as lg
from tests import test_mfma_family_gpu as mf
from tests import test_tile2d_family_gpu as t2
from tests.test_parity_gpu import tol_of
from tests.util import oracle_mesh, rel_err

pytestmark = pytest.mark.gpu

_Q = "quadrilateral"
_GRID = "SEIGEN_HIP_GRID_BLOCKS"

# id; family, dtype, dim, degree, cell, symmetric stress, what is_sym() reports; environment(monkeypatch, grid); block();
# oracle(rng) -> mesh, ElasticOperators, sigma, its matrix; source_nodes(mesh, nd, rng); the six kernel names; density
# convention; per-application tolerance
Row = collections.namedtuple("Row", "id family dtype dim P cell sym reports_sym environment block oracle source_nodes names "
                                    "density tol")


def _fresh_oracle(mesh, P, sponge):
    def build(rng):
        m = mesh()
        E = OracleLF4(m, P).E
        sigma = sponge(m, rng)
        return m, E, sigma, E.ops.absorption_matrix(sigma, 4)
    return build


@functools.lru_cache(maxsize=None)
def _shared_oracle(n, P):
    return mf.SharedOracle(n, P, 6000 + P)


def _lent_oracle(n, P):
    def lend(rng):
        shared = _shared_oracle(tuple(n), P)
        m, orc = shared.lend()
        return m, orc.E, shared.sigma, shared.absorb
    return lend


def _mfma_row(i, r, n=None, grid_switch=False):
    dtype, P, sym, n0, gq = r
    n = n0 if n is None else n
    L = tuple(0.4 * k for k in n)

    def environment(mp, grid=None):
        mf._environment(mp, "mfma", gq, {_GRID: grid} if grid_switch else None)
    return Row("mfma-" + mf._row_id((dtype, P, sym, n, gq)), "mfma", dtype, 3, P, "left", sym, sym, environment,
               lambda: mf._block(dtype, P, n, L), _lent_oracle(n, P), lambda m, nd, rng: mf._source_nodes(n, nd, rng),
               mf._stage_names(dtype, P, sym, mf._fact(dtype, P, gq)), sc.DENSITIES[i % 3], mf._tolerances(dtype, P)[0])


def _tile2d_row(i, r):
    dtype, P, cell, sym, n, tile_grid, switches = r
    L, ncls = t2._size(n), 1 if cell == _Q else 2
    return Row("tile2d-" + t2._row_id(r), "tile2d", dtype, 2, P, cell, sym, sym,
               lambda mp, grid=None: t2._environment(mp, tile_grid, switches), lambda: t2._block(dtype, P, cell, n, L),
               _fresh_oracle(lambda: oracle_mesh(2, n, L, cell), P, lambda m, rng: t2._sponge(m, ncls, rng)),
               lambda m, nd, rng: t2._source_nodes(m.ncells, nd, rng), t2._stage_names(dtype, P, cell, sym),
               sc.DENSITIES[i % 3], t2._tolerances(dtype, P, cell)[0])


def _hex_row(i, r, n=None, grid_switch=False):
    P, sym, n0, affine = r
    n = n0 if n is None else n
    L = hexf._size(n)

    def environment(mp, grid=None):
        hexf._environment(mp, P, affine)
        if grid_switch:
            mp.delenv(_GRID, raising=False)
            if grid is not None:
                mp.setenv(_GRID, grid)
    return Row("hex-" + hexf._row_id((P, sym, n, affine)), "hexm" if P >= 3 else "hex_lane", "f64", 3, P, _Q, sym, sym, environment,
               lambda: hexf._block(P, n, L), _fresh_oracle(lambda: omesh.structured(3, n, L, quadrilateral=True), P, mf._sponge),
               lambda m, nd, rng: t2._source_nodes(m.ncells, nd, rng), hexf._stage_names(P, sym), sc.DENSITIES[i % 3],
               tol_of(P, _Q))


def _lane_generic_row(family, i, r):
    dim, P, cell, sym, n, switches = r
    ncls = lg._ncls(dim, cell)
    return Row(lg._row_id(family)(r), family, "f64", dim, P, cell, sym, lg._reports_sym(family, sym),
               lambda mp, grid=None: lg._environment(mp, family, dim, sym, switches), lambda: lg._block(dim, P, cell, n),
               _fresh_oracle(lambda: oracle_mesh(dim, n, lg._size(n), cell), P, lambda m, rng: lg._sponge(m, ncls, rng)),
               lambda m, nd, rng: t2._source_nodes(m.ncells, nd, rng), lg._stage_names(family, dim, P, cell, sym),
               sc.DENSITIES[i % 3], tol_of(P, cell))


ROWS = ([_mfma_row(i, r) for i, r in enumerate(mf.ROWS)] + [_tile2d_row(i, r) for i, r in enumerate(t2.ROWS)]
        + [_hex_row(i, r) for i, r in enumerate(hexf.ROWS)]
        + [_lane_generic_row("lane", i, r) for i, r in enumerate(lg.LANE_ROWS)]
        + [_lane_generic_row("generic", i, r) for i, r in enumerate(lg.GENERIC_ROWS)])

# The forced grid has 8 blocks of four waves.  mfma: an item is 16 cubes of one of the six classes - (15, 4, 3) has 72, the
# block of tests/test_item_loop_gpu.py's tier A; hexm: an item is 16 cubes - (13, 8, 5) has 33.  FACT = 1 in double at
# degree 3, the float objects at degree 2, DQ_3 from a full tensor.
GRID_BLOCK_MFMA, GRID_BLOCK_HEXM = (15, 4, 3), (13, 8, 5)
GRID_ROWS = [_mfma_row(1, ("f64", 3, True, None, "1"), GRID_BLOCK_MFMA, True),
             _mfma_row(2, ("f32", 2, False, None, None), GRID_BLOCK_MFMA, True),
             _hex_row(1, (3, False, None, None), GRID_BLOCK_HEXM, True)]


def _inputs(row):
    """the row's StageCase and what else its block is given; the seed is the row's name"""
    rng = np.random.default_rng(zlib.crc32(row.id.encode()))
    m, E, sigma, absorb = row.oracle(rng)
    nc = m.ncells
    lam, mu = rng.uniform(0.4, 0.8, nc), rng.uniform(0.2, 0.4, nc)
    rho = sc.draw_density(row.density, nc, rng)
    nodes = row.source_nodes(m, E.nd, rng)
    vals = sc.draw_stress((2, len(nodes), row.dim, row.dim), rng, row.sym)
    case = sc.build(E, lam, mu, rho, row.density == "physical", row.sym, sigma, absorb, nodes, vals, rng)
    return case, lam, mu, rng


def _set_up(row, blk, case, lam, mu):
    from seigen_amd import _lib
    if row.density == "scalar":                 # the explicit reference's u1 = rho u0 + ...
        blk.set_params(case.density, case.dt, lam, mu)
    else:
        blk.set_params(1.0, case.dt, lam, mu)
        blk.set_density(case.density, physical=case.physical)
    if case.sigma is not None:
        blk.set_absorption(case.sigma, 4)
    blk.set_source(case.nodes, case.src_vals)
    blk.set_field(_lib.FIELD_S, case.inputs["UH1"]["S"])
    blk.set_field(_lib.FIELD_U, case.inputs["UH1"]["U"])
    assert blk.is_sym() == row.reports_sym
    names = [blk.stage_kernel_name(st) for st in range(6)]
    assert names == row.names, names


def _stored(row, a):
    """what a block holds of an uploaded array: rounded to float once in an FP32 block"""
    return a.astype(np.float32).astype(np.float64) if row.dtype == "f32" else a


def _sentinel(blk, field, shape):
    """NaN; in a stress field of a block in symmetric storage a symmetric 1e30, which keeps the storage"""
    from seigen_amd import _lib
    stress = field in (_lib.FIELD_S, _lib.FIELD_SH)
    return np.full(shape, 1e30 if stress and blk.is_sym() else np.nan)


def _figure(row, what, got, want, failures):
    """the figure, printed before anything is asserted on it; a miss is kept for the end of the row"""
    e = rel_err(got, want)
    print("ERR stage-alone %s %s %s %s %.3e" % (row.family, row.dtype, row.id, what, e))
    if not (np.isfinite(got).all() and e < row.tol):
        failures.append((what, e))
    return e


def _upload(blk, case, given):
    """all four fields: `given` by name, a sentinel in the others; returns what was uploaded by field index"""
    from seigen_amd import _lib
    index = dict(U=_lib.FIELD_U, UH=_lib.FIELD_UH, S=_lib.FIELD_S, SH=_lib.FIELD_SH)
    up = {}
    for name in sc.FIELDS:
        up[index[name]] = given[name] if name in given else _sentinel(blk, index[name], case.shape[name])
        blk.set_field(index[name], up[index[name]])
    return up


def _stage_alone(row, blk, case, stage, given, want, failures, what=None):
    """upload, one run_stage, the output against `want`, the other three fields bitwise as uploaded; returns the output"""
    from seigen_amd import _lib
    index = dict(U=_lib.FIELD_U, UH=_lib.FIELD_UH, S=_lib.FIELD_S, SH=_lib.FIELD_SH)
    up = _upload(blk, case, given)
    assert blk.is_sym() == row.reports_sym
    blk.run_stage(sc.STAGES.index(stage))
    out = blk.get_field(index[sc.OUTPUT[stage]])
    _figure(row, what or stage, out, want, failures)
    for field, a in up.items():
        if field != index[sc.OUTPUT[stage]]:
            assert np.array_equal(blk.get_field(field), _stored(row, a), equal_nan=True), (stage, "wrote field", field)
    return out


def _sponge_cell(case):
    """a cell whose sponge goes through the pre-pass (a sigma that varies over the cell), else one with a sponge, else 0"""
    if case.sigma is None:
        return 0
    s = np.asarray(case.sigma).reshape(case.shape["U"][0], -1)
    varying = np.flatnonzero(np.ptp(s, axis=1) > 0)
    some = np.flatnonzero(np.abs(s).max(axis=1) > 0)
    return int(varying[0]) if len(varying) else (int(some[0]) if len(some) else 0)


def _six_stages(row, blk, case, failures):
    assert sc.STAGES == ("UH1", "STEMP", "U1", "SH1", "UTEMP", "S1")
    return [_stage_alone(row, blk, case, stage, case.inputs[stage], case.expected[stage], failures) for stage in sc.STAGES]


@pytest.mark.parametrize("row", ROWS, ids=lambda r: r.id)
def test_stage_alone(gpu, monkeypatch, row):
    from seigen_amd import _lib
    row.environment(monkeypatch)
    case, lam, mu, rng = _inputs(row)
    failures = []
    blk = row.block()
    try:
        _set_up(row, blk, case, lam, mu)
        _six_stages(row, blk, case, failures)

        # stage U1 twice in one handle: the second time after new U and SH only (UH, the sponge and S stay)
        _stage_alone(row, blk, case, "U1", case.inputs["U1"], case.expected["U1"], failures, "U1 again")
        again, want, _ = case.draw("U1", rng, keep={"UH": case.inputs["U1"]["UH"]})
        blk.set_field(_lib.FIELD_U, again["U"])
        blk.set_field(_lib.FIELD_SH, again["SH"])
        blk.run_stage(_lib.STAGE_U1)
        _figure(row, "U1 after new U, SH", blk.get_field(_lib.FIELD_U), want, failures)

        # stage UTEMP, then U of one sponge cell through sg_set_field_range, then stage UTEMP: the pre-pass is redone
        given = case.inputs["UTEMP"]
        _stage_alone(row, blk, case, "UTEMP", given, case.expected["UTEMP"], failures, "UTEMP again")
        cell = _sponge_cell(case)
        moved = dict(given, U=given["U"].copy())
        moved["U"][cell] = rng.uniform(-1, 1, moved["U"][cell].shape)
        blk.set_field_range(_lib.FIELD_U, cell, moved["U"][cell:cell + 1])
        blk.run_stage(_lib.STAGE_UTEMP)
        want = sc.stage_result(case.terms("UTEMP", moved))
        assert rel_err(want, case.expected["UTEMP"]) > 100 * row.tol
        _figure(row, "UTEMP after U of cell %d" % cell, blk.get_field(_lib.FIELD_UH), want, failures)
    finally:
        blk.close()
    assert not failures, (row.tol, failures)


@pytest.mark.parametrize("row", GRID_ROWS, ids=lambda r: r.id)
def test_forced_grid_is_bitwise_the_library_s_own(gpu, monkeypatch, row):
    """more items than the forced grid has waves, so a wave goes round its item loop again with the fused epilogue"""
    cubes = int(np.prod(GRID_BLOCK_MFMA if row.family == "mfma" else GRID_BLOCK_HEXM))
    assert -(-cubes // 16) * (6 if row.family == "mfma" else 1) > 8 * 4
    case, lam, mu, rng = _inputs(row)
    failures, outs = [], {}
    for grid in (None, "8"):
        row.environment(monkeypatch, grid)
        blk = row.block()
        try:
            _set_up(row, blk, case, lam, mu)
            outs[grid] = _six_stages(row, blk, case, failures)
        finally:
            blk.close()
    for stage, own, forced in zip(sc.STAGES, outs[None], outs["8"]):
        assert np.array_equal(own, forced), (stage, rel_err(forced, own))
    assert not failures, (row.tol, failures)


def test_the_rows_are_the_family_modules_rows():
    assert len(ROWS) == len(mf.ROWS) + len(t2.ROWS) + len(hexf.ROWS) + len(lg.LANE_ROWS) + len(lg.GENERIC_ROWS)
    assert len({r.id for r in ROWS}) == len(ROWS)
    assert {r.family for r in ROWS} == {"mfma", "tile2d", "hexm", "hex_lane", "lane", "generic"}
    assert {r.family for r in GRID_ROWS} == {"mfma", "hexm"}
    for family in ("mfma", "tile2d"):
        assert {r.dtype for r in ROWS if r.family == family} == {"f64", "f32"}
    for family in {r.family for r in ROWS}:
        assert {r.density for r in ROWS if r.family == family} == set(sc.DENSITIES)
