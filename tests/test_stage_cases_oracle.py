"""tests/stage_cases.py held to the oracle, and the reason it exists, without a GPU.

One configuration per (dimension, cell kind, degree) of the rows of tests/test_stage_alone_gpu.py - the smallest block of
those rows that has at least four cells, so that every kind of sponge cell and a neighbouring cell's density exist - and
every density convention (scalar, per cell, per cell physical):

  formulas   the six formulas chained at a whole-step dt reproduce OracleLF4.step - u1, s1, last["sh1"] and
             w = dt u1 + c3 last["utemp"] - but for the regrouping G(w) against dt sh1 + c3 sh2.  Measured over all
             configurations and conventions, three steps: largest difference 6.4e-16 relative (max-norm); bound REGROUP_BOUND =
             10 x that.
  balance    build() reaches its condition everywhere: every term of every stage at least MIN_SHARE of the result.
  power      each mutation of MUTATIONS moves the result of its stage by at least ten times the tolerance of a GPU row: 10
             tol_of() in FP64, 10 x 2e-5 in FP32.  Measured: "c_new 0.999" 2.7e-4 at the least (7e-4 typical), "sponge
             dropped" 0.25 at the least (0.48 typical), the density mutations 4.6e-2 at the least.
  blindness  the same mistakes through three whole steps at the family rows' dt = 0.04 h / P^2, on (3, 1, 2) at P4 and
             (5, 3, 3) at P1 with h = 0.4 and the rows' extras, against the whole-step tolerances (FP64 10 tol_of() = 1e-10,
             FP32 5e-5).  BLIND lists what stays under the tolerance - asserted - and what is visible today - asserted to be
             visible, so the table cannot rot.  Every figure is printed (pytest -s)."""
import functools

import numpy as np
import pytest

from oracle.lf4 import OracleLF4
from tests import stage_cases as sc
from tests import test_hex_family_gpu as hexf
from tests import test_lane_generic_family_gpu as lg
from tests import test_mfma_family_gpu as mf
from tests import test_tile2d_family_gpu as t2
from tests.test_parity_gpu import tol_of
from tests.util import oracle_mesh, rel_err

_Q = "quadrilateral"
REGROUP_BOUND = 6.4e-15
FP32_STAGE_TOL, FP32_STEPS_TOL = 2e-5, 5e-5


def _sizes(dim, cell, n):
    """the block's size as its family module has it (the widths differ between modules; any of them serves here)"""
    if dim == 3 and cell != _Q:
        return tuple(0.4 * k for k in n)
    return tuple(w * k for w, k in zip((0.4, 0.3, 0.35), n))


def _ncells(dim, cell, n):
    return int(np.prod(n)) * (1 if cell == _Q else {1: 1, 2: 2, 3: 6}[dim])


def _configurations():
    blocks = {}
    rows = [(3, "left", r[1], r[3]) for r in mf.ROWS] + [(2, r[2], r[1], r[4]) for r in t2.ROWS]
    rows += [(3, _Q, r[0], r[2]) for r in hexf.ROWS]
    rows += [(r[0], r[2], r[1], r[4]) for r in lg.LANE_ROWS + lg.GENERIC_ROWS]
    for dim, cell, P, n in rows:
        blocks.setdefault((dim, cell, P), set()).add(tuple(n))
    out = []
    for (dim, cell, P), ns in sorted(blocks.items()):
        big = [n for n in ns if _ncells(dim, cell, n) >= 4]
        out.append((dim, cell, P, min(big, key=lambda n: (_ncells(dim, cell, n), n))))
    return out


CONFIGS = _configurations()


def _cfg_id(c):
    return "%dd-%s-P%d-%s" % (c[0], c[1], c[2], "x".join(map(str, c[3])))


@functools.lru_cache(maxsize=None)
def _oracle(cfg):
    """mesh, OracleLF4, sponge sigma and its matrix (kept off the oracle), material - built once per configuration"""
    dim, cell, P, n = cfg
    m = oracle_mesh(dim, n, _sizes(dim, cell, n), cell)
    orc = OracleLF4(m, P)
    rng = np.random.default_rng(100 * dim + 10 * P + len(cell))
    sigma = lg._sponge(m, lg._ncls(dim, cell), rng)
    absorb = orc.E.ops.absorption_matrix(sigma, 4)
    lam, mu = rng.uniform(0.4, 0.8, m.ncells), rng.uniform(0.2, 0.4, m.ncells)
    return m, orc, sigma, absorb, lam, mu


@functools.lru_cache(maxsize=None)
def _case(cfg, convention, sym=True):
    dim, cell, P, n = cfg
    m, orc, sigma, absorb, lam, mu = _oracle(cfg)
    rng = np.random.default_rng(7 + 1000 * P + 10 * dim + sc.DENSITIES.index(convention))
    nodes = t2._source_nodes(m.ncells, orc.E.nd, rng)
    vals = sc.draw_stress((2, len(nodes), dim, dim), rng, sym)
    rho = sc.draw_density(convention, m.ncells, rng)
    return sc.build(orc.E, lam, mu, rho, convention == "physical", sym, sigma, absorb, nodes, vals, rng)


def test_the_configurations_are_those_of_the_gpu_rows():
    kinds = {c[:3] for c in CONFIGS}
    assert len(kinds) == len(CONFIGS)
    assert kinds == ({(1, "left", P) for P in (1, 2, 3, 4)} | {(2, c, P) for c in t2.CELLS for P in (1, 2, 3, 4)}
                     | {(3, c, P) for c in ("left", _Q) for P in (1, 2, 3, 4)})
    assert all(_ncells(c[0], c[1], c[3]) >= 4 for c in CONFIGS)


@pytest.mark.parametrize("cfg", CONFIGS, ids=_cfg_id)
def test_formulas_chained_are_a_step_of_the_oracle(cfg):
    """three steps with sponge, source, per-cell material and each density convention"""
    dim, cell, P, n = cfg
    m, orc, sigma, absorb, lam, mu = _oracle(cfg)
    nc, nd = m.ncells, orc.E.nd
    dt = 0.04 * min(s / k for s, k in zip(_sizes(dim, cell, n), n)) / P ** 2
    worst = 0.0
    for convention in sc.DENSITIES:
        rng = np.random.default_rng(31 + P + sc.DENSITIES.index(convention))
        rho = sc.draw_density(convention, nc, rng)
        nodes = t2._source_nodes(nc, nd, rng)
        vals = sc.draw_stress((3, len(nodes), dim, dim), rng, convention != "cell")
        orc.dt, orc.l, orc.mu, orc.density, orc.density_physical = dt, lam, mu, rho, convention == "physical"
        orc.u0 = rng.uniform(-1, 1, (nc, nd, dim))
        orc.s0 = sc.draw_stress((nc, nd, dim, dim), rng, convention != "cell")
        fields = {"U": orc.u0, "S": orc.s0, "UH": np.full((nc, nd, dim), np.nan), "SH": np.full((nc, nd, dim, dim), np.nan)}
        ops = sc.Operators(orc.E, lam, mu, absorb)
        orc.E.absorb = absorb
        try:
            for k in range(3):
                Ssrc = sc.scatter_source(nc, nd, dim, nodes, vals[k])
                orc.source = lambda t, S=Ssrc: S
                orc.step((k + 1) * dt)
                sc.chain_step(ops, fields, dt, rho, convention == "physical", Ssrc)
        finally:
            orc.E.absorb, orc.source = None, None
        errs = dict(u=rel_err(fields["U"], orc.u1), s=rel_err(fields["S"], orc.s1), sh=rel_err(fields["SH"], orc.last["sh1"]),
                    w=rel_err(fields["UH"], dt * orc.u1 + dt ** 3 / 24.0 * orc.last["utemp"]))
        print("REGROUP %s %s %s" % (_cfg_id(cfg), convention, {k: "%.2e" % e for k, e in errs.items()}))
        assert rel_err(orc.u1, fields["U"] * 0) > 0
        worst = max(worst, max(errs.values()))
    assert worst < REGROUP_BOUND, worst


@pytest.mark.parametrize("convention", sc.DENSITIES)
@pytest.mark.parametrize("cfg", CONFIGS, ids=_cfg_id)
def test_every_term_has_weight(cfg, convention):
    for sym in (True, False):
        case = _case(cfg, convention, sym)
        assert case.dt == sc.DT and 1.0 < case.dt < 3.0 and np.log2(case.dt) % 1
        for stage in sc.STAGES:
            share = case.share[stage]
            print("BALANCE %s %s %s %s %s" % (_cfg_id(cfg), convention, "sym" if sym else "full", stage,
                                              {k: "%.2f" % v for k, v in share.items()}))
            assert min(share.values()) >= sc.MIN_SHARE, (stage, share)
            assert set(sc.OPERANDS[stage]) == set(case.inputs[stage])
            for f in ("S", "SH"):
                if f in case.inputs[stage]:
                    a = case.inputs[stage][f]
                    assert np.array_equal(a, np.swapaxes(a, -1, -2)) == (sym or cfg[0] == 1)
        # the terms a stage has: the sponge wherever F is, the source wherever G is
        assert [list(case.share[s]) for s in sc.STAGES] == [["lin", "sponge"], ["lin", "source"], ["self", "aux", "lin", "sponge"],
                                                            ["lin", "source"], ["aux", "lin", "sponge"], ["self", "lin", "source"]]


@pytest.mark.parametrize("convention", sc.DENSITIES)
@pytest.mark.parametrize("cfg", CONFIGS, ids=_cfg_id)
def test_every_mutation_moves_its_stage(cfg, convention):
    case = _case(cfg, convention)
    need = max(10 * tol_of(cfg[2], cfg[1]), 10 * FP32_STAGE_TOL)
    done = 0
    for name, (stages, conventions) in sc.MUTATIONS.items():
        if conventions is not None and convention not in conventions:
            continue
        for stage in stages:
            moved = rel_err(sc.stage_result(case.terms(stage, mutation=name)), case.expected[stage])
            print("POWER %s %s %s %-42s %.2e" % (_cfg_id(cfg), convention, stage, name, moved))
            assert moved >= need, (name, stage, moved)
            done += 1
    assert done == {"scalar": 11, "cell": 12, "physical": 14}[convention]
    # a stage a mutation does not name is left alone
    assert np.array_equal(sc.stage_result(case.terms("STEMP", mutation="sponge dropped")), case.expected["STEMP"])


# ---------------------------------------------------------------------------------------------------------------------------
#  what three whole steps at a stable dt can see
# ---------------------------------------------------------------------------------------------------------------------------
# what is wrong: degree, (stage, terms, factor) or (mutation, stage), steps mutated, then per field read back after the steps
# the tolerance it is compared with and whether it stays below it (True: blind, asserted; False: visible today, asserted too)
_F64, _F32, _EPS32 = 1e-10, FP32_STEPS_TOL, 6e-8
BLIND = [
    ("U1 fused term off by 20 %", 4, ("U1", ("lin", "sponge"), 0.8), 3, {"U": (_F32, True), "S": (_F32, True)}),
    ("UTEMP fused term off by 20 %", 4, ("UTEMP", ("lin", "sponge"), 0.8), 3,
     {"U": (_F32, True), "S": (_F32, True), "UH": (_F32, False)}),
    ("U1 fused term off by 0.1 %", 4, ("c_new 0.999", "U1"), 3, {"U": (_F32, True), "S": (_F32, True), "U ": (_F64, False)}),
    ("UTEMP fused term off by 0.1 %", 4, ("c_new 0.999", "UTEMP"), 3, {"U": (_F32, True), "S": (_F32, True), "S ": (_F64, False)}),
    ("S1 source coefficient dt", 4, ("source coefficient dt", "S1"), 3, {"U": (_F64, True), "S": (_F64, True)}),
    ("U1 sponge dropped, one step", 4, ("sponge dropped", "U1"), 1, {"U": (_EPS32, True)}),
    ("U1 sponge dropped, one step", 1, ("sponge dropped", "U1"), 1, {"U": (_F32, True), "U ": (_F64, False)}),
]


@functools.lru_cache(maxsize=None)
def _table_block(P):
    n = (3, 1, 2) if P == 4 else (5, 3, 3)
    m = oracle_mesh(3, n, tuple(0.4 * k for k in n))
    orc = OracleLF4(m, P)
    rng = np.random.default_rng(50 + P)
    sigma = mf._sponge(m, rng)
    return n, m, orc, orc.E.ops.absorption_matrix(sigma, 4), rng.uniform(0.4, 0.8, m.ncells), rng.uniform(0.2, 0.4, m.ncells)


@pytest.mark.parametrize("row", BLIND, ids=lambda r: "%s-P%d" % (r[0].replace(" ", "_"), r[1]))
def test_whole_steps_do_not_see_it(row):
    what, P, change, nmut, watch = row
    n, m, orc, absorb, lam, mu = _table_block(P)
    nc, nd = m.ncells, orc.E.nd
    dt = 0.04 * 0.4 / P ** 2
    rng = np.random.default_rng(60 + P)
    start = {"U": rng.uniform(-1, 1, (nc, nd, 3)), "S": sc.draw_stress((nc, nd, 3, 3), rng, True),
             "UH": np.zeros((nc, nd, 3)), "SH": np.zeros((nc, nd, 3, 3))}
    nodes = mf._source_nodes(n, nd, rng)
    vals = sc.draw_stress((3, len(nodes), 3, 3), rng, True)
    ops = sc.Operators(orc.E, lam, mu, absorb)

    def run(mutated):
        f = dict(start)
        for k in range(3):
            Ssrc = sc.scatter_source(nc, nd, 3, nodes, vals[k])
            kw = {}
            if mutated and k < nmut:
                kw = dict(scale=change) if len(change) == 3 else dict(mutation=change[0], mutate_stage=change[1])
            sc.chain_step(ops, f, dt, 1.1, False, Ssrc, **kw)
        return f

    good, bad = run(False), run(True)
    for field, (tol, blind) in watch.items():
        moved = rel_err(bad[field.strip()], good[field.strip()])
        print("BLIND %-32s P%d %-2s moved %.2e tolerance %.0e %s" % (what, P, field.strip(), moved, tol,
                                                                    "blind" if blind else "visible today"))
        assert moved > 0
        assert (moved < tol) == blind, (what, field, moved, tol)
