"""Point injectors on the device (include/seigen_hip.h sg_inject / sg_set_injectors; kernels_inject.hip): every layout
against amp * psi of sg_injector_weights, the transpose of the receivers through sg_correlate, series against the oracle in
every way a step can be driven (bitwise equal to one another), with a sponge under the injected cell, the dot-product test
of a forward and an adjoint handle through the public calls alone, ElasticLF4.rewind, and a split block against the single
one.

Shapes are the smallest at which each layout can go wrong: the 16-cube layouts with points in lanes 0 and 15 and in a later
group, the 64-cube layout with two groups, more than one class per cube, f32 rows.  Tolerances: bitwise where the
arithmetic is specified (one fma from zero, one add); 1 ulp, and in fact every bit, against the host's exactly rounded
same-order sum (the reverse order differs: the check tells orders apart); the suite's
whole-step bound 10 tol_of() (tests/test_parity_gpu.py) against the oracle."""
import os
import subprocess
import sys
import time
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle.lf4 import OracleLF4  # noqa: E402
from seigen_amd import _lib  # noqa: E402
from seigen_amd.backend import HipBlock, injector_weights  # noqa: E402
from tests.test_injectors_host import make_cfg  # noqa: E402
from tests.test_parity_gpu import tol_of  # noqa: E402
from tests.util import oracle_mesh, rel_err  # noqa: E402

# (name, dim, degree, cubes, diagonal, dtype, SEIGEN_HIP_PATH, symmetric-stress storage, expected kernel-name prefix)
ROWS = [
    ("mfma-P4-sym", 3, 4, (20, 2, 2), "left", "f64", None, True, "sg::mfma_stage_"),
    ("mfma-P4-full", 3, 4, (20, 2, 2), "left", "f64", None, False, "sg::mfma_stage_"),
    ("mfma-P3-sym", 3, 3, (20, 2, 2), "left", "f64", None, True, "sg::mfma_stage_"),
    ("mfma-P3-full", 3, 3, (20, 2, 2), "left", "f64", None, False, "sg::mfma_stage_"),
    ("mfma-P4-f32", 3, 4, (20, 2, 2), "left", "f32", None, True, "sg::mfma_stage_"),
    ("tile-tri-P3", 2, 3, (8, 8), "left", "f64", None, True, "sg::tile2d_stage<"),
    ("tile-quad-DQ2", 2, 2, (8, 8), "quadrilateral", "f64", None, True, "sg::tile2d_stage<"),
    ("tile-tri-P3-f32", 2, 3, (8, 8), "left", "f32", None, True, "sg::tile2d_stage<"),
    ("lane-3d-P1", 3, 1, (70, 2, 2), "left", "f64", "lane", True, "sg::lane_"),
    ("hexm-DQ3", 3, 3, (16, 2, 2), "quadrilateral", "f64", None, True, "sg::hexm_"),
    ("generic-1d-P2", 1, 2, (5,), "left", "f64", None, True, "sg::stage_kernel"),
]
BY_NAME = {r[0]: r for r in ROWS}
SWITCHES = ("SEIGEN_HIP_PATH", "SEIGEN_HIP_GRAPH", "SEIGEN_HIP_SPONGE_AFFINE", "SEIGEN_HIP_SYM", "SEIGEN_HIP_SOURCE_LAUNCH")


def _env(monkeypatch, **kw):
    for var in SWITCHES:
        monkeypatch.delenv(var, raising=False)
    for k, v in kw.items():
        if v is not None:
            monkeypatch.setenv(k, v)


def _block(row, monkeypatch, n=None, **env):
    name, dim, degree, n0, diagonal, dtype, path, sym, prefix = row
    n = n0 if n is None else n
    _env(monkeypatch, SEIGEN_HIP_PATH=path, **env)
    h = [1.0 / k for k in n]
    blk = HipBlock(dim, degree, n, h, [0.0] * dim, diagonal, dtype=dtype)
    blk._n, blk._hh = n, h
    blk._cfg = make_cfg(dim, degree, n, h, diagonal == "quadrilateral")
    blk._dt = 0.05 * min(h) / degree ** 2
    blk.set_params(1.0, blk._dt, 0.5, 0.25)
    if not sym and blk.is_sym():
        blk.leave_sym()
    return blk


def _point_in_cube(blk, cube, frac=(0.31, 0.57, 0.23)):
    n, h, c = blk._n, blk._hh, []
    for a in range(blk.dim):
        c.append(cube % n[a])
        cube //= n[a]
    return [(c[a] + frac[a]) * h[a] for a in range(blk.dim)]


def _gw(row):
    return {"sg::mfma_stage_": 16, "sg::tile2d_stage<": 16, "sg::hexm_": 16, "sg::lane_": 64, "sg::stage_kernel": 1}[row[8]]


def _amplitudes(rng, npts, dim, sym, lead=()):
    """[..., npts, dim + dim * dim]: the velocity's values, then the stress's row-major - symmetric to the bit where asked"""
    au = rng.uniform(-1.0, 1.0, lead + (npts, dim))
    as_ = rng.uniform(-1.0, 1.0, lead + (npts, dim, dim))
    if sym:
        as_ = np.triu(as_) + np.swapaxes(np.triu(as_, 1), -1, -2)
    return np.concatenate([au, as_.reshape(lead + (npts, dim * dim))], axis=-1)


def _exact_sum(terms):
    """sum_r fma(a_r, p_r, v) from zero in the order given, every fma rounded once: exact rational arithmetic, then the
    correctly rounded conversion"""
    v = 0.0
    for a, p in terms:
        v = float(Fraction(a) * Fraction(p) + Fraction(v))
    return v


def _expected(blk, dtype, pts, amp, reverse=False):
    """the fields a one-shot injection into zero fields leaves: per cell the points in the order listed (or in the reverse)"""
    dim, nd = blk.dim, blk.nd
    cell, psi = injector_weights(blk._cfg, pts, nd)
    assert (cell >= 0).all()
    u = np.zeros(blk.field_shape(_lib.FIELD_U))
    s = np.zeros(blk.field_shape(_lib.FIELD_S))
    for c in np.unique(cell):
        rows = [k for k in range(len(pts)) if cell[k] == c][::-1 if reverse else 1]
        for a in range(nd):
            for q in range(dim + dim * dim):
                v = _exact_sum([(float(amp[k, q]), float(psi[k, a])) for k in rows])
                if q < dim:
                    u[c, a, q] = v
                else:
                    s[c, a, (q - dim) // dim, (q - dim) % dim] = v
    if dtype == "f32":
        u, s = u.astype(np.float32).astype(np.float64), s.astype(np.float32).astype(np.float64)
    return cell, u, s


def _ulps(got, want, dtype):
    sp = np.spacing(np.abs(want).astype(np.float32 if dtype == "f32" else np.float64)).astype(np.float64)
    return float((np.abs(got - want) / sp).max())


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_one_shot_into_zero_fields(gpu, monkeypatch, row):
    """sg_inject into zero fields leaves amp * psi of sg_injector_weights in the owning cells and nothing elsewhere: one point
    per cell bitwise (points in the first and the last lane of a group, in a later group and in the last cube); three points
    in one cell, listed between others, and one on a grid line (the lower cell's) to 1 ulp of the exactly rounded same-order
    sum.  A symmetric amplitude table keeps symmetric storage, one that is not leaves it."""
    name, dim, degree, n, diagonal, dtype, path, sym, prefix = row
    blk = _block(row, monkeypatch)
    assert blk.stage_kernel_name(0).startswith(prefix), blk.stage_kernel_name(0)
    was_sym = blk.is_sym()
    gw, ncube = _gw(row), int(np.prod(n))
    cubes = sorted({0, min(gw - 1, ncube - 1), min(gw + 1, ncube - 1), ncube - 1})
    rng = np.random.default_rng(len(name))
    zero_u, zero_s = np.zeros(blk.field_shape(_lib.FIELD_U)), np.zeros(blk.field_shape(_lib.FIELD_S))
    # one point per cell
    pts = np.array([_point_in_cube(blk, c) for c in cubes])
    amp = _amplitudes(rng, len(pts), dim, sym)
    cell, eu, es = _expected(blk, dtype, pts, amp)
    assert len(set(cell)) == len(pts)
    blk.inject(pts, amp, 3)
    assert blk.is_sym() == (was_sym and sym)
    gu, gs = blk.get_field(_lib.FIELD_U), blk.get_field(_lib.FIELD_S)
    assert np.abs(eu).max() > 0 and np.abs(es).max() > 0
    assert np.array_equal(gu, eu) and np.array_equal(gs, es), (name, np.abs(gu - eu).max(), np.abs(gs - es).max())
    # velocity alone and stress alone leave the other field untouched
    blk.set_field(_lib.FIELD_U, zero_u)
    blk.set_field(_lib.FIELD_S, zero_s)
    blk.inject(pts, amp[:, :dim], 1)
    assert np.array_equal(blk.get_field(_lib.FIELD_U), eu) and not blk.get_field(_lib.FIELD_S).any()
    blk.inject(pts, amp[:, dim:], 2)
    assert np.array_equal(blk.get_field(_lib.FIELD_U), eu) and np.array_equal(blk.get_field(_lib.FIELD_S), es)
    # three points in one cell between points of other cells, and one on a grid line
    blk.set_field(_lib.FIELD_U, zero_u)
    blk.set_field(_lib.FIELD_S, zero_s)
    p0 = np.array(_point_in_cube(blk, cubes[1]))
    eps = 1e-3 * np.array(blk._hh)
    line = np.array(_point_in_cube(blk, min(1, ncube - 1)))
    line[0] = blk._hh[0]                       # the grid line between cube 0 and cube 1: the lower cube's
    pts = np.array([p0, line, _point_in_cube(blk, cubes[-1]), p0 + eps, p0 - eps])
    amp = _amplitudes(rng, len(pts), dim, sym)
    cell, eu, es = _expected(blk, dtype, pts, amp)
    assert cell[0] == cell[3] == cell[4] and len(set(cell)) == 3
    assert cell[1] // blk.ncls == 0, "a point on a grid line belongs to the lower cube"
    blk.inject(pts, amp, 3)
    gu, gs = blk.get_field(_lib.FIELD_U), blk.get_field(_lib.FIELD_S)
    assert np.array_equal(gu == 0, eu == 0) and np.array_equal(gs == 0, es == 0)
    assert _ulps(gu, eu, dtype) <= 1 and _ulps(gs, es, dtype) <= 1, (name, _ulps(gu, eu, dtype), _ulps(gs, es, dtype))
    # every operation of the sum is specified and correctly rounded, so the order listed is met to the bit - and another
    # order is not: in double the same sum over the cell's points in reverse differs somewhere
    assert np.array_equal(gu, eu) and np.array_equal(gs, es), (name, _ulps(gu, eu, dtype), _ulps(gs, es, dtype))
    if dtype == "f64":      # (the rounding to float of an f32 block absorbs the last bits of the double sum)
        _, ru, rs = _expected(blk, dtype, pts, amp, reverse=True)
        assert not (np.array_equal(ru, eu) and np.array_equal(rs, es))
    # a stress table that is not symmetric makes a block in symmetric storage leave it at the call: all d x d lines are
    # written, on top of what the fields hold
    if blk.is_sym():
        a2 = _amplitudes(rng, 1, dim, False)
        _, du, ds = _expected(blk, "f64", pts[2:3], a2)
        blk.inject(pts[2:3], a2, 3)
        assert not blk.is_sym()
        wu, ws = gu + du, gs + ds
        if dtype == "f32":
            wu, ws = wu.astype(np.float32).astype(np.float64), ws.astype(np.float32).astype(np.float64)
        assert np.array_equal(blk.get_field(_lib.FIELD_U), wu) and np.array_equal(blk.get_field(_lib.FIELD_S), ws)
    blk.close()


@pytest.mark.parametrize("name", ["mfma-P4-sym", "tile-tri-P3", "hexm-DQ3"])
def test_injection_is_the_transpose_of_the_receivers(gpu, monkeypatch, name):
    """Handle b holds a random field; handle a holds zeros and gets a unit amplitude in velocity component c at a point.  Then
    sum_cells sg_correlate(a, b)[uu] = sum_c |det J| psi^T Mhat b.u[cell][:, c] is b's receiver sample of component c at the
    point, to 1e-12 of the field's scale."""
    row = BY_NAME[name]
    dim = row[1]
    a, b = _block(row, monkeypatch), _block(row, monkeypatch)
    rng = np.random.default_rng(17)
    ub = rng.uniform(-1.0, 1.0, b.field_shape(_lib.FIELD_U))
    b.set_field(_lib.FIELD_U, ub)
    ncube = int(np.prod(row[3]))
    line = np.array(_point_in_cube(a, 1))
    line[0] = a._hh[0]
    pts = np.array([_point_in_cube(a, 15), _point_in_cube(a, ncube - 1), line])
    b.set_receivers(pts, 1, 1, 1)
    b.end_step()                                # a sample of the fields as they stand
    want = b.get_receivers()[0]
    assert want.shape == (len(pts), dim) and np.abs(want).min() > 0
    zero_u = np.zeros(a.field_shape(_lib.FIELD_U))
    for k in range(len(pts)):
        for c in range(dim):
            a.set_field(_lib.FIELD_U, zero_u)
            amp = np.zeros((1, dim))
            amp[0, c] = 1.0
            a.inject(pts[k:k + 1], amp, 1)
            a.reset_correlation()
            a.correlate(b)
            got = a.get_correlation()[:, 0].sum()
            assert abs(got - want[k, c]) <= 1e-12, (name, k, c, got, want[k, c])
    a.close()
    b.close()


# ---- series against the oracle -------------------------------------------------------------------------------------

# small shapes of the same families: the oracle steps them in a second or two
SERIES_ROWS = [
    ("mfma-P4-sym", 3, 4, (3, 2, 2), "left", "f64", None, True, "sg::mfma_stage_"),
    ("tile-tri-P3", 2, 3, (5, 3), "left", "f64", None, False, "sg::tile2d_stage<"),
    ("lane-2d-P2", 2, 2, (5, 3), "left", "f64", "lane", True, "sg::lane_"),
    ("generic-1d-P2", 1, 2, (5,), "left", "f64", None, True, "sg::stage_kernel"),
]
WAYS = ("graph", "eager", "single", "stages")


def _initial(X, dim):
    u = np.stack([np.sin(2 * X[..., 0] + i) * np.cos(X[..., -1] - i) for i in range(dim)], axis=-1)
    s = np.zeros(X.shape[:-1] + (dim, dim))
    for i in range(dim):
        for j in range(dim):
            s[..., i, j] = np.cos(X[..., 0] + 0.5 * (i + j)) * (1 + X[..., -1])
    return u, s


def _advance(blk, way, nsteps):
    if way in ("graph", "eager"):
        blk.step(nsteps)
    elif way == "single":
        for _ in range(nsteps):
            blk.step(1)
    else:
        for _ in range(nsteps):
            for st in range(6):
                blk.run_stage(st)
            blk.end_step()


def _add(field_u, field_s, cell, psi, amp, dim):
    for k in range(len(cell)):
        field_u[cell[k]] += psi[k][:, None] * amp[k, :dim][None, :]
        field_s[cell[k]] += psi[k][:, None, None] * amp[k, dim:].reshape(dim, dim)[None]


@pytest.mark.parametrize("row", SERIES_ROWS, ids=[r[0] for r in SERIES_ROWS])
def test_series_against_the_oracle(gpu, monkeypatch, row):
    """Ten steps with velocity and stress entries: a series of 6 entries armed at step 0 (it runs out after step 6), an
    arming with what = 0 refused after step 3 (the old series goes on), a series of 2 armed after step 7.  The oracle adds
    amp * psi on the host after the steps; sg_step under graph replay, with SEIGEN_HIP_GRAPH=0, step by step and host-driven
    stages with sg_end_step each agree with it within 10 tol_of() and with one another bit for bit."""
    name, dim, degree, n, diagonal, dtype, path, sym, prefix = row
    rng = np.random.default_rng(23)
    out = {}
    for way in WAYS:
        blk = _block(row, monkeypatch, SEIGEN_HIP_GRAPH="0" if way == "eager" else None)
        if way == "graph":
            assert blk.stage_kernel_name(0).startswith(prefix), blk.stage_kernel_name(0)
            ncube = int(np.prod(n))
            p0 = np.array(_point_in_cube(blk, ncube // 2))
            line = np.array(_point_in_cube(blk, min(1, ncube - 1)))
            line[0] = blk._hh[0]
            pts = np.array([p0, line, p0 + 1e-3 * np.array(blk._hh)])
            A = _amplitudes(rng, len(pts), dim, sym, (6,))
            B = _amplitudes(rng, len(pts), dim, sym, (2,))
            u0, s0 = _initial(blk.node_coords(), dim)
        blk.set_field(_lib.FIELD_U, u0)
        blk.set_field(_lib.FIELD_S, s0)
        assert blk.set_injectors(pts, A, 3).all()
        _advance(blk, way, 3)
        z = np.zeros(1)
        assert blk.lib.sg_set_injectors(blk.h, len(pts), pts.ctypes.data, 0, 6, A.ctypes.data, None) == -1
        assert blk.lib.sg_set_injectors(blk.h, len(pts), None, 3, 6, z.ctypes.data, None) == -1
        _advance(blk, way, 4)
        blk.set_injectors(pts, B, 3)
        _advance(blk, way, 3)
        assert blk.counters()["steps"] == 10
        out[way] = (blk.get_field(_lib.FIELD_U), blk.get_field(_lib.FIELD_S))
        blk.close()
    for way in WAYS[1:]:
        assert np.array_equal(out[way][0], out["graph"][0]) and np.array_equal(out[way][1], out["graph"][1]), way
    # the oracle, once
    blk = _block(row, monkeypatch)
    cell, psi = injector_weights(blk._cfg, pts, blk.nd)
    orc = OracleLF4(oracle_mesh(dim, n, (1.0,) * dim, diagonal), degree)
    orc.dt, orc.l, orc.mu, orc.density = blk._dt, 0.5, 0.25, 1.0
    blk.close()
    orc.u0, orc.s0 = u0.copy(), s0.copy()
    for step in range(1, 11):
        orc.step(step * orc.dt)
        entry = A[step - 1] if step <= 6 else (B[step - 8] if step in (8, 9) else None)
        if entry is not None:
            u, s = orc.u1.copy(), orc.s1.copy()
            _add(u, s, cell, psi, entry, dim)
            orc.u0 = orc.u1 = u
            orc.s0 = orc.s1 = s
    tol = 10 * tol_of(degree, diagonal)
    eu, es = rel_err(out["graph"][0], orc.u1), rel_err(out["graph"][1], orc.s1)
    print("series %s: rel err u %.2e s %.2e (bound %.1e)" % (name, eu, es, tol))
    assert eu < tol and es < tol, (name, eu, es)


SPONGE_ROWS = [
    ("mfma-P4-sym", 3, 4, (3, 2, 2), "left", "f64", None, True, "sg::mfma_stage_"),
    ("lane-3d-P1", 3, 1, (5, 2, 2), "left", "f64", "lane", True, "sg::lane_"),
]


@pytest.mark.parametrize("sponge", ["strip", "ramp"])
@pytest.mark.parametrize("row", SPONGE_ROWS, ids=[r[0] for r in SPONGE_ROWS])
def test_injection_into_a_sponge_cell(gpu, monkeypatch, row, sponge):
    """The series test under a sponge: velocity and stress entries at two points inside sponge cells, ten steps (graph
    replay: the eight-step graph and the one-step graph twice), against the oracle, eager and under graph replay: a constant
    sigma on a strip of cells and a ramp that is affine in x (SEIGEN_HIP_SPONGE_AFFINE=1: the affine pre-pass on the lane row
    too).  The F stages absorb B u from a pre-pass that is kept from stage UTEMP to the next step's UH1 and U1: an entry
    added to u1 in between makes it stale, and this test goes red if it is used again."""
    name, dim, degree, n, diagonal, dtype, path, sym, prefix = row
    m = oracle_mesh(dim, n, (1.0,) * dim, diagonal)
    Xq = m.node_coords(1)
    if sponge == "strip":
        sigma = np.where(Xq[..., 0].min(axis=1, keepdims=True) >= 1.0 / n[0] - 1e-9, 25.0, 0.0) * np.ones_like(Xq[..., 0])
    else:
        sigma = 4.0 + 11.0 * Xq[..., 0] + 7.0 * Xq[..., 1] + 23.0 * Xq[..., 2]
    rng = np.random.default_rng(31)
    K = 10
    got = {}
    for way in ("eager", "graph"):
        blk = _block(row, monkeypatch, SEIGEN_HIP_GRAPH="0" if way == "eager" else None, SEIGEN_HIP_SPONGE_AFFINE="1")
        assert blk.stage_kernel_name(0).startswith(prefix), blk.stage_kernel_name(0)
        blk.set_absorption(sigma, 1)
        if way == "eager":
            ncube = int(np.prod(n))
            pts = np.array([_point_in_cube(blk, ncube - 1), _point_in_cube(blk, ncube - 2, (0.6, 0.2, 0.7))])
            series = _amplitudes(rng, len(pts), dim, sym, (K,))
            u0, s0 = _initial(blk.node_coords(), dim)
            cell, psi = injector_weights(blk._cfg, pts, blk.nd)
            assert cell[0] != cell[1] and sigma[cell].min() > 0, "the injected cells must absorb"
        blk.set_field(_lib.FIELD_U, u0)
        blk.set_field(_lib.FIELD_S, s0)
        blk.set_injectors(pts, series, 3)
        blk.step(K)
        got[way] = (blk.get_field(_lib.FIELD_U), blk.get_field(_lib.FIELD_S))
        dt = blk._dt
        blk.close()
    assert np.array_equal(got["eager"][0], got["graph"][0]) and np.array_equal(got["eager"][1], got["graph"][1])
    orc = OracleLF4(m, degree)
    orc.dt, orc.l, orc.mu, orc.density = dt, 0.5, 0.25, 1.0
    orc.E.set_absorption(sigma, 1)
    orc.u0, orc.s0 = u0.copy(), s0.copy()
    for step in range(1, K + 1):
        orc.step(step * dt)
        u, s = orc.u1.copy(), orc.s1.copy()
        _add(u, s, cell, psi, series[step - 1], dim)
        orc.u0 = orc.u1 = u
        orc.s0 = orc.s1 = s
    tol = 10 * tol_of(degree, diagonal)
    eu, es = rel_err(got["graph"][0], orc.u1), rel_err(got["graph"][1], orc.s1)
    print("sponge %s %s: rel err u %.2e s %.2e (bound %.1e)" % (name, sponge, eu, es, tol))
    assert eu < tol and es < tol, (name, sponge, eu, es)


DOT_ROWS = [("mfma-P4-sym", (4, 2, 2), 8), ("tile-tri-P3", (5, 4), 8)]


@pytest.mark.parametrize("name,n,K", DOT_ROWS, ids=[r[0] for r in DOT_ROWS])
def test_forward_and_adjoint_handles_pass_the_dot_product_test(gpu, monkeypatch, name, n, K):
    """Two handles of one shape, rho = 1, zero fields, dt and -dt.  The forward one gets a point force q_0 (sg_inject), q_1 ..
    q_{K-1} (sg_set_injectors) at x_s and receivers at three x_r: d_k after step k.  The adjoint one gets random r at the x_r
    in reversed order and a receiver at x_s: p.  A step with -dt is the adjoint of a step in the energy inner product, whose
    velocity weight is constant, so sum_k r_k . d_k = sum_j q_j . p_{K-1-j}, within 10 tol_of() of sum |r_k . d_k| (the
    oracle's own figure is below 1e-15).  sg_step(K): graph replay."""
    row = BY_NAME[name]
    dim, degree, diagonal = row[1], row[2], row[4]
    fwd, adj = _block(row, monkeypatch, n=n), _block(row, monkeypatch, n=n)
    adj.set_params(1.0, -fwd._dt, 0.5, 0.25)
    rng = np.random.default_rng(41)
    ncube = int(np.prod(n))
    xs = np.array([_point_in_cube(fwd, ncube // 2)])
    line = np.array(_point_in_cube(fwd, 1))
    line[0] = fwd._hh[0]
    xr = np.array([_point_in_cube(fwd, 0, (0.6, 0.2, 0.7)), line, _point_in_cube(fwd, ncube - 1)])
    q = rng.uniform(-1.0, 1.0, (K, 1, dim))
    r = rng.uniform(-1.0, 1.0, (K, len(xr), dim))          # r[k - 1] = r_k, k = 1 .. K
    fwd.inject(xs, q[0], 1)
    fwd.set_injectors(xs, q[1:], 1)
    fwd.set_receivers(xr, 1, 1, K)
    fwd.step(K)
    d = fwd.get_receivers()
    adj.inject(xr, r[K - 1], 1)
    adj.set_injectors(xr, r[K - 2::-1], 1)
    adj.set_receivers(xs, 1, 1, K)
    adj.step(K)
    p = adj.get_receivers()
    assert d.shape == (K, len(xr), dim) and p.shape == (K, 1, dim)
    lhs = float(np.sum(r * d))
    rhs = float(sum(np.sum(q[j] * p[K - 1 - j]) for j in range(K)))
    scale = float(sum(abs(np.sum(r[k] * d[k])) for k in range(K)))
    print("dot-product test %s: lhs %.17g rhs %.17g, |lhs - rhs| / sum |r.d| = %.2e" % (name, lhs, rhs, abs(lhs - rhs) / scale))
    assert scale > 0 and abs(lhs - rhs) <= 10 * tol_of(degree, diagonal) * scale, (lhs, rhs, scale)
    fwd.close()
    adj.close()


def test_rewind_returns_the_fields(gpu, monkeypatch):
    """Six steps forward through ElasticLF4.run, then rewind(6): the fields return to 1e-11 (the bound of
    tests/test_fullsize_gpu.py for the same stage order).  With a source, a sponge or injectors active rewind refuses."""
    import seigen_amd
    import seigen_amd.helpers as helpers
    from seigen_amd import ElasticLF4, Expression, Function, FunctionSpace, RectangleMesh
    _env(monkeypatch)
    helpers.log = seigen_amd.elastic.log = lambda s: None
    dim, P = 2, 3
    mesh = RectangleMesh(6, 5, 1.0, 1.0, diagonal="left")
    el = ElasticLF4.create(mesh, "DG", P, dimension=dim, solver="explicit", output=False)
    el.l, el.mu, el.density = 0.6, 0.3, 1.0
    el.dt = 0.05 * (1.0 / 6) / P ** 2
    uex = Expression(tuple("sin(%r*x[%d]) + 0.3*cos(2.5*x[0])" % (2.0 + i, i) for i in range(dim)))
    sex = Expression(tuple(tuple("0.2*sin(%r*x[%d])*cos(1.5*x[%d])" % (1.0 + i + j, min(i, j), max(i, j)) for j in range(dim)) for i in range(dim)))
    el.u0.assign(Function(el.U).interpolate(uex))
    el.s0.assign(Function(el.S).interpolate(sex))
    u0, s0 = el.u0.dat.data_cells.copy(), el.s0.dat.data_cells.copy()
    el.run(6 * el.dt * (1 + 1e-9))
    assert el.block.counters()["steps"] == 6
    assert np.abs(el.u1.dat.data_cells - u0).max() > 1e-6, "the forward steps must change the state"
    el.rewind(6)
    du, ds = np.abs(el.u1.dat.data_cells - u0).max(), np.abs(el.s1.dat.data_cells - s0).max()
    assert du < 1e-11 and ds < 1e-11, (du, ds)
    # dt is the forward one again
    el.block.step(1)
    # refusals
    el.set_injectors([[0.4, 0.4]], np.ones((3, 1, dim)))
    with pytest.raises(ValueError, match="injectors"):
        el.rewind(1)
    el.set_injectors([[0.4, 0.4]], None)
    el.rewind(1)
    el.absorption_function = Function(FunctionSpace(mesh, "DG", 1))
    with pytest.raises(ValueError, match="sponge"):
        el.rewind(1)
    el.absorption_function = None
    el.source_function = Function(el.S)
    with pytest.raises(ValueError, match="source"):
        el.rewind(1)
    with pytest.raises(ValueError, match="velocity"):
        el.inject([[0.4, 0.4]], np.ones((1, dim)), what="pressure")
    with pytest.raises(ValueError, match="owning"):
        el.inject([[1.4, 0.4]], np.ones((1, dim)))


def _solver(dim, P, n):
    from seigen_amd import BoxMesh, ElasticLF4, Expression, Function, RectangleMesh
    mesh = RectangleMesh(n[0], n[1], 1.0, 1.0, diagonal="left") if dim == 2 else BoxMesh(n[0], n[1], n[2], 1.0, 1.0, 1.0)
    el = ElasticLF4.create(mesh, "DG", P, dimension=dim, solver="explicit", output=False)
    el.l, el.mu, el.density = 0.6, 0.3, 1.0
    el.dt = 0.05 * (1.0 / max(n)) / P ** 2
    uex = Expression(tuple("sin(%r*x[%d]) + 0.3*cos(2.5*x[0])" % (2.0 + i, i) for i in range(dim)))
    sex = Expression(tuple(tuple("0.2*sin(%r*x[%d])*cos(1.5*x[%d])" % (1.0 + i + j, min(i, j), max(i, j)) for j in range(dim)) for i in range(dim)))
    el.u0.assign(Function(el.U).interpolate(uex))
    el.s0.assign(Function(el.S).interpolate(sex))
    return el


@pytest.mark.parametrize("dim,P,n", [(2, 3, (6, 5)), (3, 4, (3, 2, 2))], ids=["tile-P3", "mfma-P4"])
def test_rewind_of_a_forced_run_with_observers(gpu, monkeypatch, dim, P, n):
    """The sequence INTEGRATION.md section 3 documents for the forward field: a point-force series, receivers and the monitor
    armed, run(T), the traces read, then rewind step by step beside the adjoint solver (-dt, residuals injected in reversed
    order, sg_correlate after every step pair: the zero-lag loop, an imaging condition - the material gradient's mid-step
    pairing is tests/test_gradient_gpu.py's).  After m steps back the fields
    are those a twin run holds after K - m steps of the same forced run (1e-11, the re-wind bound of
    tests/test_fullsize_gpu.py, of the fields' scale): the injected entries are taken out again, not only the steps undone.
    The receivers' and the monitor's traces are the run's, untouched by the re-wound steps, whose count does not move."""
    import seigen_amd
    import seigen_amd.helpers as helpers
    _env(monkeypatch)
    helpers.log = seigen_amd.elastic.log = lambda s: None
    K = 7
    rng = np.random.default_rng(53)
    xs = np.array([[0.41, 0.57, 0.33][:dim], [0.5, 0.23, 0.61][:dim]])        # the second on a grid line of the 2-D mesh
    xr = np.array([[0.2, 0.3, 0.4][:dim], [0.8, 0.6, 0.7][:dim]])
    q = 1e-3 * rng.uniform(-1.0, 1.0, (K, len(xs), dim))

    def forced(k):
        el = _solver(dim, P, n)
        el.set_injectors(xs, q)
        el.set_receivers(xr, every=1)
        el.set_monitor(1)
        if k:
            el.run(k * el.dt * (1 + 1e-9))
            assert el.block.counters()["steps"] == k
        return el

    el = forced(K)
    t, tr = el.receiver_traces()
    tm, mon = el.monitor_trace()
    assert tr["velocity"].shape == (K, len(xr), dim) and len(tm) == K
    # the adjoint side of the documented loop beside it: -dt, the residuals (here: the traces) at the receivers, reversed
    from seigen_amd.elastic import sensitivity
    adj = _solver(dim, P, n)
    adj.u0.dat.data = 0.0 * adj.u0.dat.data
    adj.s0.dat.data = 0.0 * adj.s0.dat.data
    adj.dt = -el.dt
    adj.setup()
    adj.set_injectors(xr, tr["velocity"][::-1] * 2.0)
    back = 0
    for k in range(K):
        adj.block.step(1)
        el.rewind(1)
        adj.correlate(el, weights=(el.dt, el.dt, el.dt))
        back += 1
        if back not in (2, 5, K):
            continue
        twin = forced(K - back)
        wu, ws = twin.u1.dat.data_cells.copy(), twin.s1.dat.data_cells.copy()
        gu, gs = el.u1.dat.data_cells, el.s1.dat.data_cells
        du, ds = np.abs(gu - wu).max() / max(1.0, np.abs(wu).max()), np.abs(gs - ws).max() / max(1.0, np.abs(ws).max())
        print("rewind of a forced run, %d-D P%d, %d steps back: u %.2e s %.2e" % (dim, P, back, du, ds))
        assert du < 1e-11 and ds < 1e-11, (back, du, ds)
    Kmat = sensitivity(dim, adj.density, adj.l, adj.mu, adj.correlation())
    assert all(np.isfinite(Kmat[k]).all() for k in ("rho", "lambda", "mu")) and np.abs(Kmat["rho"]).max() > 0
    assert back == K and el.block.counters()["steps"] == K
    t2, tr2 = el.receiver_traces()
    tm2, mon2 = el.monitor_trace()
    assert np.array_equal(tr2["velocity"], tr["velocity"]) and np.array_equal(t2, t)
    assert all(np.array_equal(mon2[k], mon[k]) for k in mon)
    # without the log the entries would stay in: the forced run differs from the free one by far more than the bound
    free = _solver(dim, P, n)
    assert np.abs(free.u1.dat.data_cells - el.u1.dat.data_cells).max() > 1e-6
    # forward again from the re-wound state: the count goes on, and a later rewind takes out only what is younger
    el.block.set_receivers(np.zeros((0, dim)))          # (the traces are full: stepping on needs them read out and disarmed)
    el.block.set_monitor(0, 0)
    el.block.step(2)
    el.inject(xs, q[0])
    el.rewind(2)
    gu = el.u1.dat.data_cells
    assert np.abs(gu - wu).max() / max(1.0, np.abs(wu).max()) < 1e-11


# ---- a split block ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fake():
    from fake_rccl.build import build
    return build()


def _injectors_on_a_split_block(fake, tmp_path, n, grid, degree, steps, cell="left"):
    """The ranks of `grid` over the transport double (tests/injector_exchange_worker.py), the exchange inside the library,
    ONE sg_step(n), against the single block here: every rank's fields equal the single block's bit for bit, and every point
    has one owner.  Returns the ranks' files."""
    from injector_exchange_worker import points_of, series_of
    from native_exchange_worker import setup_block
    dim, world = len(n), int(np.prod(grid))
    env = dict(os.environ, SEIGEN_RCCL_LIB=fake, FAKE_RCCL_TIMEOUT_S="60", FAKE_RCCL_LOG=str(tmp_path / "fake"),
               HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2", FAKE_RCCL_ASYNC="1", FAKE_RCCL_SLOT_BYTES="1048576")
    env.pop("FAKE_RCCL_HOST", None)
    for var in SWITCHES:
        env.pop(var, None)
    logs = [open(tmp_path / ("rank%d.log" % r), "w") for r in range(world)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "injector_exchange_worker.py"), str(tmp_path), str(world),
                               str(r), ",".join(map(str, grid)), ",".join(map(str, n)), str(degree), str(steps), cell],
                              cwd=ROOT, env=env, stdout=logs[r], stderr=subprocess.STDOUT) for r in range(world)]
    deadline = time.time() + 300
    errs = []
    for r, p in enumerate(procs):
        try:
            p.wait(timeout=max(1.0, deadline - time.time()))
        except subprocess.TimeoutExpired:
            p.kill()
            p.wait()
        logs[r].close()
        if p.returncode != 0:
            errs.append("rank %d: exit %r\n%s" % (r, p.returncode, open(tmp_path / ("rank%d.log" % r)).read()[-3000:]))
    assert not errs, "\n-----\n".join(errs)
    points = points_of(dim)
    blk = HipBlock(dim, degree, n, [1.0 / n[a] for a in range(dim)], [0.0] * dim, cell, 0)
    setup_block(blk, n, degree, "source")
    assert blk.set_injectors(points, series_of(steps, dim), 3).all()
    blk.step(steps)
    u, s = blk.get_field(_lib.FIELD_U), blk.get_field(_lib.FIELD_S)
    blk.close()
    owners = np.zeros(len(points), dtype=int)
    ranks = [np.load(tmp_path / ("rank%d.npz" % r)) for r in range(world)]
    for r, d in enumerate(ranks):
        assert int(d["steps"]) == steps
        owners += d["owned"]
        assert np.array_equal(d["u"], u[d["cells"]]) and np.array_equal(d["s"], s[d["cells"]]), "rank %d" % r
    assert np.all(owners == 1), owners
    return ranks


def test_injectors_on_a_split_block(gpu, fake, tmp_path):
    """Two ranks over the transport double, the exchange inside the library, ONE sg_step(n): injectors of velocity and stress
    in a cell touching the cut, on the cut plane itself (the lower block's) and in the interior.  Every rank's fields equal
    the single block's bit for bit, and every point has one owner."""
    _injectors_on_a_split_block(fake, tmp_path, (16, 4, 4), (1, 1, 2), 4, 6)


def test_injectors_on_a_split_block_2d(gpu, fake, tmp_path):
    """The same on triangles: P3 on the mesh (9, 6), two ranks (1, 2) - the 2-D tile family, blocks of four sides.  A stress
    entry makes comm_step exchange the first stage's input once more before the next step (csrc/comm.cpp: the traces of s1
    that stage S1 sent are older than the entry); points in a cell touching the cut, on the cut line itself and in the
    interior.  Bitwise the single block, one owner per point - and the extra exchanges really ran."""
    steps = 6
    ranks = _injectors_on_a_split_block(fake, tmp_path, (9, 6), (1, 2), 3, steps, "left")
    for d in ranks:
        assert all(str(k).startswith("sg::tile2d_stage<") for k in d["kernels"]), d["kernels"]
        # the first stage's input at the start of the call, six stage outputs per step, and one more behind each of the
        # series' steps - 2 stress entries (added at the end of steps 1 .. steps - 2, each followed by another step)
        assert int(d["exchanges"]) == 1 + 6 * steps + (steps - 2)
    assert ranks[0]["owned"][:2].all() and ranks[1]["owned"][2:].all()      # the point on the cut line is the lower block's


def _free_port():
    import socket
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    return port


def test_stress_injectors_through_the_host_driven_exchange(gpu, fake, tmp_path):
    """ElasticLF4.set_injectors with a stress series on 2 ranks, grid (1, 1, 2), gloo group, SEIGEN_HALO_NATIVE=0: the
    Python exchanger drives stage by stage and ends every step with sg_end_step.  A stress entry in a cell touching the cut
    is younger than the traces of s1 that stage S1 sent; HaloExchanger.step sends them again.  Every rank's fields equal the
    single rank's bit for bit."""
    from dist_worker import run_case
    from injector_dist_worker import POINTS, injectors_on_create, stress_series
    n, grid, degree, steps = (16, 4, 4), (1, 1, 2), 4, 6
    env = dict(os.environ, SEIGEN_RCCL_LIB=fake, FAKE_RCCL_TIMEOUT_S="60", FAKE_RCCL_LOG=str(tmp_path / "fake"),
               HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2", SEIGEN_DIST_BACKEND="gloo", SEIGEN_HIP_DEVICE="0",
               SEIGEN_HALO_NATIVE="0")
    env.pop("FAKE_RCCL_HOST", None)
    for var in SWITCHES:
        env.pop(var, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "injector_dist_worker.py"), str(tmp_path),
           str(degree), str(steps), ",".join(map(str, n)), ",".join(map(str, grid))]
    with open(tmp_path / "ranks.log", "w") as log:
        r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=log, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, open(tmp_path / "ranks.log").read()[-4000:]
    with injectors_on_create(POINTS, stress_series(steps)):
        el, u, s = run_case(n, degree, steps, None, True)
    assert np.abs(s).max() > 0
    for rank in range(2):
        d = np.load(tmp_path / ("rank%d.npz" % rank))
        assert int(d["native"]) == 0
        assert np.array_equal(d["u"], u[d["cells"]]) and np.array_equal(d["s"], s[d["cells"]]), "rank %d" % rank
