"""One handle, reconfigured between stepping calls, against the oracle after every stepping call.

The oracle rows of the other modules make a handle, configure it once and call sg_step(3).  Here the script of
tests/lifetime_script.py runs on one living handle per case - every kernel family, both stress storages, both number types -
through the graph cache and its epoch, sg_step's split into replays of graph8 and graph1, the reuse of the sponge pre-pass
across uploads and un-fused operators, sources that start, run out and change, symmetric-stress storage left in mid-run, eager
steps with timing, host-driven stages, receivers armed, read, re-armed and disarmed - and its mirror, an OracleLF4 told the
same thing at every call with the semantics of include/seigen_hip.h, says what the fields, the work fields, the counters,
is_sym() and the receivers' samples must be at every checkpoint.  Each case pins its six stage kernels by name before
anything runs and again when the storage changes.  Each case runs twice, with graph replay (SEIGEN_HIP_GRAPH unset) and
without (SEIGEN_HIP_GRAPH=0): both against the oracle, and against each other bit for bit.

Bounds.  FP64, at a checkpoint: max(10 tol_of(P, cell), 10 x the committed floor there) - the suite's figure for whole
steps, or ten times what the two CPU references (numpy oracle, plain-C port: tests/golden/lifetime_floor.json) differ by at
that checkpoint, whichever is larger: the device differs from either by fused multiply-adds and the matrix pipe's
accumulation order as well, the margin the suite gives three steps over one application.  The floor stays below 4e-14 over
the 111 steps of the script, so the first term decides everywhere.  Float: no float reference exists; 5e-5, the suite's
figure for three steps, times ceil(k / 3) for the k steps since both fields were last uploaded whole (at most 30).  One
application of F or G: tol_of / 2e-5.  A receiver sample sum_a phi_a(xi) field_a: the bound of the fields times
sum_a |phi_a(xi)| (the largest over the receivers) times the field's largest value.

The two solver-class cases call ElasticLF4.run() three times on one object, changing dt, the absorption, the source
expression and the receivers' `every` in between: every run() calls setup() on a handle that holds fields, graphs and a
pre-pass buffer.  Each run restarts t at dt, as the reference's loop does (elastic.py:279).

CPU side: the numpy mirrors of all fifteen cases take 28 s on 8 threads.

Largest relative error over all checkpoints and both runs of a case on an MI355X (a record, not a bound, taken before the
two eager steps around the upload of a few cells joined the script; FP64 bound 1e-10,
DQ_4 5e-10, float 5e-5 .. 3.5e-4):
  generic-1d-P2 1.6e-15   generic-2d-P2 4.6e-15   lane-2d-P2 4.1e-15     lane-hex-DQ2 4.2e-15   lane-hex-DQ2-affine 5.1e-15
  tile-tri-P3 7.3e-15     tile-quad-P2 3.5e-15    mfma-P3-sym 1.1e-14    mfma-P3-full 1.3e-14   mfma-P4-sym 6.9e-14
  mfma-P4-full 7.6e-14    hexm-DQ3 2.0e-14        hexm-DQ4 1.5e-13       mfma-P4-f32 5.9e-7     tile-tri-P3-f32 6.2e-7
  solver class: tile-2d-P2 3.3e-14, mfma-3d-P3 1.2e-13
Seeded in a scratch build, case mfma-P3-sym: sg_set_density without its epoch bump fails the replay run at checkpoint 4
(density.cell, step 23: 0.38); transfer() without mark_field_written on uploads fails the eager run at checkpoint 8
(sponge.upload, step 33: 0.055)."""
import json
import math
import os

import numpy as np
import pytest

from oracle.lf4 import OracleLF4
from tests import lifetime_script as ls
from tests.lifetime_script import CASES, rel_field_error
from tests.test_parity_gpu import tol_of
from tests.util import oracle_mesh

pytestmark = pytest.mark.gpu

FLOOR_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lifetime_floor.json")
FIELDS = ("u", "s", "uh", "sh")


def _environment(monkeypatch, case, graph):
    for var in ls.SWITCHES:
        monkeypatch.delenv(var, raising=False)
    if case.path:
        monkeypatch.setenv("SEIGEN_HIP_PATH", case.path)
    for var, val in case.env.items():
        monkeypatch.setenv(var, val)
    if graph is not None:
        monkeypatch.setenv("SEIGEN_HIP_GRAPH", graph)


def _block(case):
    from seigen_amd.backend import HipBlock
    return HipBlock(case.dim, case.degree, case.n, [1.0 / k for k in case.n], [0.0] * case.dim, case.cell, dtype=case.dtype)


def _bounds(case, floor):
    """(bound of checkpoint number c after k steps of its stretch, bound of one application)"""
    if case.dtype == "f32":
        return (lambda c, k: 5e-5 * math.ceil(k / 3.0)), 2e-5
    tol = tol_of(case.degree, case.cell)
    return (lambda c, k: max(10 * tol, 10 * floor[c])), tol


def compare(case, mode, got, want, floor):
    """every observation of a run against the mirror's; returns the largest error / bound and the largest error"""
    assert [(o["i"], o["op"]) for o in got] == [(o["i"], o["op"]) for o in want]
    step_bound, tol1 = _bounds(case, floor)
    worst, worst_err, c, last = 0.0, 0.0, 0, None
    for g, w in zip(got, want):
        where = "%s %s op %d %s (%s)" % (case.name, mode, w["i"], w["op"], w["tag"])
        if w["op"] == "kernels":
            assert g["names"] == w["names"], where
        elif w["op"] == "set_receivers":
            assert np.array_equal(g["owned"], w["owned"]), where
        elif w["op"] in ("apply_F", "apply_G"):
            k = "uh" if w["op"] == "apply_F" else "sh"
            err = rel_field_error(g[k], w[k])
            print("LIFETIME %s: %.3e of %.1e" % (where, err, tol1))
            assert err < tol1, where
        elif w["op"] == "get_receivers":
            assert g["traces"].shape == w["traces"].shape, where
            nu = case.dim if w["what"] & 1 else 0
            for j in range(len(w["traces"])):
                diff = np.abs(g["traces"][j] - w["traces"][j])
                eu = diff[:, :nu].max() / w["scales"][j][0] if nu else 0.0
                es = diff[:, nu:].max() / w["scales"][j][1] if diff.shape[1] > nu else 0.0
                bound = last * w["lebesgue"]
                print("LIFETIME %s sample %d: %.3e %.3e of %.1e" % (where, j, eu, es, bound))
                assert max(eu, es) < bound, (where, j)
                worst, worst_err = max(worst, max(eu, es) / bound), max(worst_err, eu, es)
            assert len(w["traces"]) == 0 or np.abs(w["traces"]).max() > 0
        else:
            assert (g["steps"], g["launches"]) == (w["steps"], w["launches"]), where
            assert g["sym"] == w["sym"], where
            bound = last = step_bound(c, w["stretch"])
            errs = [rel_field_error(g[k], w[k]) for k in FIELDS]
            print("LIFETIME %s checkpoint %d, step %d: %s of %.1e" % (where, c, w["steps"], " ".join("%.3e" % e for e in errs), bound))
            assert max(errs) < bound, (where, c, errs)
            worst, worst_err = max(worst, max(errs) / bound), max(worst_err, max(errs))
            c += 1
    return worst, worst_err


def moved(want):
    """the oracle's state really moved between any two checkpoints"""
    cps = [w for w in want if w["op"] in ls.STEPPING]
    for a, b in zip(cps, cps[1:]):
        assert rel_field_error(b["u"], a["u"]) > 1e-4 and rel_field_error(b["s"], a["s"]) > 1e-4, b["i"]
    return len(cps)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_a_lifetime_against_the_oracle(gpu, monkeypatch, case):
    script, want = ls.mirror_run(case)
    floor = None
    if case.dtype == "f64":
        with open(FLOOR_FILE) as f:
            floor = json.load(f)[case.name]
        assert len(floor) == moved(want)
    else:
        moved(want)
    runs = {}
    for mode, graph in (("replay", None), ("eager", "0")):
        _environment(monkeypatch, case, graph)
        blk = _block(case)
        try:
            runs[mode] = ls.run_script(blk, script)
        finally:
            blk.close()
        print("LIFETIME-WORST %s %s: %.4f of its bound, %.2e" % ((case.name, mode) + compare(case, mode, runs[mode], want, floor)))
    for a, b in zip(runs["replay"], runs["eager"]):
        for k in FIELDS + ("traces",):
            if k in a:
                assert np.array_equal(a[k], b[k]), (case.name, a["i"], a["op"], k)


# ---- the solver class: three run() calls on one object -----------------------------------------------------------------------

SOLVER_CASES = [("tile-2d-P2", 2, 2, (6, 5)), ("mfma-3d-P3", 3, 3, (3, 2, 2))]


@pytest.mark.parametrize("spec", SOLVER_CASES, ids=[s[0] for s in SOLVER_CASES])
def test_three_runs_of_one_solver_object(gpu, monkeypatch, spec):
    import seigen_amd
    import seigen_amd.helpers as helpers
    from seigen_amd import BoxMesh, ElasticLF4, Expression, Function, FunctionSpace, RectangleMesh
    name, dim, P, n = spec
    for var in ls.SWITCHES:
        monkeypatch.delenv(var, raising=False)
    helpers.log = seigen_amd.elastic.log = lambda s: None
    L = (1.0,) * dim
    mesh = RectangleMesh(n[0], n[1], 1.0, 1.0, diagonal="left") if dim == 2 else BoxMesh(n[0], n[1], n[2], 1.0, 1.0, 1.0)
    om = oracle_mesh(dim, n, L)
    el = ElasticLF4.create(mesh, "DG", P, dimension=dim, solver="explicit", output=False)
    names = [el.block.stage_kernel_name(st) for st in range(6)]
    family = "sg::tile2d_stage<" if dim == 2 else "sg::mfma_stage_"
    assert all(nm.startswith(family) for nm in names), names
    orc = OracleLF4(om, P)
    nc = om.ncells
    Xo = om.node_coords(P)
    el.l = orc.l = 0.6
    el.mu = orc.mu = 0.3
    el.density = orc.density = 1.05
    uex = Expression(tuple("sin(%r*x[%d]) + 0.3*cos(2.5*x[0])" % (2.0 + i, i) for i in range(dim)))
    sex = Expression(tuple(tuple("0.2*sin(%r*x[%d])*cos(1.5*x[%d])" % (1.0 + i + j, i, j) for j in range(dim)) for i in range(dim)))
    el.u0.assign(Function(el.U).interpolate(uex))
    el.s0.assign(Function(el.S).interpolate(sex))
    orc.u0 = uex.evaluate(Xo).reshape(nc, -1, dim)
    orc.s0 = sex.evaluate(Xo).reshape(nc, -1, dim, dim)
    box = " && ".join("x[%d] >= 0.2123 && x[%d] <= 0.7345" % (a, a) for a in range(dim))
    rows = lambda code: tuple(tuple(code if i == j else "0.0" for j in range(dim)) for i in range(dim))      # noqa: E731
    sources = [Expression(rows("%s ? (1.0 + 0.5*x[0])*sin(150.0*t) : 0.0" % box), t=0), Expression(rows("%s ? 0.7 + x[0] : 0.0" % box)), None]
    sponges = [(4, "x[0] <= 0.4 ? 25.0 : 0.0"), (2, "x[0] >= 0.5 ? 10.0 + 20.0*x[0] : 0.0"), None]
    case = ls.Case(name, dim, P, n, "left", "f64", None, True, {}, None)
    pts = ls.receiver_points(case)[:-2]                    # the two outside the mesh: the solver class refuses them
    cell, phi = ls.receiver_basis(case, pts)
    assert (cell >= 0).all()
    h = min(1.0 / k for k in n)
    tol = 10 * tol_of(P, "left")
    for k, (dt, nsteps, every) in enumerate(((0.03 * h / P ** 2, 11, 1), (0.02 * h / P ** 2, 9, 2), (0.025 * h / P ** 2, 10, 3))):
        el.dt = orc.dt = dt
        if sponges[k] is None:
            el.absorption_function = None
            orc.E.absorb = None
        else:
            q, code = sponges[k]
            aex = Expression(code)
            el.absorption_function = Function(FunctionSpace(mesh, "DG", q))
            el.absorption = aex
            orc.E.set_absorption(aex.evaluate(om.node_coords(q)).reshape(nc, -1), q)
        sx = sources[k]
        if sx is None:
            el.source_expression = el.source_function = None
            orc.source = None
        else:
            el.source_expression = sx
            el.source_function = Function(el.S)
            el.source = sx

            def osource(t, sx=sx):
                if "t" in getattr(sx, "_params", {}):
                    sx.t = t
                return sx.evaluate(Xo).reshape(nc, -1, dim, dim)
            orc.source = osource
        el.set_receivers(pts, every=every, fields=("velocity", "stress"))
        u1, s1 = el.run(nsteps * dt * (1 + 1e-9))
        assert el.block.counters()["steps"] == sum((11, 9, 10)[:k + 1])
        want_u, want_s = [], []
        for j in range(nsteps):
            orc.step((j + 1) * dt)                    # every run() starts again at t = dt (elastic.py:279)
            if (j + 1) % every == 0:
                want_u.append([phi[r] @ orc.u1[cell[r]] for r in range(len(pts))])
                want_s.append([np.tensordot(phi[r], orc.s1[cell[r]], axes=(0, 0)) for r in range(len(pts))])
        eu, es = rel_field_error(u1.dat.data_cells, orc.u1), rel_field_error(s1.dat.data_cells, orc.s1)
        print("LIFETIME solver %s run %d: %.3e %.3e of %.1e" % (name, k, eu, es, tol))
        assert max(eu, es) < tol, (name, k, eu, es)
        t, tr = el.receiver_traces()
        assert np.allclose(t, [(j + 1) * dt for j in range(nsteps) if (j + 1) % every == 0], rtol=1e-12, atol=0)
        leb = np.abs(phi).sum(axis=1).max()
        assert tr["velocity"].shape == np.shape(want_u) and tr["stress"].shape == np.shape(want_s)
        assert np.abs(tr["velocity"] - want_u).max() < tol * leb * np.abs(orc.u1).max(), (name, k)
        assert np.abs(tr["stress"] - want_s).max() < tol * leb * np.abs(orc.s1).max(), (name, k)
    el.block.close()
