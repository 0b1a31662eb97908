"""The monitor: L2 norms and elastic energy taken on the device inside the time loop (include/seigen_hip.h sg_measure /
sg_set_monitor / sg_get_monitor; kernels_measure.hip).  Every layout and storage mode against the oracle's norm of the
downloaded fields, bitwise equality across the ways a step can be driven, beside receivers and a source in the same graphs,
the all-or-nothing rules, a split block against the single one, and the energy of the reference's 2-D eigenmode through
the solver class against the oracle's state step by step."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import harness as oharness  # noqa: E402
from oracle import mesh as omesh  # noqa: E402
from oracle import refelem  # noqa: E402
from seigen_amd import _lib  # noqa: E402
from seigen_amd.backend import HipBlock  # noqa: E402

from test_receivers_gpu import FAMILIES, make_case, receiver_points  # noqa: E402

# the receivers' thirteen rows, and: the FP32 P3 block of the 3-D matrix-pipe layout and an FP32 2-D tile block (kernel
# objects of their own); a lane block
# of more than 64 cubes that is no multiple of 64; a 2-D tile block of 288 items = 72 chunks; a generic block of 1030 items
# = 258 chunks, more than the 256 threads of pass 2
ROWS = FAMILIES + [
    ("mfma-P3-f32", 3, 3, (4, 3, 2), "left", "f32", None, True),
    ("tile-tri-P3-f32", 2, 3, (5, 3), "left", "f32", None, True),
    ("lane-2d-77", 2, 2, (11, 7), "left", "f64", "lane", True),
    ("tile-tri-P1-48x48", 2, 1, (48, 48), "left", "f64", None, True),
    ("generic-1d-P1-1030", 1, 1, (1030,), "left", "f64", None, True),
]
ROW = {r[0]: r for r in ROWS}
SMALL = ["generic-2d-P2", "tile-tri-P3", "mfma-P4-sym", "hexm-DQ3"]


def _block(spec, monkeypatch, graph=None):
    name, dim, degree, n, diagonal, dtype, path, sym = spec
    if path:
        monkeypatch.setenv("SEIGEN_HIP_PATH", path)
    else:
        monkeypatch.delenv("SEIGEN_HIP_PATH", raising=False)
    if graph is None:
        monkeypatch.delenv("SEIGEN_HIP_GRAPH", raising=False)
    else:
        monkeypatch.setenv("SEIGEN_HIP_GRAPH", "1" if graph else "0")
    blk, dt = make_case(dim, degree, n, diagonal, dtype, sym)
    return blk


def physical_weights(dim, rho, lam, mu):
    return np.stack([rho / 2.0, 1.0 / (4.0 * mu), -lam / (4.0 * mu * (dim * lam + 2.0 * mu))], axis=-1)


def host_sample(dim, degree, n, diagonal, u, s, w):
    """{ U2, S2, T2, EK, ES } of downloaded fields: the norms from oracle.harness.l2_norm (the trace field built here), the
    energies from the same forms weighted cell by cell"""
    quad = diagonal == "quadrilateral"
    mesh = omesh.structured(dim, n, (1.0,) * dim, diagonal if not quad else "left", quadrilateral=quad)
    t = np.einsum('cnii->cn', s)
    U2 = oharness.l2_norm(mesh, degree, u) ** 2
    S2 = oharness.l2_norm(mesh, degree, s) ** 2
    T2 = oharness.l2_norm(mesh, degree, t[..., None]) ** 2
    xq, wq = refelem.el_quadrature(dim, 2 * degree, getattr(mesh, "kind", "simplex"))
    phi, _ = refelem.el_tabulate(dim, degree, xq, getattr(mesh, "kind", "simplex"))
    M = np.einsum('q,qa,qb->ab', wq, phi, phi)
    dj = np.abs(mesh.detJ)
    Qu = np.einsum('cak,ab,cbk->c', u, M, u)
    s2 = s.reshape(s.shape[0], s.shape[1], -1)
    Qs = np.einsum('cak,ab,cbk->c', s2, M, s2)
    Qt = np.einsum('ca,ab,cb->c', t, M, t)
    if w is None:
        return np.array([U2, S2, T2, 0.0, 0.0])
    w = np.broadcast_to(np.asarray(w, dtype=np.float64), (u.shape[0], 3))
    return np.array([U2, S2, T2, np.sum(dj * w[:, 0] * Qu), np.sum(dj * (w[:, 1] * Qs + w[:, 2] * Qt))])


@pytest.mark.parametrize("spec", ROWS, ids=[r[0] for r in ROWS])
def test_every_layout_measures_what_the_oracle_does(gpu, monkeypatch, spec):
    """sg_measure after a few steps (padding lanes and stale mirror lines then hold what the stage kernels leave there)
    against the oracle's norm of the downloaded fields: no weights, one physical triple, random per-cell weights with
    lambda, mu > 0.  1e-11 relative, the project's per-operator parity bound: the two sides differ in the order of
    summation only, over at most ~2e5 terms."""
    name, dim, degree, n, diagonal, dtype, path, sym = spec
    blk = _block(spec, monkeypatch)
    blk.step(3)
    u, s = blk.get_field(_lib.FIELD_U), blk.get_field(_lib.FIELD_S)
    rng = np.random.default_rng(7)
    rho, lam, mu = (rng.uniform(0.5, 2.0, blk.ncells) for _ in range(3))
    per_cell = physical_weights(dim, rho, lam, mu)
    scalar = physical_weights(dim, np.float64(1.3), np.float64(0.5), np.float64(0.25))
    for w in (None, scalar, per_cell):
        got = blk.measure(w)
        want = host_sample(dim, degree, n, diagonal, u, s, w)
        print(name, "none" if w is None else w.shape, got, np.abs(got - want) / np.maximum(np.abs(want), 1e-300))
        assert np.isfinite(got).all() and want[0] > 0 and want[1] > 0 and want[2] > 0
        if w is None:
            assert got[3] == 0.0 and got[4] == 0.0
        scale = np.abs(want)
        assert np.all(np.abs(got - want) <= 1e-11 * scale), (name, got, want)
    blk.close()


def _drive(blk, way, steps):
    if way in ("graph", "eager"):
        blk.step(steps)
    elif way == "timing":
        blk.enable_timing(True)
        blk.step(steps)
    elif way == "single":
        for _ in range(steps):
            blk.step(1)
    else:
        for _ in range(steps):
            for st in range(6):
                blk.run_stage(st)
            blk.end_step()


def _cell_weights(spec):
    """random per-cell weights (lambda, mu > 0) for the block of a row"""
    ncells = int(np.prod(spec[3])) * (1 if spec[4] == "quadrilateral" else {1: 1, 2: 2, 3: 6}[spec[1]])
    rho, lam, mu = (np.random.default_rng(7).uniform(0.5, 2.0, (3, ncells)))
    return physical_weights(spec[1], rho, lam, mu)


@pytest.mark.parametrize("name", SMALL)
@pytest.mark.parametrize("every", [1, 3])
def test_trace_bitwise_across_the_ways_of_stepping(gpu, monkeypatch, name, every):
    """11 steps - the 8-step graph, the 1-step graph and, with every = 3, steps inside a replay that are no sample steps -
    as graph replay, eager launches, eager launches with timing on, sg_step(1) repeated and sg_run_stage x 6 + sg_end_step:
    one trace, bit for bit; and sample j is sg_measure of a twin handle stepped `every` steps at a time.  The monitor is
    armed with one triple of weights, on the rows mfma-P4-sym and tile-tri-P3 with random per-cell weights."""
    spec, steps = ROW[name], 11
    w = physical_weights(spec[1], np.float64(1.3), np.float64(0.5), np.float64(0.25))
    if name in ("mfma-P4-sym", "tile-tri-P3"):
        w = _cell_weights(spec)
    out = {}
    for way in ("graph", "eager", "timing", "single", "stages"):
        blk = _block(spec, monkeypatch, graph=(way != "eager"))
        blk.set_monitor(every, steps // every, w)
        _drive(blk, way, steps)
        out[way] = blk.get_monitor()
        assert blk.counters()["steps"] == steps
        blk.close()
    assert out["graph"].shape == (steps // every, 5) and np.all(out["graph"][:, :4] > 0)
    assert w.ndim == 1 or len({tuple(r) for r in w}) > 1
    for way in ("eager", "timing", "single", "stages"):
        assert np.array_equal(out[way], out["graph"]), way
    twin = _block(spec, monkeypatch, graph=True)
    for j in range(steps // every):
        twin.step(every)
        assert np.array_equal(twin.measure(w), out["graph"][j]), j
    twin.close()


@pytest.mark.parametrize("name", SMALL)
def test_monitor_beside_receivers_and_a_source(gpu, monkeypatch, name):
    """Monitor and receivers armed together (the source of make_case is active throughout): both traces equal, bit for
    bit, the ones of a run with each armed alone - graph replay and eager launches."""
    spec, steps, every = ROW[name], 11, 2
    pts, _ = receiver_points(spec[1], spec[3])
    w = physical_weights(spec[1], np.float64(1.0), np.float64(0.5), np.float64(0.25))
    for graph in (True, False):
        got = {}
        for arm in ("both", "monitor", "receivers"):
            blk = _block(spec, monkeypatch, graph=graph)
            if arm != "receivers":
                blk.set_monitor(every, steps // every, w)
            if arm != "monitor":
                blk.set_receivers(pts, 3, 3, steps // 3)
            blk.step(steps)
            got[arm] = (blk.get_monitor() if arm != "receivers" else None, blk.get_receivers() if arm != "monitor" else None)
            blk.close()
        assert got["both"][0].shape == (steps // every, 5) and got["both"][1].shape[0] == steps // 3
        assert np.array_equal(got["both"][0], got["monitor"][0]) and np.array_equal(got["both"][1], got["receivers"][1])
        assert np.abs(got["both"][1]).max() > 0 and np.all(got["both"][0][:, 0] > 0)


def _set(blk, every, capacity, w=None, per_cell=0):
    return blk.lib.sg_set_monitor(blk.h, every, capacity, None if w is None else w.ctypes.data, per_cell)


def test_monitor_calls_are_all_or_nothing(gpu, monkeypatch):
    spec = ROW["mfma-P4-sym"]
    w = physical_weights(3, np.float64(1.0), np.float64(0.5), np.float64(0.25))
    # an unarmed handle, and one that was armed and disarmed, are a handle that never saw the monitor
    never, blk, twin = (_block(spec, monkeypatch) for _ in range(3))
    never.step(9)
    blk.set_monitor(1, 4, w)
    blk.set_monitor(0, 0)
    assert blk.get_monitor().shape == (0, 5)
    blk.step(9)
    assert blk.counters()["launches"] == never.counters()["launches"] and blk.counters()["steps"] == 9
    assert [blk.stage_kernel_name(st) for st in range(6)] == [never.stage_kernel_name(st) for st in range(6)]
    for f in (_lib.FIELD_U, _lib.FIELD_S):
        assert np.array_equal(blk.get_field(f), never.get_field(f))
    never.close()
    twin.step(9)
    for b in (blk, twin):
        b.set_monitor(1, 4, w)
        b.step(3)
    before = blk.get_monitor()
    assert before.shape == (3, 5)
    # sg_step whose samples would overflow: refused before anything is queued (graph replay and eager alike)
    for n in (2, 5):
        assert blk.lib.sg_step(blk.h, n) == -3
    assert blk.counters()["steps"] == 12 and np.array_equal(blk.get_monitor(), before)
    for f in (_lib.FIELD_U, _lib.FIELD_S, _lib.FIELD_UH, _lib.FIELD_SH):
        assert np.array_equal(blk.get_field(f), twin.get_field(f)), f
    # bad arguments: SG_ERR_ARG, the monitor armed before keeps recording
    assert _set(blk, -1, 4, w) == -1
    assert _set(blk, 1, 0, w) == -1
    assert _set(blk, 1, 4, None, 1) == -1
    assert blk.lib.sg_measure(blk.h, None, 1, np.zeros(5).ctypes.data) == -1
    buf = np.zeros(before.size + 1 + 5)
    ns = C.c_int64()
    assert blk.lib.sg_get_monitor(blk.h, buf.ctypes.data, buf.nbytes, C.byref(ns)) == -1
    blk.step(1)
    twin.step(1)
    assert np.array_equal(blk.get_monitor(), twin.get_monitor()) and blk.get_monitor().shape == (4, 5)
    # full: one more step is refused by sg_step and by sg_end_step (which does not count it)
    assert blk.lib.sg_step(blk.h, 1) == -3
    for st in range(6):
        blk.run_stage(st)
    assert blk.lib.sg_end_step(blk.h) == -3
    assert blk.counters()["steps"] == 13 and blk.get_monitor().shape == (4, 5)
    full = blk.get_monitor()
    # every = 0 disarms; the step in flight can then end
    blk.set_monitor(0, 0)
    assert blk.get_monitor().shape == (0, 5)
    blk.end_step()
    blk.step(9)
    assert blk.counters()["steps"] == 23 and np.all(full[:, 0] > 0)
    # re-arming discards the samples and counts steps from the arming call
    blk.set_monitor(2, 3, w)
    assert blk.get_monitor().shape == (0, 5)
    blk.step(3)
    assert blk.get_monitor().shape == (1, 5)
    blk.step(3)
    assert blk.get_monitor().shape == (3, 5)
    blk.close()
    twin.close()


@pytest.mark.parametrize("dim,degree,n,grid", [(2, 2, (6, 4), (2, 1)), (3, 3, (4, 3, 2), (2, 1, 1))])
def test_split_block_sums_to_the_single_block(gpu, dim, degree, n, grid):
    """A block split in two along x, stepped as test_harness_gpu.py test_multiblock_equals_single_block steps its blocks
    (FIRST, exchange, SECOND; sg_end_step): the sum of the two blocks' samples is the single block's to 1e-12 relative (the
    fields are equal bitwise; the sums are grouped differently, so the bits are not promised)."""
    torch = pytest.importorskip("torch")
    from seigen_amd.mesh import Partition
    from test_harness_gpu import _LocalExchange
    from util import seeded
    h = [1.0 / k for k in n]
    w = physical_weights(dim, np.float64(1.0), np.float64(0.5), np.float64(0.25))
    steps, every = 4, 2
    single = HipBlock(dim, degree, n, h, [0.0] * dim, "left")
    u0, s0 = seeded(single.field_shape(_lib.FIELD_U), 11), seeded(single.field_shape(_lib.FIELD_S), 12)
    s0 = 0.5 * (s0 + np.swapaxes(s0, -1, -2))
    dt = 0.02 * min(h) / degree ** 2
    single.set_params(1.0, dt, 0.5, 0.25)
    single.set_field(_lib.FIELD_U, u0)
    single.set_field(_lib.FIELD_S, s0)
    single.set_monitor(every, steps // every, w)
    single.step(steps)
    want = single.get_monitor()
    single.close()
    world = int(np.prod(grid))
    parts = [Partition(n, r, world, grid) for r in range(world)]
    ncls = {2: 2, 3: 6}[dim]
    blocks = []
    for p in parts:
        ax = [np.arange(p.start[a], p.start[a] + p.n[a]) for a in range(dim)]
        cube = (ax[0][None, :] + n[0] * ax[1][:, None]).reshape(-1) if dim == 2 else \
            (ax[0][None, None, :] + n[0] * (ax[1][None, :, None] + n[1] * ax[2][:, None, None])).reshape(-1)
        sel = (cube[:, None] * ncls + np.arange(ncls)[None, :]).reshape(-1)
        b = HipBlock(dim, degree, p.n, h, [p.start[a] * h[a] for a in range(dim)], "left", p.nbr_mask)
        b.set_params(1.0, dt, 0.5, 0.25)
        b.set_field(_lib.FIELD_U, u0[sel])
        b.set_field(_lib.FIELD_S, s0[sel])
        b.set_monitor(every, steps // every, w)
        blocks.append(b)
    _LocalExchange(blocks, parts).step(steps, True)
    got = sum(b.get_monitor() for b in blocks)
    for b in blocks:
        b.close()
    assert want.shape == (steps // every, 5) and np.all(want[:, :4] > 0)
    scale = np.abs(want)
    print(np.abs(got - want) / scale)
    assert np.all(np.abs(got - want) <= 1e-12 * scale)


def _state_floor():
    with open(os.path.join(ROOT, "tests", "golden", "lifetime_floor.json")) as f:
        return max(max(v) for v in json.load(f).values())


def test_energy_of_the_eigenmode_through_the_solver_class(gpu):
    """test_oracle_pins.py test_energy_is_conserved_by_lf4's problem (2-D eigenmode, N = 8, P2, dt = 0.25 / 8, 362 steps)
    through ElasticLF4.set_monitor(1) / run: `energy` at every step equals the oracle's formula on OracleLF4's state at that
    step within twice the round-off floor of the state that tests/test_lifetime_oracle.py measures between two references
    (tests/golden/lifetime_floor.json, its largest figure 3.954e-14: the energy is quadratic in the state); the trace passes
    the oracle test's own thresholds; and with dt four times larger the blow-up shows in the trace alone.
    The test prints the largest relative difference of the energy before it asserts.  Observed on an MI355X: 9.113e-16
    over the 362 steps, against the tolerance 7.908e-14; the unstable run's energy goes from 1.343 to NaN within 90 steps."""
    from seigen_amd.harness.eigenmode import Eigenmode2DLF4
    N, P, dt, steps = 8, 2, 0.25 / 8, 362
    em = Eigenmode2DLF4(N, P, dt, output=False)
    em.elastic.set_monitor(1)
    em.eigenmode2d(T=(steps + 0.5) * dt)
    t, tr = em.elastic.monitor_trace()
    e = tr["energy"]
    assert e.shape == (steps,) and abs(t[-1] - steps * dt) < 1e-9
    assert np.allclose(tr["kinetic"] + tr["strain"], e, rtol=1e-15)
    one = em.elastic.energy()
    assert one["energy"] == e[-1] and one["u_l2"] == tr["u_l2"][-1] and one["s_l2"] == tr["s_l2"][-1]

    om = oharness.Eigenmode2D(N, P, dt)
    el = om.elastic
    X = el.node_coords()
    el.u0 = om.u_exact(X, 0.0)
    el.s0 = om.s_exact(X, el.dt / 2)
    M = el.E.ops.M
    lam, mu = el.l, el.mu
    want = []
    for k in range(steps):
        el.step((k + 1) * el.dt)
        u, s = el.u0.reshape(-1, 2), el.s0.reshape(-1, 2, 2)
        ek = 0.5 * sum(u[:, i] @ (M @ u[:, i]) for i in range(2))
        trc = s[:, 0, 0] + s[:, 1, 1]
        es = 0.0
        for i in range(2):
            for j in range(2):
                eij = (s[:, i, j] - (lam / (2 * (lam + mu)) * trc if i == j else 0.0)) / (2 * mu)
                es += 0.5 * (s[:, i, j] @ (M @ eij))
        want.append(ek + es)
    want = np.array(want)
    rel = np.abs(e - want) / want
    tol = 2.0 * _state_floor()
    print("energy against the oracle: max relative difference %.3e (tolerance %.3e)" % (rel.max(), tol))
    assert rel.max() <= tol
    per = [e[i * 181:(i + 1) * 181].mean() for i in range(2)]
    assert abs(per[1] - per[0]) / per[0] < 1e-4
    assert e.std() / e.mean() < 5e-2

    bad = Eigenmode2DLF4(N, P, 4 * dt, output=False)
    bad.elastic.set_monitor(1)
    bad.eigenmode2d(T=(steps // 4 + 0.5) * 4 * dt)
    _, trb = bad.elastic.monitor_trace()
    eb = trb["energy"]
    print("unstable run: energy %.3e -> %.3e over %d steps" % (eb[0], eb[-1], len(eb)))
    assert len(eb) == steps // 4 and (not np.isfinite(eb).all() or eb[-1] > 10.0 * eb[0])
