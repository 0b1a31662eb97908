"""The gauges on the GPU (include/seigen_hip.h sg_set_gauges / sg_get_gauges / sg_probe_gradient; seigen_amd/csrc/gauge.cpp,
kernels_gauge.hip): the broken gradient of the velocity, its divergence, curl and symmetric part at physical points - once
behind everything queued, or recorded inside the time loop by the sixth end-of-step hook.

ROWS: those of tests/test_grad_gpu.py (grad_cases.rows(): every family, f32, padding lanes in the first and last group, the
125-node hexahedron), blocks with unequal h.  The reference is the restatement tests/gauge_cases.py gauge_reference over the
tables the library exports (tests/test_gauges_host.py holds it against analytic gradients), the bound
|device - restatement| <= 4 (nd + dim) 2^-53 A, A_ij = sum_r |J_rj| sum_a |D_r[a]| |u[a][i]|: both sides are sums of nd + dim
rounded products over the same tables - fma chains on the device, numpy's sums in the restatement - and each lies within
gamma_(nd + dim) A of the exact sum; kinds 1 to 3 take the sum of the A of the entries they combine.  FP32 blocks convert first.

1 test_probe_against_the_restatement: every row, 32 points (interior, on faces, edges and vertices of cubes, one outside), all
  kinds, both velocity fields; rows not owned exactly 0.0; fields, counters and storage mode untouched.
2 test_probe_at_a_node: a gauge at a DG node against sg_get_gradient at that node of the cell that owns the point, within
  8 (nd + dim) 2^-53 A (different summation sets on tensor-product cells, and a located xi: not bitwise).
3 test_series_against_the_restatement: one row per layout; six sg_step(1) with u1 downloaded after each, every = 2, within the
  bound; then bitwise the same trace from sg_step(6) under graph replay, eager launches with timing on, and host-driven stages
  ending in sg_end_step.
4 test_refusal_and_arming, test_other_hooks_are_untouched, test_never_armed_is_the_plain_step.
5 test_split_block: two ranks over tests/fake_rccl, a point on the cut: the merged traces and probes bitwise the single block's.
6 test_solver_class: ElasticLF4.set_gauges / gauge_traces, set_fibre / fibre_traces and Function.gradient_at on the 2-D
  explosive source.

Measured on an MI355X, the largest |device - restatement| / (2^-53 A) of test 1 over both fields and all kinds, against the
bound's factor 4 (nd + dim): mfma-P4-sym 1.74 of 152, mfma-P3-sym 2.44 of 92, tile-tri-P3 2.96 of 48, tile-quad-P2 2.02 of 44,
hexm-DQ3 2.18 of 268, lane-2d-P2 2.11 of 32, generic-2d-P2 2.64 of 32, mfma-P3-f32 2.64 of 92, tile-tri-P3-f32 1.95 of 48,
lane-1d-P2 2.42 of 16, hexm-DQ4 2.96 of 512, lane-2d-P2-wide 2.54 of 32.  Test 2, |gauge - nodal gradient| / (2^-53 A) against
8 (nd + dim): at most 51.88 of 88 (tile-quad-P2), 37.40 of 1024 (hexm-DQ4), 20.59 of 96 (tile-tri-P3); 0.00 on mfma-P4-sym and
generic-2d-P2, whose random nodes were located in their own cells at the lattice's own xi.  Test 3: at most 1.83 of 32.

Seeded faults in scratch builds of the library, run through tests 1 to 4 on an MI355X:
  J transposed (Jk[jj * 3 + r])       fails tests 1, 2 and 3 and test_other_hooks_are_untouched on the three 3-D simplex rows
                                      (mfma-P4-sym, mfma-P3-sym, mfma-P3-f32), whose classes have a non-symmetric J; passes the
                                      others: the J of triangles, intervals and tensor-product cells is diagonal.
  the hook's counter not set before   fails test_refusal_and_arming with graph replay on both rows (the sample of a replay
  a replay (stages.cpp replay_steps)  behind an eager step is never written); passes with SEIGEN_HIP_GRAPH=0 and everywhere a
                                      handle only ever replays, where the counter happens to be right.
  a descending in the chain           NOT caught: every test passes.  Both orders lie within the bound, and all ways of
                                      stepping share the kernel, so the bitwise comparisons agree with each other.  The order
                                      of the header is held by the code alone; a test that predicts the bits (an exactly
                                      rounded fma chain on the host) is what would pin it.
  the upper cell on a grid line       seen on the CPU only: tests/test_gauges_host.py shows that the restatement at a point on
                                      a grid line differs from the upper cell's polynomial by more than 1e-3 of the scale.
One real defect was found by test_split_block: the one-shot's zero fill of its temporary trace ran on the null stream and could
land after the kernel on the handle's non-blocking stream (a probe row of zeros, once in three runs); the fill is now queued
on the handle's stream."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from seigen_amd import _lib  # noqa: E402
from seigen_amd.backend import HipBlock, locate_points  # noqa: E402
from tests import gauge_cases as gk  # noqa: E402
from tests import grad_cases as gc  # noqa: E402

SWITCHES = ("SEIGEN_HIP_PATH", "SEIGEN_HIP_GRAPH", "SEIGEN_HIP_SPONGE_AFFINE", "SEIGEN_HIP_SYM", "SEIGEN_HIP_SOURCE_LAUNCH",
            "SEIGEN_HIP_XCORR", "SEIGEN_HIP_OVERLAP", "SEIGEN_HIP_PLAIN_COPY", "SEIGEN_HIP_GRID_BLOCKS")
ROWS = gc.rows()
ROW = {r[0]: r for r in ROWS}
IDS = [r[0] for r in ROWS]
EPS = 2.0 ** -53
FIELDS = (_lib.FIELD_U, _lib.FIELD_S, _lib.FIELD_UH, _lib.FIELD_SH)
LAYOUT_ROWS = ["mfma-P4-sym", "mfma-P3-f32", "tile-tri-P3", "tile-quad-P2", "hexm-DQ3", "lane-2d-P2", "generic-2d-P2"]
_CASES = {}


def _env(monkeypatch, row, graph=None):
    for var in SWITCHES:
        monkeypatch.delenv(var, raising=False)
    if row[6]:
        monkeypatch.setenv("SEIGEN_HIP_PATH", row[6])
    if graph is not None:
        monkeypatch.setenv("SEIGEN_HIP_GRAPH", graph)


def _block(row):
    name, dim, degree, n, diagonal, dtype, path = row
    h = gk.row_h(row)
    blk = HipBlock(dim, degree, n, h, [0.0] * dim, diagonal, dtype=dtype)
    blk.set_params(1.0, 0.1 * min(h) / degree ** 2, 0.5, 0.25)
    return blk


def _kinds(dim):
    return [k for k in (0, 1, 2, 3) if not (k == 2 and dim == 1)]


def _case(row):
    """the configuration of the row's block, 32 points - random interior ones, points on faces, edges and vertices of cubes,
    the block's upper corner, one point outside - and two random velocity fields of order one (exact in float for an f32
    row): computed once per row and left unchanged"""
    key = row[:6]
    if key not in _CASES:
        name, dim, degree, n, diagonal, dtype = key
        cfg = gk.row_cfg(row)
        rng = np.random.default_rng(2000 + len(_CASES))
        special = 3 * len({1, min(2, dim), dim}) + 2
        pts = gk.sample_points(cfg, rng, ninterior=32 - special)
        assert len(pts) == 32
        ncls = 1 if diagonal == "quadrilateral" else gc.NCLS[dim]
        nd = len(gc.lattice(1 if diagonal == "quadrilateral" else 0, dim, degree))
        u = {}
        for f in (_lib.FIELD_U, _lib.FIELD_UH):
            x = rng.uniform(-1, 1, (int(np.prod(n)) * ncls, nd, dim))
            u[f] = x.astype(np.float32).astype(np.float64) if dtype == "f32" else x
            u[f].setflags(write=False)
        pts.setflags(write=False)
        _CASES[key] = dict(cfg=cfg, pts=pts, u=u, nd=nd)
    return _CASES[key]


def _counts(blk):
    c = blk.counters()
    return c["launches"], c["steps"], c["halo_pack_launches"], c["halo_bytes_packed"]


def _smooth_block(row):
    """a block of the row with a smooth non-zero start (a symmetric stress)"""
    blk = _block(row)
    dim = row[1]
    X = blk.node_coords()
    u = np.stack([np.sin(2 * X[..., 0] + i) * np.cos(X[..., -1] - i) for i in range(dim)], axis=-1)
    s = np.zeros(X.shape[:-1] + (dim, dim))
    for i in range(dim):
        for j in range(dim):
            s[..., i, j] = np.cos(X[..., 0] + 0.5 * (i + j)) * (1 + X[..., -1])
    blk.set_field(_lib.FIELD_U, u)
    blk.set_field(_lib.FIELD_S, s)
    return blk


# ---- 1. the probe against the restatement ------------------------------------------------------------------------------------

@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_probe_against_the_restatement(gpu, monkeypatch, row):
    _env(monkeypatch, row)
    case = _case(row)
    cfg, pts, nd = case["cfg"], case["pts"], case["nd"]
    dim = row[1]
    blk = _block(row)
    try:
        assert blk.nd == nd
        for f in (_lib.FIELD_U, _lib.FIELD_UH):
            blk.set_field(f, case["u"][f])
            assert np.array_equal(blk.get_field(f), case["u"][f])          # the block holds these values exactly
        before = [blk.get_field(f) for f in FIELDS]
        sym, counters = blk.is_sym(), _counts(blk)
        cell, _ = locate_points(cfg, pts)
        assert cell[-1] == -1 and (cell[:-1] >= 0).all()
        for f in (_lib.FIELD_U, _lib.FIELD_UH):
            for kind in _kinds(dim):
                got, owned = blk.probe_gradient(f, kind, pts)
                assert got.shape == (32, gc.ncomp_of(dim, kind)) and np.array_equal(owned, cell >= 0)
                ratio, factor, exact = gk.ratio_and_factor(cfg, pts, case["u"][f], kind, got, nd)
                print("%s field %d kind %d: largest |device - restatement| / (2^-53 A) = %.2f, bound %d" % (row[0], f, kind, ratio, factor))
                assert ratio <= factor, (f, kind)
                assert exact and (got[-1] == 0.0).all(), (f, kind)         # the point outside: exactly 0.0
                assert np.abs(got[:-1]).max() > 1e-3
        for f, x in zip(FIELDS, before):
            assert np.array_equal(blk.get_field(f), x), f
        assert blk.is_sym() == sym and _counts(blk) == counters
    finally:
        blk.close()


# ---- 2. the probe at a node ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_probe_at_a_node(gpu, monkeypatch, row):
    """16 random DG nodes: the point of node a of cell c is owned by a cell c' (c itself, or the lower one where the node lies
    on a grid line or on a diagonal) that has a node a' there too; the gauge equals sg_get_gradient at (c', a') within
    8 (nd + dim) 2^-53 A"""
    _env(monkeypatch, row)
    case = _case(row)
    cfg, nd = case["cfg"], case["nd"]
    dim = row[1]
    blk = _block(row)
    try:
        u = case["u"][_lib.FIELD_U]
        blk.set_field(_lib.FIELD_U, u)
        X = blk.node_coords()
        rng = np.random.default_rng(77)
        cells, nodes = rng.integers(0, blk.ncells, 16), rng.integers(0, nd, 16)
        pts = X[cells, nodes]
        own, _ = locate_points(cfg, pts)
        assert (own >= 0).all()
        dist = np.abs(X[own] - pts[:, None, :]).max(axis=-1)               # [16, nd]
        at = dist.argmin(axis=1)
        assert (dist[np.arange(16), at] <= 1e-12).all()
        G = blk.get_gradient(_lib.FIELD_U, 0)[own, at].reshape(16, dim * dim)
        got, owned = blk.probe_gradient(_lib.FIELD_U, 0, pts)
        assert owned.all()
        A = gk.scale_of(gk.gauge_parts(cfg, pts, u)[2], 0)
        ratio = float((np.abs(got - G) / (EPS * A)).max())
        print("%s: largest |gauge - nodal gradient| / (2^-53 A) = %.2f, bound %d" % (row[0], ratio, 8 * (nd + dim)))
        assert ratio <= 8 * (nd + dim)
    finally:
        blk.close()


# ---- 3. the series -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", LAYOUT_ROWS)
def test_series_against_the_restatement(gpu, monkeypatch, name):
    row = ROW[name]
    case = _case(row)
    cfg, pts, nd = case["cfg"], case["pts"], case["nd"]
    dim = row[1]
    kind = (3, 0, 1, 2)[LAYOUT_ROWS.index(name) % 4]
    steps, every = 6, 2
    out = {}
    for way in ("single", "graph", "timing", "stages"):
        _env(monkeypatch, row, "1" if way == "graph" else "0")
        blk = _smooth_block(row)
        try:
            owned = blk.set_gauges(pts, kind, every, steps // every)
            assert np.array_equal(owned, locate_points(cfg, pts)[0] >= 0)
            assert blk.get_gauges().shape == (0, 32, gc.ncomp_of(dim, kind))
            if way == "single":
                fields = []
                for _ in range(steps):
                    blk.step(1)
                    fields.append(blk.get_field(_lib.FIELD_U))
            elif way == "graph":
                blk.step(steps)
            elif way == "timing":
                blk.enable_timing(True)
                blk.step(steps)
            else:
                for _ in range(steps):
                    for st in range(6):
                        blk.run_stage(st)
                    blk.end_step()
            out[way] = blk.get_gauges()
            assert blk.counters()["steps"] == steps
        finally:
            blk.close()
    tr = out["single"]
    assert tr.shape == (steps // every, 32, gc.ncomp_of(dim, kind)) and np.abs(tr).max() > 1e-3
    for j in range(steps // every):
        u1 = fields[(j + 1) * every - 1]
        ratio, factor, exact = gk.ratio_and_factor(cfg, pts, u1, kind, tr[j], nd)
        print("%s kind %d sample %d: largest |device - restatement| / (2^-53 A) = %.2f, bound %d" % (name, kind, j, ratio, factor))
        assert ratio <= factor and exact, j
    assert not np.array_equal(tr[0], tr[1])
    for way in ("graph", "timing", "stages"):
        assert np.array_equal(out[way], tr), way


# ---- 4. refusal and arming -------------------------------------------------------------------------------------------------------

def _set(blk, pts, kind, every, capacity, npts=None):
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    return blk.lib.sg_set_gauges(blk.h, len(pts) if npts is None else npts, pts.ctypes.data, kind, every, capacity, None)


@pytest.mark.parametrize("graph", ["1", "0"])
@pytest.mark.parametrize("name", ["tile-tri-P3", "lane-1d-P2"])
def test_refusal_and_arming(gpu, monkeypatch, name, graph):
    row = ROW[name]
    _env(monkeypatch, row, graph)
    case = _case(row)
    pts, dim = case["pts"], row[1]
    ncomp = gc.ncomp_of(dim, 3)
    blk, twin = _smooth_block(row), _smooth_block(row)
    try:
        for b in (blk, twin):
            b.set_gauges(pts, 3, 2, 2)
        # capacity 2 with every = 2: the samples of steps 2 and 4 fit, the one of step 6 does not - by the receivers' rule a call
        # is refused when (steps + n) / every > capacity, before anything is queued
        before = [blk.get_field(f) for f in FIELDS]
        counters = _counts(blk)
        assert blk.lib.sg_step(blk.h, 6) == -3 and b"gauge" in blk.lib.sg_last_error(blk.h)
        assert _counts(blk) == counters and blk.get_gauges().shape[0] == 0
        for f, x in zip(FIELDS, before):
            assert np.array_equal(blk.get_field(f), x), f
        for b in (blk, twin):
            b.step(4)
        assert blk.lib.sg_step(blk.h, 5) == -3                              # the samples of steps 6 and 8: no room
        assert blk.lib.sg_step(blk.h, 2) == -3
        full = blk.get_gauges()
        assert full.shape == (2, 32, ncomp) and np.array_equal(full, twin.get_gauges()) and np.abs(full).max() > 1e-3
        for f in FIELDS:
            assert np.array_equal(blk.get_field(f), twin.get_field(f)), f
        blk.step(1)                                                        # step 5 takes no sample: accepted
        twin.step(1)
        for st in range(6):
            blk.run_stage(st)
        assert blk.lib.sg_end_step(blk.h) == -3 and blk.counters()["steps"] == 5      # step 6 is due a sample: refused, not counted
        # bad arguments: SG_ERR_ARG, and the gauges armed before keep their samples
        assert _set(blk, pts, 4, 1, 4) == -1 and _set(blk, pts, -1, 1, 4) == -1
        assert _set(blk, pts, 3, 0, 4) == -1 and _set(blk, pts, 3, 1, -1) == -1 and _set(blk, pts, 3, 1, 4, npts=-1) == -1
        assert blk.lib.sg_set_gauges(blk.h, 3, None, 3, 1, 4, None) == -1
        if dim == 1:
            assert _set(blk, pts, 2, 1, 4) == -1
        host = np.zeros(32 * 9)
        p = np.ascontiguousarray(pts)

        def probe(field=_lib.FIELD_U, kind=3, nbytes=32 * ncomp * 8, out=host.ctypes.data):
            return blk.lib.sg_probe_gradient(blk.h, field, kind, 32, p.ctypes.data, out, nbytes, None)
        assert probe() == 0
        assert probe(field=_lib.FIELD_S) == -1 and probe(field=_lib.FIELD_SH) == -1 and probe(field=4) == -1
        assert probe(kind=4) == -1 and probe(nbytes=32 * ncomp * 8 - 8) == -1 and probe(nbytes=32 * ncomp * 8 + 8) == -1 and probe(out=None) == -1
        if dim == 1:
            assert probe(kind=2, nbytes=32 * 8) == -1
        import ctypes
        n = ctypes.c_int64()
        buf = np.zeros((2, 32, ncomp))
        assert blk.lib.sg_get_gauges(blk.h, buf.ctypes.data, buf.nbytes - 8, ctypes.byref(n)) == -1
        assert blk.lib.sg_get_gauges(blk.h, buf.ctypes.data, buf.nbytes + 8, ctypes.byref(n)) == -1
        assert blk.lib.sg_get_gauges(blk.h, buf.ctypes.data, buf.nbytes, ctypes.byref(n)) == 0 and n.value == 2
        assert np.array_equal(buf, full)
        # re-arming discards the samples and counts steps from the arming call; no points disarm
        blk.set_gauges(pts, 1, 3, 2)
        assert blk.get_gauges().shape == (0, 32, 1)
        blk.end_step()                                                     # the stages of step 6 were queued above: it ends here
        blk.step(2)
        assert blk.get_gauges().shape == (1, 32, 1) and np.abs(blk.get_gauges()).max() > 1e-3      # (a replay behind an eager step)
        blk.set_gauges(np.zeros((0, dim)))
        assert blk.get_gauges().shape == (0, 0, 0)
        blk.step(7)
        assert blk.counters()["steps"] == 15 and blk.get_gauges().shape == (0, 0, 0)
    finally:
        blk.close()
        twin.close()


@pytest.mark.parametrize("name", ["mfma-P4-sym", "tile-tri-P3"])
def test_other_hooks_are_untouched(gpu, monkeypatch, name):
    """receivers, monitor, spectra, peak maps, injectors and gauges armed together against the same without gauges: every
    other hook's output and the four fields are bitwise the same; the gauges' last sample is the restatement of the final u1
    (the injectors' series ends a step earlier)"""
    row = ROW[name]
    _env(monkeypatch, row)
    case = _case(row)
    cfg, pts, nd, dim = case["cfg"], case["pts"], case["nd"], row[1]
    steps = 8
    rng = np.random.default_rng(9)
    series = 1e-2 * rng.uniform(-1, 1, (steps - 1, 4, dim))
    w = np.exp(-2j * np.pi * np.outer(np.arange(4), [0.1, 0.3]))
    res = {}
    for with_gauges in (True, False):
        blk = _smooth_block(row)
        try:
            blk.set_receivers(pts[:5], 3, 2, 4)
            if with_gauges:
                blk.set_gauges(pts, 0, 1, steps)
            blk.set_monitor(1, steps)
            blk.set_spectra(wu=w, ws=w, every=2)
            blk.set_peaks(3, 1, steps)
            blk.set_injectors(pts[:4], series, 1)
            blk.step(3)
            blk.step(steps - 3)
            res[with_gauges] = dict(rec=blk.get_receivers(), mon=blk.get_monitor(), peaks=[blk.get_peaks(k) for k in (0, 1)],
                                    spc=[blk.get_spectrum(k, f) for k in (0, 1) for f in (0, 1)], fields=[blk.get_field(f) for f in FIELDS],
                                    sym=blk.is_sym())
            if with_gauges:
                tr = blk.get_gauges()
        finally:
            blk.close()
    a, b = res[True], res[False]
    assert a["rec"].shape[0] == 4 and np.array_equal(a["rec"], b["rec"]) and np.array_equal(a["mon"], b["mon"]) and a["sym"] == b["sym"]
    for x, y in zip(a["peaks"], b["peaks"]):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])
    for x, y in zip(a["spc"] + a["fields"], b["spc"] + b["fields"]):
        assert np.array_equal(x, y)
    assert tr.shape == (steps, 32, dim * dim)
    ratio, factor, exact = gk.ratio_and_factor(cfg, pts, a["fields"][0], 0, tr[-1], nd)
    print("%s: last sample against the final u1: %.2f of %d" % (name, ratio, factor))
    assert ratio <= factor and exact


@pytest.mark.parametrize("graph", ["1", "0"])
def test_never_armed_is_the_plain_step(gpu, monkeypatch, graph):
    """a block that armed gauges and disarmed them again steps like one that never did: the same stage kernels, the same fields"""
    row = ROW["tile-tri-P3"]
    _env(monkeypatch, row, graph)
    pts = _case(row)["pts"]
    plain, blk = _smooth_block(row), _smooth_block(row)
    try:
        names = [blk.stage_kernel_name(st) for st in range(6)]
        blk.set_gauges(pts, 3, 1, 8)
        assert [blk.stage_kernel_name(st) for st in range(6)] == names == [plain.stage_kernel_name(st) for st in range(6)]
        for b in (plain, blk):
            b.step(4)
        blk.set_gauges(np.zeros((0, 2)))
        for b in (plain, blk):
            b.step(4)
        for f in FIELDS:
            assert np.array_equal(blk.get_field(f), plain.get_field(f)), f
        assert _counts(blk) == _counts(plain)
    finally:
        plain.close()
        blk.close()


# ---- 5. a split block -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fake():
    from fake_rccl.build import build
    return build()


def _fake_env(fake, tmp_path, **extra):
    env = dict(os.environ, SEIGEN_RCCL_LIB=fake, FAKE_RCCL_TIMEOUT_S="60", FAKE_RCCL_LOG=str(tmp_path / "fake"),
               HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2")
    env.pop("FAKE_RCCL_HOST", None)
    for var in SWITCHES:
        env.pop(var, None)
    env.update(extra)
    return env


@pytest.mark.parametrize("grid,n,degree,kind", [((2, 1), (72, 6), 3, 3), ((1, 1, 2), (16, 4, 4), 4, 2)], ids=["2d-tile-P3", "3d-mfma-P4"])
def test_split_block(gpu, fake, tmp_path, monkeypatch, grid, n, degree, kind):
    """two ranks driving the C-ABI with the exchange inside the library: gauges in the interior, on the cut, on the mesh's
    corners are owned exactly once, and the merged traces and probes equal the single block's bitwise"""
    from native_exchange_worker import setup_block
    for var in SWITCHES:
        monkeypatch.delenv(var, raising=False)
    dim, world, steps, every = len(n), 2, 6, 2
    axis = grid.index(2)
    rng = np.random.default_rng(3)
    pts = rng.uniform(0.05, 0.95, (8, dim))
    on_cut = rng.uniform(0.1, 0.9, (2, dim))
    on_cut[:, axis] = 0.5
    on_cut[1, (axis + 1) % dim] = 0.5                                       # ... and on a grid line across it
    pts = np.concatenate([pts, on_cut, np.zeros((1, dim)), np.ones((1, dim))])
    np.save(tmp_path / "points.npy", pts)
    env = _fake_env(fake, tmp_path, FAKE_RCCL_ASYNC="1", FAKE_RCCL_SLOT_BYTES="1048576")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "gauge_exchange_worker.py"), str(tmp_path), str(world), str(r),
                               ",".join(map(str, grid)), ",".join(map(str, n)), str(degree), str(steps), "left", "-", str(every), str(kind),
                               str(tmp_path / "points.npy")],
                              cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(world)]
    errs = []
    for p in procs:
        try:
            so, se = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            p.kill()
            so, se = p.communicate()
        if p.returncode != 0:
            errs.append(so[-1500:] + se[-3000:])
    assert not errs, "\n-----\n".join(errs)
    blk = HipBlock(dim, degree, n, [1.0 / n[a] for a in range(dim)], [0.0] * dim, "left", 0)
    try:
        setup_block(blk, n, degree, "plain")
        assert blk.set_gauges(pts, kind, every, steps // every).all()
        blk.step(steps)
        single = blk.get_gauges()
        probe, powned = blk.probe_gradient(_lib.FIELD_U, kind, pts)
    finally:
        blk.close()
    assert single.shape == (steps // every, len(pts), gc.ncomp_of(dim, kind)) and np.abs(single).max() > 0 and powned.all()
    assert np.array_equal(probe, single[-1])                                # the probe of the final field is the last sample
    owners = np.zeros(len(pts), dtype=int)
    merged, merged_probe = np.zeros_like(single), np.zeros_like(probe)
    for r in range(world):
        d = np.load(tmp_path / ("rank%d.npz" % r))
        assert int(d["steps"]) == steps
        own = d["owned"]
        owners += own
        assert np.array_equal(own, d["powned"]) and not d["traces"][:, ~own].any() and not d["probe"][~own].any()
        merged += d["traces"]
        merged_probe += d["probe"]
    assert np.all(owners == 1), owners
    assert np.array_equal(merged, single) and np.array_equal(merged_probe, probe)


# ---- 6. the solver class ----------------------------------------------------------------------------------------------------------

def test_solver_class(gpu, monkeypatch):
    """The 2-D explosive source (100 m x 50 m at h = 2.5, P2, dt = 1e-3, 60 steps).  Dilatation-rate gauges at DG nodes near the
    source, every 5th step: the last sample against Function.gradient("div") of the final field at those nodes - of the cell
    that owns each point - within 8 (nd + dim) 2^-53 A (test 2's bound), and Function.gradient_at bitwise the last sample.  A fibre
    below the surface: every channel's last sample against the strain-rate restatement of the downloaded final field at the
    fibre's points, combined with the same weights, within the weighted sum of the bounds of the entries it combines plus the
    rounding of the combination, sum_p w_p sum_ij |t_i t_j| (4 (nd + dim) 2^-53 A_ij + 8 2^-53 |E_ij|)."""
    for var in SWITCHES:
        monkeypatch.delenv(var, raising=False)
    import seigen_amd
    import seigen_amd.helpers as helpers
    import seigen_amd.harness.explosive_source as hx
    from seigen_amd.functionspace import block_config
    from seigen_amd.harness.explosive_source import ExplosiveSourceLF4
    monkeypatch.setattr(helpers, "log", lambda s: None)
    monkeypatch.setattr(seigen_amd.elastic, "log", lambda s: None)
    monkeypatch.setattr(hx, "log", lambda s: None)
    Lx, Ly, h, dt, nsteps, every = 100.0, 50.0, 2.5, 1e-3, 60, 5
    T = nsteps * dt * (1 + 1e-9)
    # gauges at nodes
    el = ExplosiveSourceLF4().setup(Lx, Ly, h, degree=2, dt=dt)
    blk = el.block
    cfg = block_config(el.mesh, el.degree)
    X = blk.node_coords()
    near = np.flatnonzero((np.abs(X[:, 0, 0] - 45.0) < 3.0) & (X[:, 0, 1] > 45.0))
    rng = np.random.default_rng(4)
    cells, nodes = rng.choice(near, 12), rng.integers(0, blk.nd, 12)
    pts = X[cells, nodes]
    el.set_gauges(pts, kind="dilatation", every=every)
    with pytest.raises(ValueError):
        el.set_gauges(pts, kind="strain")
    with pytest.raises(ValueError):
        el.set_gauges([[-5.0, 10.0]])
    el.run(T)
    t, tr = el.gauge_traces()
    assert tr.shape == (nsteps // every, 12) and len(t) == nsteps // every and abs(t[-1] - nsteps * dt) < 1e-9
    assert np.abs(tr[-1]).max() > 0.0
    own, _ = locate_points(cfg, pts)
    dist = np.abs(X[own] - pts[:, None, :]).max(axis=-1)
    at = dist.argmin(axis=1)
    assert (own >= 0).all() and (dist[np.arange(12), at] <= 1e-9).all()
    div = el.u1.gradient("div").cpu().numpy()[own, at]
    u1 = blk.get_field(_lib.FIELD_U)
    A = gk.scale_of(gk.gauge_parts(cfg, pts, u1)[2], 1)[:, 0]
    ratio = float((np.abs(tr[-1] - div)[A > 0] / (EPS * A[A > 0])).max())
    print("dilatation rate, last sample against the nodal divergence: %.2f of %d" % (ratio, 8 * (blk.nd + 2)))
    assert ratio <= 8 * (blk.nd + 2)
    got, owned = el.u1.gradient_at(pts, "div")
    assert owned.all() and got.shape == (12,) and np.array_equal(got, tr[-1])
    with pytest.raises(ValueError):
        el.s1.gradient_at(pts)
    blk.close()
    # a fibre
    el = ExplosiveSourceLF4().setup(Lx, Ly, h, degree=2, dt=dt)
    blk = el.block
    el.set_fibre((38.0, 46.3), (52.0, 44.1), nchannels=6, gauge_length=3.0, nq=4, every=every)
    el.run(T)
    t, ax = el.fibre_traces()
    tg, eps = el.gauge_traces()
    assert ax.shape == (nsteps // every, 6) and eps.shape == (nsteps // every, 24, 2, 2) and np.array_equal(t, tg)
    assert np.abs(ax[-1]).max() > 0.0
    from seigen_amd.elastic import fibre_combine, fibre_points
    fp, tvec, w = fibre_points(2, (38.0, 46.3), (52.0, 44.1), 6, 3.0, 4)
    assert np.array_equal(ax, fibre_combine(tvec, w, 6, 4, eps))
    u1 = blk.get_field(_lib.FIELD_U)
    cell, G, A = gk.gauge_parts(cfg, fp, u1)
    assert (cell >= 0).all()
    E = gc.kind_of(G, 3)
    want = fibre_combine(tvec, w, 6, 4, E[None])[0]
    S = gk.scale_of(A, 3).reshape(24, 2, 2)
    tt = np.abs(np.outer(tvec, tvec))
    tol = ((tt[None] * (4 * (blk.nd + 2) * EPS * S + 8 * EPS * np.abs(E))).sum(axis=(1, 2)).reshape(6, 4) * w).sum(axis=1)
    print("fibre, last sample: largest |device - restatement| / tolerance = %.3f" % float((np.abs(ax[-1] - want) / tol).max()))
    assert (np.abs(ax[-1] - want) <= tol).all()
    blk.close()
