"""Receivers recorded on the device inside the time loop (include/seigen_hip.h sg_set_receivers / sg_get_receivers;
kernels_recv.hip): every kernel family against the host evaluation of the downloaded fields, bitwise equality across the
ways a step can be driven, the reference's explosive-source receiver run against the oracle's traces, the all-or-nothing
rules, and multi-rank runs - inside the library's exchange and through the solver class - against the single block."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from seigen_amd import _lib  # noqa: E402
from seigen_amd.backend import HipBlock  # noqa: E402

from test_receivers_host import point_kinds  # noqa: E402

# (name, dim, degree, cubes, diagonal, dtype, SEIGEN_HIP_PATH, symmetric initial stress)
FAMILIES = [
    ("generic-1d-P2", 1, 2, (7,), "left", "f64", None, True),
    ("generic-2d-P2", 2, 2, (4, 3), "left", "f64", "generic", True),
    ("lane-2d-P2", 2, 2, (5, 3), "left", "f64", "lane", True),
    ("lane-hex-DQ2", 3, 2, (3, 2, 2), "quadrilateral", "f64", "lane", True),
    ("tile-tri-P3", 2, 3, (5, 3), "left", "f64", None, True),
    ("tile-quad-P2", 2, 2, (5, 3), "quadrilateral", "f64", None, True),
    ("mfma-P3-sym", 3, 3, (4, 3, 2), "left", "f64", None, True),
    ("mfma-P3-full", 3, 3, (4, 3, 2), "left", "f64", None, False),
    ("mfma-P4-sym", 3, 4, (4, 3, 2), "left", "f64", None, True),
    ("mfma-P4-full", 3, 4, (4, 3, 2), "left", "f64", None, False),
    ("mfma-P4-f32", 3, 4, (4, 3, 2), "left", "f32", None, True),
    ("hexm-DQ3", 3, 3, (3, 2, 2), "quadrilateral", "f64", None, True),
    ("hexm-DQ4", 3, 4, (3, 2, 2), "quadrilateral", "f64", None, True),
]


def make_case(dim, degree, n, diagonal, dtype, sym, stream=None):
    """a block of the unit box with smooth fields, an active box-Ricker source and a sponge; returns (block, dt).
    stream: a hipStream_t of the caller's (as an integer) for the block to launch on, None: the block's own"""
    h = [1.0 / k for k in n]
    blk = HipBlock(dim, degree, n, h, [0.0] * dim, diagonal, stream=stream, dtype=dtype)
    dt = 0.1 * min(h) / degree ** 2
    blk.set_params(1.0, dt, 0.5, 0.25)
    X = blk.node_coords()
    u = np.stack([np.sin(2 * X[..., 0] + i) * np.cos(X[..., -1] - i) for i in range(dim)], axis=-1)
    s = np.zeros(X.shape[:-1] + (dim, dim))
    for i in range(dim):
        for j in range(dim):
            s[..., i, j] = np.cos(X[..., 0] + 0.5 * (i + j) + (0.3 * i if not sym else 0.0)) * (1 + X[..., -1])
    blk.set_field(_lib.FIELD_U, u)
    blk.set_field(_lib.FIELD_S, s)
    blk.set_source_box_ricker([0.3] * dim, [0.6] * dim, 400.0, 3 * dt, dt, dt, 64)
    Xq = blk.node_coords(2)
    blk.set_absorption(np.where(Xq[..., 0] >= 0.6, 20.0 + 30.0 * Xq[..., 0], 0.0), 2)
    if not sym:
        assert not blk.is_sym()
    return blk, dt


def receiver_points(dim, n):
    pts = point_kinds(n, (1.0,) * dim, seed=3)
    inside = np.all((pts >= 0.0) & (pts <= 1.0), axis=1)
    return pts[inside], pts[~inside]


def host_samples(blk, pts, every, nsamples):
    """the twin's fields downloaded after every `every`-th step, evaluated with sg_tabulate_cell at the located point"""
    cell, xi = _locate_on(blk, pts)
    kind = 1 if (blk.nfaces == 2 * blk.dim and blk.dim > 1) else 0
    phi = np.empty((len(pts), blk.nd))
    _lib.check(_lib.load().sg_tabulate_cell(kind, blk.dim, blk.degree, len(pts), np.ascontiguousarray(xi).ctypes.data,
                                            phi.ctypes.data))
    out = []
    for _ in range(nsamples):
        blk.step(every)
        u, s = blk.get_field(_lib.FIELD_U), blk.get_field(_lib.FIELD_S)
        out.append([np.concatenate([phi[k] @ u[cell[k]], np.tensordot(phi[k], s[cell[k]], axes=(0, 0)).reshape(-1)])
                    for k in range(len(pts))])
    return np.array(out)


def _locate_on(blk, pts):
    from seigen_amd.backend import locate_points
    cfg = _lib.SgConfig()
    cfg.dim, cfg.degree = blk.dim, blk.degree
    for a in range(3):
        cfg.n[a] = blk._n[a] if a < blk.dim else 1
        cfg.h[a] = 1.0 / blk._n[a] if a < blk.dim else 1.0
    cfg.diagonal = 2 if (blk.nfaces == 2 * blk.dim and blk.dim > 1) else 0
    return locate_points(cfg, pts)


def _block(spec, monkeypatch):
    name, dim, degree, n, diagonal, dtype, path, sym = spec
    if path:
        monkeypatch.setenv("SEIGEN_HIP_PATH", path)
    else:
        monkeypatch.delenv("SEIGEN_HIP_PATH", raising=False)
    blk, dt = make_case(dim, degree, n, diagonal, dtype, sym)
    blk._n = n
    return blk


@pytest.mark.parametrize("spec", FAMILIES, ids=[f[0] for f in FAMILIES])
@pytest.mark.parametrize("every", [1, 3])
def test_every_family_samples_the_fields(gpu, monkeypatch, spec, every):
    """Every sample equals the host evaluation of the fields downloaded at that step (a twin handle stepped every `every`
    steps), receivers inside cells, on cube faces, edges and vertices, on the inner simplex faces and on the mesh
    boundary; a point outside the mesh is owned by nobody.  8k + 3 steps: graph8 and graph1 both replay."""
    name, dim, degree, n, diagonal, dtype, path, sym = spec
    pts, outside = receiver_points(dim, n)
    steps = 19
    blk, twin = _block(spec, monkeypatch), _block(spec, monkeypatch)
    owned = blk.set_receivers(np.concatenate([pts, outside]), 3, every, steps // every)
    assert owned[:len(pts)].all() and not owned[len(pts):].any()
    blk.step(steps)
    got = blk.get_receivers()
    assert got.shape == (steps // every, len(pts) + len(outside), dim + dim * dim)
    assert not got[:, len(pts):].any()
    want = host_samples(twin, pts, every, steps // every)
    scale = np.abs(want).max()
    assert scale > 0 and np.isfinite(got).all()
    tol = (1e-6 if dtype == "f32" else 1e-14) * scale
    err = np.abs(got[:, :len(pts)] - want).max()
    assert err <= tol, (name, err / scale, blk.stage_kernel_name(0))
    blk.close()
    twin.close()


@pytest.mark.parametrize("spec", [FAMILIES[4], FAMILIES[9], FAMILIES[0]], ids=["tile-tri-P3", "mfma-P4-full", "generic-1d"])
def test_traces_bitwise_across_the_ways_of_stepping(gpu, monkeypatch, spec):
    """Graph replay, eager launches with timing on, sg_step(1) repeated and sg_run_stage x 6 + sg_end_step give the same
    traces bit for bit."""
    name, dim, degree, n = spec[:4]
    pts, _ = receiver_points(dim, n)
    steps, every = 19, 3
    out = {}
    for way in ("graph", "timing", "single", "stages"):
        blk = _block(spec, monkeypatch)
        blk.set_receivers(pts, 3, every, steps // every)
        if way == "graph":
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
        out[way] = blk.get_receivers()
        assert blk.counters()["steps"] == steps
        blk.close()
    assert out["graph"].shape[0] == steps // every and np.abs(out["graph"]).max() > 0
    for way in ("timing", "single", "stages"):
        assert np.array_equal(out[way], out["graph"]), way


@pytest.mark.parametrize("mode,fixture", [("interpolate", "explosive_oracle.npz"), ("project", "explosive_oracle_project.npz")])
def test_explosive_source_receiver_run(gpu, mode, fixture):
    """The reference's receiver run (uy.py:25-43: dt = 1e-3, T = 2.5, three receivers on grid lines, every 5th step) through
    ElasticLF4.set_receivers: against the oracle's committed traces and against the host-sampled record_receivers."""
    from seigen_amd.harness.explosive_source import ExplosiveSourceLF4
    d = np.load(os.path.join(ROOT, "tests", "golden", fixture))
    recv = ((45.0, 149.0), (90.0, 149.0), (140.0, 149.0))
    ex = ExplosiveSourceLF4()
    el = ex.setup(dt=1e-3, source_mode=mode)
    el.set_receivers(recv, every=5)
    el.run(2.5)
    t, tr = el.receiver_traces()
    np.testing.assert_allclose(t, d["times"], atol=1e-9)
    scale = np.abs(d["traces"]).max()
    assert np.abs(tr["velocity"] - d["traces"]).max() < 1e-9 * scale
    ex2 = ExplosiveSourceLF4()
    ex2.setup(dt=1e-3, source_mode=mode)
    t2, tr2 = ex2.record_receivers(2.5, receivers=recv, every=5)
    assert np.array_equal(t, t2)
    assert np.abs(tr["velocity"] - tr2).max() < 1e-13 * scale


def _rc_set(blk, pts, what, every, capacity, nrec=None):
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    return blk.lib.sg_set_receivers(blk.h, len(pts) if nrec is None else nrec, pts.ctypes.data, what, every, capacity, None)


def test_receiver_calls_are_all_or_nothing(gpu, monkeypatch):
    spec = FAMILIES[8]
    pts, _ = receiver_points(3, spec[3])
    blk, twin = _block(spec, monkeypatch), _block(spec, monkeypatch)
    for b in (blk, twin):
        b.set_receivers(pts, 3, 1, 4)
        b.step(3)
    before = blk.get_receivers()
    assert before.shape[0] == 3
    # sg_step whose samples would overflow: refused before anything is queued (graph replay and eager alike)
    for n in (2, 5):
        assert blk.lib.sg_step(blk.h, n) == -3
    assert blk.counters()["steps"] == 3 and np.array_equal(blk.get_receivers(), before)
    for f in (_lib.FIELD_U, _lib.FIELD_S, _lib.FIELD_UH, _lib.FIELD_SH):
        assert np.array_equal(blk.get_field(f), twin.get_field(f)), f
    # bad arguments: SG_ERR_ARG, the receivers armed before keep recording
    assert _rc_set(blk, pts, 3, 0, 4) == -1
    assert _rc_set(blk, pts, 0, 1, 4) == -1
    assert _rc_set(blk, pts, 4, 1, 4) == -1
    assert _rc_set(blk, pts, 3, 1, 4, nrec=-1) == -1
    buf = np.zeros(before.size + 1)
    ns = C.c_int64()
    assert blk.lib.sg_get_receivers(blk.h, buf.ctypes.data, buf.nbytes, C.byref(ns)) == -1
    blk.step(1)
    twin.step(1)
    assert np.array_equal(blk.get_receivers(), twin.get_receivers()) and blk.get_receivers().shape[0] == 4
    # full: one more step is refused by sg_step and by sg_end_step (which does not count it); read out, disarm, go on
    assert blk.lib.sg_step(blk.h, 1) == -3
    for st in range(6):
        blk.run_stage(st)
    assert blk.lib.sg_end_step(blk.h) == -3
    assert blk.counters()["steps"] == 4 and blk.get_receivers().shape[0] == 4
    full = blk.get_receivers()
    blk.set_receivers(np.zeros((0, 3)))
    assert blk.get_receivers().shape == (0, 0, 0)
    blk.end_step()
    blk.step(9)
    assert blk.counters()["steps"] == 14 and blk.get_receivers().shape == (0, 0, 0)
    assert np.abs(full).max() > 0
    # re-arming discards the samples and counts steps from the arming call
    blk.set_receivers(pts, 1, 2, 3)
    assert blk.get_receivers().shape == (0, len(pts), 3)
    blk.step(3)
    assert blk.get_receivers().shape == (1, len(pts), 3)
    blk.step(3)
    assert blk.get_receivers().shape == (3, len(pts), 3)
    blk.close()
    twin.close()


@pytest.fixture(scope="module")
def fake():
    from fake_rccl.build import build
    return build()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _fake_env(fake, tmp_path, **extra):
    env = dict(os.environ, SEIGEN_RCCL_LIB=fake, FAKE_RCCL_TIMEOUT_S="60", FAKE_RCCL_LOG=str(tmp_path / "fake"),
               HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2")
    env.pop("FAKE_RCCL_HOST", None)
    env.update(extra)
    return env


@pytest.mark.parametrize("grid,n,every", [((2, 2, 2), (32, 4, 4), 1), ((1, 1, 2), (16, 4, 4), 2)])
def test_receivers_inside_the_native_exchange(gpu, fake, tmp_path, grid, n, every):
    """Ranks driving the C-ABI with the exchange inside the library (async transport double): receivers on block faces,
    edges, the centre corner and in the interior are owned exactly once, and their rows equal the single block's bitwise."""
    from native_exchange_worker import setup_block
    world, degree, steps = int(np.prod(grid)), 4, 6
    pts = np.array([[0.5, 0.5, 0.5], [0.5, 0.3, 0.7], [0.3, 0.5, 0.6], [0.6, 0.7, 0.5], [0.5, 0.5, 0.2], [0.2, 0.5, 0.5],
                    [0.35, 0.6, 0.45], [0.1, 0.9, 0.8], [0.0, 0.0, 0.0], [1.0, 0.5, 0.5], [0.71, 0.23, 0.5]])
    np.save(tmp_path / "points.npy", pts)
    env = _fake_env(fake, tmp_path, FAKE_RCCL_ASYNC="1", FAKE_RCCL_SLOT_BYTES="1048576")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "receiver_exchange_worker.py"), str(tmp_path),
                               str(world), str(r), ",".join(map(str, grid)), ",".join(map(str, n)), str(degree), str(steps),
                               "source", str(every), str(tmp_path / "points.npy")],
                              cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(world)]
    errs = []
    for p in procs:
        try:
            so, se = p.communicate(timeout=400)
        except subprocess.TimeoutExpired:
            p.kill()
            so, se = p.communicate()
        if p.returncode != 0:
            errs.append(so[-1500:] + se[-3000:])
    assert not errs, "\n-----\n".join(errs)
    blk = HipBlock(3, degree, n, [1.0 / n[a] for a in range(3)], [0.0] * 3, "left", 0)
    setup_block(blk, n, degree, "source")
    assert blk.set_receivers(pts, 3, every, steps // every).all()
    blk.step(steps)
    single = blk.get_receivers()
    blk.close()
    assert single.shape == (steps // every, len(pts), 12) and np.abs(single).max() > 0
    owners = np.zeros(len(pts), dtype=int)
    for r in range(world):
        d = np.load(tmp_path / ("rank%d.npz" % r))
        assert int(d["steps"]) == steps
        own = d["owned"]
        owners += own
        assert np.array_equal(d["traces"][:, own], single[:, own]), "rank %d" % r
        assert not d["traces"][:, ~own].any()
    assert np.all(owners == 1), owners


@pytest.mark.parametrize("native", ["force", "0"])
def test_receivers_through_the_solver_class_on_four_ranks(gpu, fake, tmp_path, native):
    """ElasticLF4.set_receivers / receiver_traces on 4 ranks, grid (1, 2, 2), P4 with the source, gloo group - the exchange
    inside the library, or host-driven with sg_end_step ending every step: rank 0's traces equal the single rank's bitwise."""
    from receiver_dist_worker import POINTS, receivers_on_create
    from dist_worker import run_case
    n, grid, degree, steps, every = (16, 4, 4), (1, 2, 2), 4, 6, 2
    env = _fake_env(fake, tmp_path, SEIGEN_DIST_BACKEND="gloo", SEIGEN_HIP_DEVICE="0", SEIGEN_HALO_NATIVE=native)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "4", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "receiver_dist_worker.py"), str(tmp_path),
           str(degree), str(steps), ",".join(map(str, n)), ",".join(map(str, grid)), str(every)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    d = np.load(tmp_path / "traces.npz")
    assert int(d["native"]) == (1 if native == "force" else 0)
    with receivers_on_create(POINTS, every):
        el, _, _ = run_case(n, degree, steps, None, True)
    t, tr = el.receiver_traces()
    assert tr["velocity"].shape == (steps // every, len(POINTS), 3) and np.abs(tr["velocity"]).max() > 0
    assert np.array_equal(d["times"], t)
    assert np.array_equal(d["velocity"], tr["velocity"]) and np.array_equal(d["stress"], tr["stress"])
