"""The material-gradient recipe of INTEGRATION.md section 3 on the device, through public calls alone
(ElasticLF4.set_injectors / set_receivers / run / rewind / inject / correlate, and block.run_stage + end_step for the adjoint's
two halves), one row per layout, every row with per-cell lambda, mu, the physical per-cell rho, a point-force series at an
interior point and at a point on a grid line, three receivers, K = 6 steps in 3-D and 12 in 2-D (tests/gradient_loop.py
ROWS / row_case; tests/test_gradient_oracle.py checks on the CPU that the accumulators stand clear of the bounds used here).

(a) the device's accumulators (uu, ss, tt) per cell against the oracle's loop, measured against scale_k = the sum over the
    calls of the largest per-cell term the oracle formed (the sums cancel): 10 tol_of() x scale in double, 5e-5 x scale for
    f32 blocks - the suite's step tolerances, as the dot-product test of tests/test_injectors_gpu.py uses them.
(b) the adjoint's step driven as velocity half, two correlates with a rewind of the other handle between them, stress half,
    end_step leaves bitwise the fields of step(1) from the same state, at every step of the loop.
(c) -1/2 K_rho of the device's accumulators against central differences of J through device forward runs, four cells (the
    interior source's, a receiver's, two that hold neither), 1e-6 of the largest difference: the differences' step (relative
    1e-5: truncation 1e-10, round-off of J about 1e-16 / 1e-5) plus the parity of the runs.

Measured on an MI355X.  (a) |device - oracle| / scale, largest over cells and (uu, ss, tt): mfma-P4-sym 1.3e-15, mfma-P3-sym
7.2e-15, tile-tri-P3 6.8e-15, tile-quad-P2 1.7e-15, hexm-DQ3 8.3e-16, lane-2d-P2 4.0e-16, generic-2d-P2 9.4e-16, mfma-P3-f32
1.3e-7, tile-tri-P3-f32 4.6e-8, with the final max |acc_k| at 1e-2 .. 0.46 of scale_k.  (b) equal bits at every step of every
row.  (c) tile-tri-P3 2.2e-10, mfma-P4-sym 6.3e-10 of the largest difference."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from seigen_amd import _lib  # noqa: E402
from seigen_amd.elastic import sensitivity  # noqa: E402
from tests import gradient_loop as gl  # noqa: E402
from tests.test_parity_gpu import tol_of  # noqa: E402

SWITCHES = ("SEIGEN_HIP_PATH", "SEIGEN_HIP_GRAPH", "SEIGEN_HIP_SPONGE_AFFINE", "SEIGEN_HIP_SYM", "SEIGEN_HIP_SOURCE_LAUNCH",
            "SEIGEN_HIP_XCORR")
PREFIX = {"mfma": "sg::mfma_stage_", "tile": "sg::tile2d_stage<", "hexm": "sg::hexm_", "lane": "sg::lane_",
          "generic": "sg::stage_kernel"}
VELOCITY_HALF = (_lib.STAGE_UH1, _lib.STAGE_STEMP, _lib.STAGE_U1)
STRESS_HALF = (_lib.STAGE_SH1, _lib.STAGE_UTEMP, _lib.STAGE_S1)


def _quiet(monkeypatch, path):
    import seigen_amd
    import seigen_amd.helpers as helpers
    for var in SWITCHES:
        monkeypatch.delenv(var, raising=False)
    if path:
        monkeypatch.setenv("SEIGEN_HIP_PATH", path)
    monkeypatch.setattr(helpers, "log", lambda s: None)
    monkeypatch.setattr(seigen_amd.elastic, "log", lambda s: None)


def _solver(row, mat, dt):
    """an ElasticLF4 of the row on the unit box: zero fields, per-cell lambda, mu and the physical per-cell rho"""
    from seigen_amd import BoxMesh, ElasticLF4, RectangleMesh
    name, dim, degree, n, diagonal, dtype, path = row
    quad = diagonal == "quadrilateral"
    if dim == 2:
        mesh = RectangleMesh(n[0], n[1], 1.0, 1.0, diagonal="left" if quad else diagonal, quadrilateral=quad)
    else:
        mesh = BoxMesh(n[0], n[1], n[2], 1.0, 1.0, 1.0, hexahedral=quad)
    el = ElasticLF4.create(mesh, "DG", degree, dimension=dim, solver="explicit", output=False, dtype=dtype)
    el.l, el.mu, el.density = (np.array(a, dtype=np.float64) for a in mat)
    el.density_physical = True
    el.dt = dt
    blk = el.block
    assert blk.ncells == len(mat[0])
    blk.set_field(_lib.FIELD_U, np.zeros(blk.field_shape(_lib.FIELD_U)))
    blk.set_field(_lib.FIELD_S, np.zeros(blk.field_shape(_lib.FIELD_S)))
    return el


def _forward(row, case, mat=None):
    """the forward run of the row: (solver holding x_K, d [K, R, dim])"""
    fwd = _solver(row, case["mat"] if mat is None else mat, case["dt"])
    fwd.set_injectors(case["xs"], case["q"])
    fwd.set_receivers(case["xr"], every=1)
    fwd.run(case["K"] * case["dt"] * (1 + 1e-9))
    assert fwd.block.counters()["steps"] == case["K"]
    return fwd, fwd.receiver_traces()[1]["velocity"]


def _fields(el):
    return el.block.get_field(_lib.FIELD_U), el.block.get_field(_lib.FIELD_S)


def gradient_recipe(row, case, twin_check=False):
    """The recipe as INTEGRATION.md section 3 prints it.  Returns (J, accumulators [ncells, 3], the adjoint solver's
    material-gradient dict); with twin_check a second adjoint solver takes step(1) where the first runs the mid-step sequence,
    and the two are compared bit for bit after every step."""
    name, dim, degree, n, diagonal, dtype, path = row
    K, dt, xs, q, xr, mat = case["K"], case["dt"], case["xs"], case["q"], case["xr"], case["mat"]
    fwd, d = _forward(row, case)
    family = name.split("-")[0]
    assert fwd.block.stage_kernel_name(0).startswith(PREFIX[family]), fwd.block.stage_kernel_name(0)
    res = d - case["obs"]                                       # [K, R, dim]: sample k - 1 belongs to step k
    J = 0.5 * float(np.sum(res ** 2))
    from seigen_amd.backend import locate_points
    from seigen_amd.functionspace import block_config
    cell_r, _ = locate_points(block_config(fwd.mesh, fwd.degree), xr)
    series = res[::-1] * (2.0 / fwd.density[cell_r])[None, :, None]   # W^-1 R^T r = (2 / rho_cell) r psi; the last residual first
    adjoints = [_solver(row, mat, -dt) for _ in range(2 if twin_check else 1)]
    for a in adjoints:
        a.setup()
        a.set_injectors(xr, series)
    adj = adjoints[0]
    if family == "mfma":        # the matrix-pipe rows are the symmetric-storage ones: zero fields and velocity entries keep it
        assert fwd.block.is_sym() and all(a.block.is_sym() for a in adjoints), name
    for j in range(K):
        k = K - j
        for stage in VELOCITY_HALF:
            adj.block.run_stage(stage)                          # adj: stepped velocity, not yet stepped stress
        if k < K:
            fwd.inject(xs, -q[k])                               # the + state is step k's own result: its entry q_k out again
        adj.correlate(fwd, (1.0, 1.0, 1.0))
        fwd.rewind(1)                                           # the state step k started from, entry q_{k-1} included
        adj.correlate(fwd, (-1.0, -1.0, -1.0))
        for stage in STRESS_HALF:
            adj.block.run_stage(stage)
        adj.block.end_step()                                    # adds the next residual
        if twin_check:
            adjoints[1].block.step(1)
            (ua, sa), (ub, sb) = _fields(adj), _fields(adjoints[1])
            assert np.abs(ua).max() > 0 and np.abs(sa).max() > 0
            assert np.array_equal(ua, ub) and np.array_equal(sa, sb), (name, j, np.abs(ua - ub).max(), np.abs(sa - sb).max())
    if family == "mfma":
        assert fwd.block.is_sym() and all(a.block.is_sym() for a in adjoints), name
    corr = adj.correlation()
    acc = np.stack([corr["uu"], corr["ss"], corr["tt"]], axis=-1)
    grad = {k: -0.5 * v for k, v in sensitivity(dim, adj.density, adj.l, adj.mu, corr).items()}
    # the forward handle is back at its start (the first entry alone: no stress yet); a re-wound step is no step of the run
    uf, sf = _fields(fwd)
    assert fwd.block.counters()["steps"] == K and np.abs(sf).max() <= 1e-4 * np.abs(uf).max()
    for el in [fwd] + adjoints:
        el.block.close()
    return J, acc, grad


@pytest.mark.parametrize("row", gl.ROWS, ids=[r[0] for r in gl.ROWS])
def test_accumulators_against_the_oracle_s_loop(gpu, monkeypatch, row):
    """(a) and (b).  |device - oracle| <= bound x scale per cell and entry, bound 10 tol_of() in double and 5e-5 for f32 blocks
    (measured 4e-16 .. 7e-15 and 5e-8 .. 1.3e-7: the module's docstring); J itself to 1e-9 (1e-3 in f32: twelve f32 steps)."""
    name, dim, degree, n, diagonal, dtype, path = row
    _quiet(monkeypatch, path)
    case, ref = gl.row_case(row), gl.row_reference(row)
    J, acc, grad = gradient_recipe(row, case, twin_check=True)
    want, scale = ref["acc"]["midstep"], ref["scale"]["midstep"]
    bound = 5e-5 if dtype == "f32" else 10 * tol_of(degree, diagonal)
    err = np.abs(acc - want).max(axis=0) / scale
    print("gradient loop %s: |device - oracle| / scale (uu, ss, tt) = %s (bound %.1e); max |acc| / scale = %s; J %.6e against %.6e"
          % (name, err, bound, np.abs(want).max(axis=0) / scale, J, ref["J"]))
    assert acc.shape == want.shape and np.isfinite(acc).all()
    assert np.all(np.abs(acc - want) <= bound * scale[None, :]), (name, err)
    assert abs(J - ref["J"]) <= (1e-3 if dtype == "f32" else 1e-9) * ref["J"]


@pytest.mark.parametrize("name", list(gl.DENSITY_ROWS))
def test_density_gradient_on_the_device(gpu, monkeypatch, name):
    """(c): J through device forward runs with one cell's rho moved by +-1e-5 (relative), four cells; -1/2 K_rho of the
    device's accumulators equals the differences to 1e-6 of the largest (measured 2.2e-10 and 6.3e-10)."""
    row = [r for r in gl.ROWS if r[0] == name][0]
    dim, path = row[1], row[6]
    _quiet(monkeypatch, path)
    case, ref = gl.row_case(row), gl.row_reference(row)
    mat, cells = case["mat"], gl.density_cells(row)
    J, acc, grad = gradient_recipe(row, case)

    def J_of(m):
        fwd, d = _forward(row, case, m)
        fwd.block.close()
        return 0.5 * float(np.sum((d - case["obs"]) ** 2))

    fd = gl.central_differences(J_of, mat, cells, params=("rho",))["rho"]
    miss = np.abs(grad["rho"][cells] - fd).max() / np.abs(fd).max()
    print("device density gradient %s: cells %s, differences %s, -K_rho / 2 %s, miss %.2e of the largest difference"
          % (name, cells, fd, grad["rho"][cells], miss))
    assert miss <= 1e-6, (name, miss)
