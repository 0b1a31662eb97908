"""CPU-only tests of the point injectors (include/seigen_hip.h sg_injector_weights / sg_inject / sg_set_injectors): the
exports are bound; psi = Mhat^-1 phi(xi) / |det J| has the delta property on every element; ownership is the receivers';
the kernel objects of namespace sg::inject in the built library are the listed ones, each with the GPU test that launches
it; and, on the oracle, the two facts the feature's documentation rests on - a step with -dt is the ADJOINT of a step in the
energy inner product (so injected residuals and -dt stepping give the adjoint field), and the INVERSE of a step is the other
stage order with -dt (what ElasticLF4.rewind runs).

The grouping of the owned points by cell (hostapi.cpp injector_plan: cells ascending, a cell's points in the order given) has
no export of its own, so no test here can see it: tools/host_asan_driver.cpp injector_plans walks it under the sanitizers
(cells ascending, rows of a cell in ascending point index; tests/test_host_asan.py runs that), and
tests/test_injectors_gpu.py test_one_shot_into_zero_fields meets the sum in the order listed to the bit, where the same sum
in reverse order differs."""
import os
import subprocess

import numpy as np
import pytest

from oracle.lf4 import OracleLF4
from seigen_amd import _lib
from seigen_amd.backend import injector_weights, locate_points
from tests.util import oracle_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sg_injector_weights", "sg_inject", "sg_set_injectors")

# Every kernel object of namespace sg::inject (kernels_inject.hip) with the tests of tests/test_injectors_gpu.py that launch
# it: the rule of tests/test_correlate_host.py for sg::xcorr.
INJECT_KERNELS = {
    "sg::inject::point_add<double>": "test_one_shot_into_zero_fields, every f64 row; test_series_against_the_oracle",
    "sg::inject::point_add<float>": "test_one_shot_into_zero_fields, rows mfma-P4-f32 and tile-tri-P3-f32",
}


def make_cfg(dim, degree, n, h, quad=False, cube0=None, nbr_mask=0):
    cfg = _lib.SgConfig()
    cfg.dim, cfg.degree = dim, degree
    for a in range(3):
        cfg.n[a] = int(n[a]) if a < dim else 1
        cfg.h[a] = float(h[a]) if a < dim else 1.0
        cfg.origin[a] = 0.0
        cfg.cube0[a] = int(cube0[a]) if (cube0 is not None and a < dim) else 0
    cfg.diagonal = 2 if quad else 0
    cfg.nbr_mask = nbr_mask
    return cfg


def nodes_of(dim, degree, quad):
    if quad:
        return (degree + 1) ** dim
    return {1: degree + 1, 2: (degree + 1) * (degree + 2) // 2, 3: (degree + 1) * (degree + 2) * (degree + 3) // 6}[dim]


def mass_matrix(dim, degree, quad):
    nd = nodes_of(dim, degree, quad)
    M = np.empty((nd, nd))
    assert _lib.load().sg_reference_operator_cell(1 if quad else 0, dim, degree, 2, 0, M.ctypes.data, M.nbytes) == nd * nd
    return M


def basis_at(cfg, pts, quad):
    """(cell, phi [npts, nd]) of the receivers' evaluation: sg_locate_points, then sg_tabulate_cell"""
    cell, xi = locate_points(cfg, pts)
    nd = nodes_of(cfg.dim, cfg.degree, quad)
    phi = np.empty((len(pts), nd))
    _lib.check(_lib.load().sg_tabulate_cell(1 if quad else 0, cfg.dim, cfg.degree, len(pts), np.ascontiguousarray(xi).ctypes.data,
                                            phi.ctypes.data))
    return cell, phi


def test_injector_symbols_are_bound():
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "seigen_hip.h")).read()
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(L, name)
        assert "int %s(" % name in hdr
    assert L.sg_abi_version() == 2


ELEMENTS = [(dim, degree, False) for dim in (1, 2, 3) for degree in (1, 2, 3, 4)] + \
           [(dim, degree, True) for dim in (2, 3) for degree in (1, 2, 3, 4)]


@pytest.mark.parametrize("dim,degree,quad", ELEMENTS, ids=["%s%d-%dd" % ("DQ" if q else "P", p, d) for d, p, q in ELEMENTS])
def test_psi_is_the_delta_of_the_element(dim, degree, quad):
    """sum_a psi_a (|det J| Mhat v)_a = v(x) for random polynomials v of the element's degree (random nodal values), at
    random interior points and at points on grid lines, to 1e-12 of max |v| (cond(Mhat) at P4 is about 1e3)."""
    rng = np.random.default_rng(100 * dim + 10 * degree + quad)
    n, h = (3, 2, 2)[:dim], (0.5, 0.25, 0.4)[:dim]
    cfg = make_cfg(dim, degree, n, h, quad)
    L = np.array([n[a] * h[a] for a in range(dim)])
    pts = rng.uniform(0.02, 0.98, (12, dim)) * L
    line = rng.uniform(0.02, 0.98, (6, dim)) * L
    for k in range(len(line)):              # one, two, ... coordinates on a grid line
        for a in range(1 + k % dim):
            line[k, a] = h[a] * rng.integers(1, n[a])
    pts = np.concatenate([pts, line])
    nd = nodes_of(dim, degree, quad)
    cell, psi = injector_weights(cfg, pts, nd)
    cell_r, phi = basis_at(cfg, pts, quad)
    assert np.array_equal(cell, cell_r) and (cell >= 0).all()
    M, detj = mass_matrix(dim, degree, quad), float(np.prod(h))
    worst = 0.0
    for _ in range(5):
        v = rng.uniform(-1.0, 1.0, nd)
        worst = max(worst, np.abs(psi @ (detj * (M @ v)) - phi @ v).max() / np.abs(v).max())
    assert worst <= 1e-12, worst
    # a point outside the mesh: nobody's, psi = 0
    cell, psi = injector_weights(cfg, -np.ones((1, dim)), nd)
    assert cell[0] == -1 and not psi.any()


@pytest.mark.parametrize("grid", [(2, 2, 2), (1, 1, 4)], ids=["2x2x2", "slabs"])
def test_ownership_is_the_receivers(grid):
    """Under a partition every point inside the mesh has one owner, a point outside none, and the owner and the psi are the
    ones the whole mesh gives: the blocks' sg_injector_weights against sg_locate_points."""
    dim, degree, N = 3, 2, (4, 4, 4)
    h = [0.25] * 3
    rng = np.random.default_rng(5)
    pts = np.concatenate([rng.uniform(0.0, 1.0, (20, 3)),
                          [[0.5, 0.5, 0.5], [0.5, 0.3, 0.7], [0.25, 0.5, 0.75], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [1.0, 0.5, 0.1]],
                          [[-0.1, 0.5, 0.5], [0.5, 1.2, 0.5]]])
    nd = nodes_of(dim, degree, False)
    whole_cell, whole_psi = injector_weights(make_cfg(dim, degree, N, h), pts, nd)
    assert (whole_cell[:-2] >= 0).all() and (whole_cell[-2:] == -1).all()
    owners = np.zeros(len(pts), dtype=int)
    for bz in range(grid[2]):
        for by in range(grid[1]):
            for bx in range(grid[0]):
                b = (bx, by, bz)
                n = [N[a] // grid[a] for a in range(3)]
                cfg = make_cfg(dim, degree, n, h, cube0=[b[a] * n[a] for a in range(3)])
                cell, psi = injector_weights(cfg, pts, nd)
                cell_l, _ = locate_points(cfg, pts)
                assert np.array_equal(cell, cell_l)
                owners += cell >= 0
                assert np.array_equal(psi[cell >= 0], whole_psi[cell >= 0]) and not psi[cell < 0].any()
    assert np.array_equal(owners, (whole_cell >= 0).astype(int)), owners


def _top_level_head(sig):
    depth = 0
    for i, c in enumerate(sig):
        if c == "<":
            depth += 1
        elif c == ">":
            depth -= 1
        elif c == "(" and depth == 0:
            return sig[:i]
    return sig


def test_inject_kernel_objects_are_the_listed_ones():
    readelf = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-readelf")
    assert os.path.exists(readelf), "llvm-readelf (shipped with ROCm) not found at %s: set ROCM_PATH" % readelf
    out = subprocess.run([readelf, "--dyn-syms", "--demangle", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    found = []
    for line in out.splitlines():
        f = line.split(None, 7)
        if len(f) < 8 or f[3] != "OBJECT" or "sg::inject::" not in f[7]:
            continue
        head = _top_level_head(f[7])
        if "sg::inject::" in head:
            found.append(head[head.index("sg::inject::"):])
    assert sorted(found) == sorted(INJECT_KERNELS), found
    assert all(INJECT_KERNELS.values())


# ---- the two identities, on the oracle -------------------------------------------------------------------------------

def energy_inner(M, detj, dim, lam, mu, xa, xb):
    """<x, y>_E = sum_c |det J| (wk u^T Mhat u' + ws s : Mhat : s' + wt tr Mhat tr') with the physical weights of sg_measure,
    rho = 1"""
    (ua, sa), (ub, sb) = xa, xb
    lam, mu = np.broadcast_to(lam, (ua.shape[0],)), np.broadcast_to(mu, (ua.shape[0],))
    wk, ws, wt = 0.5, 1.0 / (4.0 * mu), -lam / (4.0 * mu * (dim * lam + 2.0 * mu))
    uu = np.einsum("cai,ab,cbi->c", ua, M, ub)
    ss = np.einsum("caij,ab,cbij->c", sa, M, sb)
    tt = np.einsum("ca,ab,cb->c", np.trace(sa, axis1=-2, axis2=-1), M, np.trace(sb, axis1=-2, axis2=-1))
    return detj * float(np.sum(wk * uu + ws * ss + wt * tt))


def oracle_case(dim, degree, n, per_cell, seed):
    L = (1.0,) * dim
    m = oracle_mesh(dim, n, L, "left")
    orc = OracleLF4(m, degree)
    rng = np.random.default_rng(seed)
    h = [L[a] / n[a] for a in range(dim)]
    orc.dt = 0.05 * min(h) / degree ** 2
    if per_cell:
        orc.l, orc.mu = rng.uniform(0.4, 0.8, m.ncells), rng.uniform(0.2, 0.4, m.ncells)
    else:
        orc.l, orc.mu = 0.5, 0.25
    orc.density = 1.0
    return orc, h, rng


ADJOINT_CASES = [("2d-P2", 2, 2, (3, 3), 6, False), ("2d-P2-per-cell", 2, 2, (3, 3), 6, True), ("2d-P4", 2, 4, (2, 2), 5, False),
                 ("3d-P2", 3, 2, (2, 2, 2), 4, False)]


@pytest.mark.parametrize("name,dim,degree,n,K,per_cell", ADJOINT_CASES, ids=[c[0] for c in ADJOINT_CASES])
def test_a_step_with_minus_dt_is_the_adjoint_of_a_step(name, dim, degree, n, K, per_cell):
    """Forward K steps from random (u0, s0), s symmetric, recording d_k = R u after step k.  The adjoint state starts from
    zero, gets R* r_{K-k} before step k + 1 and steps with -dt (stages in their normal order); R* r = r psi / wk in the energy
    inner product, psi from sg_injector_weights.  Then sum_k r_k . d_k = <lambda_K, x_0>_E, to 1e-13 of sum |r_k . d_k|
    (3e-16 .. 9e-16 measured)."""
    orc, h, rng = oracle_case(dim, degree, n, per_cell, 7)
    nd = orc.E.nd
    cfg = make_cfg(dim, degree, n, h)
    pts = rng.uniform(0.05, 0.95, (3, dim))
    pts[1, 0] = h[0]                         # one receiver on a grid line
    cell, phi = basis_at(cfg, pts, False)
    cell_i, psi = injector_weights(cfg, pts, nd)
    assert np.array_equal(cell, cell_i)
    M, detj = mass_matrix(dim, degree, False), float(np.prod(h))
    u0 = rng.uniform(-1.0, 1.0, orc.u0.shape)
    s0 = rng.uniform(-1.0, 1.0, orc.s0.shape)
    s0 = 0.5 * (s0 + np.swapaxes(s0, -1, -2))
    orc.u0, orc.s0 = u0.copy(), s0.copy()
    d = []
    for k in range(K):
        orc.step((k + 1) * orc.dt)
        d.append(np.array([phi[j] @ orc.u1[cell[j]] for j in range(len(pts))]))
    r = rng.uniform(-1.0, 1.0, (K, len(pts), dim))
    adj, _, _ = oracle_case(dim, degree, n, per_cell, 7)
    adj.dt = -orc.dt
    for k in range(K):
        u = adj.u0.copy()
        for j in range(len(pts)):
            u[cell[j]] += psi[j][:, None] * (r[K - 1 - k, j] / 0.5)[None, :]
        adj.u0 = u
        adj.step(0.0)
    lhs = sum(float(np.sum(r[k] * d[k])) for k in range(K))
    rhs = energy_inner(M, detj, dim, orc.l, orc.mu, (adj.u1, adj.s1), (u0, s0))
    scale = sum(abs(float(np.sum(r[k] * d[k]))) for k in range(K))
    assert abs(lhs - rhs) <= 1e-13 * scale, (name, abs(lhs - rhs) / scale)


def _velocity_half(o, dt):
    E = o.E
    uh1 = E.apply_F(o.s0, o.u0)
    uh2 = E.apply_F(E.apply_G(uh1, o.l, o.mu), o.u0)
    o.u0 = o.u1 = o.u0 + dt * uh1 + dt ** 3 / 24.0 * uh2


def _stress_half(o, dt):
    E = o.E
    sh1 = E.apply_G(o.u0, o.l, o.mu)
    sh2 = E.apply_G(E.apply_F(sh1, o.u0), o.l, o.mu)
    o.s0 = o.s1 = o.s0 + dt * sh1 + dt ** 3 / 24.0 * sh2


def test_the_inverse_of_a_step_is_the_other_stage_order():
    """K forward steps, then K steps in the order (3, 4, 5, 0, 1, 2) with -dt, return smooth data to round-off; K steps with
    -dt in the normal order do not (a difference above 1e-6): they apply the adjoint, not the inverse."""
    dim, degree, n, K = 2, 2, (3, 3), 6
    orc, h, _ = oracle_case(dim, degree, n, False, 3)
    X = orc.node_coords()
    u0 = np.stack([np.sin(2 * X[..., 0] + i) * np.cos(X[..., 1] - i) for i in range(dim)], axis=-1)
    s0 = np.zeros(orc.s0.shape)
    for i in range(dim):
        for j in range(dim):
            s0[..., i, j] = np.cos(X[..., 0] + 0.5 * (i + j)) * (1 + X[..., 1])
    # the hand-written halves are the oracle's step
    orc.u0, orc.s0 = u0.copy(), s0.copy()
    orc.step(orc.dt)
    chk, _, _ = oracle_case(dim, degree, n, False, 3)
    chk.u0, chk.s0 = u0.copy(), s0.copy()
    _velocity_half(chk, chk.dt)
    _stress_half(chk, chk.dt)
    assert np.array_equal(chk.u0, orc.u1) and np.array_equal(chk.s0, orc.s1)
    for k in range(1, K):
        orc.step((k + 1) * orc.dt)
    assert np.abs(orc.u1 - u0).max() > 1e-6, "the forward steps must change the state"
    uK, sK = orc.u1.copy(), orc.s1.copy()
    for _ in range(K):
        _stress_half(orc, -orc.dt)
        _velocity_half(orc, -orc.dt)
    assert np.abs(orc.u0 - u0).max() < 1e-13 and np.abs(orc.s0 - s0).max() < 1e-13
    adj, _, _ = oracle_case(dim, degree, n, False, 3)
    adj.u0, adj.s0 = uK, sK
    adj.dt = -adj.dt
    for _ in range(K):
        adj.step(0.0)
    assert max(np.abs(adj.u1 - u0).max(), np.abs(adj.s1 - s0).max()) > 1e-6
