"""Helpers of tests/test_gauges_host.py, tests/test_gauges_gpu.py, tests/gauge_exchange_worker.py and tools/gauge_cost.py (no
test itself): the restatement in numpy of what a gauge computes (include/seigen_hip.h sg_set_gauges / sg_probe_gradient) from
the tables the library exports, the scale its rounding is measured against, the points of the tests, and polynomial fields
with their analytic gradient at any point."""
import numpy as np

from seigen_amd.backend import gradient_tables, locate_points
from tests import grad_cases as gc

EPS = 2.0 ** -53


def row_h(row):
    """unequal cell sizes of a row of grad_cases.rows(): those of tests/test_grad_gpu.py"""
    dim, n = row[1], row[3]
    return [(0.5, 0.25, 0.2)[a] * 3.0 / n[a] for a in range(dim)]


def row_cfg(row):
    name, dim, degree, n, diagonal = row[:5]
    return gc.block_cfg(dim, degree, n, diagonal, h=row_h(row))


def _ncls(cfg):
    return 1 if cfg.diagonal == 2 else gc.NCLS[cfg.dim]


def gauge_parts(cfg, pts, u):
    """(cell [R], G [R, dim, dim], A [R, dim, dim]) of the points: the owning cell (-1: none), the restatement of the gradient
        D_r[a] = sg_tabulate_grad_cell at sg_locate_points' xi,  t_r[i] = sum_a D_r[a] u[cell][a][i],  G_ij = sum_r J[k][r][j] t_r[i]
    with sg_gradient_tables' J, k = cell % ncls, and A_ij = sum_r |J_rj| sum_a |D_r[a]| |u[a][i]|; rows without a cell are 0"""
    d = cfg.dim
    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, d)
    u = np.asarray(u, dtype=np.float64)
    cell, xi = locate_points(cfg, pts)
    D = gc.tabulate_grad_cell(1 if cfg.diagonal == 2 else 0, d, cfg.degree, xi)            # [R, nd, dim]
    J = gradient_tables(cfg)[1][:, :d, :d]
    ok = cell >= 0
    c = np.where(ok, cell, 0)
    Jk = J[c % _ncls(cfg)]
    t = np.einsum("par,pai->pri", D, u[c])
    G = np.einsum("prj,pri->pij", Jk, t)
    A = np.einsum("prj,pri->pij", np.abs(Jk), np.einsum("par,pai->pri", np.abs(D), np.abs(u[c])))
    G[~ok] = 0.0
    A[~ok] = 0.0
    return cell, G, A


def _flat(x, npts):
    return np.asarray(x).reshape(npts, -1)


def gauge_reference(cfg, pts, u, kind):
    """[R, ncomp]: what the device records at the points for the velocity u [cells, nd, dim]; rows without a cell are 0"""
    cell, G, A = gauge_parts(cfg, pts, u)
    return _flat(gc.kind_of(G, kind), len(cell))


def scale_of(A, kind):
    """[R, ncomp]: the A of a kind - the gradient's own, or the sum of those of the entries the kind combines"""
    d = A.shape[-1]
    n = A.shape[0]
    if kind == 0:
        return _flat(A, n)
    if kind == 1:
        return _flat(np.trace(A, axis1=-2, axis2=-1), n)
    if kind == 2:
        if d == 3:
            return np.stack([A[:, 2, 1] + A[:, 1, 2], A[:, 0, 2] + A[:, 2, 0], A[:, 1, 0] + A[:, 0, 1]], axis=-1)
        return _flat(A[:, 1, 0] + A[:, 0, 1], n)
    S = A + np.swapaxes(A, -1, -2)
    for i in range(d):
        S[:, i, i] = A[:, i, i]
    return _flat(S, n)


def ratio_and_factor(cfg, pts, u, kind, got, nd, slack=4):
    """(largest |got - restatement| / (2^-53 A) over the owned rows with A > 0, the bound's factor slack (nd + dim), and whether
    every row with A = 0 or without a cell agrees exactly)"""
    cell, G, A = gauge_parts(cfg, pts, u)
    want = _flat(gc.kind_of(G, kind), len(cell))
    S = scale_of(A, kind)
    got = _flat(got, len(cell))
    pos = S > 0
    exact = bool(np.array_equal(got[~pos], want[~pos]))
    ratio = float((np.abs(got - want)[pos] / (EPS * S[pos])).max()) if pos.any() else 0.0
    return ratio, slack * (nd + cfg.dim), exact


# ---- points ---------------------------------------------------------------------------------------------------------------
def extent(cfg):
    return np.array([cfg.n[a] * cfg.h[a] for a in range(cfg.dim)])


def _on_lines(cfg, rng, p, axes):
    """p with the coordinates of `axes` moved onto grid lines of the block (its lower side only where the mesh begins there:
    a point on the side towards a lower neighbour is that neighbour's)"""
    for a in axes:
        k = int(rng.integers(1 if cfg.cube0[a] > 0 else 0, cfg.n[a] + 1))
        p[a] = cfg.origin[a] + (cfg.cube0[a] + k) * cfg.h[a]
    return p


def sample_points(cfg, rng, ninterior=20, nspecial=3, outside=True):
    """points of the block: `ninterior` random ones, then `nspecial` each on faces (one coordinate on a grid line), edges (two,
    dim > 1) and vertices (all) of cubes - the block's corners are candidates - and one outside the mesh"""
    d = cfg.dim
    lo = np.array([cfg.origin[a] + cfg.cube0[a] * cfg.h[a] for a in range(d)])
    L = extent(cfg)
    pts = [lo + rng.uniform(0.02, 0.98, d) * L for _ in range(ninterior)]
    for naxes in sorted({1, min(2, d), d}):
        for _ in range(nspecial):
            axes = rng.permutation(d)[:naxes]
            pts.append(_on_lines(cfg, rng, lo + rng.uniform(0.02, 0.98, d) * L, axes))
    pts.append(lo + L)                                   # the upper corner: every coordinate on the last grid line
    if outside:
        pts.append(lo - 0.3 * L)
    return np.array(pts)


# ---- polynomial fields with their gradient anywhere --------------------------------------------------------------------------
class CellPolynomials(object):
    """a different polynomial of the element's space in every cell and component (grad_cases.exponents: total degree P on
    simplices, per-axis degree P on tensor-product cells), the monomials taken about the cell's first node"""

    def __init__(self, rng, tensor, dim, P, X):
        self.E = gc.exponents(tensor, dim, P)
        self.X0 = X[:, 0, :].copy()
        self.span = np.abs(X - X[:, :1, :]).max(axis=(0, 1))
        self.coef = rng.uniform(-1, 1, (X.shape[0], dim, len(self.E)))
        self.dim = dim

    def values(self, cells, x):
        """u [R, dim] at the points x [R, dim] by the polynomials of `cells` [R]"""
        Y = (x - self.X0[cells]) / self.span
        mono = np.prod(Y[:, None, :] ** self.E[None, :, :], axis=-1)
        return np.einsum("pim,pm->pi", self.coef[cells], mono)

    def gradient(self, cells, x):
        """G [R, dim, dim], G[., i, j] = d u_i / d x_j"""
        Y = (x - self.X0[cells]) / self.span
        G = np.zeros((len(cells), self.dim, self.dim))
        for j in range(self.dim):
            Ej = self.E.copy()
            Ej[:, j] = np.maximum(Ej[:, j] - 1, 0)
            dm = self.E[None, :, j] * np.prod(Y[:, None, :] ** Ej[None, :, :], axis=-1) / self.span[j]
            G[:, :, j] = np.einsum("pim,pm->pi", self.coef[cells], dm)
        return G

    def nodal(self, X):
        """u [cells, nd, dim] at the nodes X [cells, nd, dim]"""
        cells = np.repeat(np.arange(X.shape[0]), X.shape[1])
        return self.values(cells, X.reshape(-1, self.dim)).reshape(X.shape[0], X.shape[1], self.dim)
