"""Helpers of tests/test_grad_host.py, tests/test_grad_gpu.py and tools/grad_cost.py (no test itself): the restatement in numpy
of what sg_get_gradient_dev computes, from the tables the library exports, the bound of its rounding, the kinds made of a
gradient, the exact equispaced Lagrange basis in fractions, and polynomial fields with their analytic gradients."""
import ctypes as C
from fractions import Fraction

import numpy as np

from seigen_amd import _lib
from seigen_amd.backend import gradient_tables

NCLS = {1: 1, 2: 2, 3: 6}

# ---- the rows of tests/test_grad_gpu.py: the nine of tests/gradient_loop.py (one per layout, f32 and padding in the first and
# last group among them) and three of their own.  (name, dim, degree, cubes, diagonal, dtype, SEIGEN_HIP_PATH)
EXTRA_ROWS = [
    ("lane-1d-P2", 1, 2, (7,), "left", "f64", "lane"),                      # 7 cells
    ("hexm-DQ4", 3, 4, (3, 2, 2), "quadrilateral", "f64", None),            # 125 nodes: the values of an item are sliced
    ("lane-2d-P2-wide", 2, 2, (13, 5), "left", "f64", "lane"),              # 65 cubes: two groups of 64, 63 padding lanes
]


def rows():
    from tests import gradient_loop as gl
    return list(gl.ROWS) + EXTRA_ROWS


def row_gw(row):
    return 1 if row[6] == "generic" else (64 if row[6] == "lane" else 16)


def row_shape(row):
    """(gw, ncls, nd, dim) of a row"""
    name, dim, degree, n, diagonal = row[:5]
    quad = diagonal == "quadrilateral"
    return row_gw(row), 1 if quad else NCLS[dim], len(lattice(1 if quad else 0, dim, degree)), dim


def ncomp_of(dim, kind):
    return {0: dim * dim, 1: 1, 2: 3 if dim == 3 else 1, 3: dim * dim}[kind]


def block_cfg(dim, degree, n, diagonal="left", h=None, origin=None, cube0=None):
    """the SgConfig of a block; h defaults to unequal cell sizes (0.5, 0.25, 0.2)[:dim] scaled by 1 / n"""
    cfg = _lib.SgConfig()
    cfg.dim, cfg.degree = dim, degree
    h = h or [(0.5, 0.25, 0.2)[a] / n[a] * 3 for a in range(dim)]
    for a in range(3):
        cfg.n[a] = int(n[a]) if a < dim else 1
        cfg.h[a] = float(h[a]) if a < dim else 1.0
        cfg.origin[a] = float(origin[a]) if (origin is not None and a < dim) else 0.0
        cfg.cube0[a] = int(cube0[a]) if (cube0 is not None and a < dim) else 0
    cfg.diagonal = {"left": 0, "right": 1, "quadrilateral": 2}[diagonal]
    return cfg


def tables_of(cfg):
    """{"C": [dim, nd, nd], "J": [ncls, dim, dim], "tensor", "dim", "degree", "nd", "ncls", "line": [dim, nd, nd] bool}"""
    Ct, J = gradient_tables(cfg)
    d, nd = cfg.dim, Ct.shape[1]
    tensor = cfg.diagonal == 2
    line = np.ones((d, nd, nd), dtype=bool)
    if tensor:
        # the entries of the line through a along axis r: b and a agree in every digit but r's (node = a1 + n1 (a2 + n1 a3))
        n1 = cfg.degree + 1
        digits = np.stack([np.arange(nd) // n1 ** i % n1 for i in range(d)], axis=-1)
        for r in range(d):
            other = [i for i in range(d) if i != r]
            line[r] = (digits[:, None, other] == digits[None, :, other]).all(axis=-1)
    return {"C": Ct, "J": J[:, :d, :d].copy(), "tensor": tensor, "dim": d, "degree": cfg.degree, "nd": nd, "ncls": J.shape[0],
            "line": line}


def _used(t):
    """C with the entries the device does not visit (a tensor-product cell: off the line) set to zero"""
    return np.where(t["line"], t["C"], 0.0)


def grad_reference(t, u):
    """G[cell, a, i, j] = sum_r J[k][r][j] sum_b C_r[a][b] u[cell, b, i], k = cell % ncls: the restatement, in double"""
    u = np.asarray(u, dtype=np.float64)
    cls = np.arange(u.shape[0]) % t["ncls"]
    tr = np.einsum("rab,cbi->crai", _used(t), u)
    return np.einsum("crj,crai->caij", t["J"][cls], tr)


def grad_scale(t, u):
    """A[cell, a, i, j] = sum_r |J_rj| sum_b |C_r[a][b]| |u[b][i]|: what the rounding of either side is measured against"""
    u = np.abs(np.asarray(u, dtype=np.float64))
    cls = np.arange(u.shape[0]) % t["ncls"]
    tr = np.einsum("rab,cbi->crai", np.abs(_used(t)), u)
    return np.einsum("crj,crai->caij", np.abs(t["J"][cls]), tr)


def kind_of(G, kind):
    """kinds 1 to 3 of a gradient [.., dim, dim] by the combinations include/seigen_hip.h states, each operation rounded on its
    own as numpy rounds it"""
    d = G.shape[-1]
    if kind == 0:
        return G
    if kind == 1:
        s = G[..., 0, 0]
        for i in range(1, d):
            s = s + G[..., i, i]
        return s
    if kind == 2:
        if d == 3:
            return np.stack([G[..., 2, 1] - G[..., 1, 2], G[..., 0, 2] - G[..., 2, 0], G[..., 1, 0] - G[..., 0, 1]], axis=-1)
        return G[..., 1, 0] - G[..., 0, 1]
    E = 0.5 * (G + np.swapaxes(G, -1, -2))
    for i in range(d):
        E[..., i, i] = G[..., i, i]
    return E


# ---- the exact basis ---------------------------------------------------------------------------------------------------
def lattice(cell_type, dim, P):
    """the nodes' lattice coordinates, first coordinate fastest (refelem.hpp lattice_points)"""
    if cell_type == 1 and dim > 1:
        return [tuple(a // (P + 1) ** i % (P + 1) for i in range(dim)) for a in range((P + 1) ** dim)]
    if dim == 1:
        return [(a,) for a in range(P + 1)]
    if dim == 2:
        return [(a1, a2) for a2 in range(P + 1) for a1 in range(P + 1 - a2)]
    return [(a1, a2, a3) for a3 in range(P + 1) for a2 in range(P + 1 - a3) for a1 in range(P + 1 - a3 - a2)]


def _factor(P, n, lam):
    """f_n(lam) = prod_{k < n} (P lam - k) / (k + 1) and its derivative"""
    terms = [(P * lam - k) / (k + 1) for k in range(n)]
    f = Fraction(1)
    for x in terms:
        f *= x
    df = Fraction(0)
    for m in range(n):
        p = Fraction(P, m + 1)
        for k in range(n):
            if k != m:
                p *= terms[k]
        df += p
    return f, df


def _line(P, b, x):
    """the 1-D Lagrange polynomial of node b / P on the equispaced nodes 0 .. 1 and its derivative"""
    f, df = Fraction(1), Fraction(0)
    for m in range(P + 1):
        if m == b:
            continue
        p = Fraction(P, b - m)
        for k in range(P + 1):
            if k != b and k != m:
                p *= (P * x - k) / (b - k)
        df += p
        f *= (P * x - m) / (b - m)
    return f, df


def exact_basis(cell_type, dim, P, x):
    """(phi [nd], dphi [nd][dim]) at the reference point x (Fractions), exactly"""
    phi, dphi = [], []
    if cell_type == 1 and dim > 1:
        for al in lattice(1, dim, P):
            fs = [_line(P, al[i], x[i]) for i in range(dim)]
            v = Fraction(1)
            for f, _ in fs:
                v *= f
            phi.append(v)
            g = []
            for r in range(dim):
                p = fs[r][1]
                for i in range(dim):
                    if i != r:
                        p *= fs[i][0]
                g.append(p)
            dphi.append(g)
        return phi, dphi
    lam = [1 - sum(x)] + list(x)
    for al in lattice(0, dim, P):
        full = (P - sum(al),) + tuple(al)
        fs = [_factor(P, full[v], lam[v]) for v in range(dim + 1)]
        v = Fraction(1)
        for f, _ in fs:
            v *= f
        phi.append(v)

        def d_lam(v):
            p = fs[v][1]
            for o in range(dim + 1):
                if o != v:
                    p *= fs[o][0]
            return p
        d0 = d_lam(0)
        dphi.append([d_lam(r + 1) - d0 for r in range(dim)])
    return phi, dphi


def tabulate_cell(cell_type, dim, P, xi):
    xi = np.ascontiguousarray(xi, dtype=np.float64).reshape(-1, dim)
    nd = len(lattice(cell_type, dim, P))
    phi = np.empty((len(xi), nd))
    _lib.check(_lib.load().sg_tabulate_cell(cell_type, dim, P, len(xi), xi.ctypes.data, phi.ctypes.data))
    return phi


def tabulate_grad_cell(cell_type, dim, P, xi):
    xi = np.ascontiguousarray(xi, dtype=np.float64).reshape(-1, dim)
    nd = len(lattice(cell_type, dim, P))
    dphi = np.empty((len(xi), nd, dim))
    _lib.check(_lib.load().sg_tabulate_grad_cell(cell_type, dim, P, len(xi), xi.ctypes.data, dphi.ctypes.data))
    return dphi


# ---- polynomial fields -------------------------------------------------------------------------------------------------
def exponents(tensor, dim, P):
    """the monomials of the element's space: total degree <= P on simplices, per-axis degree <= P on tensor-product cells"""
    grid = np.stack(np.meshgrid(*[np.arange(P + 1)] * dim, indexing="ij"), axis=-1).reshape(-1, dim)
    return grid if tensor else grid[grid.sum(axis=1) <= P]


def polynomial_field(rng, tensor, dim, P, X):
    """a different polynomial of degree P in every cell for every component, at the nodes X [cells, nd, dim], and its analytic
    gradient: (u [cells, nd, dim], G [cells, nd, dim, dim]); the monomials are taken about the cell's first node"""
    E = exponents(tensor, dim, P)
    ncells, nd = X.shape[:2]
    coef = rng.uniform(-1, 1, (ncells, dim, len(E)))
    Y = X - X[:, :1, :]
    span = np.abs(Y).max(axis=(0, 1))
    Y = Y / span                      # monomials of order one
    mono = np.prod(Y[:, :, None, :] ** E[None, None, :, :], axis=-1)              # [cells, nd, m]
    u = np.einsum("cim,cam->cai", coef, mono)
    G = np.zeros((ncells, nd, dim, dim))
    for j in range(dim):
        Ej = E.copy()
        Ej[:, j] = np.maximum(Ej[:, j] - 1, 0)
        dm = E[None, None, :, j] * np.prod(Y[:, :, None, :] ** Ej[None, None, :, :], axis=-1) / span[j]
        G[..., j] = np.einsum("cim,cam->cai", coef, dm)
    return u, G


def node_coords(cfg):
    d = cfg.dim
    ncls = 1 if cfg.diagonal == 2 else NCLS[d]
    nd = len(lattice(1 if cfg.diagonal == 2 else 0, d, cfg.degree))
    ncube = int(np.prod([cfg.n[a] for a in range(d)]))
    X = np.empty((ncube * ncls, nd, d))
    _lib.check(_lib.load().sg_block_node_coords(C.byref(cfg), cfg.degree, X.ctypes.data, X.nbytes))
    return X
