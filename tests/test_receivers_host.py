"""Point location of the receivers (include/seigen_hip.h sg_locate_points), device-free: the C++ rule against the one of
seigen_amd/functionspace.py locate - the stand-in for the point location behind vtktools.vtu.ProbeData in the reference's
receiver script (tests/explosive_source/uy.py:36-43) - on every dimension, cell kind, diagonal and degree, for points
inside cells, on cube faces, edges and vertices, on the faces between the simplices of a cube, on the mesh boundary and
outside the mesh; and the ownership rule across the blocks of a partition."""
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from seigen_amd import _lib  # noqa: E402
from seigen_amd.backend import locate_points  # noqa: E402
from seigen_amd.functionspace import FunctionSpace, block_config, locate  # noqa: E402
from seigen_amd.mesh import Mesh, Partition  # noqa: E402


def point_kinds(n, L, seed=0):
    """Points of every kind for a mesh of n cubes per axis on [0, L]: random interior points, points on cube faces, edges
    and vertices, on the inner simplex faces (equal fractions along two axes: the Kuhn / "left" cuts; fractions adding up
    to one: the "right" cut), on the mesh boundary, and outside it."""
    d = len(n)
    h = np.array(L) / np.array(n)
    rng = np.random.default_rng(seed)
    pts = []
    cube = lambda: rng.integers(0, n)                                        # noqa: E731
    for _ in range(12):                                                      # interior
        pts.append((cube() + rng.uniform(0.05, 0.95, d)) * h)
    for m in range(1, d + 1):                                                # faces (m = 1), edges (2), vertices (d)
        for axes in itertools.combinations(range(d), m):
            for _ in range(3):
                f = rng.uniform(0.05, 0.95, d)
                f[list(axes)] = 0.0
                pts.append((cube() + f) * h)
    if d >= 2:
        for a, b in itertools.combinations(range(d), 2):                    # inner simplex faces
            for _ in range(3):
                f = rng.uniform(0.05, 0.95, d)
                f[b] = f[a]
                pts.append((cube() + f) * h)
                f = rng.uniform(0.05, 0.95, d)
                f[b] = 1.0 - f[a]
                pts.append((cube() + f) * h)
        for _ in range(3):                                                  # all fractions equal (3-D: the cube's diagonal)
            pts.append((cube() + rng.uniform(0.05, 0.95)) * h)
    for a in range(d):                                                       # mesh boundary, and just outside / far outside
        for side in (0.0, L[a]):
            f = (rng.integers(0, n) + rng.uniform(0.05, 0.95, d)) * h
            f[a] = side
            pts.append(f.copy())
            f[a] = side + (-1 if side == 0.0 else 1) * 0.3 * h[a]
            pts.append(f.copy())
    pts.append(np.full(d, -7.0 * h[0]))
    pts.append(np.array(L) * 3.0)
    return np.array(pts)


CASES = [(1, "left", False)] + [(2, diag, False) for diag in ("left", "right")] + [(2, "left", True), (3, "left", False),
                                                                                   (3, "left", True)]


@pytest.mark.parametrize("dim,diagonal,quad", CASES)
@pytest.mark.parametrize("degree", [1, 2, 3, 4])
def test_locate_points_matches_the_python_rule(dim, diagonal, quad, degree):
    n = {1: (5,), 2: (4, 3), 3: (3, 2, 2)}[dim]
    L = {1: (2.0,), 2: (2.0, 0.75), 3: (1.5, 1.0, 0.5)}[dim]
    mesh = Mesh(n, L, diagonal, quad)
    space = FunctionSpace(mesh, "DG", degree)
    pts = point_kinds(n, L, seed=dim * 10 + degree)
    cell, xi = locate_points(block_config(mesh, degree), pts)
    nfound = 0
    for k, p in enumerate(pts):
        want = locate(space, p)
        if want is None:
            assert cell[k] == -1, (p, cell[k])
            continue
        nfound += 1
        assert cell[k] == want[0], (p, cell[k], want[0])
        assert np.abs(xi[k] - want[1]).max() < 1e-13, (p, xi[k], want[1])
    assert nfound == len(pts) - 2 * dim - 2      # everything but the points outside the mesh


def test_locate_points_on_the_explosive_source_receivers():
    """uy.py's receivers lie on vertical grid lines (h = 2.5): the lower cube - the left side of the field - is chosen."""
    mesh = Mesh((120, 60), (300.0, 150.0))
    space = FunctionSpace(mesh, "DG", 2)
    pts = np.array([[45.0, 149.0], [90.0, 149.0], [140.0, 149.0]])
    cell, xi = locate_points(block_config(mesh, 2), pts)
    for k in range(3):
        c, x = locate(space, pts[k])
        assert cell[k] == c and np.abs(xi[k] - x).max() < 1e-13
        assert (cell[k] // 2) % 120 == int(pts[k][0] / 2.5) - 1          # the cube left of the line


def test_locate_points_refuses_bad_arguments():
    L = _lib.load()
    cfg = block_config(Mesh((2, 2), (1.0, 1.0)), 2)
    pts = np.zeros((1, 2))
    cell, xi = np.zeros(1, dtype=np.int64), np.zeros((1, 2))
    assert L.sg_locate_points(cfg, -1, pts.ctypes.data, cell.ctypes.data, xi.ctypes.data) == -1
    assert L.sg_locate_points(cfg, 1, None, cell.ctypes.data, xi.ctypes.data) == -1
    assert L.sg_locate_points(None, 1, pts.ctypes.data, cell.ctypes.data, xi.ctypes.data) == -1
    assert L.sg_locate_points(cfg, 0, None, None, None) == _lib.SG_OK


def _global_cell(part, ncls, local):
    """block-local cell -> cell of the whole mesh"""
    cube, k = divmod(int(local), ncls)
    c, g, mul = [], 0, 1
    for a in range(part.dim):
        c.append(cube % part.n[a])
        cube //= part.n[a]
    for a in range(part.dim):
        g += (c[a] + part.start[a]) * mul
        mul *= part.global_n[a]
    return g * ncls + k


@pytest.mark.parametrize("n,L,grid,quad", [
    ((4, 4, 4), (1.0, 1.0, 1.0), (2, 2, 2), False),
    ((2, 2, 6), (0.5, 0.5, 1.5), (1, 1, 3), False),
    ((4, 3, 3), (2.0, 1.5, 1.5), (2, 1, 3), True),
    ((6, 4), (3.0, 2.0), (3, 2), False),
])
@pytest.mark.parametrize("degree", [2, 4])
def test_every_point_inside_has_exactly_one_owner(n, L, grid, quad, degree):
    """Under a partition each point inside the mesh - block faces, edges and corners included - is owned by exactly one
    block, in the cell the single block finds, with bitwise the same reference coordinates; a point outside by none."""
    d = len(n)
    whole = Mesh(n, L, quadrilateral=quad)
    pts = point_kinds(n, L, seed=7 + degree)
    h = np.array(L) / np.array(n)
    # the block interfaces: block corners and points on the faces between blocks
    starts = [sorted({Partition(n, r, int(np.prod(grid)), grid).start[a] for r in range(int(np.prod(grid)))}) for a in range(d)]
    corners = np.array([[s * h[a] for a, s in enumerate(c)] for c in itertools.product(*starts)])
    pts = np.concatenate([pts, corners, corners + 0.37 * h * (np.arange(d) == 0)])
    cell1, xi1 = locate_points(block_config(whole, degree), pts)
    ncls = whole.cells_per_block
    owners = np.zeros(len(pts), dtype=int)
    for r in range(int(np.prod(grid))):
        part = Partition(n, r, int(np.prod(grid)), grid)
        m = Mesh(n, L, quadrilateral=quad)
        m.set_partition(part)
        cell, xi = locate_points(block_config(m, degree), pts)
        for k in np.nonzero(cell >= 0)[0]:
            owners[k] += 1
            assert _global_cell(part, ncls, cell[k]) == cell1[k], (pts[k], r)
            assert np.array_equal(xi[k], xi1[k]), (pts[k], r)
    inside = cell1 >= 0
    assert np.all(owners[inside] == 1), pts[inside][owners[inside] != 1]
    assert np.all(owners[~inside] == 0)
    assert inside.sum() == len(pts) - 2 * d - 2
