"""CPU-only tests of the gauges (include/seigen_hip.h sg_set_gauges / sg_get_gauges / sg_probe_gradient and the device-free
sg_gauge_weights): the weights against the tabulated derivative at the located point; the restatement tests/gauge_cases.py
gauge_reference - what tests/test_gauges_gpu.py compares the device with - against the analytic gradient of polynomials of the
element's space at arbitrary points; ownership under a partition; the kernel objects of namespace sg::gauge in the built
library; the fibre helper of seigen_amd/elastic.py on an affine field."""
import ctypes as C
import os

import numpy as np
import pytest

from seigen_amd import _lib
from seigen_amd.backend import gauge_weights, locate_points
from seigen_amd.elastic import fibre_combine, fibre_points
from tests import gauge_cases as gk
from tests import grad_cases as gc
from tests.test_grad_host import _head

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Every kernel object of namespace sg::gauge (kernels_gauge.hip) with the rows of tests/test_gauges_gpu.py that launch it.
# tests/test_host_logic.py pins the objects named sg::name(; this list keeps the same rule for the nested namespace.
GAUGE_KERNELS = {
    "sg::gauge::sample<double>": "every f64 row of test_probe_against_the_restatement and test_series_against_the_restatement",
    "sg::gauge::sample<float>": "rows mfma-P3-f32 and tile-tri-P3-f32 of the same tests",
}

BLOCKS = [(dim, P, diagonal) for dim, diags in ((1, ("left",)), (2, ("left", "right", "quadrilateral")), (3, ("left", "quadrilateral")))
          for diagonal in diags for P in (1, 2, 3, 4)]
IDS = ["%dd-%s-P%d" % (b[0], b[2], b[1]) for b in BLOCKS]
N = (3, 2, 2)


def _cfg(block, **kw):
    dim, P, diagonal = block
    return gc.block_cfg(dim, P, N[:dim], diagonal, **kw)


def gauge_objects():
    import subprocess
    readelf = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-readelf")
    assert os.path.exists(readelf), "llvm-readelf (shipped with ROCm) not found at %s: set ROCM_PATH" % readelf
    out = subprocess.run([readelf, "--dyn-syms", "--demangle", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    found = []
    for line in out.splitlines():
        f = line.split(None, 7)
        if len(f) < 8 or f[3] != "OBJECT":
            continue
        head = _head(f[7])
        if "sg::gauge::" in head:
            found.append(head[head.index("sg::gauge::"):])
    return found


def test_gauge_kernel_objects_are_the_listed_ones():
    found = gauge_objects()
    assert len(found) == len(set(found)), "a kernel object appears twice"
    assert not set(found) - set(GAUGE_KERNELS), "in the library but not listed: %s" % sorted(set(found) - set(GAUGE_KERNELS))
    assert not set(GAUGE_KERNELS) - set(found), "listed but not in the library: %s" % sorted(set(GAUGE_KERNELS) - set(found))
    assert all(GAUGE_KERNELS.values())


def test_symbols_are_bound_and_refuse_without_a_device():
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "seigen_hip.h")).read()
    for name in ("sg_set_gauges", "sg_get_gauges", "sg_probe_gradient", "sg_gauge_weights"):
        assert name in _lib.SYMBOLS and hasattr(L, name) and " %s(" % name in hdr
    pts, out, n = np.zeros((1, 2)), np.zeros(4), C.c_int64()
    assert L.sg_set_gauges(None, 1, pts.ctypes.data, 0, 1, 1, None) == -1
    assert L.sg_get_gauges(None, out.ctypes.data, 32, C.byref(n)) == -1
    assert L.sg_probe_gradient(None, 0, 0, 1, pts.ctypes.data, out.ctypes.data, 32, None) == -1
    cfg = gc.block_cfg(2, 2, (3, 3))
    cell, D = np.zeros(1, dtype=np.int64), np.zeros((1, 2, 6))
    assert L.sg_gauge_weights(C.byref(cfg), 1, pts.ctypes.data, cell.ctypes.data, D.ctypes.data) == 6
    assert L.sg_gauge_weights(C.byref(cfg), 0, None, None, None) == 6
    assert L.sg_gauge_weights(None, 1, pts.ctypes.data, cell.ctypes.data, D.ctypes.data) == -1
    assert L.sg_gauge_weights(C.byref(cfg), -1, pts.ctypes.data, cell.ctypes.data, D.ctypes.data) == -1
    assert L.sg_gauge_weights(C.byref(cfg), 1, None, cell.ctypes.data, D.ctypes.data) == -1
    assert L.sg_gauge_weights(C.byref(cfg), 1, pts.ctypes.data, None, D.ctypes.data) == -1
    assert L.sg_gauge_weights(C.byref(cfg), 1, pts.ctypes.data, cell.ctypes.data, None) == -1
    for dim, degree, diagonal in ((0, 2, 0), (4, 2, 0), (2, 0, 0), (2, 5, 0), (1, 2, 2)):
        bad = gc.block_cfg(2, 2, (3, 3))
        bad.dim, bad.degree, bad.diagonal = dim, degree, diagonal
        assert L.sg_gauge_weights(C.byref(bad), 1, pts.ctypes.data, cell.ctypes.data, D.ctypes.data) == -1, (dim, degree, diagonal)
    bad = gc.block_cfg(2, 2, (3, 3))
    bad.h[1] = 0.0
    assert L.sg_gauge_weights(C.byref(bad), 1, pts.ctypes.data, cell.ctypes.data, D.ctypes.data) == -1


# ---- the weights -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", BLOCKS, ids=IDS)
def test_weights_are_the_tabulated_derivative_at_the_located_point(block):
    """sg_gauge_weights = sg_tabulate_grad_cell at sg_locate_points' xi, bitwise, as [dim][nd] rows; -1 and zeros outside; on a
    grid line the lower cell"""
    dim, P, diagonal = block
    cfg = _cfg(block, origin=(0.3, -0.2, 0.15), cube0=(2, 1, 3))
    nd = len(gc.lattice(int(diagonal == "quadrilateral"), dim, P))
    pts = gk.sample_points(cfg, np.random.default_rng(7 * dim + P))
    cell, xi = locate_points(cfg, pts)
    cell_w, D = gauge_weights(cfg, pts, nd)
    assert np.array_equal(cell, cell_w)
    assert cell[-1] == -1 and (cell[:-1] >= 0).all()
    tab = gc.tabulate_grad_cell(int(diagonal == "quadrilateral"), dim, P, xi)          # [R, nd, dim]
    assert np.array_equal(D[cell >= 0], np.transpose(tab, (0, 2, 1))[cell >= 0])
    assert (D[-1] == 0.0).all() and np.abs(D[0]).max() > 0.0
    # a point on the grid line between cube 0 and cube 1 along x, elsewhere inside cube 0: the cell is one of cube 0
    ncls = gk._ncls(cfg)
    p = np.array([cfg.origin[a] + (cfg.cube0[a] + 0.37) * cfg.h[a] for a in range(dim)])
    p[0] = cfg.origin[0] + (cfg.cube0[0] + 1) * cfg.h[0]
    c, x = locate_points(cfg, p[None])
    assert c[0] // ncls == 0
    # ... and the upper corner of the block lies in its last cube
    c, _ = locate_points(cfg, pts[-2][None])
    assert c[0] // ncls == int(np.prod(N[:dim])) - 1


# ---- the restatement against analytic gradients -----------------------------------------------------------------------------
@pytest.mark.parametrize("block", BLOCKS, ids=IDS)
def test_restatement_reproduces_polynomials_at_points(block):
    """u a different polynomial of the element's space in every cell and component, interpolated at sg_block_node_coords of a
    block with unequal h, a non-zero origin and cube0; gauge_reference at 20 random interior points and at points on faces,
    edges and vertices of cubes against the analytic gradient of the OWNING cell's polynomial there (on a grid line the lower
    cell's): agreement to 1e-11 * scale, scale = the largest |gradient| of the block; all four kinds."""
    dim, P, diagonal = block
    quad = diagonal == "quadrilateral"
    cfg = _cfg(block, origin=(0.3, -0.2, 0.15), cube0=(2, 1, 3))
    X = gc.node_coords(cfg)
    rng = np.random.default_rng(100 * dim + P)
    poly = gk.CellPolynomials(rng, quad, dim, P, X)
    u = poly.nodal(X)
    pts = gk.sample_points(cfg, rng)
    cell, G, A = gk.gauge_parts(cfg, pts, u)
    own = cell >= 0
    assert own.sum() == len(pts) - 1 and len(pts) >= 20 + 3 * len({1, min(2, dim), dim}) + 2
    want = poly.gradient(cell[own], pts[own])
    scale = np.abs(want).max()
    err = np.abs(G[own] - want).max() / scale
    print("largest |restatement - analytic| / scale: %.3e" % err)
    assert err <= 1e-11
    for kind in (0, 1, 2, 3):
        if kind == 2 and dim == 1:
            continue
        got = gk.gauge_reference(cfg, pts, u, kind)
        ref = gc.kind_of(want, kind).reshape(own.sum(), -1)
        assert got.shape == (len(pts), gc.ncomp_of(dim, kind))
        assert np.abs(got[own] - ref).max() <= 1e-11 * scale * 2 and (got[~own] == 0.0).all(), kind
    # a seeded fault is seen: the upper cell on a grid line reads another polynomial
    if P >= 1:
        p = np.array([cfg.origin[a] + (cfg.cube0[a] + 0.37) * cfg.h[a] for a in range(dim)])
        p[0] = cfg.origin[0] + (cfg.cube0[0] + 1) * cfg.h[0]
        c, _ = locate_points(cfg, p[None])
        g_low = gk.gauge_parts(cfg, p[None], u)[1][0]
        q = p.copy()
        q[0] += 1e-7 * cfg.h[0]
        c_up, _ = locate_points(cfg, q[None])
        assert c_up[0] != c[0]
        g_up = poly.gradient(c_up, p[None])[0]
        assert np.abs(g_low - poly.gradient(c, p[None])[0]).max() <= 1e-11 * scale
        assert np.abs(g_low - g_up).max() > 1e-3 * scale


# ---- ownership --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", [(2, 3, "left"), (2, 2, "quadrilateral"), (3, 2, "left"), (3, 2, "quadrilateral")],
                         ids=["2d-tri", "2d-quad", "3d-tet", "3d-hex"])
def test_every_inside_point_has_one_owner_with_the_single_blocks_weights(block):
    """a 2 x 2 (x 2) partition of a 4 x 4 (x 2) mesh, stated by cube0 with a common origin: every point inside the mesh - on the
    cuts, on their crossing, on the mesh's boundary - is owned by exactly one block, the point outside by none, and the
    owner's weights are the single block's bitwise"""
    dim, P, diagonal = block
    n = (4, 4, 2)[:dim]
    origin = (0.3, -0.2, 0.15)
    h = [0.11, 0.07, 0.13][:dim]
    whole = gc.block_cfg(dim, P, n, diagonal, h=h, origin=origin)
    nd = len(gc.lattice(int(diagonal == "quadrilateral"), dim, P))
    rng = np.random.default_rng(5)
    pts = gk.sample_points(whole, rng, ninterior=20, nspecial=6)
    cut = np.array([origin[a] + (n[a] // 2) * h[a] for a in range(dim)])
    extra = [cut.copy()]
    for a in range(dim):
        p = np.array([origin[b] + rng.uniform(0.1, 0.9) * n[b] * h[b] for b in range(dim)])
        p[a] = cut[a]
        extra.append(p)
    pts = np.concatenate([np.array(extra), pts])
    cell, D = gauge_weights(whole, pts, nd)
    owners = np.zeros(len(pts), dtype=int)
    halves = [(0, n[a] // 2) for a in range(dim)]
    for corner in np.ndindex(*(2,) * dim):
        sub_n = [n[a] // 2 for a in range(dim)]
        cube0 = [corner[a] * halves[a][1] for a in range(dim)]
        sub = gc.block_cfg(dim, P, sub_n, diagonal, h=h, origin=origin, cube0=cube0)
        c, Ds = gauge_weights(sub, pts, nd)
        owners += c >= 0
        assert np.array_equal(Ds[c >= 0], D[c >= 0]), corner
        assert (Ds[c < 0] == 0.0).all()
    assert (owners[:-1] == 1).all() and owners[-1] == 0 and cell[-1] == -1 and (cell[:-1] >= 0).all()


# ---- the fibre ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", [(2, 2, "left"), (3, 1, "quadrilateral")], ids=["2d-tri-P2", "3d-hex-DQ1"])
def test_fibre_channels_of_an_affine_field(block):
    """u = B x + c: the strain rate is sym(B) everywhere, so every channel of a fibre - whatever its gauge length and nq, across
    cells and along grid lines - returns t . sym(B) . t to round-off, from the restatement's strain-rate gauges"""
    dim, P, diagonal = block
    cfg = _cfg(block)
    X = gc.node_coords(cfg)
    rng = np.random.default_rng(11)
    B, c = rng.uniform(-1, 1, (dim, dim)), rng.uniform(-1, 1, dim)
    u = np.einsum("ij,caj->cai", B, X) + c
    L = gk.extent(cfg)
    p0, p1 = 0.1 * L, np.array([0.9, 0.8, 0.7][:dim]) * L
    for nchannels, gauge_length, nq in ((5, 0.05 * L.min(), 4), (1, 0.3 * L.min(), 2), (3, 0.0, 1)):
        pts, t, w = fibre_points(dim, p0, p1, nchannels, gauge_length, nq)
        assert pts.shape == (nchannels * nq, dim) and abs(w.sum() - 1.0) < 1e-15 and abs(np.linalg.norm(t) - 1.0) < 1e-15
        eps = gk.gauge_reference(cfg, pts, u, 3).reshape(1, len(pts), dim, dim)
        got = fibre_combine(t, w, nchannels, nq, eps)
        want = t @ (0.5 * (B + B.T)) @ t
        assert got.shape == (1, nchannels) and np.abs(got - want).max() <= 1e-12 * np.abs(B).max() / min(cfg.h[a] for a in range(dim))
    with pytest.raises(ValueError):
        fibre_points(dim, p0, p0, 3, 0.1, 2)
    with pytest.raises(ValueError):
        fibre_points(dim, p0, p1, 0, 0.1, 2)
