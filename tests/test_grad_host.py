"""CPU-only tests of the gradient (include/seigen_hip.h sg_get_gradient_dev and its device-free companions sg_tabulate_grad_cell,
sg_gradient_tables, sg_gradient_plan): the tabulated derivative of the basis against the exact one in fractions; the tables
against the tabulation and the mesh tables; the restatement tests/grad_cases.py grad_reference - what tests/test_grad_gpu.py
compares the device with - against the analytic gradient of polynomials of the element's space; the plan of every row of the
GPU tests; the kernel objects of namespace sg::grad in the built library."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from seigen_amd import _lib
from seigen_amd.backend import gradient_plan, gradient_tables
from tests import grad_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53

# Every kernel object of namespace sg::grad (kernels_grad.hip) with the rows of tests/test_grad_gpu.py that launch it.
# tests/test_host_logic.py pins the objects named sg::name(; this list keeps the same rule for the nested namespace.
GRAD_KERNELS = {
    "sg::grad::lanes<double, double>": "double tensor: every f64 row with gw = 16 or 64 (mfma-*, tile-*, hexm-DQ3, hexm-DQ4, lane-*)",
    "sg::grad::lanes<double, float>": "float tensor: the same rows",
    "sg::grad::lanes<float, double>": "double tensor: rows mfma-P3-f32, tile-tri-P3-f32",
    "sg::grad::lanes<float, float>": "float tensor: the f32 rows",
    "sg::grad::flat<double, double>": "double tensor: row generic-2d-P2 (the generic family has double blocks only)",
    "sg::grad::flat<double, float>": "float tensor: row generic-2d-P2",
}


def _head(sig):
    """a demangled signature up to the `(` that opens the argument list, template arguments skipped"""
    depth = 0
    for i, c in enumerate(sig):
        if c == "<":
            depth += 1
        elif c == ">":
            depth -= 1
        elif c == "(" and depth == 0:
            return sig[:i]
    return sig


def grad_objects(path=None):
    readelf = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-readelf")
    assert os.path.exists(readelf), "llvm-readelf (shipped with ROCm) not found at %s: set ROCM_PATH" % readelf
    out = subprocess.run([readelf, "--dyn-syms", "--demangle", path or _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    found = []
    for line in out.splitlines():
        f = line.split(None, 7)
        if len(f) < 8 or f[3] != "OBJECT":
            continue
        head = _head(f[7])
        if "sg::grad::" in head:
            found.append(head[head.index("sg::grad::"):])
    return found


def test_grad_kernel_objects_are_the_listed_ones():
    found = grad_objects()
    assert len(found) == len(set(found)), "a kernel object appears twice"
    assert not set(found) - set(GRAD_KERNELS), "in the library but not listed: %s" % sorted(set(found) - set(GRAD_KERNELS))
    assert not set(GRAD_KERNELS) - set(found), "listed but not in the library: %s" % sorted(set(GRAD_KERNELS) - set(found))
    assert all(GRAD_KERNELS.values())


def test_symbols_are_bound_and_refuse_without_a_device():
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "seigen_hip.h")).read()
    for name in ("sg_get_gradient_dev", "sg_get_gradient", "sg_gradient_tables", "sg_gradient_plan", "sg_tabulate_grad_cell"):
        assert name in _lib.SYMBOLS and hasattr(L, name) and " %s(" % name in hdr
    buf = np.zeros(16)
    out = np.zeros(6, dtype=np.int64)
    assert L.sg_get_gradient_dev(None, 0, 0, 0, 1, buf.ctypes.data, 0, 128) == -1
    assert L.sg_get_gradient(None, 0, 0, 0, 1, buf.ctypes.data, 128) == -1
    xi = np.zeros((1, 2))
    d = np.zeros((1, 6, 2))
    assert L.sg_tabulate_grad_cell(0, 2, 2, 1, xi.ctypes.data, d.ctypes.data) == 0
    for bad in ((2, 2, 2), (0, 0, 2), (0, 4, 2), (0, 2, 0), (0, 2, 9), (-1, 2, 2)):
        assert L.sg_tabulate_grad_cell(bad[0], bad[1], bad[2], 1, xi.ctypes.data, d.ctypes.data) == -1, bad
    assert L.sg_tabulate_grad_cell(0, 2, 2, -1, xi.ctypes.data, d.ctypes.data) == -1
    assert L.sg_tabulate_grad_cell(0, 2, 2, 1, None, d.ctypes.data) == -1
    assert L.sg_tabulate_grad_cell(0, 2, 2, 1, xi.ctypes.data, None) == -1
    assert L.sg_gradient_tables(None, None, None) == -1
    for dim, degree, diagonal in ((0, 2, 0), (4, 2, 0), (2, 0, 0), (2, 5, 0), (1, 2, 2)):
        cfg = gc.block_cfg(2, 2, (3, 3))
        cfg.dim, cfg.degree, cfg.diagonal = dim, degree, diagonal
        assert L.sg_gradient_tables(C.byref(cfg), None, None) == -1, (dim, degree, diagonal)
    cfg = gc.block_cfg(2, 2, (3, 3))
    cfg.h[1] = 0.0
    assert L.sg_gradient_tables(C.byref(cfg), None, None) == -1
    assert L.sg_gradient_tables(C.byref(gc.block_cfg(3, 4, (2, 2, 2))), None, None) == 3 * 35 * 35       # the size query
    ok = (16, 6, 35, 3, 9, 8, 8, 0, 12)
    assert L.sg_gradient_plan(*ok, out.ctypes.data) == 0
    assert L.sg_gradient_plan(*ok, None) == -1
    for k, v in ((0, 32), (1, 0), (2, 0), (3, 0), (3, 4), (4, 0), (4, 10), (5, 2), (6, 16), (7, -1), (8, -1)):
        bad = list(ok)
        bad[k] = v
        assert L.sg_gradient_plan(*bad, out.ctypes.data) == -1, (k, v)
    # an item whose velocity block leaves no room for one node's values within 64 KiB has no plan
    assert L.sg_gradient_plan(64, 1, 125, 3, 9, 8, 8, 0, 64, out.ctypes.data) == -1


# ---- the tabulation against the exact basis ----------------------------------------------------------------------------
POINTS = {1: [(3,), (11,), (16,), (0,), (17,)], 2: [(3, 5), (1, 1), (7, 9), (0, 4), (12, 0)],
          3: [(2, 3, 5), (1, 1, 1), (4, 6, 7), (0, 5, 2), (9, 3, 0)]}
TAB_CASES = [(ct, dim, P) for ct in (0, 1) for dim in (1, 2, 3) for P in (1, 2, 3, 4, 8) if not (ct == 1 and dim == 1)]
# the largest |lib - exact| / max_a |exact| of sg_tabulate_grad_cell measured on the CPU (see the test's docstring) ...
GRAD_FIGURE = {"low": 2.8e-16, 8: 5.8e-13}
TAB_SEEN = {}


def _figures(ct, dim, P):
    """(figure of sg_tabulate_cell, figure of sg_tabulate_grad_cell): the largest |lib - exact| / max_a |exact| over the points
    (and axes); the differences are taken exactly, in fractions, at the doubles the library was handed"""
    if (ct, dim, P) not in TAB_SEEN:
        xi = np.array(POINTS[dim][:2 if (P == 8 and dim == 3) else 5], dtype=np.float64) / 17.0
        phi, dphi = gc.tabulate_cell(ct, dim, P, xi), gc.tabulate_grad_cell(ct, dim, P, xi)
        fp = fg = 0.0
        for p in range(len(xi)):
            e_phi, e_d = gc.exact_basis(ct, dim, P, [Fraction(float(v)) for v in xi[p]])
            nd = len(e_phi)
            fp = max(fp, float(max(abs(Fraction(float(phi[p, a])) - e_phi[a]) for a in range(nd)) / max(abs(v) for v in e_phi)))
            for r in range(dim):
                top = max(abs(e_d[a][r]) for a in range(nd))
                fg = max(fg, float(max(abs(Fraction(float(dphi[p, a, r])) - e_d[a][r]) for a in range(nd)) / top))
        TAB_SEEN[(ct, dim, P)] = (fp, fg)
    return TAB_SEEN[(ct, dim, P)]


@pytest.mark.parametrize("case", TAB_CASES, ids=["%s-%dd-P%d" % ("simplex" if c[0] == 0 else "tensor", c[1], c[2]) for c in TAB_CASES])
def test_tabulated_derivative_against_the_exact_basis(case):
    """sg_tabulate_grad_cell against the equispaced Lagrange basis differentiated exactly (fractions) at points k / 17, the
    vertices and faces among them.  Measured on the CPU, the largest |lib - exact| / max_a |exact|:
        degrees 1 .. 4:  2.76e-16 (hexahedra DQ_3; simplices at most 1.05e-16, P1 exactly 0)
        degree 8:        5.71e-13 (triangles; tetrahedra 5.40e-13, hexahedra 1.55e-15)
    and the bound is 8 x those.  The yardstick, sg_tabulate_cell measured the same way: 1.9e-16 for degrees 1 .. 4, 8.98e-13 at
    degree 8; the gradient's figure is at most 2.41 x the basis' own in any case, far below (P + 1) * dim."""
    ct, dim, P = case
    fp, fg = _figures(ct, dim, P)
    print("basis %.3e  derivative %.3e" % (fp, fg))
    assert fg <= 8 * GRAD_FIGURE[8 if P == 8 else "low"]
    assert fg <= (P + 1) * dim * max(fp, EPS / 4)


# ---- the tables ----------------------------------------------------------------------------------------------------------
TABLE_BLOCKS = [(dim, P, diagonal) for dim, diags in ((1, ("left",)), (2, ("left", "right", "quadrilateral")), (3, ("left", "quadrilateral")))
                for diagonal in diags for P in (1, 2, 3, 4)]
TABLE_IDS = ["%dd-%s-P%d" % (b[0], b[2], b[1]) for b in TABLE_BLOCKS]


@pytest.mark.parametrize("block", TABLE_BLOCKS, ids=TABLE_IDS)
def test_tables_are_the_tabulation_and_the_mesh_tables(block):
    dim, P, diagonal = block
    quad = diagonal == "quadrilateral"
    cfg = gc.block_cfg(dim, P, (3, 2, 2)[:dim], diagonal)
    Ct, J = gradient_tables(cfg)
    lat = np.array(gc.lattice(int(quad), dim, P), dtype=np.float64)
    dphi = gc.tabulate_grad_cell(int(quad), dim, P, lat / float(P))             # [a][b][r]
    assert np.array_equal(Ct, np.transpose(dphi, (2, 0, 1)))
    h = np.array([cfg.h[a] for a in range(3)])
    if quad:
        want = np.zeros((1, 3, 3))
        for a in range(dim):
            want[0, a, a] = 1.0 / h[a]
        assert np.array_equal(J, want)
        # what the device uses of C on a tensor-product cell: along axis r the 1-D matrix C1 = C[0][:n1][:n1] on the line through
        # a, and nothing off it (there the tabulation leaves rounding noise of the 1-D basis at another node, not zeros)
        t = gc.tables_of(cfg)
        n1 = P + 1
        C1 = Ct[0, :n1, :n1]
        digits = np.stack([np.arange(n1 ** dim) // n1 ** i % n1 for i in range(dim)], axis=-1)
        for r in range(dim):
            assert np.array_equal(Ct[r][t["line"][r]], C1[digits[:, r]].ravel())
            assert np.abs(Ct[r][~t["line"][r]]).max() <= 16 * EPS * np.abs(C1).max()
    else:
        ncls, nfaces = gc.NCLS[dim], dim + 1
        nf = len(gc.lattice(0, dim - 1, P)) if dim > 1 else 1
        nb, nbn = np.zeros((ncls, nfaces, 5), dtype=np.int32), np.zeros((ncls, nfaces, nf), dtype=np.int32)
        cn, jinv = np.zeros((ncls, nfaces, 3)), np.zeros((ncls, 3, 3))
        assert _lib.load().sg_mesh_tables(dim, P, cfg.diagonal, h.ctypes.data, nb.ctypes.data, nbn.ctypes.data, cn.ctypes.data,
                                          jinv.ctypes.data) == 0
        assert np.array_equal(J, jinv)
    # the derivative of a partition of unity vanishes
    assert np.abs(Ct.sum(axis=2)).max() <= 64 * EPS * np.abs(Ct).max()


# ---- the restatement against analytic gradients -----------------------------------------------------------------------------
@pytest.mark.parametrize("block", TABLE_BLOCKS, ids=TABLE_IDS)
def test_restatement_reproduces_polynomials(block):
    """u a different polynomial of the element's space in every cell and component (total degree P on simplices, per-axis
    degree P on tensor-product cells), interpolated at sg_block_node_coords of a block with unequal h, a non-zero origin and
    cube0, through grad_reference, against the analytic gradient at the nodes: |difference| <= 64 (nd + dim) 2^-53 A,
    A[a, i, j] = sum_r |J_rj| sum_b |C_r[a][b]| |u[b][i]|.  The largest ratio |difference| / (2^-53 A) seen on the CPU: 107.7
    (hexahedra DQ_4, bound 64 x 128 = 8192; tetrahedra P4 24.2 of 2432; the 1-D P1 row 0.76 of 192) - the rounding of the node
    coordinates, several cells from the origin, is most of it."""
    dim, P, diagonal = block
    quad = diagonal == "quadrilateral"
    cfg = gc.block_cfg(dim, P, (3, 2, 2)[:dim], diagonal, origin=(0.3, -0.2, 0.15), cube0=(2, 1, 3))
    t = gc.tables_of(cfg)
    X = gc.node_coords(cfg)
    assert X.shape[0] == int(np.prod((3, 2, 2)[:dim])) * t["ncls"]           # every class, in every cube
    u, G = gc.polynomial_field(np.random.default_rng(100 * dim + P), quad, dim, P, X)
    got = gc.grad_reference(t, u)
    A = gc.grad_scale(t, u)
    assert A.min() > 0.0
    ratio = np.abs(got - G) / (EPS * A)
    print("largest |difference| / (2^-53 A): %.2f of %d" % (ratio.max(), 64 * (t["nd"] + dim)))
    assert ratio.max() <= 64 * (t["nd"] + dim)
    # a seeded fault is seen: the transposed J fails wherever J is not symmetric, the class ignored wherever there are several
    JT = np.swapaxes(t["J"], -1, -2)
    if not np.array_equal(JT, t["J"]):
        assert (np.abs(gc.grad_reference(dict(t, J=JT.copy()), u) - G) / (EPS * A)).max() > 1e6
    J0 = np.repeat(t["J"][:1], t["ncls"], axis=0)
    if not np.array_equal(J0, t["J"]):
        assert (np.abs(gc.grad_reference(dict(t, J=J0), u) - G) / (EPS * A)).max() > 1e6
    if dim == 3 and not quad:
        assert not np.array_equal(JT, t["J"]) and not np.array_equal(J0, t["J"])          # the tetrahedra have both


# ---- the plan --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", gc.rows(), ids=[r[0] for r in gc.rows()])
def test_plan_of_every_row_and_kind(row):
    gw, ncls, nd, dim = gc.row_shape(row)
    ncube = int(np.prod(row[3]))
    ncells = ncube * ncls
    dev_bytes = 4 if row[5] == "f32" else 8
    ranges = [(0, ncells), (1, min(ncells - 2, 2 * ncls + 1)), (ncells - ncls - 1, ncls + 1), (ncells - 1, 1), (0, 0)]
    if gw > 1 and ncells > gw * ncls + ncls + 2:          # across the first group boundary, where the block has one
        ranges.append((gw * ncls - ncls - 1, 2 * ncls + 3))
    xout = np.zeros(6, dtype=np.int64)
    for kind in (0, 1, 2, 3):
        if kind == 2 and dim == 1:
            continue
        ncomp = gc.ncomp_of(dim, kind)
        for caller_bytes in (8, 4):
            for c0, k in ranges:
                p = gradient_plan(gw, ncls, nd, dim, ncomp, dev_bytes, caller_bytes, c0, k)
                if k == 0:
                    assert p["grid"] == 0 and p["nitems"] == 0
                    continue
                # the items are those of the transfers
                _lib.check(_lib.load().sg_xfer_plan(gw, ncls, nd, ncomp, dev_bytes, caller_bytes, c0, k, xout.ctypes.data))
                assert (p["item0"], p["nitems"]) == (int(xout[0]), int(xout[1]))
                first, last = c0, c0 + k - 1
                if gw > 1:
                    assert p["item0"] == first // ncls // gw * ncls and p["item0"] + p["nitems"] == (last // ncls // gw + 1) * ncls
                # the slices cover every output node exactly once
                nps, slices = p["nodes_per_slice"], p["slices"]
                seen = np.zeros(nd, dtype=int)
                for s in range(slices):
                    assert s * nps < nd, "an empty slice"
                    seen[s * nps:min(nd, (s + 1) * nps)] += 1
                assert (seen == 1).all()
                if gw == 1:
                    assert p["lds_bytes"] == 0 and slices == 1 and p["grid"] == -(-k * nd // 256)
                else:
                    pitch = gw + 1
                    image = -(-nd * dim * pitch * 8 // 16) * 16
                    assert p["lds_bytes"] == image + nps * ncomp * pitch * 8 <= 65536
                    assert p["grid"] == p["nitems"] * slices
                    # no smaller number of slices would fit
                    if slices > 1:
                        assert image + -(-nd // (slices - 1)) * ncomp * pitch * 8 > 65536
    if row[0] == "hexm-DQ4":
        p = gradient_plan(gw, ncls, nd, dim, 9, 8, 8, 0, ncells)
        assert 125 * 3 * 17 * 8 == 51000 and p["slices"] == 12 and p["nodes_per_slice"] == 11
        assert gradient_plan(gw, ncls, nd, dim, 1, 8, 8, 0, ncells)["slices"] == 2
    if row[0] == "mfma-P4-sym":
        assert gradient_plan(gw, ncls, nd, dim, 9, 8, 8, 0, ncells)["slices"] == 1                 # P4 tetrahedra fit in one slice


def test_plan_grid_is_capped():
    import re
    hdr = open(os.path.join(ROOT, "include", "seigen_hip.h")).read()
    cap = int(re.search(r"#define SG_XFER_GRID_CAP (\d+)", hdr).group(1))
    ncells = 6 * 16 * (cap // 6 + 7)
    p = gradient_plan(16, 6, 35, 3, 9, 8, 8, 0, ncells)
    assert p["nitems"] * p["slices"] > cap and p["grid"] == cap
    p = gradient_plan(1, 2, 6, 2, 4, 8, 8, 0, 64 * cap)
    assert p["grid"] == cap
