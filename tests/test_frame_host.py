"""CPU-only tests of the frames (include/seigen_hip.h sg_get_frame_dev / sg_frame_plan / sg_frame_weights): the kernel objects of
namespace sg::frame in the built library are the listed ones, each with the GPU row that launches it; the plan's extents,
ownership and limits; the plan against the existing locator - the cell of every pixel is what sg_locate_points finds at the
pixel's physical centre, and the pixel centres on the inner faces of the simplices (ties) resolve to the same, lowest class:
the precondition of the comparisons of tests/test_frame_gpu.py; the listed groups cover the cubes of a frame exactly."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from seigen_amd import _lib
from seigen_amd.backend import frame_plan, frame_weights, locate_points, make_frame
from tests import frame_cases as fc
from tests.test_injectors_host import nodes_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Every kernel object of namespace sg::frame (kernels_frame.hip) with the rows of tests/test_frame_gpu.py that launch it.
# tests/test_host_logic.py pins the objects named sg::name(; this list keeps the same rule for the nested namespace.
FRAME_KERNELS = {
    "sg::frame::lanes<double, double>": "double tensor: every f64 row with gw = 16 or 64 (mfma-*, tile-*, hexm-DQ3, lane-2d-P2, the f64 group rows)",
    "sg::frame::lanes<double, float>": "float tensor: the same rows",
    "sg::frame::lanes<float, double>": "double tensor: rows mfma-P3-f32, tile-tri-P3-f32, tile-tri-P3-f32-groups",
    "sg::frame::lanes<float, float>": "float tensor: the f32 rows",
    "sg::frame::flat<double, double>": "double tensor: row generic-2d-P2 (the generic family has double blocks only)",
    "sg::frame::flat<double, float>": "float tensor: row generic-2d-P2",
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


def _frame_objects():
    readelf = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-readelf")
    assert os.path.exists(readelf), "llvm-readelf (shipped with ROCm) not found at %s: set ROCM_PATH" % readelf
    out = subprocess.run([readelf, "--dyn-syms", "--demangle", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    found = []
    for line in out.splitlines():
        f = line.split(None, 7)
        if len(f) < 8 or f[3] != "OBJECT":
            continue
        head = _head(f[7])
        if "sg::frame::" in head:
            found.append(head[head.index("sg::frame::"):])
    return found


def test_frame_kernel_objects_are_the_listed_ones():
    found = _frame_objects()
    assert len(found) == len(set(found)), "a kernel object appears twice"
    assert not set(found) - set(FRAME_KERNELS), "in the library but not listed: %s" % sorted(set(found) - set(FRAME_KERNELS))
    assert not set(FRAME_KERNELS) - set(found), "listed but not in the library: %s" % sorted(set(FRAME_KERNELS) - set(found))
    assert all(FRAME_KERNELS.values())


def _cap():
    hdr = open(os.path.join(ROOT, "include", "seigen_hip.h")).read()
    return int(re.search(r"#define SG_FRAME_GRID_CAP (\d+)", hdr).group(1))


def test_symbols_are_bound_and_refuse_null_without_a_device():
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "seigen_hip.h")).read()
    for name in ("sg_get_frame_dev", "sg_frame_plan", "sg_frame_groups", "sg_frame_weights"):
        assert name in _lib.SYMBOLS and hasattr(L, name) and " %s(" % name in hdr
    fr = make_frame(2, 2)
    buf = np.zeros(8)
    assert L.sg_get_frame_dev(None, 0, C.byref(fr), buf.ctypes.data, 0, None, 64) == -1
    cfg = fc.block_cfg(2, 2, (7, 5))
    out = np.zeros(12, dtype=np.int64)
    assert L.sg_frame_plan(None, C.byref(fr), out.ctypes.data) == -1
    assert L.sg_frame_plan(C.byref(cfg), None, out.ctypes.data) == -1
    assert L.sg_frame_plan(C.byref(cfg), C.byref(fr), None) == -1
    assert L.sg_frame_weights(C.byref(cfg), 2, C.byref(fr), None, None, None) == -1
    assert L.sg_frame_groups(C.byref(cfg), C.byref(fr), out.ctypes.data, 0) == -1      # no room for the groups


def _refused(cfg, m, slice=None):
    out = np.zeros(12, dtype=np.int64)
    fr = make_frame(cfg.dim, m, slice)
    return _lib.load().sg_frame_plan(C.byref(cfg), C.byref(fr), out.ctypes.data) == -1


def test_plan_extents_ownership_and_limits():
    cfg = fc.block_cfg(3, 2, (5, 3, 3))
    p = frame_plan(cfg, make_frame(3, (2, 3, 4)))
    assert p["P"] == (10, 9, 12) and p["Q"] == 24 and p["owns"] and p["layer"] == (-1, -1, -1)
    p = frame_plan(cfg, make_frame(3, (8, 8, 5), {2: 0.5}))       # m is ignored along the sliced axis
    assert p["P"] == (40, 24, 1) and p["Q"] == 64 and p["owns"] and p["layer"] == (-1, -1, 1)
    p = frame_plan(cfg, make_frame(3, 2, {0: 0.5, 1: 0.5}))       # a line
    assert p["P"] == (1, 1, 6) and p["Q"] == 2 and p["layer"] == (2, 1, -1)
    # the limits
    assert _refused(cfg, (9, 1, 1)) and _refused(cfg, (0, 1, 1)) and _refused(cfg, (1, -1, 1))
    assert _refused(cfg, (5, 13, 1), {2: 0.5})
    assert not _refused(cfg, (8, 8, 1)) and _refused(cfg, (8, 8, 2))           # Q = 64 is the last one taken
    cfg2 = fc.block_cfg(2, 3, (7, 5))
    assert not _refused(cfg2, (8, 8))
    # (Q = 65 = 5 * 13 has no factors within m <= 8: the products just above 64 stand for it)
    assert _refused(cfg, (3, 3, 8)) and _refused(cfg, (5, 4, 4)) and _refused(cfg, (8, 3, 3))
    assert _refused(cfg, 2, {0: 0.1, 1: 0.1, 2: 0.1})                          # no free axis
    assert _refused(fc.block_cfg(1, 2, (9,)), 2, {0: 0.5})
    assert _refused(cfg, 2, {2: float("nan")})
    fr = make_frame(3, 2)
    fr.fixed[1] = 2
    out = np.zeros(12, dtype=np.int64)
    assert _lib.load().sg_frame_plan(C.byref(cfg), C.byref(fr), out.ctypes.data) == -1
    # ownership: the lower layer on a grid plane where the mesh has one, nothing outside the mesh, and by block of a split mesh
    for z, layer in ((0.0, 0), (0.2, 0), (1.0 / 3, 0), (1.0 / 3 + 1e-6, 1), (2.0 / 3, 1), (1.0, 2)):
        p = frame_plan(cfg, make_frame(3, 2, {2: z}))
        assert p["owns"] and p["layer"] == (-1, -1, layer), (z, p)
    for z in (-0.01, 1.01, 7.0):
        p = frame_plan(cfg, make_frame(3, 2, {2: z}))
        assert not p["owns"] and p["ngroups"] == 0 and p["grid"] == 0 and p["units"] == 0 and p["P"] == (10, 6, 1)
    lower = fc.block_cfg(3, 2, (5, 3, 2), mesh_n=(5, 3, 3))
    upper = fc.block_cfg(3, 2, (5, 3, 1), cube0=(0, 0, 2), mesh_n=(5, 3, 3))
    for z, who in ((0.5, "lower"), (2.0 / 3, "lower"), (0.7, "upper"), (1.0, "upper")):
        a, b = frame_plan(lower, make_frame(3, 2, {2: z})), frame_plan(upper, make_frame(3, 2, {2: z}))
        assert (a["owns"], b["owns"]) == (who == "lower", who == "upper"), (z, a, b)
        assert (b["layer"][2] if b["owns"] else a["layer"][2]) == (0 if who == "upper" else 1)


BLOCKS = [
    ("tri-left", 2, 2, (7, 5), "left"),
    ("tri-right", 2, 3, (7, 5), "right"),
    ("quad", 2, 2, (7, 5), "quadrilateral"),
    ("tet", 3, 2, (5, 3, 3), "left"),
    ("hex", 3, 2, (5, 3, 3), "quadrilateral"),
    ("line", 1, 2, (9,), "left"),
]


def _unit_classes(dim, diagonal, t):
    """the classes of the unit cube whose simplex holds the cube fraction t within the locator's 1e-12, from the P1 node
    coordinates of the unit block (its cells' vertices) by barycentric coordinates in numpy"""
    cfg = fc.block_cfg(dim, 1, (1,) * dim, diagonal)
    ncls = {1: 1, 2: 2, 3: 6}[dim]
    X = np.empty((ncls, dim + 1, dim))
    _lib.check(_lib.load().sg_block_node_coords(C.byref(cfg), 1, X.ctypes.data, X.nbytes))
    inside = []
    for k in range(ncls):
        A = np.vstack([X[k].T, np.ones(dim + 1)])
        lam = np.linalg.solve(A, np.append(t, 1.0))
        if lam.min() >= -1e-12:
            inside.append(k)
    return inside


@pytest.mark.parametrize("block", BLOCKS, ids=[b[0] for b in BLOCKS])
def test_plan_against_the_locator(block):
    name, dim, degree, n, diagonal = block
    quad = diagonal == "quadrilateral"
    cfg = fc.block_cfg(dim, degree, n, diagonal)
    nd = nodes_of(dim, degree, quad)
    ncls = 1 if quad else {1: 1, 2: 2, 3: 6}[dim]
    ties = {}
    for m, slice in fc.frames_of(dim, n):
        px = fc.pixels(cfg, m, slice)
        assert px["owns"]
        fr = px["frame"]
        cls, xi, phi = frame_weights(cfg, degree, fr, nd)
        assert len(px["cube"]) == px["P"][0] * px["P"][1] * px["P"][2]
        assert len({tuple(i) for i in px["index"]}) == len(px["cube"])          # every pixel once
        assert set(px["q"]) == set(range(px["Q"]))
        cell, xi_phys = locate_points(cfg, px["centre"])
        assert np.array_equal(cell, px["cube"] * ncls + cls[px["q"]]), (name, m, slice)
        assert np.abs(xi_phys - xi[px["q"]]).max() <= 1e-12, (name, m, slice)
        want = np.empty_like(phi)
        _lib.check(_lib.load().sg_tabulate_cell(1 if quad else 0, dim, degree, len(xi), np.ascontiguousarray(xi).ctypes.data, want.ctypes.data))
        assert np.array_equal(phi, want)
        if slice is None and not quad and dim > 1:
            # pixel centres on the inner faces of the simplices: more than one class holds them, the lowest wins - on the
            # unit block and, by the comparison above, for the physical locator too
            nt = 0
            mm = [fr.m[a] for a in range(dim)]
            for q in range(px["Q"]):
                j = [q % mm[0], q // mm[0] % mm[1]] + ([q // (mm[0] * mm[1])] if dim == 3 else [])
                t = np.array([(j[a] + 0.5) / mm[a] for a in range(dim)])
                inside = _unit_classes(dim, diagonal, t)
                assert inside and cls[q] == inside[0], (name, m, q, inside, cls[q])
                nt += len(inside) > 1
            ties[m] = nt
    if not quad and dim == 2:
        assert ties[1] == 1 and ties[4] == 4 and ties[(2, 3)] == 0, ties      # j = k or j + k = m - 1
    if not quad and dim == 3:
        assert ties[(2, 2, 2)] > 0, ties


@pytest.mark.parametrize("path,gw", [(None, 16), ("lane", 64), ("generic", 1)])
def test_listed_groups_cover_the_frame(monkeypatch, path, gw):
    """the kernel's walk: lane w of listed group g is cube g * gw + w; the cubes of the frame's layer occur exactly once, in a
    listed group, and no listed group is without one; units and grid follow"""
    if path:
        monkeypatch.setenv("SEIGEN_HIP_PATH", path)
    else:
        monkeypatch.delenv("SEIGEN_HIP_PATH", raising=False)
    cap = _cap()
    n = (5, 4, 7)
    cfg = fc.block_cfg(3, 2, n)
    ncube = n[0] * n[1] * n[2]
    for m, slice in fc.frames_of(3, n) + [((1, 1, 1), {0: 0.5, 2: 0.5})]:
        p = frame_plan(cfg, make_frame(3, m, slice))
        assert p["gw"] == gw and p["owns"]
        g = p["groups"]
        assert np.all(np.diff(g) > 0) and g.min() >= 0 and g.max() * gw < ncube
        cubes = (g[:, None].astype(np.int64) * gw + np.arange(gw)[None, :]).ravel()
        cubes = cubes[cubes < ncube]
        c = np.stack([cubes % n[0], cubes // n[0] % n[1], cubes // (n[0] * n[1])], axis=-1)
        keep = np.ones(len(cubes), dtype=bool)
        for a in range(3):
            if p["layer"][a] >= 0:
                keep &= c[:, a] == p["layer"][a]
        want = np.prod([1 if p["layer"][a] >= 0 else n[a] for a in range(3)])
        assert keep.sum() == want and len(set(cubes[keep])) == want
        assert set(cubes[keep] // gw) == set(g)                                 # no listed group without a cube of the layer
        if gw == 1:
            assert p["units"] == want * p["Q"] and p["grid"] == min(cap, -(-p["units"] // 256))
        else:
            assert p["units"] == -(-len(g) // (64 // gw)) * 6 and p["grid"] == min(cap, -(-p["units"] // 4))
        assert 1 <= p["grid"] <= cap
