"""CPU-only tests of the host logic: the C-ABI library loads and exports every symbol the
header declares, the device-free setup code (reference operators, mesh tables, node
coordinates) agrees with the oracle, the Expression parser, partitioning, step counting."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from oracle import mesh as omesh
from oracle import refelem
from seigen_amd import _lib
from seigen_amd.expression import Expression
from seigen_amd.mesh import Partition, UnitSquareMesh, UnitCubeMesh, RectangleMesh, IntervalMesh
from seigen_amd.functionspace import FunctionSpace, VectorFunctionSpace, TensorFunctionSpace, Function

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lib():
    return _lib.load()


# ------------------------------------------------------------------------------ C-ABI surface
def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "seigen_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(sg_[A-Za-z_]+)\s*\(", hdr))
    assert declared, "no declarations found in the header"
    assert declared == set(_lib.SYMBOLS), (declared ^ set(_lib.SYMBOLS))
    L = lib()
    for name in declared:
        assert hasattr(L, name), "libseigen_hip.so does not export %s" % name


def test_mfma_family_instantiations_are_the_listed_ones():
    """The kernel objects of the 3-D matrix-pipe family in the built library are exactly MFMA_KERNELS, the list
    tests/test_mfma_family_gpu.py checks row by row against the oracle: no instantiation joins or leaves unseen."""
    import subprocess
    from tests.test_mfma_family_gpu import MFMA_KERNELS
    readelf = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-readelf")
    assert os.path.exists(readelf), "llvm-readelf (shipped with ROCm) not found at %s: set ROCM_PATH" % readelf
    out = subprocess.run([readelf, "--dyn-syms", "--demangle", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    pat = re.compile(r"\bOBJECT\b.*?\b(sg::(?:mfma_stage_[FG]|sponge_affine_mfma)<[^>]*>)\(")
    found = {m.group(1) for m in map(pat.search, out.splitlines()) if m}
    assert not MFMA_KERNELS - found, "listed but not in the library: %s" % sorted(MFMA_KERNELS - found)
    assert not found - MFMA_KERNELS, "in the library but not listed in MFMA_KERNELS: %s" % sorted(found - MFMA_KERNELS)
    assert len(found) == 140


def _kernel_objects():
    """the demangled names of the library's kernel objects: the host-side handles of its __global__ functions, OBJECT
    symbols whose names are function signatures (`void ` in front of a template's)"""
    import subprocess
    readelf = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-readelf")
    assert os.path.exists(readelf), "llvm-readelf (shipped with ROCm) not found at %s: set ROCM_PATH" % readelf
    out = subprocess.run([readelf, "--dyn-syms", "--demangle", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    pat = re.compile(r"\bOBJECT\b.*?\s(?:void )?(sg::\w+(?:<[^>]*>)?)\(")
    return [m.group(1) for m in map(pat.search, out.splitlines()) if m]


@pytest.mark.parametrize("family,count", [("tile2d_stage", 320), ("hexm_stage", 20), ("hex_stage", 16), ("lane_stage", 80),
                                          ("stage_kernel", 40)])
def test_tile2d_and_hexahedral_family_instantiations_are_the_listed_ones(family, count):
    """The kernel objects of the 2-D tile family, of the two hexahedral families, of the lane-per-cell family and of the
    generic family in the built library are exactly TILE2D_KERNELS, HEXM_KERNELS, HEX_LANE_KERNELS, LANE_KERNELS and
    GENERIC_KERNELS, the lists tests/test_tile2d_family_gpu.py, tests/test_hex_family_gpu.py and
    tests/test_lane_generic_family_gpu.py check row by row against the oracle: no instantiation joins or leaves unseen."""
    import subprocess
    from tests.test_hex_family_gpu import HEXM_KERNELS, HEX_LANE_KERNELS
    from tests.test_lane_generic_family_gpu import GENERIC_KERNELS, LANE_KERNELS
    from tests.test_tile2d_family_gpu import TILE2D_KERNELS
    listed = {"tile2d_stage": TILE2D_KERNELS, "hexm_stage": HEXM_KERNELS, "hex_stage": HEX_LANE_KERNELS,
              "lane_stage": LANE_KERNELS, "stage_kernel": GENERIC_KERNELS}[family]
    readelf = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-readelf")
    assert os.path.exists(readelf), "llvm-readelf (shipped with ROCm) not found at %s: set ROCM_PATH" % readelf
    out = subprocess.run([readelf, "--dyn-syms", "--demangle", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    pat = re.compile(r"\bOBJECT\b.*?\b(sg::%s<[^>]*>)\(" % family)
    found = {m.group(1) for m in map(pat.search, out.splitlines()) if m}
    assert not listed - found, "listed but not in the library: %s" % sorted(listed - found)
    assert not found - listed, "in the library but not listed: %s" % sorted(found - listed)
    assert len(found) == count


# The kernel objects that are no stage kernel of a family (kernels.hip, kernels_recv.hip), each with a test that launches it.
AUX_KERNELS = {
    "sg::layout_kernel<double>": "every set_field / get_field of a double block, e.g. test_parity_gpu.py",
    "sg::layout_kernel<float>": "every set_field / get_field of a float block: test_fp32_gpu.py",
    "sg::mirror_kernel<double>": "a non-symmetric stress uploaded to an interleaved block: the full-tensor rows of the family modules",
    "sg::mirror_kernel<float>": "the f32 full-tensor rows of test_tile2d_family_gpu.py and test_mfma_family_gpu.py",
    "sg::pack_kernel<double>": "every halo_pack of a split: test_harness_gpu.py test_multiblock_equals_single_block",
    "sg::pack_kernel<float>": "the f32 splits of test_tile2d_family_gpu.py and test_mfma_family_gpu.py",
    "sg::source_kernel<double>": "every source outside the 2-D tile family: the rows of test_lane_generic_family_gpu.py",
    "sg::source_kernel<float>": "the f32 rows of test_mfma_family_gpu.py",
    "sg::sponge_pre_kernel<double>": "general nodal sponge cells of the pre-pass families: the lane rows of test_lane_generic_family_gpu.py",
    "sg::sponge_pre_kernel<float>": "the f32 rows of test_mfma_family_gpu.py",
    "sg::receiver_sample<double>": "test_receivers_gpu.py",
    "sg::receiver_sample<float>": "test_receivers_gpu.py, case mfma-P4-f32",
    "sg::sponge_pre_affine_kernel<double, 1>": "the 1-D SEIGEN_HIP_SPONGE_AFFINE=1 rows of test_lane_generic_family_gpu.py",
    "sg::sponge_pre_affine_kernel<double, 2>": "the 2-D SEIGEN_HIP_SPONGE_AFFINE=1 row of test_lane_generic_family_gpu.py",
    "sg::sponge_pre_affine_kernel<double, 3>": "the hexm rows and the DQ_2 affine row of test_hex_family_gpu.py",
    "sg::sponge_pre_affine_kernel<float, 3>": "the f32 rows of test_mfma_family_gpu.py",
    # float blocks exist on the 3-D MFMA family and the 2-D tile family only (api.cpp sg_create, hostlogic.hpp family_f32);
    # 1-D has neither, and the 2-D tile kernels take no pre-pass (family_sponge_pre), so sg_set_absorption never plans
    # affine cells for them: launch_sponge_pre_affine's two arms are dead code kept for the dispatch's regularity
    "sg::sponge_pre_affine_kernel<float, 1>": "no caller can reach",
    "sg::sponge_pre_affine_kernel<float, 2>": "no caller can reach",
    "sg::step_counter_kernel": "every graph-replayed step with a source or receivers: test_graph_source_gpu.py",
}


def test_every_kernel_object_belongs_to_exactly_one_list():
    """Every kernel object of the library is in exactly one of the seven lists - six stage families, whose every member a
    row compares with the oracle, and AUX_KERNELS - and nothing listed is missing: no kernel joins the library without a
    decision about who tests it."""
    from tests.test_hex_family_gpu import HEXM_KERNELS, HEX_LANE_KERNELS
    from tests.test_lane_generic_family_gpu import GENERIC_KERNELS, LANE_KERNELS
    from tests.test_mfma_family_gpu import MFMA_KERNELS
    from tests.test_tile2d_family_gpu import TILE2D_KERNELS
    lists = [MFMA_KERNELS, TILE2D_KERNELS, HEXM_KERNELS, HEX_LANE_KERNELS, LANE_KERNELS, GENERIC_KERNELS, frozenset(AUX_KERNELS)]
    assert [len(k) for k in lists] == [140, 320, 20, 16, 80, 40, 19]
    listed = frozenset().union(*lists)
    total = sum(len(k) for k in lists)
    assert len(listed) == total == 635, "a kernel is in two lists"
    found = _kernel_objects()
    assert len(found) == len(set(found)), "a kernel object appears twice"
    assert not set(found) - listed, "in the library but in no list: %s" % sorted(set(found) - listed)
    assert not listed - set(found), "listed but not in the library: %s" % sorted(listed - set(found))
    assert len(found) == total
    assert all(note for note in AUX_KERNELS.values())
    assert sorted(k for k, note in AUX_KERNELS.items() if note == "no caller can reach") == [
        "sg::sponge_pre_affine_kernel<float, 1>", "sg::sponge_pre_affine_kernel<float, 2>"]


def test_create_fails_loudly_without_device_or_bad_args():
    L = lib()
    cfg = _lib.SgConfig()
    cfg.dim, cfg.degree = 7, 1
    h = C.c_void_p()
    rc = L.sg_create(C.byref(cfg), C.byref(h))
    assert rc != 0 and not h.value
    assert L.sg_last_error(None)
    from tests.conftest import have_gpu
    if not have_gpu():
        # no CPU fallback: a valid configuration must still fail without a HIP device
        cfg.dim, cfg.degree = 2, 1
        cfg.n[0] = cfg.n[1] = 2
        cfg.h[0] = cfg.h[1] = 0.5
        rc = L.sg_create(C.byref(cfg), C.byref(h))
        assert rc == -2 and not h.value
        assert b"no HIP device" in L.sg_last_error(None)
        from seigen_amd import ElasticLF4
        with pytest.raises(_lib.SeigenHipError):
            ElasticLF4.create(UnitSquareMesh(2, 2), "DG", 1, dimension=2, output=False)


# ------------------------------------------------------------------------------ reference element
def refop(dim, P, which, q=0):
    L = lib()
    n = L.sg_reference_operator(dim, P, which, q, None, 0)
    assert n > 0
    out = np.empty(n)
    assert L.sg_reference_operator(dim, P, which, q, out.ctypes.data, out.nbytes) == n
    return out


@pytest.mark.parametrize("dim", [1, 2, 3])
@pytest.mark.parametrize("P", [1, 2, 3, 4])
def test_reference_operators_match_oracle_quadrature(dim, P):
    """C++ (exact monomial integration, long double) vs oracle (Gauss-Jacobi quadrature of the
    closed-form Lagrange basis): D_r = Mhat^-1 Shat_r, Mhat, facet lifts."""
    nd = refelem.nnodes(dim, P)
    xq, wq = refelem.simplex_quadrature(dim, 2 * P)
    phi, dphi = refelem.tabulate(dim, P, xq)
    M = np.einsum('q,qa,qb->ab', wq, phi, phi)
    Minv = np.linalg.inv(M)
    D_or = np.stack([Minv @ np.einsum('q,qa,qb->ab', wq, dphi[:, :, r], phi) for r in range(dim)])
    D = refop(dim, P, 0).reshape(dim, nd, nd)
    Mh = refop(dim, P, 2).reshape(nd, nd)
    assert np.abs(D - D_or).max() / np.abs(D_or).max() < 1e-12
    assert np.abs(Mh - M).max() / np.abs(M).max() < 1e-13
    nf = refelem.nnodes(dim - 1, P) if dim > 1 else 1
    Lf = refop(dim, P, 1).reshape(dim + 1, nd, nf)
    fn = refop(dim, P, 4).reshape(dim + 1, nf).astype(int)
    xf, wf = refelem.simplex_quadrature(dim - 1, 2 * P)
    bary = np.concatenate([1 - xf.sum(1, keepdims=True), xf], axis=1)
    V = np.vstack([np.zeros(dim), np.eye(dim)])
    for f in range(dim + 1):
        assert (fn[f] == refelem.face_nodes(dim, P, f)).all()
        pts = bary @ V[refelem.face_vertices(dim, f)]
        ph, _ = refelem.tabulate(dim, P, pts)
        Mf = np.einsum('q,qa,qb->ab', wf * math.factorial(dim - 1), ph, ph)   # unit facet measure
        full = Minv @ Mf
        mask = np.ones(nd, bool)
        mask[fn[f]] = False
        assert np.abs(full[:, mask]).max() < 1e-11          # basis functions off the facet vanish on it
        assert np.abs(Lf[f] - full[:, fn[f]]).max() / np.abs(full).max() < 1e-12


@pytest.mark.parametrize("dim,P,q", [(1, 1, 2), (2, 2, 4), (3, 2, 2), (2, 3, 4)])
def test_sponge_tensor(dim, P, q):
    nd, nq = refelem.nnodes(dim, P), refelem.nnodes(dim, q)
    A = refop(dim, P, 3, q).reshape(nd, nq, nd)
    xq, wq = refelem.simplex_quadrature(dim, 2 * P + q)
    phi, _ = refelem.tabulate(dim, P, xq)
    psi, _ = refelem.tabulate(dim, q, xq)
    xm, wm = refelem.simplex_quadrature(dim, 2 * P)
    pm, _ = refelem.tabulate(dim, P, xm)
    Minv = np.linalg.inv(np.einsum('q,qa,qb->ab', wm, pm, pm))
    A_or = np.einsum('ak,q,qk,qc,qb->acb', Minv, wq, phi, psi, phi)
    assert np.abs(A - A_or).max() / np.abs(A_or).max() < 1e-11


def test_tabulate_matches_closed_form():
    from seigen_amd.norms import tabulate
    rng = np.random.default_rng(0)
    for dim in (1, 2, 3):
        for P in (1, 3, 6):
            xi = rng.dirichlet(np.ones(dim + 1), size=20)[:, 1:]
            phi, _ = refelem.tabulate(dim, P, xi)
            assert np.abs(tabulate(dim, P, xi) - phi).max() < 1e-10


# ------------------------------------------------------------------------------ mesh tables
@pytest.mark.parametrize("dim,P,diag", [(1, 2, "left"), (2, 1, "left"), (2, 3, "left"), (2, 2, "right"),
                                        (3, 1, "left"), (3, 2, "left"), (3, 4, "left")])
def test_mesh_tables_match_explicit_connectivity(dim, P, diag):
    """Neighbour class / facet / node matching / scaled normals of the structured mesh (C++)
    against the oracle's connectivity derived from vertex ids on a 3^dim patch."""
    L = lib()
    ncls = {1: 1, 2: 2, 3: 6}[dim]
    nfaces = dim + 1
    nf = refelem.nnodes(dim - 1, P) if dim > 1 else 1
    h = np.array([0.5, 0.25, 0.2][:dim])
    nb = np.zeros((ncls, nfaces, 5), dtype=np.int32)
    nbn = np.zeros((ncls, nfaces, nf), dtype=np.int32)
    cn = np.zeros((ncls, nfaces, 3))
    jinv = np.zeros((ncls, 3, 3))
    hh = np.ascontiguousarray(h)
    rc = L.sg_mesh_tables(dim, P, 1 if diag == "right" else 0, hh.ctypes.data, nb.ctypes.data, nbn.ctypes.data,
                          cn.ctypes.data, jinv.ctypes.data)
    assert rc == 0
    n = (3,) * dim
    m = omesh.structured(dim, n, tuple(3 * h), diag)
    X = m.node_coords(P)
    centre = sum(1 * (3 ** a) for a in range(dim))      # cube (1,1,1)
    nbr_of = {}
    for (c1, f1, c2, f2) in m.interior_facets:
        nbr_of[(c1, f1)] = (c2, f2)
        nbr_of[(c2, f2)] = (c1, f1)
    strides = [3 ** a for a in range(dim)]
    for k in range(ncls):
        cell = centre * ncls + k
        assert np.allclose(jinv[k, :dim, :dim], m.Jinv[cell], atol=1e-13)
        for f in range(nfaces):
            c2, f2 = nbr_of[(cell, f)]
            axis, d_, kn, fn_, _ = nb[k, f]
            cube2 = centre + (d_ * strides[axis] if axis >= 0 else 0)
            assert c2 == cube2 * ncls + kn and f2 == fn_
            normal, area = m.facet_geometry(np.array([cell]), np.array([f]))
            assert np.allclose(cn[k, f, :dim], normal[0] * area[0] / abs(m.detJ[cell]), atol=1e-12)
            fnodes = refelem.face_nodes(dim, P, f)
            for b in range(nf):
                assert np.allclose(X[cell, fnodes[b]], X[c2, nbn[k, f, b]], atol=1e-12)
    # facets on one cube side get distinct ordinals 0..hpc-1
    for side in range(2 * dim):
        ords = sorted(nb[k, f, 4] for k in range(ncls) for f in range(nfaces)
                      if nb[k, f, 0] == side // 2 and (nb[k, f, 1] > 0) == bool(side & 1))
        assert ords == list(range(2 if dim == 3 else 1))


@pytest.mark.parametrize("mesh,om", [
    (IntervalMesh(5, 2.0), omesh.IntervalMesh(5, 2.0)),
    (UnitSquareMesh(3, 4), omesh.UnitSquareMesh(3, 4)),
    (RectangleMesh(4, 3, 2.0, 1.5, "right"), omesh.RectangleMesh(4, 3, 2.0, 1.5, "right")),
    (UnitCubeMesh(2, 3, 2), omesh.UnitCubeMesh(2, 3, 2)),
])
def test_node_coordinates(mesh, om):
    for P in (1, 2, 4):
        fs = FunctionSpace(mesh, "DG", P)
        np.testing.assert_allclose(fs.node_coords(), om.node_coords(P), rtol=0, atol=1e-13)


# ------------------------------------------------------------------------------ Expression
def test_expression_parser():
    X = np.random.default_rng(1).uniform(0, 300, (50, 2))
    x, y = X[:, 0], X[:, 1]
    e = Expression("x[0] <= 20 || x[0] >= 280 || x[1] <= 20.0 ? 1000 : 0")
    np.testing.assert_array_equal(e.evaluate(X), np.where((x <= 20) | (x >= 280) | (y <= 20), 1000.0, 0.0))
    a = 159.42
    code = ("x[0] >= 44.5 && x[0] <= 45.5 && x[1] >= 148.5 && x[1] <= 149.5 ? "
            "(-1.0 + 2*a*pow(t - 0.3, 2))*exp(-a*pow(t - 0.3, 2)) : 0.0")
    e = Expression(((code, "0.0"), ("0.0", code)), a=a, t=0.31)
    Xs = np.array([[45.0, 148.75], [45.0, 140.0], [44.5, 149.5]])
    r = (-1.0 + 2 * a * (0.31 - 0.3) ** 2) * math.exp(-a * (0.31 - 0.3) ** 2)
    v = e.evaluate(Xs)
    assert v.shape == (3, 2, 2)
    np.testing.assert_allclose(v[:, 0, 0], [r, 0.0, r], rtol=1e-15)
    np.testing.assert_array_equal(v[:, 0, 1], 0.0)
    e.t = 0.3
    assert e.evaluate(Xs)[0, 1, 1] == -1.0
    e2 = Expression(('a*cos(pi*x[0])*sin(pi*x[1])*cos(a*t)', '-a*sin(pi*x[0])*cos(pi*x[1])*cos(a*t)'), a=2.0, t=0)
    np.testing.assert_allclose(e2.evaluate(X / 300)[:, 0], 2 * np.cos(np.pi * x / 300) * np.sin(np.pi * y / 300),
                               rtol=1e-14)
    assert Expression("!(x[0] > 1) ? 2e-3 : -1.5E2").evaluate(np.array([[0.5], [2.0]])).tolist() == [2e-3, -150.0]
    with pytest.raises(NameError):
        Expression("foo*x[0]").evaluate(X)


def test_source_support_with_time_unknown():
    """The per-step source table (seigen_amd/elastic.py _source_table; the reference re-interpolates
    at every step, elastic.py:285-288) is built on Expression.support_mask: where the source CAN be
    non-zero at some time.  A source that is zero at every sampled instant must not be lost."""
    rng = np.random.default_rng(1)
    X = rng.uniform(0, 10, (50, 6, 2))
    box = "x[0] >= 2 && x[0] <= 5 && x[1] >= 1 && x[1] <= 4"
    inbox = (X[..., 0] >= 2) & (X[..., 0] <= 5) & (X[..., 1] >= 1) & (X[..., 1] <= 4)
    ricker = "(-1.0 + 2*a*pow(t - 0.3, 2))*exp(-a*pow(t - 0.3, 2))"
    # the reference's shape: spatial condition ? f(t) : 0  -> exactly the box
    e = Expression((("%s ? %s : 0.0" % (box, ricker), "0.0"), ("0.0", "%s ? %s : 0.0" % (box, ricker))), a=159.42, t=0)
    np.testing.assert_array_equal(e.support_mask(X), inbox)
    # time window inside the condition: zero at t = 0 (and at any handful of samples), support still the box
    e = Expression("%s && t >= 0.30 && t <= 0.31 ? 1.0 : 0.0" % box, t=0)
    assert not e.nonzero_mask(X).any()
    np.testing.assert_array_equal(e.support_mask(X), inbox)
    # window as a factor
    e = Expression("(%s ? 2.0 : 0.0) * (t >= 0.30 && t <= 0.31 ? sin(t) : 0.0)" % box, t=0)
    np.testing.assert_array_equal(e.support_mask(X), inbox)
    # a source whose position depends on t can reach every node of the strip it moves in
    e = Expression("x[0] >= 10*t && x[0] <= 10*t + 1 && x[1] <= 4 ? 1.0 : 0.0", t=0)
    np.testing.assert_array_equal(e.support_mask(X), X[..., 1] <= 4)
    # no t at all: support = where it is non-zero
    e = Expression("%s ? 3.0 : 0.0" % box)
    np.testing.assert_array_equal(e.support_mask(X), inbox)
    # support is a superset of the instantaneous non-zero set at any time
    e = Expression("%s ? cos(7*t)*x[0] : 0.0" % box, t=0)
    for t in (0.0, 0.1, 0.2243, 1.7):
        e.t = t
        assert not (e.nonzero_mask(X) & ~e.support_mask(X)).any()


def test_function_interpolate_and_assign():
    mesh = UnitSquareMesh(2, 2)
    U = VectorFunctionSpace(mesh, "DG", 2)
    S = TensorFunctionSpace(mesh, "DG", 2)
    assert U.dof_count == 8 * 6 * 2 and S.dof_count == 8 * 6 * 4
    f = Function(U).interpolate(Expression(("x[0]", "2*x[1]")))
    X = U.node_coords()
    np.testing.assert_allclose(f.dat.data_cells[..., 0], X[..., 0])
    np.testing.assert_allclose(f.dat.data_cells[..., 1], 2 * X[..., 1])
    g = Function(U).assign(f)
    np.testing.assert_array_equal(g.dat.data, f.dat.data)
    assert f.dat.data.shape == (48, 2)
    with pytest.raises(ValueError):
        Function(S).interpolate(Expression(("x[0]", "2*x[1]")))
    with pytest.raises(NotImplementedError):
        FunctionSpace(mesh, "CG", 1)


# ------------------------------------------------------------------------------ partition / steps
def test_partition_covers_mesh():
    for n, world in (((64, 64, 64), 8), ((10, 7), 4), ((9,), 3), ((128, 128, 128), 2)):
        seen = np.zeros(n, dtype=int)
        for r in range(world):
            p = Partition(n, r, world)
            sl = tuple(slice(p.start[a], p.start[a] + p.n[a]) for a in range(len(n)))
            seen[sl] += 1
            for s in range(2 * len(n)):
                nb = p.neighbour(s)
                if nb is not None:
                    q = Partition(n, nb, world)
                    assert q.neighbour(s ^ 1) == r
                    axis = s >> 1
                    for a in range(len(n)):
                        if a != axis:
                            assert (p.start[a], p.n[a]) == (q.start[a], q.n[a])
                assert bool(p.nbr_mask >> s & 1) == (nb is not None)
        assert (seen == 1).all()


def _region_boxes(dim, n, mask, region):
    cfg = _lib.SgConfig()
    cfg.dim, cfg.degree = dim, 1
    for a in range(3):
        cfg.n[a] = n[a] if a < dim else 1
        cfg.h[a] = 1.0
    cfg.nbr_mask = mask
    buf = (C.c_int32 * (6 * 16))()
    cnt = lib().sg_region_boxes(C.byref(cfg), region, buf, 16)
    assert 0 <= cnt <= 16
    return [tuple(buf[6 * i + k] for k in range(6)) for i in range(cnt)]


@pytest.mark.parametrize("dim,n", [(3, (6, 5, 7)), (3, (2, 2, 2)), (3, (16, 3, 1)), (2, (9, 4)), (1, (5,))])
def test_region_boxes_partition_the_block_for_every_neighbour_mask(dim, n):
    """The regions of a split stage (include/seigen_hip.h, enum sg_region) for EVERY combination of
    block sides with a neighbour, all six included (a 3x3x3 process grid's centre block): the boxes
    of a region are disjoint, INTERIOR + BOUNDARY = FIRST + SECOND = ALL, the shell is exactly the
    cubes with a neighbour across one of their faces, and no region needs more boxes than a stage
    launch can carry (SG_MAX_REGION_BOXES; stages.cpp refuses beyond that)."""
    hdr = open(os.path.join(ROOT, "include", "seigen_hip.h")).read()
    max_boxes = int(re.search(r"#define SG_MAX_REGION_BOXES (\d+)", hdr).group(1))
    full = tuple(n) + (1,) * (3 - dim)
    # group width of the layout such a block gets (degree 1): 2-D blocks run the tile kernels (16), small 3-D and
    # 1-D blocks the generic kernel (1)
    gw = 16 if dim == 2 else 1
    for mask in range(1 << (2 * dim)):
        cover = {}
        for region in range(5):
            boxes = _region_boxes(dim, n, mask, region)
            assert len(boxes) <= max_boxes, (mask, region, boxes)
            seen = np.zeros(full, dtype=int)
            for (o0, o1, o2, n0, n1, n2) in boxes:
                assert n0 > 0 and n1 > 0 and n2 > 0
                seen[o0:o0 + n0, o1:o1 + n1, o2:o2 + n2] += 1
            assert seen.max() <= 1, "boxes of a region overlap"
            cover[region] = seen
        assert (cover[0] == 1).all()
        np.testing.assert_array_equal(cover[1] + cover[2], cover[0])
        np.testing.assert_array_equal(cover[3] + cover[4], cover[0])
        shell = np.zeros(full, dtype=int)
        for a in range(dim):
            idx = [slice(None)] * 3
            if mask >> (2 * a) & 1:
                idx[a] = 0
                shell[tuple(idx)] = 1
            if mask >> (2 * a + 1) & 1:
                idx[a] = full[a] - 1
                shell[tuple(idx)] = 1
        assert (cover[2] >= shell).all(), "BOUNDARY contains every cube with a neighbour block across a face"
        # Along x the shell is a whole layout group thick where the block's kernels interleave gw cubes of an
        # x-row per item (handle.hpp shell_width_x): extra cubes lie within gw - 1 of an x side with a neighbour
        # ... as long as that leaves the launch beside the exchange at least half of the rows (else: one cube)
        xsides = (mask & 1) + ((mask >> 1) & 1)
        thick = gw > 1 and 2 * (full[0] - xsides * gw) >= full[0]
        extra = cover[2] - shell
        if extra.any():
            assert thick
            ok = np.zeros(full, dtype=int)
            if mask & 1:
                ok[:min(gw, full[0])] = 1
            if mask & 2:
                ok[max(full[0] - gw, 0):] = 1
            assert (extra <= ok).all()
        elif thick and (mask & 3):
            assert False, "an x side with a neighbour block must make a group-thick shell"
        if all(full[a] >= 2 for a in range(dim)) and not thick:
            np.testing.assert_array_equal(cover[2], shell)
        assert (cover[3] >= cover[2]).all(), "FIRST contains the shell"
    if dim == 3 and min(n) >= 3:
        assert len(_region_boxes(dim, n, 0x3f, 3)) == 7      # half the interior + six slabs


def test_unknown_solver_string_raises_value_error():
    """seigen/elastic.py:64"""
    from seigen_amd import ElasticLF4
    with pytest.raises(ValueError, match="Unknown solver mode"):
        ElasticLF4.create(UnitSquareMesh(2, 2), "DG", 1, dimension=2, solver="bogus", output=False)


def test_step_count_follows_reference_loop():
    """t = dt; while t <= T + 1e-12: ...; t += dt   (seigen/elastic.py:279-313)"""
    from oracle.lf4 import count_steps
    from seigen_amd.elastic import ElasticLF4

    class Dummy(object):
        step_times = ElasticLF4.step_times
    for dt, T in ((0.0125, 5.0), (0.001, 2.5), (0.5 / 32 / 8, 5.0), (0.3, 1.0)):
        d = Dummy()
        d.dt = dt
        assert len(d.step_times(T)) == count_steps(dt, T)
    assert count_steps(0.0125, 5.0) == 400


def test_helpers():
    from seigen_amd import Vp, Vs, cfl_dt
    assert Vp(0.25, 0.5, 1.0) == 1.0 and Vs(0.25, 1.0) == 0.5
    assert abs(cfl_dt(2.5, Vp(3600.0, 3599.3664, 1.0), 0.5) - 0.012028483448806774) < 1e-15


def test_marmousi_lookup():
    """seigen/marmousi.py:4-14: 384 x 122 nearest-cell lookup in marmhard.dat.  rule="reference" is
    the reference's `data[i][-j]` evaluated literally (incl. its j = 0 slip to the surface row);
    the default differs from it only at j = 0."""
    from seigen_amd import marmousi
    data = marmousi.load_model()
    assert data.shape == (384, 122) and data.min() == 1500.0 and data.max() == 5500.0
    H = marmousi.H
    rng = np.random.default_rng(5)
    x = rng.uniform(0, 383 * H, 400)
    y = np.concatenate([rng.uniform(0, 121 * H, 380), rng.uniform(0, H, 20)])
    want = np.array([data[int(np.floor(xx / 24.0))][-int(np.floor(yy / 24.0))] for xx, yy in zip(x, y)])
    np.testing.assert_array_equal(marmousi.vp_at(data, x, y, rule="reference"), want)
    fixed = marmousi.vp_at(data, x, y)
    up = y >= H
    np.testing.assert_array_equal(fixed[up], want[up])
    np.testing.assert_array_equal(fixed[~up], data[np.floor(x[~up] / H).astype(int), 121])
    assert marmousi.vp_at(data, 3.5 * H, 1.5 * H) == data[3, 121]
    assert marmousi.vp_at(data, 100.2 * H, 120.9 * H) == data[100, 2]
    mesh = RectangleMesh(383, 121, 383 * H, 121 * H)
    V = VectorFunctionSpace(mesh, "DG", 1)
    lam, mu, vp = marmousi.cell_material(V, data)
    assert lam.shape == (383 * 121 * 2,)
    np.testing.assert_allclose(lam + 2 * mu, vp ** 2, rtol=1e-14)
    np.testing.assert_allclose(mu, vp ** 2 / 3.0, rtol=1e-14)
    rho = marmousi.gardner_density(vp)
    lam2, mu2, _ = marmousi.cell_material(V, data, density=marmousi.gardner_density)
    np.testing.assert_allclose(lam2 + 2 * mu2, rho * vp ** 2, rtol=1e-14)


def test_vtu_stream_round_trip(tmp_path):
    """Output path (seigen/elastic.py:117-124, :221-232): numbered .vtu files + .pvd index, every cell
    with its own vertices, point data named like the function - written and parsed back."""
    from seigen_amd import UnitSquareMesh, UnitCubeMesh
    from seigen_amd.functionspace import VectorFunctionSpace, TensorFunctionSpace, Function
    from seigen_amd.vtu import VtuStream, read_vtu, vertex_nodes
    for mesh, dim, degree in ((UnitSquareMesh(3, 2), 2, 3), (UnitCubeMesh(2, 1, 2), 3, 2)):
        U = VectorFunctionSpace(mesh, "DG", degree)
        u = Function(U, name="VelocityNew")
        X = U.node_coords()
        vals = np.stack([X[..., 0] + 2 * X[..., 1], X[..., 0] * X[..., 1]] + ([X[..., 2] ** 2] if dim == 3 else []), axis=-1)
        u.dat.data = vals.reshape(-1, dim)
        st = VtuStream("velocity", directory=str(tmp_path))
        f0 = st.write(u, 0.0)
        f1 = st.write(u, 0.5)
        assert (f0, f1) == ("velocity_0.vtu", "velocity_1.vtu")
        pvd = (tmp_path / "velocity.pvd").read_text()
        assert 'file="velocity_0.vtu"' in pvd and 'timestep="0.5" file="velocity_1.vtu"' in pvd
        pts, data = read_vtu(str(tmp_path / f1))
        vn = vertex_nodes(dim, degree)
        ncells = X.shape[0]
        assert pts.shape == (ncells * (dim + 1), 3)
        np.testing.assert_allclose(pts[:, :dim], X[:, vn, :].reshape(-1, dim), atol=1e-15)
        got = data["VelocityNew"]
        assert got.shape == (ncells * (dim + 1), 3)
        np.testing.assert_allclose(got[:, :dim], vals[:, vn, :].reshape(-1, dim), atol=1e-14)
        # the listed nodes really are the cell's vertices: corners of the node cloud of every cell
        for c in range(0, ncells, 3):
            hull = X[c][vn]
            lam = np.linalg.lstsq(np.vstack([hull.T, np.ones(dim + 1)]), np.vstack([X[c].T, np.ones(X.shape[1])]), rcond=None)[0]
            assert lam.min() > -1e-12                        # every node is a convex combination of them
        # probing (uy.py:36-43): a field that is linear in x is reproduced exactly anywhere
        from seigen_amd.vtu import probe
        xq = np.array([[0.31, 0.47, 0.12][:dim], [0.5, 0.5, 0.5][:dim], [1.0, 1.0, 1.0][:dim]])
        got = probe(str(tmp_path / f1), "VelocityNew", xq)
        np.testing.assert_allclose(got[:, 0], xq[:, 0] + 2 * xq[:, 1], atol=1e-13)
        S = TensorFunctionSpace(mesh, "DG", degree)
        s = Function(S, name="StressNew")
        s.dat.data = np.einsum("ni,nj->nij", vals.reshape(-1, dim), vals.reshape(-1, dim))
        ss = VtuStream("stress", directory=str(tmp_path))
        _, sd = read_vtu(str(tmp_path / ss.write(s)))
        assert sd["StressNew"].shape == (ncells * (dim + 1), 9)


@pytest.mark.parametrize("mesh,P", [(UnitSquareMesh(5, 4), 3), (UnitCubeMesh(2, 3, 2), 2), (IntervalMesh(7, 2.0), 4),
                                    (UnitSquareMesh(4, 5, quadrilateral=True), 3)])
def test_interop_permutation_recovers_a_foreign_numbering(mesh, P):
    """binding from a host with another cell / node order (Firedrake: DMPlex cells, FIAT nodes)
    needs one permutation built from node coordinates; DG nodes coincide where cells touch, so it is built cell
    by cell (seigen_amd/interop.py)."""
    from seigen_amd.interop import dg_permutation
    V = FunctionSpace(mesh, "DG", P)
    ours = V.node_coords()
    nc, nd, dim = ours.shape
    rng = np.random.default_rng(3)
    cell_perm = rng.permutation(nc)
    theirs = np.empty_like(ours)
    node_perms = []
    for c_theirs, c_ours in enumerate(cell_perm):
        q = rng.permutation(nd)
        node_perms.append(q)
        theirs[c_theirs] = ours[c_ours][q]
    perm = dg_permutation(ours.reshape(-1, dim), theirs.reshape(-1, dim), nd)
    np.testing.assert_array_equal(theirs.reshape(-1, dim)[perm], ours.reshape(-1, dim))
    assert sorted(perm) == list(range(nc * nd))
    with pytest.raises(ValueError):
        dg_permutation(ours.reshape(-1, dim), (theirs + 0.01).reshape(-1, dim), nd)



def test_bench_watchdog_ends_hung_ranks():
    """A rank that never comes back (hung init / exchange) must make `bench.py --gpus N` exit non-zero within the
    stated time: every rank arms faulthandler.dump_traceback_later(--timeout, exit=True); the self-launching parent
    would kill the process group 30 s later.  No GPU needed: the ranks hang before touching one."""
    import subprocess
    import sys
    import time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SEIGEN_BENCH_TEST_HANG="1", OMP_NUM_THREADS="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--timeout", "4"], cwd=root, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert time.time() - t0 < 90
    assert "Timeout (0:00:04)" in r.stderr and not [l for l in r.stdout.splitlines() if l.startswith("{")]


def test_traffic_digest_follows_the_kernel_sources(tmp_path):
    """bench.py quotes profiles/*/config3_traffic.json only while seigen_amd/csrc is what was profiled."""
    import bench
    d = bench.csrc_digest()
    assert len(d) == 64 and d == bench.csrc_digest()


def test_bench_dump_outputs_samples_within_budget(tmp_path):
    """bench.py --dump-outputs: a block too large to write whole is sampled - the same seeded cells every time, values
    exactly the block's at those cells, whole-block norms, float64, all ranks' files together under 64 MB."""
    import bench
    from seigen_amd import _lib

    class Block(object):              # 24^3 cubes x 6 tets, P4 (35 nodes): larger than the budget
        ncells, nd, dim = 6 * 24 ** 3, 35, 3

        def field_shape(self, f):
            return (self.ncells, self.nd, 3, 3) if f == _lib.FIELD_S else (self.ncells, self.nd, 3)

        def get_field_range(self, f, c0, n, out=None):
            shape = (n,) + self.field_shape(f)[1:]
            v = (np.arange(c0, c0 + n, dtype=np.float64) * (3.0 if f == _lib.FIELD_S else 1.0) % 7.0 - 3.0)
            a = np.broadcast_to(v.reshape((n,) + (1,) * (len(shape) - 1)), shape)
            if out is None:
                return a.copy()
            out[...] = a
            return out

    blk = Block()
    for world in (1, 2):
        d = tmp_path / ("w%d" % world)
        bench.dump_outputs(blk, str(d), 0, world)
        bench.dump_outputs(blk, str(tmp_path / ("again%d" % world)), 0, world)
        sfx = "_rank0" if world > 1 else ""
        names = ["u1", "s1", "cells", "field_norms"]
        arrs = {k: np.load(str(d / (k + sfx + ".npy"))) for k in names}
        assert all(a.dtype == np.float64 for a in arrs.values())
        assert sum(os.path.getsize(str(d / (k + sfx + ".npy"))) for k in names) * world < 64 << 20
        cells = arrs["cells"].astype(np.int64)
        assert len(cells) > 1000 and np.all(np.diff(cells) > 0) and cells[-1] < blk.ncells
        assert arrs["u1"].shape == (len(cells), 35, 3) and arrs["s1"].shape == (len(cells), 35, 3, 3)
        np.testing.assert_array_equal(arrs["u1"][:, 0, 0], cells * 1.0 % 7.0 - 3.0)
        np.testing.assert_array_equal(arrs["s1"][:, 0, 0, 0], cells * 3.0 % 7.0 - 3.0)
        for k in names:
            np.testing.assert_array_equal(arrs[k], np.load(str(tmp_path / ("again%d" % world) / (k + sfx + ".npy"))))
        allu = np.arange(blk.ncells, dtype=np.float64) % 7.0 - 3.0
        np.testing.assert_allclose(arrs["field_norms"][0], np.sqrt(np.sum(allu ** 2) * 105), rtol=1e-12)
        assert arrs["field_norms"][2] == 3.0 and arrs["field_norms"][3] == 3.0


def test_expression_evaluate_times_equals_per_step_evaluation():
    """The per-step source table (elastic.py:285-288: the source Expression re-interpolated before every step) is
    built in one vectorised pass over all steps; element for element it must be what `evaluate` gives with `t` set
    - box-limited Ricker source (explosive_source_lf4.py:36-40), a condition that depends on t, a moving support."""
    from seigen_amd.expression import Expression
    rng = np.random.default_rng(0)
    X = rng.uniform([44.0, 148.0], [46.0, 150.0], size=(60, 2))
    times = [1e-3 * (k + 1) for k in range(300)]
    box = "x[0] >= 44.5 && x[0] <= 45.5 && x[1] >= 148.5 && x[1] <= 149.5"
    code = "%s ? (-1.0 + 2*a*pow(t - 0.3, 2))*exp(-a*pow(t - 0.3, 2)) : 0.0" % box
    cases = [Expression(((code, "0.0"), ("0.0", code)), a=159.42, t=0),
             Expression("t > 0.1 && x[0] < 45 + t ? sin(x[1]*t) : (t < 0.05 ? 1.0 : 0.0)", t=0),
             Expression(("x[0]*t", "cos(t)"), t=0)]
    for e in cases:
        for chunk in (1 << 22, 128):      # one pass, and many small chunks of rows
            V = e.evaluate_times(X, times, max_elems=chunk)
            for k in (0, 7, 150, 299):
                e.t = times[k]
                assert np.array_equal(V[k], e.evaluate(X))


def test_stage_fields_of_the_library_and_of_the_host_driven_exchanger_agree():
    """Which field a stage reads and writes is stated once in the library (hostlogic.hpp lf4_stage: the stage launches
    and the native exchange take it from there) and once in seigen_amd/parallel.py (STAGE_INPUT / STAGE_OUTPUT, the
    host-driven exchanger).  The sanitizer driver prints the library's statement, one `stage k: in out` line per stage."""
    import subprocess
    from seigen_amd import parallel
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "seigen_amd", "csrc"), "host-asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(ROOT, "build_tools", "host_asan_driver")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = {int(k): (int(i), int(o)) for k, i, o in re.findall(r"^stage (\d+): (\d+) (\d+)$", r.stdout, flags=re.M)}
    assert sorted(rows) == list(range(6)), r.stdout
    assert {k: v[0] for k, v in rows.items()} == parallel.STAGE_INPUT
    assert {k: v[1] for k, v in rows.items()} == parallel.STAGE_OUTPUT


def test_second_region_is_never_empty_for_the_shipped_multi_rank_configurations():
    """The launch that runs beside the halo exchange (SG_REGION_SECOND) must have cubes to work on for every block of
    the process grids the multi-rank configurations use (advisor finding of round 3: a group-thick x shell on both
    sides of a block at most two groups wide left the interior empty): bench.py's weak scaling (64^3 per rank), config
    4 (256^3 in 2 x 2 x 2 blocks), the reference's explosive-source mesh (120 x 60 squares, P2) on 2 and 4 ranks, and
    narrow 2-D / 3-D blocks on grids cut along x."""
    from seigen_amd.mesh import Partition, _factor_grid
    cases = []
    for world in (2, 4, 8):
        grid = _factor_grid(world, 3, (64, 64, 64))
        cases.append((3, 4, tuple(64 * g for g in grid), grid))
        cases.append((2, 2, (120, 60), _factor_grid(world, 2, (120, 60))))
    cases += [(3, 4, (256, 256, 256), (2, 2, 2)), (3, 4, (96, 8, 8), (3, 1, 1)), (2, 3, (96, 8), (3, 2)),
              (3, 3, (40, 4, 4), (2, 1, 1))]
    for dim, degree, n, grid in cases:
        world = int(np.prod(grid))
        for r in range(world):
            p = Partition(n, r, world, grid)
            cfg = _lib.SgConfig()
            cfg.dim, cfg.degree = dim, degree
            for a in range(3):
                cfg.n[a] = p.n[a] if a < dim else 1
                cfg.h[a] = 1.0
            cfg.nbr_mask = p.nbr_mask
            buf = (C.c_int32 * (6 * 16))()
            cnt = lib().sg_region_boxes(C.byref(cfg), 4, buf, 16)      # SG_REGION_SECOND
            cubes = sum(buf[6 * i + 3] * buf[6 * i + 4] * buf[6 * i + 5] for i in range(cnt))
            total = int(np.prod(p.n))
            assert cnt >= 1 and cubes >= total // 5, (dim, n, grid, r, cubes, total)


def test_node_coordinates_do_not_depend_on_the_partition():
    """Advisor finding of round 3: coordinates computed from a shifted origin (a block of a partitioned mesh, a slab of
    a chunked scan, the sub-box of a source's support hint) differed by an ulp from those of the whole mesh, so a source
    box whose faces lie on node lines could select different nodes under different partitions.  With sg_config::cube0
    every path adds the integers first: bitwise the coordinates of the whole mesh - for awkward cell sizes, every block
    of a 1 x 2 x 2 and a 2 x 2 x 1 grid, the slab-by-slab scan, and the support scan restricted to a box."""
    from seigen_amd.mesh import BoxMesh
    from seigen_amd import ElasticLF4  # noqa: F401  (the scan helper lives on the solver class)
    n, L = (7, 5, 6), (300.0 * 7 / 9, 1.3, 0.77)
    mesh = BoxMesh(n[0], n[1], n[2], *L)
    V = FunctionSpace(mesh, "DG", 3)
    full = V.node_coords()
    chunks = np.concatenate([X for _, X in V.node_coords_chunks(max_nodes=3000)])
    assert np.array_equal(chunks, full)
    for grid in ((1, 2, 2), (2, 2, 1)):
        world = int(np.prod(grid))
        for r in range(world):
            m2 = BoxMesh(n[0], n[1], n[2], *L)
            p = Partition(n, r, world, grid)
            m2.set_partition(p)
            Xb = FunctionSpace(m2, "DG", 3).node_coords()
            ax = [np.arange(p.start[a], p.start[a] + p.n[a]) for a in range(3)]
            cube = (ax[0][None, None, :] + n[0] * (ax[1][None, :, None] + n[1] * ax[2][:, None, None])).reshape(-1)
            cells = (cube[:, None] * 6 + np.arange(6)[None, :]).reshape(-1)
            assert np.array_equal(Xb, full[cells]), (grid, r)
    # the sub-box evaluation of the support scan (sg_config with a cube offset), against the same cubes of the whole mesh
    cfg = _lib.SgConfig()
    cfg.dim, cfg.degree = 3, 3
    sub_o, sub_n = (2, 1, 3), (3, 2, 2)
    for a in range(3):
        cfg.n[a], cfg.h[a], cfg.origin[a], cfg.cube0[a] = sub_n[a], L[a] / n[a], 0.0, sub_o[a]
    X = np.empty((int(np.prod(sub_n)) * 6, V.nd, 3))
    assert lib().sg_block_node_coords(C.byref(cfg), 3, X.ctypes.data, X.nbytes) == 0
    ax = [np.arange(sub_o[a], sub_o[a] + sub_n[a]) for a in range(3)]
    cube = (ax[0][None, None, :] + n[0] * (ax[1][None, :, None] + n[1] * ax[2][:, None, None])).reshape(-1)
    cells = (cube[:, None] * 6 + np.arange(6)[None, :]).reshape(-1)
    assert np.array_equal(X, full[cells])


def test_partition_peers_satisfy_the_native_exchange_preconditions():
    """What sg_comm_check (csrc/comm.cpp) demands of the peers[] a rank hands to sg_comm_init, for every block grid
    mesh._factor_grid picks for 2, 4, 6 and 8 ranks (bench.py's weak-scaling and config-4 layouts among them): a peer on
    exactly the sides of nbr_mask, never the rank itself, no rank behind two different axes, and the relation is mutual -
    my peer across side s names me across side s ^ 1 (the pairing the exchange relies on when it posts its receives)."""
    from seigen_amd.mesh import Partition, _factor_grid
    for world, n in ((2, (64, 64, 64)), (4, (64, 64, 64)), (8, (64, 64, 64)), (8, (256, 256, 256)), (6, (4, 100)), (8, (16, 64, 64))):
        dim = len(n)
        grid = _factor_grid(world, dim, n)
        gn = tuple(n[a] * grid[a] for a in range(dim))
        parts = [Partition(gn, r, world, grid) for r in range(world)]
        for r, p in enumerate(parts):
            peers = [p.neighbour(s) for s in range(2 * dim)]
            assert p.nbr_mask == sum(1 << s for s in range(2 * dim) if peers[s] is not None)
            named = [(s, q) for s, q in enumerate(peers) if q is not None]
            assert all(q != r and 0 <= q < world for _, q in named)
            for s, q in named:
                assert parts[q].neighbour(s ^ 1) == r, (world, grid, r, s, q)
                assert all((s >> 1) == (t >> 1) for t, q2 in named if q2 == q), "one rank behind two axes"


def test_experiment_patches_are_indexed_and_apply():
    """tools/experiments/*.patch are the code of closed experiments; each is pinned in PATCHES.txt to the newest commit
    whose tree takes it (HEAD for those that must keep applying) and check_patches.sh verifies the index.  Needs the
    history (skipped in an export without .git)."""
    import subprocess
    if not os.path.isdir(os.path.join(ROOT, ".git")):
        pytest.skip("no git history here")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "experiments", "check_patches.sh")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("ok ") >= 11


def test_every_environment_switch_is_documented():
    """Every SEIGEN_* variable the product reads (library sources, host layer, bench.py) has a line in INTEGRATION.md."""
    import glob
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    files = glob.glob(os.path.join(ROOT, "seigen_amd", "**", "*.py"), recursive=True) + [os.path.join(ROOT, "bench.py")]
    for ext in ("cpp", "hip", "hpp"):
        files += glob.glob(os.path.join(ROOT, "seigen_amd", "csrc", "*." + ext))
    names = set()
    for f in files:
        names |= set(re.findall(r"SEIGEN_[A-Z0-9_]+", open(f).read()))
    names -= {"SEIGEN_HIP_H"}      # the header's include guard
    missing = sorted(n for n in names if n not in doc)
    assert not missing, "not in INTEGRATION.md's table: %s" % missing


def _faked_rank_file(single, n, part, cell):
    """what tests/native_exchange_worker.py saves of a rank, cut out of the single block's fields"""
    from tests.native_exchange_worker import block_cells
    idx = block_cells(n, part.start, part.n, cell)
    return dict({k: v[idx] for k, v in single.items()}, start=np.array(part.start), n=np.array(part.n))


@pytest.mark.parametrize("n,grid,cell,nd", [((9,), (3,), "left", 4), ((6, 4), (2, 2), "right", 10), ((6, 4), (2, 2), "quadrilateral", 16),
                                            ((4, 6, 2), (2, 2, 1), "left", 4), ((4, 6, 2), (2, 2, 1), "quadrilateral", 8)])
def test_native_exchange_block_comparison_fails_on_a_wrong_block(n, grid, cell, nd):
    """The bitwise comparison of tests/test_native_exchange_gpu.py (check_rank_fields over block_cells) on faked rank files:
    it passes for each rank's own cells and fails for a block shifted by one cell, for the block of the transposed grid and
    for the other cell class - the comparison would not pass by looking at the wrong cells."""
    from tests.native_exchange_worker import block_cells, cells_per_cube, check_rank_fields
    dim, world = len(n), int(np.prod(grid))
    ncells = int(np.prod(n)) * cells_per_cube(dim, cell)
    rng = np.random.default_rng(5)
    single = {"u": rng.uniform(-1, 1, (ncells, nd, dim)), "s": rng.uniform(-1, 1, (ncells, nd, dim, dim)),
              "uh": rng.uniform(-1, 1, (ncells, nd, dim))}
    parts = [Partition(n, r, world, grid) for r in range(world)]
    seen = np.concatenate([block_cells(n, p.start, p.n, cell) for p in parts])
    assert sorted(seen) == list(range(ncells)), "the blocks' cells tile the mesh"
    for r, p in enumerate(parts):
        d = _faked_rank_file(single, n, p, cell)
        check_rank_fields(d, single, n, cell, r)
        for a in range(dim):      # the start shifted by one cell along an axis (where the block still fits the mesh)
            start = list(p.start)
            start[a] += 1 if p.start[a] + p.n[a] < n[a] else -1
            with pytest.raises(AssertionError):
                check_rank_fields(dict(d, start=np.array(start)), single, n, cell, r)
        if dim > 1:
            other = "left" if cell == "quadrilateral" else "quadrilateral"
            with pytest.raises((AssertionError, IndexError)):
                check_rank_fields(d, single, n, other, r)
    if dim > 1:      # the transposed grid: the ranks counted along y first - rank r then sits at the swapped coordinates
        tgrid = (grid[1], grid[0]) + tuple(grid[2:])
        wrong = 0
        for r in range(world):
            c = Partition(n, r, world, tgrid).coords
            q = parts[parts[0].coords_to_rank((c[1], c[0]) + tuple(c[2:]))]
            d = _faked_rank_file(single, n, parts[r], cell)
            if (q.start, q.n) == (parts[r].start, parts[r].n):
                continue
            wrong += 1
            with pytest.raises(AssertionError):
                check_rank_fields(dict(d, start=np.array(q.start), n=np.array(q.n)), single, n, cell, r)
        assert wrong >= world - 2


def test_native_exchange_family_pin_fails_on_another_family():
    """The family assertion of tests/test_native_exchange_gpu.py on faked kernel names: names of the claimed family pass,
    one stage of another family - or of the other number type - fails."""
    from tests.native_exchange_worker import check_family
    tile = ["sg::tile2d_stage<3, %d, %d, 1, 1, 0, double>" % km for km in ((0, 0), (1, 0), (0, 1), (1, 0), (0, 2), (1, 1))]
    check_family(np.array(tile), "sg::tile2d_stage<", "double")
    with pytest.raises(AssertionError):
        check_family(np.array(tile), "sg::tile2d_stage<", "float")
    with pytest.raises(AssertionError):
        check_family(np.array(tile), "sg::lane_stage<")
    with pytest.raises(AssertionError):
        check_family(np.array(tile[:5] + ["sg::stage_kernel<2, 3, 1, 1, 1>"]), "sg::tile2d_stage<", "double")
    with pytest.raises(AssertionError):
        check_family(np.array(tile[:5]), "sg::tile2d_stage<")
    # hex_stage and hexm_stage are told apart, as are lane_stage and stage_kernel
    with pytest.raises(AssertionError):
        check_family(np.array(["sg::hexm_stage<3, 0, 0, 1, 1>"] * 6), "sg::hex_stage<")
