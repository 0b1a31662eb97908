"""CPU-only tests of the class frame the F stages of the 3-D matrix-pipe family work in (kernels.hpp mfma_class_frame,
include/seigen_hip.h sg_mfma_class_frame): class k of the Kuhn split is the reference simplex with the axes permuted by p[k],
so in the order p the inverse Jacobian is one bidiagonal matrix, a facet's scaled normal has its non-zero entries at fixed
columns, and the volume term needs one stress line times one scalar per direction with the difference operators
E'_m = E_m - E_(m-1).  Checked here against the block's mesh tables (sg_mesh_tables, sg_gradient_tables) for several
anisotropic cell sizes; that tables of another shape are refused is checked by tools/host_asan_driver.cpp class_frame_3d (a
program of its own, run by tests/test_host_asan.py)."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

from seigen_amd import _lib
from seigen_amd.backend import gradient_tables, mfma_class_frame
from tests import grad_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# anisotropic cell sizes: the suite's (0.3, 0.5, 0.7), one with exact binary fractions, and seeded random ones
CELLS = [(0.3, 0.5, 0.7), (2.0, 0.125, 0.75)] + [tuple(np.random.default_rng(s).uniform(0.05, 3.0, 3)) for s in (1, 2, 3)]


def _cfg(P, h):
    return gc.block_cfg(3, P, (2, 2, 2), h=list(h))


def _mesh_tables(P, h):
    nf = (P + 1) * (P + 2) // 2
    nb, nbn = np.zeros((6, 4, 5), dtype=np.int32), np.zeros((6, 4, nf), dtype=np.int32)
    cn, jinv = np.zeros((6, 4, 3)), np.zeros((6, 3, 3))
    hh = np.array(h, dtype=np.float64)
    assert _lib.load().sg_mesh_tables(3, P, 0, hh.ctypes.data, nb.ctypes.data, nbn.ctypes.data, cn.ctypes.data, jinv.ctypes.data) == 0
    return cn, jinv


def stress_line_slot(sym, i, j):
    """kernels.hpp stress_line_slot: the line of T(i, j) among a node's nine"""
    return min(i, j) * 3 + max(i, j) if sym else i * 3 + j


def test_symbol_is_bound_and_refuses_what_has_no_frame():
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "seigen_hip.h")).read()
    assert "sg_mfma_class_frame" in _lib.SYMBOLS and hasattr(L, "sg_mfma_class_frame") and " sg_mfma_class_frame(" in hdr
    none = (None,) * 6
    assert L.sg_mfma_class_frame(None, *none) == -1
    assert L.sg_mfma_class_frame(C.byref(_cfg(4, (0.3, 0.5, 0.7))), *none) == 35      # the size query
    assert L.sg_mfma_class_frame(C.byref(_cfg(1, (0.3, 0.5, 0.7))), *none) == 4
    assert L.sg_mfma_class_frame(C.byref(gc.block_cfg(2, 2, (3, 3))), *none) == -1      # triangles
    assert L.sg_mfma_class_frame(C.byref(gc.block_cfg(3, 2, (2, 2, 2), diagonal="quadrilateral")), *none) == -1      # hexahedra
    for bad in ((0.0, 0.5, 0.7), (0.3, -1.0, 0.7), (0.3, 0.5, float("nan"))):
        assert L.sg_mfma_class_frame(C.byref(_cfg(2, bad)), *none) == -1, bad
    cfg = _cfg(2, (0.3, 0.5, 0.7))
    cfg.degree = 5
    assert L.sg_mfma_class_frame(C.byref(cfg), *none) == -1


@pytest.mark.parametrize("h", CELLS, ids=lambda h: "h=%.3g,%.3g,%.3g" % h)
def test_permutations_scales_and_jacobian(h):
    fr = mfma_class_frame(_cfg(2, h))
    # the six permutations in the order of class_vertices (lexicographic)
    assert [tuple(p) for p in fr["p"]] == list(itertools.permutations(range(3)))
    cn, jinv = _mesh_tables(2, h)
    assert np.array_equal(gradient_tables(_cfg(2, h))[1], jinv)
    for k in range(6):
        p, s = fr["p"][k], fr["s"][k]
        assert np.allclose(s, [1.0 / h[p[m]] for m in range(3)], rtol=4 * 2.0 ** -53, atol=0)
        # J^-1 rebuilt from (p, s): row r = s_r e_p[r] - s_(r+1) e_p[r+1]; EXACTLY the block's table
        J = np.zeros((3, 3))
        for r in range(3):
            J[r, p[r]] = s[r]
            if r < 2:
                J[r, p[r + 1]] = -s[r + 1]
        assert np.array_equal(J, jinv[k]), (k, J, jinv[k])
        # the scaled normals: non-zero at the frame's columns {0} {0,1} {1,2} {2} and nowhere else
        cols = ((0,), (0, 1), (1, 2), (2,))
        for f in range(4):
            want = np.zeros(3)
            for c, m in enumerate(cols[f]):
                want[p[m]] = fr["cn"][k, f, c]
                assert fr["cn"][k, f, c] != 0.0
            if len(cols[f]) == 1:
                assert fr["cn"][k, f, 1] == 0.0
            assert np.array_equal(want, cn[k, f]), (k, f)


@pytest.mark.parametrize("P", [1, 2, 3, 4])
def test_difference_operators_give_the_volume_term(P):
    """sum_m E'_m s_m X[:, p_m] = sum_r E_r (J^-1 X)_r for a random X [nd, 3], to 1e-14 of the largest term"""
    rng = np.random.default_rng(40 + P)
    for h in CELLS:
        fr = mfma_class_frame(_cfg(P, h), operators=True)
        E, Ed = fr["E"], fr["Ed"]
        nd = E.shape[1]
        assert nd == (P + 1) * (P + 2) * (P + 3) // 6
        # E' takes the sums in long double and rounds once, E adds up to two folded terms in double: at most two roundings
        # in each E, one in their difference and one in E', each half an ulp of the largest entry at most
        for m in range(3):
            assert np.abs(Ed[m] - (E[m] - (E[m - 1] if m else 0.0))).max() <= 6 * 2.0 ** -53 * np.abs(E).max(), m
        _, jinv = _mesh_tables(P, h)
        X = rng.uniform(-1, 1, (nd, 3))
        for k in range(6):
            p, s = fr["p"][k], fr["s"][k]
            old = sum(E[r] @ (X @ jinv[k][r]) for r in range(3))
            new = sum(Ed[m] @ (s[m] * X[:, p[m]]) for m in range(3))
            scale = sum(np.abs(E[r]) @ np.abs(X @ jinv[k][r]) for r in range(3)).max()
            assert np.abs(new - old).max() <= 1e-14 * scale, (P, h, k, np.abs(new - old).max() / scale)


@pytest.mark.parametrize("h", CELLS[:2], ids=["suite", "binary"])
def test_line_offsets_are_the_permuted_slots(h):
    fr = mfma_class_frame(_cfg(3, h))
    for k in range(6):
        p = fr["p"][k]
        assert [int(v) for v in fr["vel"][k]] == [16 * int(p[i]) for i in range(3)]
        for sym in (0, 1):
            line = lambda a, b: 16 * stress_line_slot(sym, int(p[a]), int(p[b]))      # noqa: E731
            own, tr = fr["own"][k, sym], fr["trace"][k, sym]
            assert [int(v) for v in own] == [line(a, b) for a in range(3) for b in range(3)]
            if sym:
                assert len(set(int(v) for v in own)) == 6 and all(own[3 * a + b] == own[3 * b + a] for a in range(3) for b in range(3))
            else:
                assert sorted(int(v) for v in own) == [16 * c for c in range(9)]
            # cube faces: column p[0] on facet 0, p[2] on facet 3, rows in the frame's order
            assert [int(v) for v in tr[0][:3]] == [line(i, 0) for i in range(3)]
            assert [int(v) for v in tr[3][:3]] == [line(i, 2) for i in range(3)]
            if sym:
                # inner facets: the five lines the two columns see; facet 2 is facet 1 with the frame's 0 and 2 exchanged
                assert [int(v) for v in tr[1][:5]] == [line(0, 0), line(0, 1), line(1, 1), line(2, 0), line(2, 1)]
                assert [int(v) for v in tr[2][:5]] == [line(2, 2), line(2, 1), line(1, 1), line(0, 2), line(0, 1)]
                for f in (1, 2):
                    assert len(set(int(v) for v in tr[f][:5])) == 5
            else:
                for f in (1, 2):
                    assert [int(v) for v in tr[f]] == [line(i, f - 1) for i in range(3)] + [line(i, f) for i in range(3)]
            assert all(0 <= int(v) < 9 * 16 and int(v) % 16 == 0 for v in tr.ravel())      # unread entries still point into the node
