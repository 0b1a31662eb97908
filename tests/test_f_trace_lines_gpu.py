"""The F stages of the 3-D matrix-pipe family load only the stress lines a facet's scaled normal can see
(kernels_mfma.hip load_trace / trace_flux, mfma_tables.cpp mfma_trace_lines): one column on the facets that lie on a cube
face, two on the facets inside the cube.  A wrong column or a transposed line must show, so:

  * the cells are anisotropic (hx != hy != hz: the entries of a scaled normal differ in magnitude per axis);
  * both stress storages run - symmetric, and a NON-symmetric upload (T_ia != T_ai) that leaves symmetric mode;
  * (17, 3, 3) has a second cell group of one cube, interior neighbours and domain-boundary facets along every axis and
    padding lanes; (3, 2, 16) has one group per x row and 16 layers (the chunked item order);
  * blocks with neighbour blocks are cut along x, along y and along z, so every value of the side's axis reaches the
    remote-record loads, and must equal the single block bitwise.

Tolerances are the suite's own: FP64 tol_of() per application and 10 tol_of() for three steps (test_parity_gpu.py), FP32 2e-5
per application (test_fp32_gpu.py)."""
import functools

import numpy as np
import pytest

from oracle.lf4 import OracleLF4
from tests.test_mfma_family_gpu import _block, _environment, _f_name, _stage_names, _fact
from tests.test_parity_gpu import tol_of
from tests.util import oracle_mesh, rel_err, seeded

pytestmark = pytest.mark.gpu

H = (0.3, 0.5, 0.7)
SHAPES = [(17, 3, 3), (3, 2, 16)]


def _lengths(n):
    return tuple(H[a] * n[a] for a in range(3))


def _stress(shape, seed, sym):
    s = seeded(shape, seed)
    return 0.5 * (s + np.swapaxes(s, -1, -2)) if sym else s


@functools.lru_cache(maxsize=None)
def _oracle(n, P):
    """the oracle of block n at degree P, built once (seconds at degree 4) and shared by every test of the pair: the F
    tests use its operators, the step tests set dt, material and the initial fields themselves"""
    return OracleLF4(oracle_mesh(3, n, _lengths(n)), P)


@functools.lru_cache(maxsize=None)
def _expected_F(n, P, sym):
    """inputs and the oracle's F of them, computed once and shared by the two number types (read-only)"""
    E = _oracle(n, P).E
    nc = 6 * n[0] * n[1] * n[2]
    T = _stress((nc, E.nd, 3, 3), 100 + P, sym)
    u = seeded((nc, E.nd, 3), 200 + P)
    exp = E.apply_F(T, u)
    for a in (T, u, exp):
        a.setflags(write=False)
    return T, u, exp


@pytest.mark.parametrize("sym", [True, False], ids=["sym", "full"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("P", [1, 2, 3, 4])
@pytest.mark.parametrize("n", SHAPES, ids=lambda n: "x".join(map(str, n)))
def test_one_application_of_F(gpu, monkeypatch, n, P, dtype, sym):
    from seigen_amd import _lib
    _environment(monkeypatch, "mfma", None)
    T, u, exp = _expected_F(n, P, sym)
    blk = _block(dtype, P, n, _lengths(n))
    assert tuple(blk.field_shape(_lib.FIELD_S)) == T.shape
    blk.set_params(1.0, 0.01, 0.7, 0.3)
    blk.set_field(_lib.FIELD_S, T)
    blk.set_field(_lib.FIELD_U, u)
    assert blk.is_sym() == sym
    assert blk.stage_kernel_name(0) == _f_name(dtype, P, 0, sym, 0)
    blk.apply_F(_lib.FIELD_S, _lib.FIELD_U, _lib.FIELD_UH)
    err = rel_err(blk.get_field(_lib.FIELD_UH), exp)
    blk.close()
    print("ERR trace lines F %s P%d %s %s %.3e" % (dtype, P, "sym" if sym else "full", n, err))
    assert err < (tol_of(P, "left") if dtype == "f64" else 2e-5)


@pytest.mark.parametrize("sym", [True, False], ids=["sym", "full"])
@pytest.mark.parametrize("n", SHAPES, ids=lambda n: "x".join(map(str, n)))
def test_three_steps_at_degree_4(gpu, monkeypatch, n, sym):
    """whole LF4 steps: the fused F modes 1 (U1) and 2 (UTEMP) beside mode 0"""
    from seigen_amd import _lib
    _environment(monkeypatch, "mfma", None)
    P = 4
    orc = _oracle(n, P)
    blk = _block("f64", P, n, _lengths(n))
    orc.dt = 0.04 * min(H) / P ** 2
    orc.l, orc.mu, orc.density = 0.5, 0.25, 1.0
    orc.source, orc.density_physical = None, False
    orc.u0 = u_start = seeded(blk.field_shape(_lib.FIELD_U), 31)
    orc.s0 = _stress(blk.field_shape(_lib.FIELD_S), 32, sym)
    blk.set_params(orc.density, orc.dt, orc.l, orc.mu)
    blk.set_field(_lib.FIELD_U, orc.u0)
    blk.set_field(_lib.FIELD_S, orc.s0)
    assert blk.is_sym() == sym
    assert [blk.stage_kernel_name(st) for st in range(6)] == _stage_names("f64", P, sym, _fact("f64", P, None))
    blk.step(3)
    for k in range(3):
        orc.step((k + 1) * orc.dt)
    errs = (rel_err(blk.get_field(_lib.FIELD_U), orc.u1), rel_err(blk.get_field(_lib.FIELD_S), orc.s1),
            rel_err(blk.get_field(_lib.FIELD_UH), orc.dt * orc.u1 + orc.dt ** 3 / 24.0 * orc.last["utemp"]))
    blk.close()
    print("ERR trace lines steps %s %s u %.3e s %.3e uh %.3e" % ("sym" if sym else "full", n, *errs))
    assert max(errs) < 10 * tol_of(P, "left")
    assert rel_err(orc.u1, u_start) > 1e-4


# (whole mesh, grid of blocks): halves of (4, 3, 2) cubes side by side along x, along y, along z
CUTS = [((8, 3, 2), (2, 1, 1)), ((4, 6, 2), (1, 2, 1)), ((4, 3, 4), (1, 1, 2))]


@pytest.mark.parametrize("sym", [True, False], ids=["sym", "full"])
@pytest.mark.parametrize("P", [3, 4])
@pytest.mark.parametrize("n,grid", CUTS, ids=["cut-x", "cut-y", "cut-z"])
def test_two_blocks_are_bitwise_the_single_block(gpu, monkeypatch, n, grid, P, sym):
    """GHOST = 1 with the block side normal to each axis in turn (test_mfma_family_gpu's split rows cut along z only), with
    a sponge and a source, through the host-driven exchange; _multiblock_case asserts np.array_equal on u and s"""
    from tests.test_harness_gpu import _multiblock_case
    _environment(monkeypatch, "mfma", None)
    res = _multiblock_case(3, P, n, grid, True, extras=True, dtype="f64", sym=sym)
    assert res["names"] == sorted(set(_stage_names("f64", P, sym, _fact("f64", P, None), ghost=1))), res["names"]
    assert rel_err(res["u"], res["u0"]) > 1e-4
