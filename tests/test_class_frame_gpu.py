"""The F stages of the 3-D matrix-pipe family work in each Kuhn class's own axis order (kernels.hpp mfma_class_frame,
kernels_mfma.hip mfma_stage_F): accumulator i' holds velocity component p[i'], tensor slot (a, b) holds T(p[a], p[b]), the
volume term is one own line times s_m per direction against the difference tiles E'_m, and every load and store goes to a line
chosen by the class.  A wrong p, a wrong s_m or a transposed slot is an O(1) error on anisotropic cells, so:

  * the cells are anisotropic, H = (0.3, 0.5, 0.7) (tests/test_f_trace_lines_gpu.py, whose helpers and shapes these are);
  * (17, 3, 3) has a second cell group of one cube with padding lanes and interior and domain-boundary facets on every axis,
    (3, 2, 16) the chunked item order of the F stages;
  * one application of F and one of G against the oracle at every degree, in both number types and both stress storages, with
    the launch forms of the G stages at degree 4 (SEIGEN_HIP_GQ, SEIGEN_HIP_GSTASH) - the G stages read the same class through
    MeshDev, and one step needs both to agree on what a component is;
  * three whole steps at degree 4 (F modes 1 and 2, G mode 1) with per-cell lambda, mu and density;
  * blocks cut along x, y and z, with sponge and source, bitwise equal to the single block.

Tolerances are the suite's own: tol_of() per application, 2e-5 in float, 10 tol_of() for three steps."""
import functools

import numpy as np
import pytest

from tests.test_f_trace_lines_gpu import CUTS, H, SHAPES, _expected_F, _lengths, _oracle, _stress
from tests.test_mfma_family_gpu import _block, _environment, _f_name, _g_name, _stage_names, _fact
from tests.test_parity_gpu import tol_of
from tests.util import rel_err, seeded

pytestmark = pytest.mark.gpu

_ids = dict(ids=lambda n: "x".join(map(str, n)))


@pytest.mark.parametrize("sym", [True, False], ids=["sym", "full"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("P", [1, 2, 3, 4])
@pytest.mark.parametrize("n", SHAPES, **_ids)
def test_one_application_of_F(gpu, monkeypatch, n, P, dtype, sym):
    from seigen_amd import _lib
    _environment(monkeypatch, "mfma", None)
    T, u, exp = _expected_F(n, P, sym)
    blk = _block(dtype, P, n, _lengths(n))
    blk.set_params(1.0, 0.01, 0.7, 0.3)
    blk.set_field(_lib.FIELD_S, T)
    blk.set_field(_lib.FIELD_U, u)
    assert blk.is_sym() == sym
    assert blk.stage_kernel_name(0) == _f_name(dtype, P, 0, sym, 0)
    blk.apply_F(_lib.FIELD_S, _lib.FIELD_U, _lib.FIELD_UH)
    got = blk.get_field(_lib.FIELD_UH)
    blk.close()
    err = rel_err(got, exp)
    print("ERR class frame F %s P%d %s %s %.3e" % (dtype, P, "sym" if sym else "full", n, err))
    assert err < (tol_of(P, "left") if dtype == "f64" else 2e-5)


@functools.lru_cache(maxsize=None)
def _expected_G(n, P):
    """a velocity and the oracle's G of it (computed once, read-only)"""
    E = _oracle(n, P).E
    u = seeded((6 * n[0] * n[1] * n[2], E.nd, 3), 300 + P)
    exp = E.apply_G(u, 0.7, 0.3)
    for a in (u, exp):
        a.setflags(write=False)
    return u, exp


# (dtype, P, SEIGEN_HIP_GQ, SEIGEN_HIP_GSTASH): the factorised volume term exists in double from degree 3 and is the default
# at degree 4; the stash form exists where the factorised one runs at degree 4
G_FORMS = [(t, P, None, None) for t in ("f64", "f32") for P in (1, 2, 3, 4)] + [("f64", 4, "0", None), ("f64", 4, "1", None),
                                                                                 ("f64", 4, "1", "0"), ("f64", 4, "1", "1")]


@pytest.mark.parametrize("sym", [True, False], ids=["sym", "full"])
@pytest.mark.parametrize("dtype,P,gq,gstash", G_FORMS, ids=lambda v: "-" if v is None else str(v))
@pytest.mark.parametrize("n", SHAPES, **_ids)
def test_one_application_of_G(gpu, monkeypatch, n, dtype, P, gq, gstash, sym):
    from seigen_amd import _lib
    _environment(monkeypatch, "mfma", gq, launch={"SEIGEN_HIP_GSTASH": gstash})
    u, exp = _expected_G(n, P)
    blk = _block(dtype, P, n, _lengths(n))
    blk.set_params(1.0, 0.01, 0.7, 0.3)
    if not sym:
        blk.set_field(_lib.FIELD_S, _stress(blk.field_shape(_lib.FIELD_S), 33, False))      # leaves symmetric storage
    blk.set_field(_lib.FIELD_U, u)
    assert blk.is_sym() == sym
    assert blk.stage_kernel_name(1) == _g_name(dtype, P, 0, sym, _fact(dtype, P, gq))
    blk.apply_G(_lib.FIELD_U, _lib.FIELD_SH)
    got = blk.get_field(_lib.FIELD_SH)
    blk.close()
    err = rel_err(got, exp)
    print("ERR class frame G %s P%d gq %s stash %s %s %s %.3e" % (dtype, P, gq, gstash, "sym" if sym else "full", n, err))
    assert err < (tol_of(P, "left") if dtype == "f64" else 2e-5)


@pytest.mark.parametrize("sym", [True, False], ids=["sym", "full"])
@pytest.mark.parametrize("n", SHAPES, **_ids)
def test_three_steps_at_degree_4_with_per_cell_material(gpu, monkeypatch, n, sym):
    """whole LF4 steps: the fused F modes 1 (U1, with the per-cell density in its combine) and 2 (UTEMP) and G mode 1"""
    from seigen_amd import _lib
    _environment(monkeypatch, "mfma", None)
    P = 4
    orc = _oracle(n, P)
    blk = _block("f64", P, n, _lengths(n))
    nc = 6 * n[0] * n[1] * n[2]
    rng = np.random.default_rng(7)
    orc.dt = 0.04 * min(H) / P ** 2
    orc.l, orc.mu = rng.uniform(0.4, 0.8, nc), rng.uniform(0.2, 0.4, nc)
    orc.density, orc.density_physical = rng.uniform(0.8, 1.5, nc), True
    orc.source = None
    orc.u0 = u_start = seeded(blk.field_shape(_lib.FIELD_U), 41)
    orc.s0 = _stress(blk.field_shape(_lib.FIELD_S), 42, sym)
    try:
        blk.set_params(1.0, orc.dt, orc.l, orc.mu)
        blk.set_density(orc.density, physical=True)
        blk.set_field(_lib.FIELD_U, orc.u0)
        blk.set_field(_lib.FIELD_S, orc.s0)
        assert blk.is_sym() == sym
        assert [blk.stage_kernel_name(st) for st in range(6)] == _stage_names("f64", P, sym, _fact("f64", P, None))
        blk.step(3)
        for k in range(3):
            orc.step((k + 1) * orc.dt)
        errs = (rel_err(blk.get_field(_lib.FIELD_U), orc.u1), rel_err(blk.get_field(_lib.FIELD_S), orc.s1))
    finally:
        blk.close()
        orc.l, orc.mu, orc.density, orc.density_physical = 0.5, 0.25, 1.0, False      # the oracle is shared
    print("ERR class frame steps %s %s u %.3e s %.3e" % ("sym" if sym else "full", n, *errs))
    assert max(errs) < 10 * tol_of(P, "left")
    assert rel_err(orc.u1, u_start) > 1e-4


@pytest.mark.parametrize("sym", [True, False], ids=["sym", "full"])
@pytest.mark.parametrize("P", [3, 4])
@pytest.mark.parametrize("n,grid", CUTS, ids=["cut-x", "cut-y", "cut-z"])
def test_blocks_are_bitwise_the_single_block(gpu, monkeypatch, n, grid, P, sym):
    """GHOST = 1: a remote record is read at entry p[i'], with the side's axis p[0] (facet 0) or p[2] (facet 3) in turn;
    _multiblock_case asserts np.array_equal on u and s"""
    from tests.test_harness_gpu import _multiblock_case
    _environment(monkeypatch, "mfma", None)
    res = _multiblock_case(3, P, n, grid, True, extras=True, dtype="f64", sym=sym)
    assert res["names"] == sorted(set(_stage_names("f64", P, sym, _fact("f64", P, None), ghost=1))), res["names"]
    assert rel_err(res["u"], res["u0"]) > 1e-4
