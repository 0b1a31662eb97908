"""Every instantiation of the 3-D tetrahedral matrix-pipe family (kernels_mfma.hip) against the FP64 oracle.

MFMA_KERNELS lists what launch_ps / launch_sponge_affine_mfma can dispatch; test_host_logic.py holds it equal to the kernel
objects the built library exports, so a new template argument cannot join the family without a row here.  Each row of
ROWS - (dtype, degree, symmetric stress, block, SEIGEN_HIP_GQ) - first pins the six stage kernels it runs by the names the
library reports, then checks one application of F and G and three whole LF4 steps with every extra at once: per-cell
material, a density (scalar, per cell, per cell physical), a nodal source with a node listed twice, and a DG4 sponge with
cells of all four kinds (none, constant, general nodal, affine) side by side in every item.  SPLIT rows run the same
(dtype, degree, symmetry) as two blocks along z (GHOST = 1) against the single block, bitwise, and the single block against
the oracle.  test_rows_name_every_stage_kernel checks that the rows together reach every mfma_stage_* instantiation.

Tolerances are the suite's own: FP64 tol_of() per application and 10 tol_of() for the steps (test_parity_gpu.py), FP32
2e-5 and 5e-5 (test_fp32_gpu.py)."""
import numpy as np
import pytest

from oracle.lf4 import OracleLF4
from tests.test_parity_gpu import tol_of
from tests.util import oracle_mesh, rel_err

pytestmark = pytest.mark.gpu

_TYPES = {"f64": "double", "f32": "float"}


def _f_name(dtype, P, mode, sym, ghost):
    return "sg::mfma_stage_F<%s, %d, %d, %d, %d>" % (_TYPES[dtype], P, mode, int(sym), ghost)


def _g_name(dtype, P, mode, sym, fact):
    return "sg::mfma_stage_G<%s, %d, %d, %d, %d>" % (_TYPES[dtype], P, mode, int(sym), fact)


# launch_ps: F in three modes (0: UH1 / apply_F, 1: U1, 2: UTEMP) with or without packed remote traces; G in two modes (0: STEMP,
# SH1 / apply_G, 1: S1), the factorised volume term (FACT = 1) in double from degree 3; both stress storages everywhere.
MFMA_KERNELS = frozenset(
    [_f_name(t, P, mode, sym, ghost) for t in _TYPES for P in (1, 2, 3, 4) for mode in (0, 1, 2) for sym in (0, 1)
     for ghost in (0, 1)]
    + [_g_name(t, P, mode, sym, 0) for t in _TYPES for P in (1, 2, 3, 4) for mode in (0, 1) for sym in (0, 1)]
    + [_g_name("f64", P, mode, sym, 1) for P in (3, 4) for mode in (0, 1) for sym in (0, 1)]
    + ["sg::sponge_affine_mfma<%d>" % P for P in (1, 2, 3, 4)])

# dtype, degree, symmetric stress, block, SEIGEN_HIP_GQ (None: the library's default - on from degree 4, double only).
# Blocks: n[0] <= 16 (one group per x row), 17 (a second group of one cube), >= 16 layers (the F stages' chunked XCD order),
# one cube.
ROWS = [
    ("f64", 1, True, (17, 3, 3), None),
    ("f64", 1, False, (5, 2, 17), None),
    ("f64", 1, True, (1, 1, 1), None),
    ("f64", 2, True, (3, 2, 16), None),
    ("f64", 2, False, (17, 3, 2), None),
    ("f64", 2, False, (1, 1, 1), None),
    ("f64", 3, True, (17, 2, 2), "0"),
    ("f64", 3, False, (2, 1, 16), "0"),
    ("f64", 3, True, (1, 1, 1), "1"),
    ("f64", 3, False, (16, 1, 2), "1"),
    ("f64", 4, True, (17, 1, 2), "1"),
    ("f64", 4, False, (1, 2, 16), "1"),
    ("f64", 4, True, (3, 1, 2), "0"),
    ("f64", 4, False, (1, 1, 1), "0"),
    ("f32", 1, True, (1, 1, 1), None),
    ("f32", 1, False, (17, 3, 3), None),
    ("f32", 1, True, (4, 2, 16), None),
    ("f32", 2, True, (3, 2, 16), None),
    ("f32", 2, False, (17, 3, 2), None),
    ("f32", 3, True, (2, 1, 16), None),
    ("f32", 3, False, (17, 2, 2), None),
    ("f32", 4, True, (17, 1, 2), None),
    ("f32", 4, False, (1, 2, 16), None),
    ("f32", 4, False, (1, 1, 1), None),
]

# one split per (dtype, degree, symmetry): the first row of the kind whose block has two layers or more
SPLITS = []
for _r in ROWS:
    if _r[3][2] >= 2 and not any(s[:3] == _r[:3] for s in SPLITS):
        SPLITS.append(_r[:4])

# degree 1 where the family is the default (65 664 cells: 19 layers, ragged x) and just below it (65 532 cells)
BIG = (24, 24, 19)
BELOW = (2, 43, 127)


def _fact(dtype, P, gq):
    return int(dtype == "f64" and P >= 3 and (gq == "1" if gq is not None else P >= 4))


def _stage_names(dtype, P, sym, fact, ghost=0):
    """the instantiation each of the six stages launches (hostlogic.hpp lf4_stage)"""
    return [_f_name(dtype, P, 0, sym, ghost), _g_name(dtype, P, 0, sym, fact), _f_name(dtype, P, 1, sym, ghost),
            _g_name(dtype, P, 0, sym, fact), _f_name(dtype, P, 2, sym, ghost), _g_name(dtype, P, 1, sym, fact)]


def _row_id(r):
    return "%s-P%d-%s-%s%s" % (r[0], r[1], "sym" if r[2] else "full", "x".join(map(str, r[3])),
                               "" if len(r) < 5 or r[4] is None else "-gq" + r[4])


# the switches that pick the persistent grid, the item order and the launch form of the G stages at degree 4: unset in
# every row here; tests/test_item_loop_gpu.py sets them
LAUNCH_SWITCHES = ("SEIGEN_HIP_GRID_BLOCKS", "SEIGEN_HIP_ORDER_CHUNK", "SEIGEN_HIP_GSTASH")


def _environment(monkeypatch, path, gq, launch=None):
    """a row's switches, and nothing else that picks an instantiation or the sponge's form; launch: values for
    LAUNCH_SWITCHES (None or missing: unset)"""
    for var in ("SEIGEN_HIP_SPONGE_AFFINE", "SEIGEN_HIP_SYM", "SEIGEN_HIP_GQ", "SEIGEN_HIP_PATH"):
        monkeypatch.delenv(var, raising=False)
    if path:
        monkeypatch.setenv("SEIGEN_HIP_PATH", path)
    if gq is not None:
        monkeypatch.setenv("SEIGEN_HIP_GQ", gq)
    if launch is not None:
        assert set(launch) <= set(LAUNCH_SWITCHES), launch
        for var in LAUNCH_SWITCHES:
            if launch.get(var) is None:
                monkeypatch.delenv(var, raising=False)
            else:
                monkeypatch.setenv(var, launch[var])


def _block(dtype, P, n, L):
    from seigen_amd.backend import HipBlock
    return HipBlock(3, P, n, [L[a] / n[a] for a in range(3)], [0.0] * 3, "left", dtype=dtype)


def _stress(shape, rng, sym):
    s = rng.uniform(-1, 1, shape)
    return 0.5 * (s + np.swapaxes(s, -1, -2)) if sym else s


def _sponge(m, rng):
    """DG4 nodal sigma: cells of all four kinds - none, one value (sigma u at the node), general nodal (a matrix of its
    own), affine in x with a gradient of its own (four coefficients: sponge_affine_mfma in double, sponge_pre_affine_kernel
    in float) - by cell % 4.  A cell is 6 cube + class, so the items (16 cubes of one class) of an odd class hold the
    constant and the affine cells, those of an even class the cells with none and the cells with a matrix"""
    Xq = m.node_coords(4)
    kind = np.arange(m.ncells) % 4
    sigma = np.zeros(Xq.shape[:2])
    c, g, a = kind == 1, kind == 2, kind == 3
    sigma[c] = rng.uniform(2.0, 30.0, size=(c.sum(), 1))
    sigma[g] = rng.uniform(0.0, 30.0, size=(g.sum(), Xq.shape[1]))
    grad = rng.uniform(-20.0, 20.0, size=(a.sum(), 1, 3))
    sigma[a] = rng.uniform(5.0, 30.0, size=(a.sum(), 1)) + (grad * (Xq[a] - Xq[a][:, :1])).sum(axis=-1)
    return sigma


def _source_nodes(n, nd, rng):
    """scattered nodes, nodes of the last cube in x (the last, partly filled group where n[0] = 17), one node twice"""
    ncube = n[0] * n[1] * n[2]
    last = (np.arange(n[1] * n[2]) * n[0] + n[0] - 1)[:3]                 # cubes (n[0] - 1, j, k)
    nodes = rng.integers(0, 6 * ncube * nd, size=10)
    nodes = np.concatenate([nodes, (6 * last + 5) * nd + rng.integers(0, nd, size=len(last)), nodes[:1]])
    assert len(np.unique(nodes)) < len(nodes)
    return nodes


def _oracle_source(nc, nd, nodes, vals):
    S = np.zeros((nc * nd, 3, 3))
    np.add.at(S, nodes, vals)
    return S.reshape(nc, nd, 3, 3)


def _tolerances(dtype, P):
    return (tol_of(P, "left"), 10 * tol_of(P, "left")) if dtype == "f64" else (2e-5, 5e-5)


def _figure(what, e):
    """the figure, printed before anything is asserted on it"""
    print("ERR mfma %s %.3e" % (what, e))
    return e


class SharedOracle(object):
    """The oracle of block n at degree P, built once and lent to several rows (_check_row's `oracle`): its operators, and
    the sponge matrix of one _sponge sigma - at degree 4 the two take seconds, the steps of a row a second."""

    def __init__(self, n, P, seed):
        self.n, self.P = tuple(n), P
        self.m = oracle_mesh(3, n, tuple(0.4 * k for k in n))
        self.orc = OracleLF4(self.m, P)
        self.sigma = _sponge(self.m, np.random.default_rng(seed))
        self.sigma.setflags(write=False)
        self.orc.E.set_absorption(self.sigma, 4)
        self.absorb, self.orc.E.absorb = self.orc.E.absorb, None

    def lend(self):
        """as a fresh OracleLF4 has it: no sponge, no source, the explicit reference's density convention"""
        orc = self.orc
        orc.E.absorb, orc.source, orc.density, orc.density_physical = None, None, 1.0, False
        return self.m, orc


def _check_row(dtype, P, sym, n, gq, density, oracle=None):
    """one application of F and G, then three steps with every extra, against the oracle; returns the names the stages
    reported.  oracle: a SharedOracle of (n, P) to use instead of building one (its sigma is then the row's sponge)"""
    from seigen_amd import _lib
    L = tuple(0.4 * k for k in n)
    h = [L[a] / n[a] for a in range(3)]
    tol1, tol3 = _tolerances(dtype, P)
    rng = np.random.default_rng(1000 * P + 10 * n[0] + n[2] + (0 if dtype == "f64" else 7))
    if oracle is None:
        m = oracle_mesh(3, n, L)
        orc = OracleLF4(m, P)
    else:
        assert (oracle.n, oracle.P) == (tuple(n), P)
        m, orc = oracle.lend()
    nc = m.ncells
    lam, mu = rng.uniform(0.4, 0.8, nc), rng.uniform(0.2, 0.4, nc)

    # the instantiations, before anything runs
    blk = _block(dtype, P, n, L)
    nd = blk.nd
    T = _stress(blk.field_shape(_lib.FIELD_S), rng, sym)
    u = rng.uniform(-1, 1, blk.field_shape(_lib.FIELD_U))
    blk.set_params(1.0, 0.01, lam, mu)
    blk.set_field(_lib.FIELD_S, T)
    blk.set_field(_lib.FIELD_U, u)
    assert blk.is_sym() == sym
    names = [blk.stage_kernel_name(st) for st in range(6)]
    assert names == _stage_names(dtype, P, sym, _fact(dtype, P, gq)), names

    # one application of each operator (the MODE 0 kernels)
    blk.apply_F(_lib.FIELD_S, _lib.FIELD_U, _lib.FIELD_UH)
    assert _figure("F", rel_err(blk.get_field(_lib.FIELD_UH), orc.E.apply_F(T, u))) < tol1
    blk.apply_G(_lib.FIELD_U, _lib.FIELD_SH)
    assert _figure("G", rel_err(blk.get_field(_lib.FIELD_SH), orc.E.apply_G(u, lam, mu))) < tol1
    blk.close()

    # three whole steps
    blk = _block(dtype, P, n, L)
    orc.dt, orc.l, orc.mu = 0.04 * min(h) / P ** 2, lam, mu
    orc.u0 = rng.uniform(-1, 1, blk.field_shape(_lib.FIELD_U))
    orc.s0 = _stress(blk.field_shape(_lib.FIELD_S), rng, sym)
    u_start = orc.u0
    if density == "scalar":                 # the explicit reference's u1 = rho u0 + ...
        orc.density = 1.1
        blk.set_params(orc.density, orc.dt, lam, mu)
    else:
        orc.density = rng.uniform(0.9, 1.1, nc) if density == "cell" else rng.uniform(0.8, 1.5, nc)
        orc.density_physical = density == "physical"
        blk.set_params(1.0, orc.dt, lam, mu)
        blk.set_density(orc.density, physical=orc.density_physical)
    if oracle is None:
        sigma = _sponge(m, rng)
        orc.E.set_absorption(sigma, 4)
    else:
        sigma, orc.E.absorb = oracle.sigma, oracle.absorb
    blk.set_absorption(sigma, 4)
    nodes = _source_nodes(n, nd, rng)
    vals = _stress((3, len(nodes), 3, 3), rng, sym)
    blk.set_source(nodes, vals)
    blk.set_field(_lib.FIELD_U, orc.u0)
    blk.set_field(_lib.FIELD_S, orc.s0)
    assert blk.is_sym() == sym
    assert [blk.stage_kernel_name(st) for st in range(6)] == names
    blk.step(3)
    for k in range(3):
        orc.source = lambda t, k=k: _oracle_source(nc, nd, nodes, vals[k])
        orc.step((k + 1) * orc.dt)
    assert _figure("steps u", rel_err(blk.get_field(_lib.FIELD_U), orc.u1)) < tol3
    assert _figure("steps s", rel_err(blk.get_field(_lib.FIELD_S), orc.s1)) < tol3
    # what the last step left behind: w = dt u1 + dt^3/24 utemp (UTEMP, MODE 2) and sh1 = G(u1) + S (SH1)
    assert _figure("steps uh", rel_err(blk.get_field(_lib.FIELD_UH), orc.dt * orc.u1 + orc.dt ** 3 / 24.0 * orc.last["utemp"])) < tol3
    assert _figure("steps sh", rel_err(blk.get_field(_lib.FIELD_SH), orc.last["sh1"])) < tol3
    assert rel_err(orc.u1, u_start) > 1e-4
    blk.close()
    return names


@pytest.mark.parametrize("row", ROWS, ids=_row_id)
def test_row_against_the_oracle(gpu, monkeypatch, row):
    dtype, P, sym, n, gq = row
    _environment(monkeypatch, "mfma", gq)
    _check_row(dtype, P, sym, n, gq, ("scalar", "cell", "physical")[ROWS.index(row) % 3])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_degree_1_where_the_family_is_the_default(gpu, monkeypatch, dtype):
    """(24, 24, 19): 65 664 cells, from 65 536 the family is chosen without SEIGEN_HIP_PATH (hostapi.cpp
    choose_kernel_path)"""
    _environment(monkeypatch, None, None)
    names = _check_row(dtype, 1, dtype == "f64", BIG, None, "physical" if dtype == "f64" else "cell")
    assert all(nm.startswith("sg::mfma_stage_") for nm in names), names


def test_degree_1_below_the_threshold(gpu, monkeypatch):
    """(2, 43, 127): 65 532 cells - another family in double, and float (MFMA only) refused"""
    from seigen_amd import _lib
    _environment(monkeypatch, None, None)
    L = tuple(0.4 * k for k in BELOW)
    with pytest.raises(_lib.SeigenHipError, match="dtype f32 is implemented on the MFMA paths"):
        _block("f32", 1, BELOW, L)
    blk = _block("f64", 1, BELOW, L)
    assert blk.ncells == 65532
    blk.set_params(1.0, 0.01, 0.5, 0.25)
    names = [blk.stage_kernel_name(st) for st in range(6)]
    assert not any("mfma" in nm for nm in names), names
    blk.close()


@pytest.mark.parametrize("split", SPLITS, ids=_row_id)
def test_split_row_is_bitwise_the_single_block(gpu, monkeypatch, split):
    """GHOST = 1: two blocks along z through the host-driven exchange (test_harness_gpu._LocalExchange), bitwise equal
    to the single block, and the single block against the oracle"""
    from tests.test_harness_gpu import _multiblock_case
    dtype, P, sym, n = split
    _environment(monkeypatch, "mfma", None)
    res = _multiblock_case(3, P, n, (1, 1, 2), True, extras=True, dtype=dtype, sym=sym)
    assert res["names"] == sorted(set(_stage_names(dtype, P, sym, _fact(dtype, P, None), ghost=1))), res["names"]
    m = oracle_mesh(3, n, (1.0, 1.0, 1.0))
    orc = OracleLF4(m, P)
    nc, nd = m.ncells, orc.E.nd
    orc.dt, orc.l, orc.mu, orc.density = res["dt"], 0.5, 0.25, 1.0
    orc.E.set_absorption(res["sigma"], 4)
    orc.u0, orc.s0 = res["u0"].copy(), res["s0"].copy()
    for k in range(3):
        orc.source = lambda t, k=k: _oracle_source(nc, nd, res["src_nodes"], res["src_steps"][k])
        orc.step((k + 1) * orc.dt)
    tol3 = _tolerances(dtype, P)[1]
    assert rel_err(res["u"], orc.u1) < tol3
    assert rel_err(res["s"], orc.s1) < tol3


def test_rows_name_every_stage_kernel(gpu, monkeypatch):
    """The rows above - ROWS, the default-size blocks, SPLITS - together launch every mfma_stage_* instantiation.  Each
    row's block (two blocks with zero halo buffers attached for a split) is set up as its test sets it up and asked for its
    six kernels.  sponge_affine_mfma<P> cannot be named: it runs on every double row with affine cells and
    SEIGEN_HIP_SPONGE_AFFINE unset (api.cpp sg_set_absorption `aff_mfma`), which is every row here."""
    torch = pytest.importorskip("torch")
    from seigen_amd import _lib
    from seigen_amd.backend import HipBlock
    from seigen_amd.mesh import Partition
    seen = set()
    rows = [(r, "mfma") for r in ROWS] + [((t, 1, t == "f64", BIG, None), None) for t in ("f64", "f32")]
    for (dtype, P, sym, n, gq), path in rows:
        _environment(monkeypatch, path, gq)
        blk = _block(dtype, P, n, tuple(0.4 * k for k in n))
        blk.set_params(1.0, 0.01, 0.5, 0.25)
        if not sym:
            blk.leave_sym()
        names = [blk.stage_kernel_name(st) for st in range(6)]
        assert names == _stage_names(dtype, P, sym, _fact(dtype, P, gq)), names
        seen.update(names)
        blk.close()
    for dtype, P, sym, n in SPLITS:
        _environment(monkeypatch, "mfma", None)
        bufs = []
        for p in (Partition(n, r, 2, (1, 1, 2)) for r in range(2)):
            b = HipBlock(3, P, p.n, [1.0 / k for k in n], [p.start[a] / n[a] for a in range(3)], "left", p.nbr_mask,
                         dtype=dtype)
            b.set_params(1.0, 0.01, 0.5, 0.25)
            if not sym:
                b.leave_sym()
            for field in range(4):
                for s in range(6):
                    if p.neighbour(s) is not None:
                        bufs.append(torch.zeros(b.halo_bytes(field, s), dtype=torch.uint8, device="cuda"))
                        b.halo_attach(field, s, bufs[-1].data_ptr())
            names = [b.stage_kernel_name(st) for st in range(6)]
            assert names == _stage_names(dtype, P, sym, _fact(dtype, P, None), ghost=1), names
            seen.update(names)
            b.close()
    stage_kernels = {k for k in MFMA_KERNELS if k.startswith("sg::mfma_stage_")}
    assert len(stage_kernels) == 136
    assert stage_kernels <= seen, sorted(stage_kernels - seen)
    assert seen <= stage_kernels, sorted(seen - stage_kernels)
    for P in (1, 2, 3, 4):
        assert any(r[0] == "f64" and r[1] == P for r in ROWS), P
