"""The correlation: the zero-lag cross-correlation of two handles' fields, cell by cell, accumulated on the device
(include/seigen_hip.h sg_correlate / sg_get_correlation / sg_reset_correlation; kernels_xcorr.hip).  Every layout and every
pair of storage modes against the host's bilinear forms of the downloaded fields, the two kernel forms against each other,
accumulation and reset, the bitwise promises, the monitor's sums, the ordering against the other handle's steps, the
refusals, and the solver class on the reference's 2-D eigenmode.

The bound everywhere: 1e-11 * scale per cell and entry, the project's per-operator parity bound, with
scale_c = |det J| |w_k| sum |a|^T |Mhat| |b| (the traces' scale from |t_a|, |t_b|), summed over the calls that went into the
accumulator.  Device and host differ in the order of summation only, over at most 125^2 * 9 terms."""
import math
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import mesh as omesh  # noqa: E402
from oracle import refelem  # noqa: E402
from seigen_amd import _lib  # noqa: E402
from seigen_amd.backend import HipBlock  # noqa: E402

from test_receivers_gpu import FAMILIES, make_case  # noqa: E402

# the receivers' thirteen rows, and the monitor's further ones: the FP32 P3 block of the 3-D matrix-pipe layout and an FP32
# 2-D tile block (kernel objects of their own); a lane block of 77 cubes, no multiple of 64; a generic block of 1030 items,
# no multiple of the 64 a workgroup takes.  (4, 3, 2) cubes are two 16-cube groups with eight padding lanes; hexm-DQ4 is
# the LDS limit (one item per workgroup, 64 000 B).
ROWS = FAMILIES + [
    ("mfma-P3-f32", 3, 3, (4, 3, 2), "left", "f32", None, True),
    ("tile-tri-P3-f32", 2, 3, (5, 3), "left", "f32", None, True),
    ("lane-2d-77", 2, 2, (11, 7), "left", "f64", "lane", True),
    ("generic-1d-P1-1030", 1, 1, (1030,), "left", "f64", None, True),
]
ROW = {r[0]: r for r in ROWS}
W = np.array([0.7, -1.3, 2.1])
BOUND = 1e-11


def _env(monkeypatch, path=None, graph=None, xcorr=None):
    for name, val in (("SEIGEN_HIP_PATH", path), ("SEIGEN_HIP_XCORR", xcorr),
                      ("SEIGEN_HIP_GRAPH", None if graph is None else ("1" if graph else "0"))):
        if val:
            monkeypatch.setenv(name, val)
        else:
            monkeypatch.delenv(name, raising=False)


def _other_fields(blk, dim, sym, seed):
    """smooth fields unlike make_case's: phases from `seed`; sym: a symmetric stress, else s_ij != s_ji"""
    ph = np.random.default_rng(seed).uniform(0.0, 2.0 * np.pi, dim + dim * dim)
    X = blk.node_coords()
    u = np.stack([np.cos(3 * X[..., 0] + ph[i]) * np.sin(2 * X[..., -1] + 0.5 * i + 1.0) for i in range(dim)], axis=-1)
    s = np.zeros(X.shape[:-1] + (dim, dim))
    for i in range(dim):
        for j in range(dim):
            k = (min(i, j) * dim + max(i, j)) if sym else i * dim + j
            s[..., i, j] = np.sin(2 * X[..., 0] + ph[dim + k]) * (1.5 - X[..., -1])
    return u, s


def _block(spec, monkeypatch, sym=None, other=None, graph=None):
    """the block of a row; sym overrides the row's storage; other = seed: different smooth fields"""
    name, dim, degree, n, diagonal, dtype, path, rsym = spec
    sym = rsym if sym is None else sym
    _env(monkeypatch, path, graph)
    blk, dt = make_case(dim, degree, n, diagonal, dtype, sym)
    if other is not None:
        u, s = _other_fields(blk, dim, sym, other)
        blk.set_field(_lib.FIELD_U, u)
        blk.set_field(_lib.FIELD_S, s)
    assert dim == 1 or path == "generic" or blk.is_sym() == sym
    return blk


def _fields(blk):
    return blk.get_field(_lib.FIELD_U), blk.get_field(_lib.FIELD_S)


_GEOM = {}


def _geom(dim, degree, n, diagonal):
    """(Mhat by quadrature from oracle.refelem, |det J| per cell) of the block of the unit box"""
    key = (dim, degree, tuple(n), diagonal)
    if key not in _GEOM:
        quad = diagonal == "quadrilateral"
        mesh = omesh.structured(dim, n, (1.0,) * dim, diagonal if not quad else "left", quadrilateral=quad)
        kind = getattr(mesh, "kind", "simplex")
        xq, wq = refelem.el_quadrature(dim, 2 * degree, kind)
        phi, _ = refelem.el_tabulate(dim, degree, xq, kind)
        _GEOM[key] = (np.einsum('q,qa,qb->ab', wq, phi, phi), np.abs(mesh.detJ))
    return _GEOM[key]


def host_forms(spec, fa, fb):
    """(B [ncells, 3], scale [ncells, 3]) = |det J| (Buu, Bss, Btt) of a's fields against b's, and the same of the absolute
    values; no weights"""
    name, dim, degree, n, diagonal = spec[:5]
    M, dj = _geom(dim, degree, n, diagonal)
    (ua, sa), (ub, sb) = fa, fb
    ta, tb = np.einsum('cnii->cn', sa), np.einsum('cnii->cn', sb)
    sa2, sb2 = sa.reshape(sa.shape[0], sa.shape[1], -1), sb.reshape(sb.shape[0], sb.shape[1], -1)
    def form(x, y, m):      # x^T m y per cell, summed over the components: [c, a, k] x [a, b] x [c, b, k]
        return np.sum(x * np.matmul(m, y), axis=(1, 2))

    aM = np.abs(M)
    B = np.stack([form(ua, ub, M), form(sa2, sb2, M), form(ta[..., None], tb[..., None], M)], axis=-1)
    S = np.stack([form(np.abs(ua), np.abs(ub), aM), form(np.abs(sa2), np.abs(sb2), aM),
                  form(np.abs(ta)[..., None], np.abs(tb)[..., None], aM)], axis=-1)
    return dj[:, None] * B, dj[:, None] * S


def _unlike(x, y, scale):
    """at least one cell's ss differs between two pairings by more than 1e-3 of its scale"""
    return np.max(np.abs(x[:, 1] - y[:, 1]) / scale[:, 1]) > 1e-3


def _check(name, got, want, scale, bound=BOUND):
    err = np.abs(got - want) / np.maximum(scale, 1e-300)
    print(name, "largest |device - host| / scale per entry:", err.max(axis=0))
    assert np.isfinite(got).all() and np.all(scale.max(axis=0) > 0)
    assert np.all(np.abs(got - want) <= bound * scale), (name, err.max())


def _upper(s):
    """the tensor a symmetric-storage reader would see: (i, j) from the line (min, max)"""
    r = s.copy()
    for i in range(s.shape[-1]):
        for j in range(i):
            r[..., i, j] = s[..., j, i]
    return r


@pytest.mark.parametrize("spec", ROWS, ids=[r[0] for r in ROWS])
def test_every_layout_correlates_what_the_host_does(gpu, monkeypatch, spec):
    """Two handles with different smooth fields, stepped a few times (padding lanes and stale mirror lines then hold what
    the stage kernels leave there), one sg_correlate with non-trivial weights against the host's forms of the downloaded
    fields.  On the host first: B(a, b) is neither B(a, a) nor B(b, b), so reading one handle for both sides fails."""
    name = spec[0]
    a, b = _block(spec, monkeypatch), _block(spec, monkeypatch, other=5)
    a.step(3)
    b.step(2)
    fa, fb = _fields(a), _fields(b)
    want, scale = host_forms(spec, fa, fb)
    assert _unlike(want, host_forms(spec, fa, fa)[0], scale) and _unlike(want, host_forms(spec, fb, fb)[0], scale)
    a.correlate(b, W)
    got = a.get_correlation()
    assert got.shape == (a.ncells, 3)
    _check(name, got, W * want, np.abs(W) * scale)
    # the fields are read, not written
    for x, fx in ((a, fa), (b, fb)):
        u, s = _fields(x)
        assert np.array_equal(u, fx[0]) and np.array_equal(s, fx[1])
    a.close()
    b.close()


def test_a_wave_of_the_persistent_grid_takes_more_than_one_item(gpu, monkeypatch):
    """The matrix-pipe form runs a persistent grid of the blocks the device holds - at P4 two blocks of four waves per CU,
    2048 waves on 256 CUs - and a wave strides over the items: (16, 16, 22) cubes are 2112 items, so 64 waves take a second
    one.  Plain blocks without sponge or source, the fields as uploaded (FP64: the device holds these values exactly)."""
    dim, degree, n = 3, 4, (16, 16, 22)
    spec = ("mfma-P4-2112-items", dim, degree, n, "left")
    _env(monkeypatch)
    fields, blocks = [], []
    for seed in (3, 5):
        blk = HipBlock(dim, degree, n, [1.0 / k for k in n], [0.0] * dim, "left")
        blk.set_params(1.0, 1e-4, 0.5, 0.25)
        u, s = _other_fields(blk, dim, True, seed)
        blk.set_field(_lib.FIELD_U, u)
        blk.set_field(_lib.FIELD_S, s)
        assert blk.is_sym()
        fields.append((u, s))
        blocks.append(blk)
    a, b = blocks
    want, scale = host_forms(spec, fields[0], fields[1])
    a.correlate(b, W)
    _check(spec[0], a.get_correlation(), W * want, np.abs(W) * scale)
    a.close()
    b.close()


@pytest.mark.parametrize("name", ["mfma-P4-sym", "tile-tri-P3"])
@pytest.mark.parametrize("sym_a,sym_b", [(True, True), (True, False), (False, True), (False, False)])
def test_storage_pairs(gpu, monkeypatch, name, sym_a, sym_b):
    """(sym, sym), (sym, full), (full, sym), (full, full): a handle in full storage holds a genuinely non-symmetric stress.
    On the host first: the value differs from what a reader of the (min, max) lines of a full handle would form, and in
    (full, full) from the transposed pairing a.s_ij with b.s_ji."""
    spec = ROW[name]
    a, b = _block(spec, monkeypatch, sym=sym_a), _block(spec, monkeypatch, sym=sym_b, other=5)
    a.step(2)
    b.step(3)
    assert a.is_sym() == sym_a and b.is_sym() == sym_b
    fa, fb = _fields(a), _fields(b)
    want, scale = host_forms(spec, fa, fb)
    if not sym_a:
        assert _unlike(want, host_forms(spec, (fa[0], _upper(fa[1])), fb)[0], scale)
    if not sym_b:
        assert _unlike(want, host_forms(spec, fa, (fb[0], _upper(fb[1])))[0], scale)
    if not sym_a and not sym_b:
        assert _unlike(want, host_forms(spec, fa, (fb[0], np.swapaxes(fb[1], -1, -2)))[0], scale)
        assert _unlike(want, host_forms(spec, (fa[0], _upper(fa[1])), (fb[0], _upper(fb[1])))[0], scale)
    a.correlate(b, W)
    _check("%s %s/%s" % (name, sym_a, sym_b), a.get_correlation(), W * want, np.abs(W) * scale)
    a.close()
    b.close()


@pytest.mark.parametrize("name", ["mfma-P4-sym", "mfma-P3-sym"])
def test_forced_generic_form_agrees_with_the_matrix_pipe_form(gpu, monkeypatch, name):
    """SEIGEN_HIP_XCORR=lds (read when a handle's correlation tables are built) on a block of the 3-D matrix-pipe layout:
    the two forms agree to 2e-11 * scale - each within 1e-11 of the exact value - and both agree with the host."""
    spec = ROW[name]
    a, b = _block(spec, monkeypatch), _block(spec, monkeypatch, other=5)
    a.step(3)
    b.step(2)
    want, scale = host_forms(spec, _fields(a), _fields(b))
    a.correlate(b, W)
    first = a.get_correlation()
    a.reset_correlation(release=True)
    _env(monkeypatch, spec[6], xcorr="lds")
    a.correlate(b, W)
    forced = a.get_correlation()
    _check(name + " default", first, W * want, np.abs(W) * scale)
    _check(name + " lds", forced, W * want, np.abs(W) * scale)
    _check(name + " default against lds", first, forced, np.abs(W) * scale, 2e-11)
    a.close()
    b.close()


@pytest.mark.parametrize("name", ["mfma-P4-sym", "tile-tri-P3"])
def test_accumulation_and_reset(gpu, monkeypatch, name):
    spec = ROW[name]
    a, b = _block(spec, monkeypatch), _block(spec, monkeypatch, other=5)
    # nothing yet: SG_ERR_STATE
    buf = np.zeros((a.ncells, 3))
    assert a.lib.sg_get_correlation(a.h, buf.ctypes.data, buf.nbytes) == -3
    assert a.lib.sg_reset_correlation(a.h, 0) == 0
    want, scale = np.zeros((a.ncells, 3)), np.zeros((a.ncells, 3))
    ws = [np.array([1.0, 0.5, -2.0]), np.array([-0.25, 3.0, 1.0]), np.array([2.0, -1.0, 0.125])]
    for w in ws:
        a.step(2)
        b.step(2)
        B, S = host_forms(spec, _fields(a), _fields(b))
        want += w * B
        scale += np.abs(w) * S
        a.correlate(b, w)
    _check(name + " three calls", a.get_correlation(), want, scale)
    # reset, then one call = that call alone (a fresh accumulator), bit for bit
    a.reset_correlation()
    assert not a.get_correlation().any()
    a.correlate(b, ws[2])
    after_reset = a.get_correlation()
    a.reset_correlation(release=True)
    assert a.lib.sg_get_correlation(a.h, buf.ctypes.data, buf.nbytes) == -3
    a.correlate(b, ws[2])
    alone = a.get_correlation()
    assert np.array_equal(after_reset, alone) and alone.any()
    _check(name + " one call", alone, ws[2] * B, np.abs(ws[2]) * S)
    # w = NULL is (1, 1, 1)
    a.reset_correlation()
    a.correlate(b)
    ones = a.get_correlation()
    a.reset_correlation()
    a.correlate(b, np.ones(3))
    assert np.array_equal(ones, a.get_correlation())
    a.close()
    b.close()


@pytest.mark.parametrize("name", ["mfma-P4-sym", "tile-tri-P3", "generic-2d-P2"])
def test_bits_depend_on_the_cell_alone(gpu, monkeypatch, name):
    """Repeated into a reset accumulator: equal bits.  b = a: the bits of a second handle holding copies of a's fields.  A
    block created with nbr_mask != 0 (other stage kernels, ghost buffers) holding the same fields: the same bits per cell."""
    spec = ROW[name]
    dim, degree, n, diagonal = spec[1:5]
    a, b = _block(spec, monkeypatch), _block(spec, monkeypatch, other=5)
    a.step(3)
    b.step(2)
    a.correlate(b, W)
    first = a.get_correlation()
    a.reset_correlation()
    a.correlate(b, W)
    assert np.array_equal(first, a.get_correlation())
    # b = a against a copy of a
    ua, sa = _fields(a)
    b.set_field(_lib.FIELD_U, ua)
    b.set_field(_lib.FIELD_S, sa)
    assert b.is_sym() == a.is_sym()
    a.reset_correlation()
    a.correlate(a, W)
    own = a.get_correlation()
    a.reset_correlation()
    a.correlate(b, W)
    assert np.array_equal(own, a.get_correlation()) and own.any()
    # a block with neighbour blocks on both x sides
    _env(monkeypatch, spec[6])
    c = HipBlock(dim, degree, n, [1.0 / k for k in n], [0.0] * dim, diagonal, nbr_mask=3)
    c.set_params(1.0, 1e-3, 0.5, 0.25)
    c.set_field(_lib.FIELD_U, ua)
    c.set_field(_lib.FIELD_S, sa)
    c.correlate(c, W)
    assert np.array_equal(own, c.get_correlation())
    for x in (a, b, c):
        x.close()


@pytest.mark.parametrize("name", ["mfma-P4-sym", "tile-tri-P3", "hexm-DQ3", "generic-2d-P2"])
def test_sums_over_cells_are_the_monitor_s(gpu, monkeypatch, name):
    """b = a, w = (1, 1, 1): math.fsum over the cells of each column equals sg_measure's U2, S2, T2 to 1e-11 * sum of the
    cells' scales (the forms are then quadratic and every term's scale is the term itself or larger)."""
    spec = ROW[name]
    a = _block(spec, monkeypatch)
    a.step(3)
    _, scale = host_forms(spec, _fields(a), _fields(a))
    a.correlate(a)
    got = a.get_correlation()
    sample = a.measure(None)
    for k in range(3):
        total, bound = math.fsum(got[:, k]), BOUND * math.fsum(scale[:, k])
        print(name, "uu ss tt"[3 * k:3 * k + 2], total, sample[k], abs(total - sample[k]) / math.fsum(scale[:, k]))
        assert sample[k] > 0 and abs(total - sample[k]) <= bound
    a.close()


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_a_later_step_of_b_does_not_reach_the_correlation(gpu, monkeypatch, graph):
    """sg_step(b, 3); sg_correlate(a, b); sg_step(b, 3); get: the value of b's fields after the first three steps (downloaded
    in an identical second run; the step itself is deterministic)."""
    spec = ROW["tile-tri-P3"]
    a, b = _block(spec, monkeypatch, graph=graph), _block(spec, monkeypatch, other=5, graph=graph)
    twin = _block(spec, monkeypatch, other=5, graph=graph)
    b.step(3)
    a.correlate(b, W)
    b.step(3)
    got = a.get_correlation()
    twin.step(3)
    f3 = _fields(twin)
    want, scale = host_forms(spec, _fields(a), f3)
    twin.step(3)
    assert np.array_equal(_fields(b)[0], _fields(twin)[0])
    assert _unlike(want, host_forms(spec, _fields(a), _fields(twin))[0], scale * 1e-6), "three more steps change nothing: the test shows nothing"
    _check("ordering graph=%s" % graph, got, W * want, np.abs(W) * scale)
    for x in (a, b, twin):
        x.close()


def test_refusals_leave_the_accumulator_alone(gpu, monkeypatch):
    """Handles that differ in degree, dtype, n or kernel family: SG_ERR_ARG, the message names the difference, the
    accumulator keeps its bits; a buffer of another size likewise."""
    spec = ROW["tile-tri-P3"]
    name, dim, degree, n, diagonal, dtype, path, sym = spec
    a, b = _block(spec, monkeypatch), _block(spec, monkeypatch, other=5)
    a.correlate(b, W)
    before = a.get_correlation()
    assert before.any()
    others = [("degree", (name, dim, 2, n, diagonal, dtype, path, sym)),
              ("dtype", (name, dim, degree, n, diagonal, "f32", path, sym)),
              ("n[0]", (name, dim, degree, (6, 3), diagonal, dtype, path, sym)),
              ("layout", (name, dim, degree, n, diagonal, dtype, "generic", sym))]
    for word, other in others:
        c = _block(other, monkeypatch)
        assert a.lib.sg_correlate(a.h, c.h, W.ctypes.data) == -1
        msg = a.lib.sg_last_error(a.h).decode()
        assert word in msg, (word, msg)
        # ... and the other way round, on a handle without an accumulator: still none afterwards
        buf = np.zeros((c.ncells, 3))
        assert c.lib.sg_correlate(c.h, a.h, W.ctypes.data) == -1
        assert c.lib.sg_get_correlation(c.h, buf.ctypes.data, buf.nbytes) == -3
        assert np.array_equal(a.get_correlation(), before)
        c.close()
    assert a.lib.sg_correlate(a.h, None, W.ctypes.data) == -1
    buf = np.zeros(before.size + 1)
    assert a.lib.sg_get_correlation(a.h, buf.ctypes.data, buf.nbytes) == -1
    assert a.lib.sg_get_correlation(a.h, None, before.nbytes) == -1
    assert not buf.any() and np.array_equal(a.get_correlation(), before)
    # the handles still work
    a.correlate(b, W)
    assert np.array_equal(a.get_correlation(), 2 * before)
    a.close()
    b.close()


def test_solver_class_on_the_eigenmode(gpu, monkeypatch):
    """Two ElasticLF4 on the reference's 2-D eigenmode (N = 8, P2), the second started at another phase: `correlate` once
    per step over 10 steps with weights (dt, dt, dt) against the host's sum over the states downloaded step by step;
    `sensitivity` of the result is finite, one value per cell."""
    from seigen_amd import Function
    from seigen_amd.elastic import sensitivity
    from seigen_amd.harness.eigenmode import Eigenmode2DLF4
    _env(monkeypatch)
    N, P, dt, steps = 8, 2, 0.25 / 8, 10
    spec = ("eigenmode", 2, P, (N, N), "left")
    ems = [Eigenmode2DLF4(N, P, dt, output=False) for _ in range(2)]
    for em, t0 in zip(ems, (0.0, 0.4)):
        el = em.elastic
        el.u0.assign(Function(el.U).interpolate(em._u(t0)))
        el.s0.assign(Function(el.S).interpolate(em._s(t0 + dt / 2.0)))
        el.setup()
    fwd, adj = ems[0].elastic, ems[1].elastic
    want, scale = 0.0, 0.0
    for _ in range(steps):
        fwd.block.step(1)
        adj.block.step(1)
        B, S = host_forms(spec, _fields(fwd.block), _fields(adj.block))
        want, scale = want + dt * B, scale + dt * S
        fwd.correlate(adj, (dt, dt, dt))
    corr = fwd.correlation()
    got = np.stack([corr["uu"], corr["ss"], corr["tt"]], axis=-1)
    assert got.shape == (fwd.block.ncells, 3) and np.abs(got).max() > 0
    _check("eigenmode", got, want, scale)
    K = sensitivity(2, fwd.density, fwd.l, fwd.mu, corr)
    for k in ("rho", "lambda", "mu"):
        assert K[k].shape == (fwd.block.ncells,) and np.isfinite(K[k]).all()
    assert np.array_equal(K["rho"], corr["uu"])
    fwd.reset_correlation()
    assert not fwd.block.get_correlation().any()
