"""The production kernels against the FP64 oracle where a field's device offsets pass 2^32 bytes and 2^31 elements.

The family tests compare every kernel object with the oracle on blocks of a few hundred cells; the full-size tests reach the
large addresses but check properties (time reversal, polynomial reproduction) that a stage reading the row 2^32 bytes below
the right one can satisfy.  Here the block is huge and the oracle tiny - the window method:

* the block is tall and thin, n = (3, 2, Z) cubes (2-D: (3, Z) squares), h = (0.4, 0.3, 0.5) (2-D: (0.4, 0.5)): the cells of a
  z-layer (a row) are one contiguous range of 6 cubes (3 squares), and the groups of 16 or 64 cubes of the interleaved layout
  straddle layers;
* sg_create zeroes the fields; random data goes into three consecutive layers per window (set_field_range), the library
  runs over the whole block, and W layers around the data come back (get_field_range) to be compared with the oracle on the
  mesh (3, 2, W) carrying the same data, material and density;
* a window side inside the block is an artificial boundary of the small mesh; the two agree as long as every field of every
  stage is exactly zero in the window's outermost layer on that side.  That is asserted ON THE ORACLE before anything is
  compared (_assert_reach).  One application of F or G couples a cell to its facet neighbours.  On hexahedra and
  quadrilaterals that is one layer per application and six per LF4 step: a margin of 7 zero layers, W = 17.  In a Kuhn cube
  the tetrahedra with a facet in the cube's floor are not the ones with a facet in its ceiling (triangles alike): three
  applications cross one layer, a step two (u1: one) - margin 4, W = 11.  tests/test_large_offsets_host.py holds the rule
  on the oracle;
* the window at the top of the block keeps the real boundary: its data is in the top three layers, only its lower side is
  artificial.  In the row with a z-high neighbour (zeroed ghost buffers attached: the GHOST = 1 kernels) the top layers take
  zero traces from outside, so the window there is interior and keeps a zero margin on top as well.

Marks.  The device offset of (cube c, class k, node b, component) is ((((c / gw) ncls + k) nd + b) ncomp + comp) gw + c % gw
(device_offset below).  first_cube_past() returns the first cube one of whose lines lies at or past a mark given in
elements; a window's middle data layer holds that cube, so its data lies on both sides of the mark.  Tier A blocks end a
window past S at 2^32 bytes; tier B blocks end a window past S at 2^31 elements and on the way pass S at 2^32 and 2^33 bytes
and U at 2^32 bytes (whatever the block reaches; marks whose windows would overlap an earlier one are dropped).

A row pins its six stage kernels by name, then checks at every window: apply_F and apply_G (the MODE 0 kernels); one whole
step with per-cell lambda, mu and density (u1, s1, UH = dt u1 + dt^3/24 utemp, SH = sh1); that nothing was written elsewhere
- the W layers below the lowest window, the first 192 cells and the cells whose device offsets are the windows' minus 2^32
bytes and minus 2^31 elements, where a truncated store would land, read exactly 0 in all four fields; and that the step
changed the data.  Rows with `extras` go on to the other kernels: the monitor with per-cell weights (data is zero outside the
windows, so the sample is the sum of the windows' quadratic forms), the correlation (tier A: two handles, tier B: the
handle with itself; exactly 0 on every other cell; matrix-pipe and LDS form), the pack kernel on the high side against the
traces gathered on the host, bitwise, a second step with a nodal source (one node twice), a DG_2 sponge in the data layers
(tier A; none, constant, general nodal and affine cells) and receivers inside window cells, and last a non-symmetric stress
uploaded into the top window: the whole-field mirror kernel and the SYM = 0 kernels.

Tolerances are the suite's own: FP64 tol_of() per application and 10 tol_of() for a step, FP32 2e-5 and 5e-5
(test_mfma_family_gpu.py); monitor and correlation 1e-11 of their scale against the host forms of the downloaded fields
(test_monitor_gpu.py, test_correlate_gpu.py); receivers 1e-14 (FP32 1e-6) against the host evaluation of the downloaded
fields (test_receivers_gpu.py) and the step's tolerance against the oracle's.

The step-end hooks and the device read-outs that came later - injectors, spectra, device transfers, frames, peak maps,
gradient, gauges - run on the same rows, plans and windows in tests/test_large_offsets_hooks_gpu.py, against the restatements
of their own modules; its docstring has the parts, the yardsticks and the memory of a row.

Not covered: the generic kernels (gw = 1: the stage kernels and the `flat` kernels of xfer, frame and grad) and the simplex
lane kernels, which choose_kernel_path never picks at these sizes, and 1-D blocks.  A row needs its four fields (and the
second handle's) on the device and skips, with both numbers, where less than
1.2 times that is free."""
import ctypes as C

import numpy as np
import pytest

from oracle import mesh as omesh
from oracle import refelem
from oracle.lf4 import OracleLF4
from tests import test_hex_family_gpu as hexfam
from tests import test_mfma_family_gpu as mfmafam
from tests import test_tile2d_family_gpu as tilefam
from tests.test_parity_gpu import tol_of
from tests.util import rel_err

pytestmark = pytest.mark.gpu

_Q = "quadrilateral"
H3 = (0.4, 0.3, 0.5)
DATA = 3                       # data layers per window
BYTES_2_32, BYTES_2_33, ELEMS_2_31 = 1 << 32, 1 << 33, 1 << 31
WCORR = np.array([0.7, -1.3, 2.1])


# ---- the layout and the marks (no device) --------------------------------------------------------------------------------
class Shape(object):
    """what fixes the layout of a row's block: dimension, cell, degree, number type, kernel family"""

    def __init__(self, dim, cell, P, dtype="f64", lane=False):
        self.dim, self.cell, self.P, self.dtype = dim, cell, P, dtype
        self.tensor = cell == _Q
        self.gw = 64 if lane else 16
        self.ncls = 1 if self.tensor else (2 if dim == 2 else 6)
        self.nd = (P + 1) ** dim if self.tensor else ((P + 1) * (P + 2) // 2 if dim == 2 else (P + 1) * (P + 2) * (P + 3) // 6)
        self.itemsize = 4 if dtype == "f32" else 8
        self.cubes_per_layer = 6 if dim == 3 else 3
        self.per = self.cubes_per_layer * self.ncls               # cells per layer
        self.h = H3 if dim == 3 else (H3[0], H3[2])
        self.margin = 7 if self.tensor else 4                      # zero layers per artificial side (module docstring)
        self.W = DATA + 2 * self.margin

    def ncomp(self, field):
        return self.dim * self.dim if field == "S" else self.dim

    def n(self, layers):
        return (3, 2, layers) if self.dim == 3 else (3, layers)

    def key(self):
        return (self.dim, self.cell, self.P)


def device_offset(sh, ncomp, cube, k, b, comp):
    return ((((cube // sh.gw) * sh.ncls + k) * sh.nd + b) * ncomp + comp) * sh.gw + cube % sh.gw


def first_cube_past(sh, ncomp, mark):
    """the first cube with a line at or past element `mark`: a cube's largest offset is that of its class ncls - 1, node
    nd - 1, component ncomp - 1"""
    group = sh.ncls * sh.nd * ncomp * sh.gw                        # elements of a group of gw cubes
    g = mark // group                                               # the group that holds element `mark`
    lane = max(0, mark - ((g + 1) * group - sh.gw))
    return g * sh.gw + lane


def mark_elements(sh, unit, value):
    return value // sh.itemsize if unit == "B" else value


def mark_layer(sh, field, unit, value):
    return first_cube_past(sh, sh.ncomp(field), mark_elements(sh, unit, value)) // sh.cubes_per_layer


# the marks a block may reach; of two whose windows would overlap (FP32: 2^31 elements are 2^33 bytes) the first stays
CANDIDATES = (("S", "B", BYTES_2_32), ("U", "B", BYTES_2_32), ("S", "el", ELEMS_2_31), ("S", "B", BYTES_2_33))
TIER_END = {"A": ("S", "B", BYTES_2_32), "B": ("S", "el", ELEMS_2_31)}


class Window(object):
    """W layers from layer k0; data in layers [k0 + d0, k0 + d0 + DATA); which sides are artificial"""

    def __init__(self, sh, k0, d0, lo, hi, what, mark=None):
        self.k0, self.d0, self.lo, self.hi, self.what, self.mark = k0, d0, lo, hi, what, mark
        self.cell0, self.ncells = k0 * sh.per, sh.W * sh.per
        self.data = slice(d0 * sh.per, (d0 + DATA) * sh.per)       # within the window
        self.kind = "top" if d0 + DATA == sh.W else "mid"


def plan(sh, tier, ghost=False):
    """(layers of the block, windows): one window at every mark the block reaches, the block ending a window past the tier's
    mark, plus the window at the top"""
    end = mark_layer(sh, *TIER_END[tier])
    wins = []
    for field, unit, value in CANDIDATES:
        lm = mark_layer(sh, field, unit, value)
        k0 = lm - 1 - sh.margin
        if lm > end or any(abs(k0 - w.k0) < sh.W for w in wins):
            continue
        wins.append(Window(sh, k0, sh.margin, True, True, "%s past %d %s" % (field, value, unit), (field, unit, value)))
    wins.sort(key=lambda w: w.k0)
    Z = wins[-1].k0 + 2 * sh.W
    if ghost:
        wins.append(Window(sh, Z - sh.W, sh.margin, True, True, "top, a neighbour above"))
    else:
        wins.append(Window(sh, Z - sh.W, sh.W - DATA, True, False, "top"))
    assert wins[0].k0 >= sh.W
    return Z, wins


def field_bytes(sh, layers):
    ncube = layers * sh.cubes_per_layer
    pad = (ncube + sh.gw - 1) // sh.gw * sh.gw
    return pad * sh.ncls * sh.nd * 2 * (sh.dim + sh.dim * sh.dim) * sh.itemsize


def offset_range(sh, ncomp, w):
    """smallest and largest device offset (elements) of the window's cells in a field of ncomp components"""
    c0, c1 = w.k0 * sh.cubes_per_layer, (w.k0 + sh.W) * sh.cubes_per_layer - 1
    return device_offset(sh, ncomp, c0 - c0 % sh.gw, 0, 0, 0), device_offset(sh, ncomp, c1 | (sh.gw - 1), sh.ncls - 1, sh.nd - 1, ncomp - 1)


def elsewhere(sh, wins):
    """cell ranges that must stay zero: W layers below the lowest window, the first 192 cells, and where the windows' lines
    minus 2^32 bytes and minus 2^31 elements lie - without the windows' own cells"""
    out = [(wins[0].cell0 - sh.W * sh.per, wins[0].cell0), (0, 192)]
    group_of = lambda ncomp: sh.ncls * sh.nd * ncomp * sh.gw
    for w in wins:
        for ncomp in (sh.ncomp("U"), sh.ncomp("S")):
            lo, hi = offset_range(sh, ncomp, w)
            for shift in (BYTES_2_32 // sh.itemsize, ELEMS_2_31):
                if hi - shift < 0:
                    continue
                g0, g1 = max(lo - shift, 0) // group_of(ncomp), (hi - shift) // group_of(ncomp)
                out.append((g0 * sh.gw * sh.ncls, (g1 + 1) * sh.gw * sh.ncls))
    cut = []
    for a, b in out:                                                # without the windows
        pieces = [(a, b)]
        for w in wins:
            pieces = [q for p in pieces for q in ((p[0], min(p[1], w.cell0)), (max(p[0], w.cell0 + w.ncells), p[1])) if q[0] < q[1]]
        cut += pieces
    return sorted(set(cut))


# ---- the rows --------------------------------------------------------------------------------------------------------------
class Row(object):
    def __init__(self, name, tier, shape, sym=True, env=None, ghost=False, extras=False, family="mfma"):
        self.name, self.tier, self.sh, self.sym, self.env, self.ghost, self.extras, self.family = \
            name, tier, shape, sym, env or {}, ghost, extras, family

    def names(self):
        sh = self.sh
        if self.family == "mfma":
            gq = self.env.get("SEIGEN_HIP_GQ")
            return mfmafam._stage_names(sh.dtype, sh.P, self.sym, mfmafam._fact(sh.dtype, sh.P, gq), ghost=int(self.ghost))
        if self.family == "tile":
            return tilefam._stage_names(sh.dtype, sh.P, sh.cell, self.sym)
        return hexfam._stage_names(sh.P, self.sym)


_T = lambda P, dtype="f64": Shape(3, "left", P, dtype)
ROWS = [
    Row("A-tets-P1", "A", _T(1)),
    Row("A-tets-P2", "A", _T(2)),
    Row("A-tets-P3", "A", _T(3)),
    Row("A-tets-P4", "A", _T(4), extras=True),
    Row("A-tets-P4-full", "A", _T(4), sym=False),
    Row("A-tets-P4-gq0", "A", _T(4), env={"SEIGEN_HIP_GQ": "0"}),
    Row("A-tets-P4-gstash0", "A", _T(4), env={"SEIGEN_HIP_GSTASH": "0"}),
    Row("A-tets-P4-ghost", "A", _T(4), ghost=True),
    Row("A-tets-P4-f32", "A", _T(4, "f32")),
    Row("A-hexm-DQ3", "A", Shape(3, _Q, 3), family="hexm"),
    Row("A-hexm-DQ4", "A", Shape(3, _Q, 4), family="hexm", extras=True),
    Row("A-hexlane-DQ2", "A", Shape(3, _Q, 2, lane=True), family="hex_lane"),
    Row("A-tri-P4", "A", Shape(2, "left", 4), family="tile", extras=True),
    Row("A-tri-P4-f32", "A", Shape(2, "left", 4, "f32"), family="tile"),
    Row("A-quad-DQ4", "A", Shape(2, _Q, 4), family="tile"),
    Row("B-tets-P4", "B", _T(4), extras=True),
    Row("B-tets-P4-f32", "B", _T(4, "f32")),
    Row("B-hexm-DQ4", "B", Shape(3, _Q, 4), family="hexm"),
]
_SWITCHES = ("SEIGEN_HIP_PATH", "SEIGEN_HIP_SYM", "SEIGEN_HIP_GQ", "SEIGEN_HIP_GSTASH", "SEIGEN_HIP_GRID_BLOCKS",
             "SEIGEN_HIP_ORDER_CHUNK", "SEIGEN_HIP_SPONGE_AFFINE", "SEIGEN_HIP_SOURCE_LAUNCH", "SEIGEN_HIP_GRAPH",
             "SEIGEN_HIP_TILE_GRID", "SEIGEN_HIP_XCORR")


# ---- the oracle of a window, built once per (cell type, degree, W) -----------------------------------------------------
_ORACLES = {}


class WindowOracle(object):
    def __init__(self, sh):
        L = tuple(sh.h[a] * k for a, k in enumerate(sh.n(sh.W)))
        self.m = omesh.structured(sh.dim, sh.n(sh.W), L, "left", quadrilateral=sh.tensor)
        self.orc = OracleLF4(self.m, sh.P)
        kind = "tensor" if sh.tensor else "simplex"
        xq, wq = refelem.el_quadrature(sh.dim, 2 * sh.P, kind)
        phi, _ = refelem.el_tabulate(sh.dim, sh.P, xq, kind)
        self.mass = np.einsum('q,qa,qb->ab', wq, phi, phi)
        self.detj = np.abs(self.m.detJ)
        self.sponges = {}

    def lend(self):
        orc = self.orc
        orc.E.absorb, orc.source, orc.density, orc.density_physical = None, None, 1.0, False
        return orc

    def sponge(self, sh, w):
        """(sigma of the window [cells, nq], the oracle's matrix): DG_2, nonzero in the data layers only - by cell % 4 none,
        one value, general nodal, affine with a gradient of its own"""
        if w.kind not in self.sponges:
            rng = np.random.default_rng(77 + (w.kind == "top"))
            Xq = self.m.node_coords(2)
            sigma = np.zeros(Xq.shape[:2])
            cells = np.arange(self.m.ncells)[w.data]
            kind = cells % 4
            c, g, a = cells[kind == 1], cells[kind == 2], cells[kind == 3]
            sigma[c] = rng.uniform(2.0, 30.0, size=(len(c), 1))
            sigma[g] = rng.uniform(0.0, 30.0, size=(len(g), Xq.shape[1]))
            grad = rng.uniform(-20.0, 20.0, size=(len(a), 1, sh.dim))
            sigma[a] = rng.uniform(5.0, 30.0, size=(len(a), 1)) + (grad * (Xq[a] - Xq[a][:, :1])).sum(axis=-1)
            self.orc.E.set_absorption(sigma, 2)
            self.sponges[w.kind] = (sigma, self.orc.E.absorb)
            self.orc.E.absorb = None
        return self.sponges[w.kind]


def window_oracle(sh):
    if sh.key() not in _ORACLES:
        _ORACLES[sh.key()] = WindowOracle(sh)
    return _ORACLES[sh.key()]


def _outer_layers(sh, w):
    """the cells of the window's outermost layer on each artificial side"""
    return ([slice(0, sh.per)] if w.lo else []) + ([slice((sh.W - 1) * sh.per, sh.W * sh.per)] if w.hi else [])


def _assert_reach(sh, w, fields):
    """the condition of the window method: exactly zero in the outermost layer of every artificial side"""
    for name, a in fields.items():
        for sl in _outer_layers(sh, w):
            assert not a[sl].any(), "the oracle's %s reaches the window's outermost layer (%s)" % (name, w.what)


def _figure(row, w, what, got, want):
    e = rel_err(got, want)
    print("ERR large %s [%s] %s %.3e" % (row.name, w.what, what, e))
    return e


def _sym(a):
    return 0.5 * (a + np.swapaxes(a, -1, -2))


# ---- the block --------------------------------------------------------------------------------------------------------------
def _make_block(row, Z, ghost_bufs):
    from seigen_amd.backend import HipBlock
    sh = row.sh
    blk = HipBlock(sh.dim, sh.P, sh.n(Z), sh.h, (0.0,) * sh.dim, sh.cell, nbr_mask=(1 << 5) if row.ghost else 0, dtype=sh.dtype)
    if row.ghost:
        import torch
        for field in range(4):
            ghost_bufs.append(torch.zeros(blk.halo_bytes(field, 5), dtype=torch.uint8, device="cuda"))
            blk.halo_attach(field, 5, ghost_bufs[-1].data_ptr())
    return blk


def _get(blk, field, w):
    return blk.get_field_range(field, w.cell0, w.ncells)


def _assert_zero_elsewhere(blk, ranges, fields):
    for a, b in ranges:
        for f in fields:
            assert not blk.get_field_range(f, a, b - a).any(), "field %d was written in cells [%d, %d)" % (f, a, b)


def _window_state(sh, w, rng, sym, nc):
    """random data in the data layers, material and density on the whole window"""
    u = np.zeros((nc, sh.nd, sh.dim))
    T = np.zeros((nc, sh.nd, sh.dim, sh.dim))
    u[w.data] = rng.uniform(-1, 1, u[w.data].shape)
    t = rng.uniform(-1, 1, T[w.data].shape)
    T[w.data] = _sym(t) if sym else t
    return dict(u=u, T=T, lam=rng.uniform(0.4, 0.8, nc), mu=rng.uniform(0.2, 0.4, nc), rho=rng.uniform(0.9, 1.1, nc))


def _forms(wo, fa, fb):
    """|det J| (Buu, Bss, Btt) per cell of a's fields against b's and the same of the absolute values
    (test_correlate_gpu.host_forms on the window mesh)"""
    (ua, sa), (ub, sb) = fa, fb
    ta, tb = np.einsum('cnii->cn', sa)[..., None], np.einsum('cnii->cn', sb)[..., None]
    sa, sb = sa.reshape(sa.shape[0], sa.shape[1], -1), sb.reshape(sb.shape[0], sb.shape[1], -1)
    form = lambda x, y, m: np.sum(x * np.matmul(m, y), axis=(1, 2))
    M, aM = wo.mass, np.abs(wo.mass)
    B = np.stack([form(ua, ub, M), form(sa, sb, M), form(ta, tb, M)], axis=-1)
    S = np.stack([form(np.abs(ua), np.abs(ub), aM), form(np.abs(sa), np.abs(sb), aM), form(np.abs(ta), np.abs(tb), aM)], axis=-1)
    return wo.detj[:, None] * B, wo.detj[:, None] * S


def _need_or_skip(row, Z, handles):
    import torch
    need = handles * field_bytes(row.sh, Z)
    free = torch.cuda.mem_get_info()[0]
    if free < 1.2 * need:
        pytest.skip("%s needs %.1f GB of fields, %.1f GB are free" % (row.name, need / 1e9, free / 1e9))


# ---- one row --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_windows_at_the_marks(gpu, monkeypatch, row):
    from seigen_amd import _lib
    for var in _SWITCHES:
        monkeypatch.delenv(var, raising=False)
    for var, val in row.env.items():
        monkeypatch.setenv(var, val)
    sh = row.sh
    Z, wins = plan(sh, row.tier, row.ghost)
    _need_or_skip(row, Z, 2 if (row.extras and row.tier == "A") else 1)
    wo = window_oracle(sh)
    orc = wo.lend()
    nc = wo.m.ncells
    assert nc == sh.W * sh.per
    tol1, tol3 = (tol_of(sh.P, sh.cell), 10 * tol_of(sh.P, sh.cell)) if sh.dtype == "f64" else (2e-5, 5e-5)
    rng = np.random.default_rng(sum(map(ord, row.name)))
    state = [_window_state(sh, w, rng, row.sym, nc) for w in wins]
    zero_ranges = elsewhere(sh, wins)
    # not vacuous: every mark window's middle data layer holds the first cube past its mark, so it has lines on both sides
    assert [w.mark is None for w in wins] == [False] * (len(wins) - 1) + [True]
    for w in wins[:-1]:
        field, unit, value = w.mark
        ncomp, mark = sh.ncomp(field), mark_elements(sh, unit, value)
        cube = first_cube_past(sh, ncomp, mark)
        assert cube // sh.cubes_per_layer == w.k0 + w.d0 + 1
        assert device_offset(sh, ncomp, cube, sh.ncls - 1, sh.nd - 1, ncomp - 1) >= mark
        assert cube == 0 or device_offset(sh, ncomp, cube - 1, sh.ncls - 1, sh.nd - 1, ncomp - 1) < mark
        lo, hi = offset_range(sh, ncomp, w)
        assert lo < mark <= hi

    ghost_bufs, blks = [], []
    try:
        blk = _make_block(row, Z, ghost_bufs)
        blks.append(blk)
        assert blk.ncells == Z * sh.per and blk.nd == sh.nd
        dt = 0.04 * min(sh.h) / sh.P ** 2
        lam, mu, rho = np.full(blk.ncells, 0.5), np.full(blk.ncells, 0.25), np.ones(blk.ncells)
        for w, st in zip(wins, state):
            cells = slice(w.cell0, w.cell0 + w.ncells)
            lam[cells], mu[cells], rho[cells] = st["lam"], st["mu"], st["rho"]
        blk.set_params(1.0, dt, lam, mu)
        blk.set_density(rho, physical=False)

        def upload(b, key_u="u", key_T="T"):
            for w, st in zip(wins, state):
                b.set_field_range(_lib.FIELD_U, w.cell0, st[key_u])
                b.set_field_range(_lib.FIELD_S, w.cell0, st[key_T])

        upload(blk)
        assert blk.is_sym() == row.sym
        names = [blk.stage_kernel_name(st) for st in range(6)]
        assert names == row.names(), names

        # 1. one application of each operator (the MODE 0 kernels)
        blk.apply_F(_lib.FIELD_S, _lib.FIELD_U, _lib.FIELD_UH)
        blk.apply_G(_lib.FIELD_U, _lib.FIELD_SH)
        for w, st in zip(wins, state):
            wantF, wantG = orc.E.apply_F(st["T"], st["u"]), orc.E.apply_G(st["u"], st["lam"], st["mu"])
            _assert_reach(sh, w, {"F": wantF, "G": wantG})
            assert _figure(row, w, "F", _get(blk, _lib.FIELD_UH, w), wantF) < tol1
            assert _figure(row, w, "G", _get(blk, _lib.FIELD_SH, w), wantG) < tol1
        _assert_zero_elsewhere(blk, zero_ranges, (_lib.FIELD_UH, _lib.FIELD_SH))

        # 2. one whole step (a block with neighbours has no sg_step of its own: its stages are driven from the host, the
        # ghost buffers staying zero)
        if row.ghost:
            for stage in range(6):
                blk.run_stage(stage)
            blk.end_step()
        else:
            blk.step(1)
        after = []
        for w, st in zip(wins, state):
            orc = wo.lend()
            orc.dt, orc.l, orc.mu, orc.density = dt, st["lam"], st["mu"], st["rho"]
            orc.u0, orc.s0 = st["u"], st["T"]
            orc.step(dt)
            _assert_reach(sh, w, dict(orc.last, u1=orc.u1, s1=orc.s1))
            got = {f: _get(blk, f, w) for f in range(4)}
            assert _figure(row, w, "step u", got[_lib.FIELD_U], orc.u1) < tol3
            assert _figure(row, w, "step s", got[_lib.FIELD_S], orc.s1) < tol3
            assert _figure(row, w, "step uh", got[_lib.FIELD_UH], dt * orc.u1 + dt ** 3 / 24.0 * orc.last["utemp"]) < tol3
            assert _figure(row, w, "step sh", got[_lib.FIELD_SH], orc.last["sh1"]) < tol3
            # 4. not vacuous
            assert rel_err(orc.u1, st["u"]) > 1e-4 and rel_err(orc.s1, st["T"]) > 1e-4
            assert rel_err(got[_lib.FIELD_U], st["u"]) > 1e-4 and rel_err(got[_lib.FIELD_S], st["T"]) > 1e-4
            after.append((got[_lib.FIELD_U], got[_lib.FIELD_S]))
        # 3. nothing written elsewhere
        _assert_zero_elsewhere(blk, zero_ranges, range(4))

        if row.extras:
            _monitor(row, blk, wo, wins, after, rng)
            _correlation(row, blk, blks, wo, wins, state, after, rng, Z, upload, monkeypatch)
            _pack(row, blk, Z)
            _source_sponge_receivers(row, blk, wo, wins, state, rng, dt, tol3, upload, zero_ranges)
            _storage_change(row, blk, wo, wins, state, rng, tol1)
    finally:
        for b in blks:
            b.close()
        del ghost_bufs[:]


# ---- the other kernels ------------------------------------------------------------------------------------------------------
def _monitor(row, blk, wo, wins, after, rng):
    """sg_measure with per-cell weights: data is zero outside the windows"""
    from tests.test_monitor_gpu import physical_weights
    sh = row.sh
    w3 = physical_weights(sh.dim, *(rng.uniform(0.5, 2.0, blk.ncells) for _ in range(3)))
    want = np.zeros(5)
    for w, f in zip(wins, after):
        B, _ = _forms(wo, f, f)
        ww = w3[w.cell0:w.cell0 + w.ncells]
        want += [B[:, 0].sum(), B[:, 1].sum(), B[:, 2].sum(), (ww[:, 0] * B[:, 0]).sum(), (ww[:, 1] * B[:, 1] + ww[:, 2] * B[:, 2]).sum()]
    got = blk.measure(w3)
    print("ERR large %s monitor" % row.name, got, np.abs(got - want) / np.abs(want))
    assert np.isfinite(got).all() and np.all(want[:3] > 0)
    assert np.all(np.abs(got - want) <= 1e-11 * np.abs(want)), (got, want)


def _correlation(row, blk, blks, wo, wins, state, after, rng, Z, upload, monkeypatch):
    """tier A: two handles with different window data; tier B: the handle with itself.  Against the host forms on the window
    cells, exactly 0 on every other cell; on the matrix-pipe rows again in the LDS form"""
    from seigen_amd import _lib
    sh = row.sh
    other = blk
    theirs = after
    if row.tier == "A":
        other = _make_block(row, Z, [])
        blks.append(other)
        for st in state:
            st["u2"], st["T2"] = rng.uniform(-1, 1, st["u"].shape), _sym(rng.uniform(-1, 1, st["T"].shape))
        upload(other, "u2", "T2")
        theirs = [(_get(other, _lib.FIELD_U, w), _get(other, _lib.FIELD_S, w)) for w in wins]
    inside = np.zeros(blk.ncells, dtype=bool)
    for w in wins:
        inside[w.cell0:w.cell0 + w.ncells] = True
    for form in (None, "lds"):
        if form:
            blk.reset_correlation(release=True)
            monkeypatch.setenv("SEIGEN_HIP_XCORR", form)
        blk.correlate(other, WCORR)
        got = blk.get_correlation()
        assert not got[~inside].any(), "the correlation is not 0 outside the windows (%s)" % (form or "default")
        for w, fa, fb in zip(wins, after, theirs):
            B, S = _forms(wo, fa, fb)
            want, scale = B * WCORR, S * np.abs(WCORR)
            g = got[w.cell0:w.cell0 + w.ncells]
            err = np.abs(g - want) / np.maximum(scale, 1e-300)
            print("ERR large %s [%s] correlation %s" % (row.name, w.what, form or "default"), err[scale > 0].max())
            assert np.all(scale.max(axis=0) > 0) and np.all(np.abs(g - want) <= 1e-11 * scale)
    monkeypatch.delenv("SEIGEN_HIP_XCORR", raising=False)
    if other is not blk:
        other.close()


def _side_tables(sh):
    """(class, facet, ordinal) of the facets of a cube on its high side along the last axis, and the facet node lists - the
    library's device-free tables"""
    from seigen_amd import _lib
    lib = _lib.load()
    kind = 1 if sh.tensor else 0
    nfaces = 2 * sh.dim if sh.tensor else sh.dim + 1
    nf = (sh.P + 1) ** (sh.dim - 1) if sh.tensor else ((sh.P + 1) if sh.dim == 2 else (sh.P + 1) * (sh.P + 2) // 2)
    fn = np.empty((nfaces, nf))
    assert lib.sg_reference_operator_cell(kind, sh.dim, sh.P, 4, 0, fn.ctypes.data, fn.nbytes) == fn.size
    nb = np.zeros((sh.ncls, nfaces, 5), dtype=np.int32)
    nbn = np.zeros((sh.ncls, nfaces, nf), dtype=np.int32)
    cn, jinv, h = np.zeros((sh.ncls, nfaces, 3)), np.zeros((sh.ncls, 3, 3)), np.array(sh.h + (1.0,) * (3 - sh.dim))
    diag = 2 if sh.tensor else 0
    assert lib.sg_mesh_tables(sh.dim, sh.P, diag, h.ctypes.data, nb.ctypes.data, nbn.ctypes.data, cn.ctypes.data, jinv.ctypes.data) == 0
    facets = sorted((int(nb[c, f, 4]), c, f) for c in range(sh.ncls) for f in range(nfaces)
                    if nb[c, f, 0] == sh.dim - 1 and nb[c, f, 1] > 0)
    assert [o for o, _, _ in facets] == list(range(len(facets)))
    return facets, fn.astype(np.int64)


def _pack(row, blk, Z):
    """sg_halo_pack of S and U on the high side of the last axis against the traces of the top layer gathered on the host:
    [cube][ordinal][facet node][component], the column T.n of a stress - bitwise"""
    import torch
    from seigen_amd import _lib
    sh = row.sh
    side, axis = 2 * (sh.dim - 1) + 1, sh.dim - 1
    facets, fn = _side_tables(sh)
    n2 = sh.cubes_per_layer
    for field in (_lib.FIELD_S, _lib.FIELD_U):
        buf = torch.zeros(blk.halo_bytes(field, side), dtype=torch.uint8, device="cuda")
        blk.halo_pack(field, side, buf.data_ptr())
        blk.sync()
        got = buf.cpu().numpy().view(np.float32 if sh.dtype == "f32" else np.float64).astype(np.float64)
        got = got.reshape(n2, len(facets), fn.shape[1], sh.dim)
        top = blk.get_field_range(field, (Z - 1) * sh.per, sh.per)
        want = np.empty_like(got)
        for o, c, f in facets:
            cells = np.arange(n2) * sh.ncls + c
            tr = top[cells][:, fn[f]]
            want[:, o] = tr if field == _lib.FIELD_U else tr[..., axis]
        assert np.abs(want).max() > 0
        assert np.array_equal(got, want), "packed traces of field %d differ from the top layer's" % field


def _source_sponge_receivers(row, blk, wo, wins, state, rng, dt, tol3, upload, zero_ranges):
    """a second step from the same data with a nodal source in the data layers (one node twice), a DG_2 sponge there (tier
    A) and receivers inside window cells"""
    from seigen_amd import _lib
    from seigen_amd.backend import locate_points
    sh = row.sh
    lib = _lib.load()
    d = sh.dim
    upload(blk)
    # source: window-local nodes of the data layers
    nodes_w, glob = [], []
    for w in wins:
        cells = rng.integers(w.data.start, w.data.stop, size=6)
        nd_ = cells * sh.nd + rng.integers(0, sh.nd, size=6)
        nd_ = np.concatenate([nd_, nd_[:1]])
        nodes_w.append(nd_)
        glob.append(nd_ + w.cell0 * sh.nd)
    vals = [_sym(rng.uniform(-1, 1, (len(nw), d, d))) for nw in nodes_w]
    blk.set_source(np.concatenate(glob), np.concatenate(vals)[None])
    sponge = row.tier == "A"
    if sponge:
        sig0 = wo.sponge(sh, wins[0])[0]
        sigma = np.zeros((blk.ncells, sig0.shape[1]))
        for w in wins:
            sigma[w.cell0:w.cell0 + w.ncells] = wo.sponge(sh, w)[0]
        blk.set_absorption(sigma, 2)
    # receivers: points inside cubes of the data layers, away from the grid lines
    pts = []
    for w in wins:
        for k in range(DATA):
            for i in range(2):
                frac = rng.uniform(0.15, 0.85, size=d)
                cube = [rng.integers(0, 3)] + ([rng.integers(0, 2)] if d == 3 else []) + [w.k0 + w.d0 + k]
                pts.append([(cube[a] + frac[a]) * sh.h[a] for a in range(d)])
    pts = np.array(pts)
    cfg = _lib.SgConfig()
    cfg.dim, cfg.degree, cfg.diagonal = d, sh.P, 2 if sh.tensor else 0
    for a in range(3):
        cfg.n[a] = blk.ncells // sh.per if a == d - 1 else ((3, 2)[a] if a < d - 1 else 1)
        cfg.h[a] = sh.h[a] if a < d else 1.0
    cell, xi = locate_points(cfg, pts)
    phi = np.empty((len(pts), sh.nd))
    _lib.check(lib.sg_tabulate_cell(1 if sh.tensor else 0, d, sh.P, len(pts), np.ascontiguousarray(xi).ctypes.data, phi.ctypes.data))
    owned = blk.set_receivers(pts, 3, 1, 1)
    assert owned.all()
    assert blk.is_sym()
    blk.step(1)
    rec = blk.get_receivers()
    assert rec.shape == (1, len(pts), d + d * d)
    for iw, (w, st) in enumerate(zip(wins, state)):
        orc = wo.lend()
        orc.dt, orc.l, orc.mu, orc.density = dt, st["lam"], st["mu"], st["rho"]
        orc.u0, orc.s0 = st["u"], st["T"]
        if sponge:
            orc.E.absorb = wo.sponge(sh, w)[1]
        S = np.zeros((wo.m.ncells * sh.nd, d, d))
        np.add.at(S, nodes_w[iw], vals[iw])
        orc.source = lambda t, S=S: S.reshape(wo.m.ncells, sh.nd, d, d)
        orc.step(dt)
        _assert_reach(sh, w, dict(orc.last, u1=orc.u1, s1=orc.s1))
        gu, gs = _get(blk, _lib.FIELD_U, w), _get(blk, _lib.FIELD_S, w)
        assert _figure(row, w, "source step u", gu, orc.u1) < tol3
        assert _figure(row, w, "source step s", gs, orc.s1) < tol3
        assert _figure(row, w, "source step sh", _get(blk, _lib.FIELD_SH, w), orc.last["sh1"]) < tol3
        mine = [k for k in range(len(pts)) if w.cell0 <= cell[k] < w.cell0 + w.ncells]
        assert len(mine) == 2 * DATA
        sample = lambda u, s: np.array([np.concatenate([phi[k] @ u[cell[k] - w.cell0],
                                                         np.tensordot(phi[k], s[cell[k] - w.cell0], axes=(0, 0)).reshape(-1)]) for k in mine])
        own, ref = sample(gu, gs), sample(orc.u1, orc.s1)
        scale = np.abs(own).max()
        e_own, e_ref = np.abs(rec[0, mine] - own).max() / scale, np.abs(rec[0, mine] - ref).max() / np.abs(ref).max()
        print("ERR large %s [%s] receivers %.3e (own fields) %.3e (oracle)" % (row.name, w.what, e_own, e_ref))
        assert scale > 0 and e_own <= (1e-6 if sh.dtype == "f32" else 1e-14) and e_ref < tol3
        orc.E.absorb, orc.source = None, None
    _assert_zero_elsewhere(blk, zero_ranges, range(4))
    blk.set_receivers(np.zeros((0, d)))
    blk.set_source([], None)
    blk.set_absorption(None, 0)


def _storage_change(row, blk, wo, wins, state, rng, tol1):
    """a non-symmetric stress uploaded into the top window: the handle leaves the symmetric storage (the whole-field mirror
    kernel fills the lower lines of every window), then F runs as the SYM = 0 kernel"""
    from seigen_amd import _lib
    orc = wo.lend()
    for w, st in zip(wins, state):
        blk.set_field_range(_lib.FIELD_U, w.cell0, st["u"])
        blk.set_field_range(_lib.FIELD_S, w.cell0, st["T"])
    assert blk.is_sym()
    top = wins[-1]
    T = np.zeros_like(state[-1]["T"])
    T[top.data] = rng.uniform(-1, 1, T[top.data].shape)
    assert np.abs(T - np.swapaxes(T, -1, -2)).max() > 0.1
    blk.set_field_range(_lib.FIELD_S, top.cell0, T)
    assert not blk.is_sym()
    assert blk.stage_kernel_name(0) != row.names()[0]          # the SYM = 0 object
    blk.apply_F(_lib.FIELD_S, _lib.FIELD_U, _lib.FIELD_UH)
    for w, st in zip(wins, state):
        Tw = T if w is top else st["T"]
        assert rel_err(_get(blk, _lib.FIELD_S, w), Tw) < (1e-6 if row.sh.dtype == "f32" else 1e-15)
        assert _figure(row, w, "F after the storage change", _get(blk, _lib.FIELD_UH, w), orc.E.apply_F(Tw, st["u"])) < tol1
