"""The gradient on the GPU (include/seigen_hip.h sg_get_gradient_dev / sg_get_gradient; seigen_amd/csrc/kernels_grad.hip): the
broken gradient of a velocity field at the nodes, its divergence, curl and symmetric part.

ROWS: the nine of tests/gradient_loop.py (every family, f32, padding lanes in the first and last group) and lane-1d-P2,
hexm-DQ4 (125 nodes: the values of an item go through LDS in twelve slices) and lane-2d-P2-wide (two groups of 64, the second
one lane wide).  Fields are random of order one, the blocks have unequal h.

1 against the restatement tests/grad_cases.py grad_reference over the tables the library exports (tests/test_grad_host.py holds it
  against analytic gradients): |device - reference| <= 4 (nd + dim) 2^-53 A elementwise, A = sum_r |J_rj| sum_b |C_r[a][b]| |u[b][i]|.
  Both sides are sums of at most nd + dim terms over the same tables - fma chains on the device, numpy's sums in the reference -
  and each lies within gamma_(nd + dim) A of the exact sum; FP32 blocks convert exactly first.  Both fields, U and UH.
2 kinds 1 to 3 bitwise from the device's own kind 0 by the stated combinations in numpy; 3 the float buffer bitwise
  device_double.astype(float32); 5 ranges into a buffer pre-filled with a sentinel: test_against_the_restatement does 1, 2, 3, 5.
4 bitwise invariance: layout (gw 16, 64, 1), the caller's stream, SEIGEN_HIP_GRID_BLOCKS, a range against the full call.
6 nothing else moves; 7 refusals; 8 the solver class.

Measured on an MI355X, the largest |device - reference| / (2^-53 A) of test 1 over both fields, against the bound's factor
4 (nd + dim): mfma-P4-sym 3.64 of 152, mfma-P3-sym 3.54 of 92, tile-tri-P3 3.34 of 48, tile-quad-P2 2.10 of 44, hexm-DQ3 4.14 of
268, lane-2d-P2 1.68 of 32, generic-2d-P2 1.81 of 32, mfma-P3-f32 2.64 of 92, tile-tri-P3-f32 2.98 of 48, lane-1d-P2 1.59 of 16,
hexm-DQ4 4.30 of 512, lane-2d-P2-wide 2.16 of 32.

Seeded faults in a scratch build of kernels_grad.hip, run through test_against_the_restatement on the twelve rows (MI355X):
  J transposed (Jk[j * 3 + r])     fails the three 3-D simplex rows, whose classes have a non-symmetric J (mfma-P4-sym: ratio 2.4e17
                                   of 152, mfma-P3-sym 9.1e16, mfma-P3-f32 1.1e17); passes the nine others with their figures
                                   unchanged: the J of the triangles, of the interval and of the tensor-product cells is diagonal,
                                   its transpose the same table (tests/test_grad_host.py sees a transposed J in the restatement
                                   wherever J is not symmetric).
  the class ignored (Jtab + 0)     fails the eight rows with more than one class, all simplices of dim > 1 (ratios 1.8e16 in 2-D,
                                   1e17 .. 3e17 in 3-D); passes lane-1d-P2 and the three tensor-product rows, which have one.
  one slice dropped (the last      fails hexm-DQ3 (two slices) and hexm-DQ4 (twelve), the rows whose plan has more than one
  unit of every item skipped)      slice: their last nodes keep what the buffer held; passes the ten others.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from seigen_amd import _lib  # noqa: E402
from seigen_amd.backend import HipBlock  # noqa: E402
from tests import grad_cases as gc  # noqa: E402

SWITCHES = ("SEIGEN_HIP_PATH", "SEIGEN_HIP_GRAPH", "SEIGEN_HIP_SPONGE_AFFINE", "SEIGEN_HIP_SYM", "SEIGEN_HIP_SOURCE_LAUNCH",
            "SEIGEN_HIP_XCORR", "SEIGEN_HIP_OVERLAP", "SEIGEN_HIP_PLAIN_COPY", "SEIGEN_HIP_GRID_BLOCKS")
ROWS = gc.rows()
ROW = {r[0]: r for r in ROWS}
IDS = [r[0] for r in ROWS]
EPS = 2.0 ** -53
SENTINEL = -7.25
FIELDS = (_lib.FIELD_U, _lib.FIELD_S, _lib.FIELD_UH, _lib.FIELD_SH)
_CASES = {}


def _torch():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no GPU")
    return torch


def _env(monkeypatch, row, graph=None, path="row"):
    for var in SWITCHES:
        monkeypatch.delenv(var, raising=False)
    path = row[6] if path == "row" else path
    if path:
        monkeypatch.setenv("SEIGEN_HIP_PATH", path)
    if graph is not None:
        monkeypatch.setenv("SEIGEN_HIP_GRAPH", graph)


def _h(row):
    """unequal cell sizes"""
    dim, n = row[1], row[3]
    return [(0.5, 0.25, 0.2)[a] * 3.0 / n[a] for a in range(dim)]


def _block(row, stream=None):
    name, dim, degree, n, diagonal, dtype, path = row
    blk = HipBlock(dim, degree, n, _h(row), [0.0] * dim, diagonal, stream=stream, dtype=dtype)
    blk.set_params(1.0, 0.1 * min(_h(row)) / degree ** 2, 0.5, 0.25)
    return blk


def _case(row):
    """the tables of the row's block, two random velocity fields of order one (exact in float for an f32 row), the
    restatement's gradient of each and the scale of its rounding - computed once per row"""
    key = row[:6]
    if key not in _CASES:
        name, dim, degree, n, diagonal, dtype = key
        t = gc.tables_of(gc.block_cfg(dim, degree, n, diagonal, h=_h(row)))
        ncells = int(np.prod(n)) * t["ncls"]
        rng = np.random.default_rng(1000 + len(_CASES))
        u = {}
        for f in (_lib.FIELD_U, _lib.FIELD_UH):
            x = rng.uniform(-1, 1, (ncells, t["nd"], dim))
            u[f] = x.astype(np.float32).astype(np.float64) if dtype == "f32" else x
        _CASES[key] = dict(t=t, u=u, G={f: gc.grad_reference(t, x) for f, x in u.items()},
                           A={f: gc.grad_scale(t, x) for f, x in u.items()})
        for name in ("u", "G", "A"):                      # shared among the tests: left unchanged
            for x in _CASES[key][name].values():
                x.setflags(write=False)
    return _CASES[key]


def _within_bound(got, case, f, cells=slice(None)):
    """largest |got - reference| / (2^-53 A) and the bound's factor 4 (nd + dim)"""
    t = case["t"]
    ratio = np.abs(got - case["G"][f][cells]) / (EPS * case["A"][f][cells])
    return float(ratio.max()), 4 * (t["nd"] + t["dim"])


def _ranges(blk, gw):
    """(cell0, ncells): start and end inside a cube's classes; inside a group; across the first group boundary where there is one"""
    ncls, n = blk.ncls, blk.ncells
    r = [(1, min(n - 2, 2 * ncls + 1)), (n - ncls - 1, ncls + 1), (n // 2, 1)]
    if gw > 1 and n > gw * ncls + ncls + 2:
        r.append((gw * ncls - ncls - 1, 2 * ncls + 3))
    return [(c0, k) for c0, k in r if c0 >= 0 and k > 0 and c0 + k <= n]


def _counts(blk):
    c = blk.counters()
    return c["launches"], c["steps"], c["halo_pack_launches"], c["halo_bytes_packed"]


def _sentinel(torch, shape, dtype):
    """a tensor of `shape` in the middle of an allocation filled with the sentinel: (tensor, whole allocation)"""
    n = int(np.prod(shape))
    whole = torch.full((3 * n,), SENTINEL, dtype=dtype, device="cuda")
    return whole[n:2 * n].view(shape), whole


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_against_the_restatement(gpu, monkeypatch, row):
    """1, 2, 3 and 5 of the module's docstring on one block of the row"""
    torch = _torch()
    _env(monkeypatch, row)
    case = _case(row)
    t = case["t"]
    dim = t["dim"]
    blk = _block(row)
    try:
        assert (blk.nd, blk.ncls) == (t["nd"], t["ncls"])
        for f in (_lib.FIELD_U, _lib.FIELD_UH):
            blk.set_field(f, case["u"][f])
            assert np.array_equal(blk.get_field(f), case["u"][f])          # the block holds these values exactly
        for f in (_lib.FIELD_U, _lib.FIELD_UH):
            # ---- 1
            g = blk.get_gradient_dev(f, 0)
            assert g.dtype == torch.float64 and tuple(g.shape) == (blk.ncells, blk.nd, dim, dim)
            G = g.cpu().numpy()
            ratio, factor = _within_bound(G, case, f)
            print("%s field %d: largest |device - reference| / (2^-53 A) = %.2f, bound %d" % (row[0], f, ratio, factor))
            assert ratio <= factor
            assert np.array_equal(blk.get_gradient(f, "grad"), G)          # the host read-out is the same launch
            # ---- 2 and 3
            for kind in (0, 1, 2, 3):
                if kind == 2 and dim == 1:
                    continue
                want = gc.kind_of(G, kind)
                got = blk.get_gradient_dev(f, kind)
                assert tuple(got.shape) == want.shape == blk.gradient_shape(kind)
                assert np.array_equal(got.cpu().numpy(), want), (f, kind)
                got32 = blk.get_gradient_dev(f, kind, dtype=torch.float32)
                assert got32.dtype == torch.float32 and np.array_equal(got32.cpu().numpy(), want.astype(np.float32)), (f, kind, "float")
                # ---- 5: exactly the range is written
                for c0, k in _ranges(blk, gc.row_gw(row)):
                    for tdt in (torch.float64, torch.float32):
                        out, whole = _sentinel(torch, blk.gradient_shape(kind, k), tdt)
                        assert blk.get_gradient_dev(f, kind, out=out, cell0=c0, ncells=k) is out
                        w = whole.cpu().numpy()
                        n = out.numel()
                        assert (w[:n] == SENTINEL).all() and (w[2 * n:] == SENTINEL).all(), (f, kind, c0, k)
                        assert np.array_equal(w[n:2 * n].reshape(want[c0:c0 + k].shape), want[c0:c0 + k].astype(w.dtype)), (f, kind, c0, k)
                if kind == 0:
                    assert np.array_equal(blk.get_gradient(f, 0, cell0=1, ncells=blk.ncells - 1), G[1:])
    finally:
        blk.close()


# ---- 4. bitwise invariance ------------------------------------------------------------------------------------------------

def test_bitwise_invariance(gpu, monkeypatch):
    """the 2-D P2 triangles of one mesh on the tile family (gw = 16), the lane family (64) and the generic one (1); on a
    caller's non-blocking stream; with SEIGEN_HIP_GRID_BLOCKS=8; a cell range against the same cells of the full call"""
    torch = _torch()
    row = ("inv-2d-P2", 2, 2, (5, 3), "left", "f64", None)
    case = _case(row)
    f = _lib.FIELD_U
    seen = {}
    for label, path, grid, own_stream in (("tile", None, None, False), ("lane", "lane", None, False), ("generic", "generic", None, False),
                                          ("tile-stream", None, None, True), ("lane-grid8", "lane", "8", False), ("tile-grid8", None, "8", False)):
        _env(monkeypatch, row, path=path)
        if grid:
            monkeypatch.setenv("SEIGEN_HIP_GRID_BLOCKS", grid)
        ts = torch.cuda.Stream() if own_stream else None
        blk = _block(row, stream=int(ts.cuda_stream) if ts else None)
        try:
            blk.set_field(f, case["u"][f])
            name = blk.stage_kernel_name(_lib.STAGE_UH1)
            out = {}
            if ts:
                assert blk.stream_ptr() == int(ts.cuda_stream)
                with torch.cuda.stream(ts):
                    for kind in (0, 1, 2, 3):
                        out[kind] = blk.get_gradient_dev(f, kind).clone()          # consumed on the stream, no wait in between
                ts.synchronize()
                seen[label] = ({k: v.cpu().numpy() for k, v in out.items()}, name)
                continue
            for kind in (0, 1, 2, 3):
                out[kind] = blk.get_gradient_dev(f, kind).cpu().numpy()
                part = blk.get_gradient_dev(f, kind, cell0=3, ncells=blk.ncells - 7).cpu().numpy()
                assert np.array_equal(part, out[kind][3:blk.ncells - 4]), (label, kind)
            seen[label] = (out, name)
        finally:
            blk.close()
    names = {label: name for label, (out, name) in seen.items()}
    assert len({names["tile"], names["lane"], names["generic"]}) == 3, names          # three families ran
    for label in seen:
        for kind in (0, 1, 2, 3):
            assert np.array_equal(seen[label][0][kind], seen["tile"][0][kind]), (label, kind)
    ratio, factor = _within_bound(seen["tile"][0][0], case, f)
    assert ratio <= factor


# ---- 6. nothing else moves ------------------------------------------------------------------------------------------------

def _smooth_block(row):
    """a block of the row with smooth fields"""
    blk = _block(row)
    dim = row[1]
    X = blk.node_coords()
    u = np.stack([np.sin(2 * X[..., 0] + i) * np.cos(X[..., -1] - i) for i in range(dim)], axis=-1)
    s = np.zeros(X.shape[:-1] + (dim, dim))
    for i in range(dim):
        for j in range(dim):
            s[..., i, j] = np.cos(X[..., 0] + 0.5 * (i + j)) * (1 + X[..., -1])
    blk.set_field(_lib.FIELD_U, u)
    blk.set_field(_lib.FIELD_S, s)
    return blk


@pytest.mark.parametrize("graph", ["1", "0"])
@pytest.mark.parametrize("name", ["mfma-P4-sym", "tile-tri-P3-f32", "lane-2d-P2", "hexm-DQ4", "generic-2d-P2"])
def test_nothing_else_moves(gpu, monkeypatch, name, graph):
    """the four fields, the storage mode and the counters are as before the calls; step(n) after them is bitwise a twin's that
    never called; called between two stepping calls (graph replays where graph = 1) the result is the restatement of the
    downloaded u1 within bound 1"""
    _torch()
    row = ROW[name]
    _env(monkeypatch, row, graph)
    t = _case(row)["t"]
    dim = t["dim"]
    kinds = [k for k in (0, 1, 2, 3) if not (k == 2 and dim == 1)]
    twin = _smooth_block(row)
    blk = _smooth_block(row)
    try:
        for b in (twin, blk):
            b.step(8)
        before = [blk.get_field(f) for f in FIELDS]
        sym, counters = blk.is_sym(), _counts(blk)
        got = {k: blk.get_gradient_dev(_lib.FIELD_U, k) for k in kinds}
        got_h = blk.get_gradient_dev(_lib.FIELD_UH, 0)
        blk.get_gradient(_lib.FIELD_U, 3)
        for f, x in zip(FIELDS, before):
            assert np.array_equal(blk.get_field(f), x), f
        assert blk.is_sym() == sym and _counts(blk) == counters
        # the restatement of the downloaded fields
        for f, g in ((_lib.FIELD_U, got[0]), (_lib.FIELD_UH, got_h)):
            u = before[FIELDS.index(f)]
            ratio = np.abs(g.cpu().numpy() - gc.grad_reference(t, u)) / (EPS * gc.grad_scale(t, u))
            assert ratio.max() <= 4 * (t["nd"] + dim), (f, ratio.max())
        assert np.abs(got[0].cpu().numpy()).max() > 1e-3
        for k in kinds:
            assert np.array_equal(got[k].cpu().numpy(), gc.kind_of(got[0].cpu().numpy(), k))
        for b in (twin, blk):
            b.step(8)
        # between two replays: again the restatement of what the block holds now
        u1 = blk.get_field(_lib.FIELD_U)
        g = blk.get_gradient_dev(_lib.FIELD_U, 0).cpu().numpy()
        ratio = np.abs(g - gc.grad_reference(t, u1)) / (EPS * gc.grad_scale(t, u1))
        assert ratio.max() <= 4 * (t["nd"] + dim), ratio.max()
        for b in (twin, blk):
            b.step(3)
        for f in FIELDS:
            assert np.array_equal(blk.get_field(f), twin.get_field(f)), f
        assert blk.is_sym() == twin.is_sym()
    finally:
        twin.close()
        blk.close()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["mfma-P3-sym", "lane-1d-P2", "generic-2d-P2"])
def test_refusals_leave_the_handle_as_it_was(gpu, monkeypatch, name):
    torch = _torch()
    row = ROW[name]
    _env(monkeypatch, row)
    case = _case(row)
    dim = case["t"]["dim"]
    blk = _block(row)
    lib = blk.lib
    try:
        blk.set_field(_lib.FIELD_U, case["u"][_lib.FIELD_U])
        first = blk.get_gradient_dev(_lib.FIELD_U, 0).cpu().numpy()          # (the tables exist from here on)
        before = [blk.get_field(f) for f in FIELDS]
        sym, counters = blk.is_sym(), _counts(blk)
        n = blk.ncells * blk.nd * dim * dim
        buf = torch.full((n + 8,), SENTINEL, dtype=torch.float64, device="cuda")
        host = np.full(n + 8, SENTINEL)
        p, nb = C.c_void_p(buf.data_ptr()), n * 8

        def dev(field=_lib.FIELD_U, kind=0, c0=0, k=blk.ncells, ptr=p, dtype=0, nbytes=nb):
            return lib.sg_get_gradient_dev(blk.h, field, kind, c0, k, ptr, dtype, nbytes)

        def hst(field=_lib.FIELD_U, kind=0, c0=0, k=blk.ncells, ptr=host.ctypes.data, nbytes=nb):
            return lib.sg_get_gradient(blk.h, field, kind, c0, k, ptr, nbytes)
        for call in (dev, hst):
            assert call(field=_lib.FIELD_S) == -1 and call(field=_lib.FIELD_SH) == -1 and call(field=4) == -1 and call(field=-1) == -1
            assert call(kind=4) == -1 and call(kind=-1) == -1
            assert call(nbytes=nb - 8) == -1 and call(nbytes=nb + 8) == -1 and call(nbytes=nb // 2) == -1
            assert call(ptr=None) == -1
            assert call(c0=-1) == -1 and call(c0=1) == -1 and call(k=blk.ncells + 1, nbytes=nb + blk.nd * dim * dim * 8) == -1
            assert call(k=-1, nbytes=0) == -1
            if dim > 1:
                assert call(kind=1) == -1                                    # nbytes is the gradient's, not the divergence's
            if dim == 1:
                assert call(kind=2) == -1 and call(kind=2, nbytes=blk.ncells * blk.nd * 8) == -1
            assert b"sg_get_gradient" in lib.sg_last_error(blk.h)
        assert dev(dtype=2) == -1 and dev(dtype=-1) == -1 and dev(dtype=1) == -1      # (float: half the bytes)
        blk.sync()
        assert (buf.cpu().numpy() == SENTINEL).all() and (host == SENTINEL).all()     # nothing was written
        # an empty range is no error and writes nothing
        assert dev(c0=blk.ncells, k=0, nbytes=0) == 0 and hst(c0=0, k=0, nbytes=0) == 0
        blk.sync()
        assert (buf.cpu().numpy() == SENTINEL).all()
        for f, x in zip(FIELDS, before):
            assert np.array_equal(blk.get_field(f), x), f
        assert blk.is_sym() == sym and _counts(blk) == counters
        assert np.array_equal(blk.get_gradient_dev(_lib.FIELD_U, 0).cpu().numpy(), first)
        with pytest.raises(ValueError):
            blk.get_gradient_dev(_lib.FIELD_U, "rot")
        with pytest.raises(ValueError):
            blk.get_gradient_dev(_lib.FIELD_U, 0, out=torch.zeros((blk.ncells, blk.nd, dim, dim), dtype=torch.float64))      # host memory
        with pytest.raises(ValueError):
            blk.get_gradient_dev(_lib.FIELD_U, 1, out=torch.zeros((blk.ncells, blk.nd, 1), dtype=torch.float64, device="cuda"))
    finally:
        blk.close()


# ---- 8. the solver class --------------------------------------------------------------------------------------------------

def test_solver_class(gpu, monkeypatch):
    """dilatation(), rotation() and strain_rate() on a small 2-D run are the block's calls bitwise, Function.gradient too; the
    strain's trace equals the dilatation: summed in the order of the divergence, E00 + E11, bitwise (the diagonal of the strain
    is the gradient's own); summed in any order within the rounding of its dim - 1 additions on either side,
    |trace - div| <= 2 (dim - 1) 2^-53 sum_i |E_ii|."""
    torch = _torch()
    import seigen_amd
    import seigen_amd.helpers as helpers
    from seigen_amd import ElasticLF4, RectangleMesh
    from seigen_amd.functionspace import Function
    row = ROW["tile-tri-P3"]
    _env(monkeypatch, row)
    monkeypatch.setattr(helpers, "log", lambda s: None)
    monkeypatch.setattr(seigen_amd.elastic, "log", lambda s: None)
    mesh = RectangleMesh(5, 3, 1.0, 0.7, diagonal="left")
    el = ElasticLF4.create(mesh, "DG", 3, dimension=2, solver="explicit", output=False)
    el.l, el.mu, el.density = 0.5, 0.25, 1.0
    el.dt = 1e-3
    blk = el.block
    X = blk.node_coords()
    u = np.stack([np.sin(3 * X[..., 0] + 1) * np.cos(2 * X[..., 1]), np.cos(X[..., 0] - X[..., 1])], axis=-1)
    el.u0.from_torch(torch.from_numpy(u).cuda())
    el.run(4 * el.dt * (1 + 1e-9))
    assert np.abs(blk.get_field(_lib.FIELD_U) - u).max() > 1e-6                      # the run moved the field
    div, rot, eps = el.dilatation(), el.rotation(), el.strain_rate()
    assert tuple(div.shape) == (blk.ncells, blk.nd) and tuple(rot.shape) == (blk.ncells, blk.nd)
    assert tuple(eps.shape) == (blk.ncells, blk.nd, 2, 2)
    for got, kind in ((div, "div"), (rot, "curl"), (eps, "strain")):
        assert np.array_equal(got.cpu().numpy(), blk.get_gradient_dev(_lib.FIELD_U, kind).cpu().numpy()), kind
        assert np.array_equal(got.cpu().numpy(), el.u1.gradient(kind).cpu().numpy()), kind
        assert np.array_equal(got.cpu().numpy(), blk.get_gradient(_lib.FIELD_U, kind)), kind
    g = el.u1.gradient()
    assert tuple(g.shape) == (blk.ncells, blk.nd, 2, 2)
    assert np.array_equal(el.u1.gradient("grad", dtype=torch.float32).cpu().numpy(), g.cpu().numpy().astype(np.float32))
    E, D = eps.cpu().numpy(), div.cpu().numpy()
    assert np.abs(D).max() > 1e-3 and np.abs(rot.cpu().numpy()).max() > 1e-3
    assert np.array_equal(E[..., 0, 0] + E[..., 1, 1], D)
    assert np.array_equal(E[..., 0, 1], E[..., 1, 0])
    bound = 2 * (2 - 1) * EPS * (np.abs(E[..., 0, 0]) + np.abs(E[..., 1, 1]))
    assert (np.abs(np.trace(E, axis1=-2, axis2=-1) - D) <= bound).all()
    # the gradient against the restatement of the downloaded u1
    t = gc.tables_of(gc.block_cfg(2, 3, (5, 3), "left", h=[1.0 / 5, 0.7 / 3]))
    u1 = blk.get_field(_lib.FIELD_U)
    ratio = np.abs(g.cpu().numpy() - gc.grad_reference(t, u1)) / (EPS * gc.grad_scale(t, u1))
    assert ratio.max() <= 4 * (t["nd"] + 2)
    with pytest.raises(ValueError):
        el.s1.gradient()
    with pytest.raises(ValueError):
        Function(el.U).gradient()
