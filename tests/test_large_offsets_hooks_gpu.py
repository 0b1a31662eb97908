"""The step-end hooks and the device read-outs where a field's device offsets pass 2^32 bytes and 2^31 elements: the window
method of tests/test_large_offsets_gpu.py (its Shape, plan, Window, elsewhere, rows, block and memory rule, imported) carried
to the kernels that module does not run - injectors (kernels_inject.hip), spectra (kernels_spectra.hip), device transfers
(kernels_xfer.hip tiled, devxfer.cpp), frames (kernels_frame.hip lanes, frame.cpp), peak maps (kernels_peak.hip, peak.cpp),
the gradient (kernels_grad.hip lanes, grad.cpp) and the gauges (kernels_gauge.hip, gauge.cpp).

Yardstick.  Never the oracle and never the new call against itself: the fields of window cells come down through
get_field_range, which the other module holds to the oracle at these offsets, and go through the restatement each feature's
own module owns - peak_reference (test_peaks_host.py), _check_transform (test_spectra_gpu.py), gauge_cases.ratio_and_factor,
grad_cases.grad_reference / grad_scale / kind_of, frame_cases.host_frame with backend.frame_weights, injector_weights with
test_injectors_gpu._exact_sum - on a configuration of the window's cubes (sg_config::cube0 = the window's first layer), so
points, pixels and cells are the big block's.  Tolerances are those modules': bitwise for the peak maps, the transfers, the
kinds made of a gradient and a one-shot injection; 2 (n + 2) 2^-53 sum |w x| for the spectra; 4 (nd + dim) 2^-53 A for the
gradient and the gauges (test_grad_gpu.py, test_gauges_gpu.py); 1e-14 (FP32 blocks 1e-6) of the frame's largest value
(test_frame_gpu.py test_value_against_the_host_path) and of the receivers' (test_receivers_gpu.py).

Hook windows.  A step carries data R = step_reach() layers outward: six operator applications, one layer each on tensor
cells, one per three on tetrahedra and one per two on triangles - 6, 2 and 3 layers a step (tests/test_large_offsets_host.py
holds it on the oracle over two whole steps).  A hook window is a window's three data layers and K R layers on each side,
K = 2 steps; the block's top ends one, and where the top window's would run into the one below (the hexahedral and the 2-D
row) it starts where that one ends - the union is what counts.  Everything a hook records outside the union is the untouched initial value, exactly: peak value 0.0 and sample -1,
accumulators 0.0, fields, frames and gradients 0.0 - over the whole complement, the ranges of elsewhere() named in it.

Parts, per row.  1: peaks (3, every 1, 2 samples), spectra (tier A: both fields, two frequencies, four distinct weights
parts; tier B: the stress alone, one frequency - its imaginary part already sits past 2^31 elements - read on the device part
by part into ONE float64 tensor through sg_get_spectrum_dev: the tiled transfer from a double source), gauges (kind strain
while the other hooks run; grad, div and curl each in a re-run from the re-uploaded data, stepping being bitwise
deterministic) and receivers at two points per data layer of every window, through two calls of step(1); get_peaks_dev
against get_peaks; probe_gradient on FIELD_UH.  2: one sg_inject (what = 3, several points in one cell of every window) into
the re-uploaded data: after = before + amp psi in the order listed, bitwise, as test_injectors_gpu.py compares a one-shot; then
a two-entry series through step(1) twice, each entry against a twin without injectors that has taken the same steps - part
1's first sample for entry 0, and for entry 1 the state after step 1 uploaded again and stepped once more - bitwise too, no
entry being propagated between the twin and the comparison.  3, on the stepped fields:
get_field_dev per window into float64 and float32, set_field_dev and back, an asymmetric upload leaving symmetric storage,
the whole stress field (tier A and B-tets-P4-f32: the caller's side passes 2^32 bytes); the gradient per window (grad within
the bound, strain = kind_of of it bitwise) and of the whole block in float32 (caller's side: 2^32 bytes on the FP32 tier A
row, 2^31 elements on tier B); frames - a slice through the middle data layer of every mark window (m = 3), the volume frame
(m = 1), and on B-tets-P4-f32 the volume frame of the stress into a strided float32 view of 9 2^28 sentinel words whose
component (2, 2) starts at 2^31 elements.

Memory, by arithmetic from field_bytes (need() below; a row skips, with both numbers, under 1.2 times it), in GB as fields +
accumulators + maps + the largest read-out: A-tets-P4, A-tets-P4-full and A-hexlane-DQ2 11.5 + 22.9 + 1.4 + 4.3 = 40.1;
A-tets-P4-f32 (twice the words before 2^32 bytes, accumulators in double) 11.5 + 45.8 + 2.9 + 8.6 = 68.7; A-tri-P4-f32 12.9 +
51.5 + 6.4 + 8.6 = 79.5; B-tets-P4 45.8 + 34.4 + 5.7 + 17.2 = 103.1; B-tets-P4-f32 22.9 + 34.4 + 5.7 + 17.2 = 80.2.

Not covered: the gw = 1 family, so the `flat` kernels of xfer, frame and grad and the scalar paths of peak and spectra
(choose_kernel_path never picks it at these sizes)."""
import ctypes as C

import numpy as np
import pytest

from tests import test_large_offsets_gpu as lo
from tests.test_injectors_host import make_cfg

pytestmark = pytest.mark.gpu

K = 2                       # steps
APPLICATIONS = 6            # operator applications of one LF4 step
HOOK_ROWS = ("A-tets-P4", "A-tets-P4-full", "A-tets-P4-f32", "A-hexlane-DQ2", "A-tri-P4-f32", "B-tets-P4", "B-tets-P4-f32")
ROWS = [next(r for r in lo.ROWS if r.name == name) for name in HOOK_ROWS]
WHOLE_FIELD = ("A", "B-tets-P4-f32")     # tier or name: rows that read the whole stress field on the device
STRIDED = "B-tets-P4-f32"
STRIDE_J = 1 << 28
SENTINEL = -7.5


# ---- the plan (no device) --------------------------------------------------------------------------------------------------
def step_reach(sh):
    """layers one whole step carries data outward: one per application on tensor cells, one per three in a Kuhn cube (the
    tetrahedra with a facet in its floor are not the ones with a facet in its ceiling, nor their neighbours) and one per two in
    a Kuhn square (two triangles: floor and ceiling are neighbours)"""
    return APPLICATIONS // (1 if sh.tensor else sh.dim)


class HookWindow(object):
    """layers [k0, k1) around the data layers [d0, d0 + DATA) of the window w"""

    def __init__(self, sh, w, k0, k1):
        self.w, self.k0, self.k1, self.d0 = w, k0, k1, w.k0 + w.d0
        self.layers = k1 - k0
        self.cell0, self.ncells = k0 * sh.per, (k1 - k0) * sh.per
        self.data = slice((self.d0 - k0) * sh.per, (self.d0 - k0 + lo.DATA) * sh.per)      # within the hook window
        self.cells = slice(self.cell0, self.cell0 + self.ncells)


def hook_windows(sh, Z, wins):
    out, floor = [], 0
    for w in wins:
        d0 = w.k0 + w.d0
        k0, k1 = max(d0 - K * step_reach(sh), floor), min(d0 + lo.DATA + K * step_reach(sh), Z)
        out.append(HookWindow(sh, w, k0, k1))
        floor = k1
    return out


def complement(hws, ncells):
    """the cell ranges outside every hook window"""
    out, at = [], 0
    for hw in hws:
        if hw.cell0 > at:
            out.append((at, hw.cell0))
        at = hw.cell0 + hw.ncells
    if at < ncells:
        out.append((at, ncells))
    return out


def elsewhere_outside(sh, wins, hws):
    """elsewhere() of the other module without the hook windows' cells (they are wider than its windows on tensor cells)"""
    cut = []
    for a, b in lo.elsewhere(sh, wins):
        pieces = [(a, b)]
        for hw in hws:
            pieces = [q for p in pieces for q in ((p[0], min(p[1], hw.cell0)), (max(p[0], hw.cell0 + hw.ncells), p[1])) if q[0] < q[1]]
        cut += pieces
    return sorted(set(cut))


def spectra_shape(row):
    """(fields, nfreq): tier A both fields and two frequencies, tier B the stress and one"""
    return ((0, 1), 2) if row.tier == "A" else ((1,), 1)


def host_words(sh, field, Z):
    """values of a field in the caller's layout"""
    return Z * sh.per * sh.nd * sh.ncomp(field)


def need(row, Z):
    """bytes on the device: the four fields, the accumulators (double, in the padded device layout), the maps (12 bytes a node
    word, both fields) and the largest read-out alive at once"""
    sh = row.sh
    fields = lo.field_bytes(sh, Z)
    per_value = fields // (2 * (sh.dim + sh.dim * sh.dim))                 # bytes of one component's line set
    fset, nfreq = spectra_shape(row)
    acc = 2 * nfreq * sum(sh.ncomp("US"[k]) for k in fset) * (per_value // sh.itemsize) * 8
    maps = 2 * 12 * (per_value // sh.itemsize)
    readout = host_words(sh, "S", Z) * 8                                    # one part of a stress spectrum
    readout = max(readout, 12 * Z * sh.per * sh.nd)                         # get_peaks_dev
    if row.name == STRIDED:
        readout = max(readout, 9 * STRIDE_J * 4)
    return dict(fields=fields, acc=acc, maps=maps, readout=readout, total=fields + acc + maps + readout)


def _need_or_skip(row, Z):
    """lo._need_or_skip's rule with all the bytes of this module's row"""
    import torch
    n = need(row, Z)
    free = torch.cuda.mem_get_info()[0]
    print("MEM large hooks %s needs %.1f GB (fields %.1f, accumulators %.1f, maps %.1f, read-out %.1f), %.1f GB are free"
          % (row.name, n["total"] / 1e9, n["fields"] / 1e9, n["acc"] / 1e9, n["maps"] / 1e9, n["readout"] / 1e9, free / 1e9))
    if free < 1.2 * n["total"]:
        pytest.skip("%s needs %.1f GB, %.1f GB are free" % (row.name, n["total"] / 1e9, free / 1e9))
    lo._need_or_skip(row, Z, 1)


def window_cfg(sh, k0, layers):
    """the configuration of the cubes of layers [k0, k0 + layers): a block of the same mesh"""
    d = sh.dim
    return make_cfg(d, sh.P, sh.n(layers), sh.h, sh.tensor, cube0=(0,) * (d - 1) + (k0,))


def points_of(sh, hws, rng):
    """two points per data layer of every window inside cubes, fractions 0.15 .. 0.85 (as lo._source_sponge_receivers)"""
    d, pts = sh.dim, []
    for hw in hws:
        for k in range(lo.DATA):
            for i in range(2):
                frac = rng.uniform(0.15, 0.85, size=d)
                cube = [rng.integers(0, 3)] + ([rng.integers(0, 2)] if d == 3 else []) + [hw.d0 + k]
                pts.append([(cube[a] + frac[a]) * sh.h[a] for a in range(d)])
    return np.array(pts)


# ---- helpers of the test ---------------------------------------------------------------------------------------------------
class Run(object):
    """what the parts share"""


def _say(R, hw, what, figure):
    print("ERR large hooks %s [%s] %s %s" % (R.row.name, hw.w.what if hw is not None else "block", what, figure))


def _f32(R, a):
    return a.astype(np.float32).astype(np.float64) if R.sh.dtype == "f32" else a


def _upload(R):
    from seigen_amd import _lib
    for hw, st in zip(R.hws, R.state):
        R.blk.set_field_range(_lib.FIELD_U, hw.cell0, st["u"])
        R.blk.set_field_range(_lib.FIELD_S, hw.cell0, st["T"])
        for f in (_lib.FIELD_UH, _lib.FIELD_SH):
            R.blk.set_field_range(f, hw.cell0, np.zeros_like(st["u"] if f == _lib.FIELD_UH else st["T"]))
    assert R.blk.is_sym() == R.row.sym


def _down(R, field):
    return [R.blk.get_field_range(field, hw.cell0, hw.ncells) for hw in R.hws]


def _two_steps(R):
    """step(1) twice: ([windows][2 samples] of u, the same of s)"""
    from seigen_amd import _lib
    us, ss = [], []
    for _ in range(K):
        R.blk.step(1)
        us.append(_down(R, _lib.FIELD_U))
        ss.append(_down(R, _lib.FIELD_S))
    return [np.array([us[j][i] for j in range(K)]) for i in range(len(R.hws))], [np.array([ss[j][i] for j in range(K)]) for i in range(len(R.hws))]


def _zero_on_device(t, ranges, what):
    """t [ncells, ...] on the device: exactly zero over the cell ranges"""
    for a, b in ranges:
        assert not bool(t[a:b].any()), "%s is not zero in cells [%d, %d)" % (what, a, b)


def _local(R, hw, cell):
    mine = [k for k in range(len(cell)) if hw.cell0 <= cell[k] < hw.cell0 + hw.ncells]
    return mine


# ---- one row ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_hooks_and_readouts_at_the_marks(gpu, monkeypatch, row):
    from seigen_amd import _lib
    from seigen_amd.backend import locate_points
    for var in lo._SWITCHES:
        monkeypatch.delenv(var, raising=False)
    for var, val in row.env.items():
        monkeypatch.setenv(var, val)
    sh = row.sh
    Z, wins = lo.plan(sh, row.tier, row.ghost)
    _need_or_skip(row, Z)
    R = Run()
    R.row, R.sh, R.Z, R.wins = row, sh, Z, wins
    R.hws = hook_windows(sh, Z, wins)
    R.outside = complement(R.hws, Z * sh.per)
    R.named = elsewhere_outside(sh, wins, R.hws)
    assert R.named and all(any(a >= c and b <= d for c, d in R.outside) for a, b in R.named)     # the complement holds them
    rng = R.rng = np.random.default_rng(sum(map(ord, row.name)) + 1)
    R.state = []
    for hw in R.hws:
        st = lo._window_state(sh, hw.w, rng, row.sym, sh.W * sh.per)
        u, T = np.zeros((hw.ncells, sh.nd, sh.dim)), np.zeros((hw.ncells, sh.nd, sh.dim, sh.dim))
        u[hw.data], T[hw.data] = st["u"][hw.w.data], st["T"][hw.w.data]
        R.state.append(dict(u=_f32(R, u), T=_f32(R, T)))
    R.cfg = make_cfg(sh.dim, sh.P, sh.n(Z), sh.h, sh.tensor)
    R.wcfg = [window_cfg(sh, hw.k0, hw.layers) for hw in R.hws]
    R.pts = points_of(sh, R.hws, rng)
    R.cell, R.xi = locate_points(R.cfg, R.pts)
    for hw, cfg in zip(R.hws, R.wcfg):                    # the window configuration names the big block's cells and points
        mine = _local(R, hw, R.cell)
        assert len(mine) == 2 * lo.DATA                     # each window holds its share
        c, xi = locate_points(cfg, R.pts[mine])
        assert np.array_equal(c + hw.cell0, R.cell[mine]) and np.array_equal(xi, R.xi[mine])
    blk = None
    try:
        blk = R.blk = lo._make_block(row, Z, [])
        assert blk.ncells == Z * sh.per and blk.nd == sh.nd
        R.dt = 0.04 * min(sh.h) / sh.P ** 2
        blk.set_params(1.0, R.dt, 0.5, 0.25)
        _upload(R)
        assert [blk.stage_kernel_name(st) for st in range(6)] == row.names()
        _hooks_while_stepping(R)
        _one_shot_injection(R)
        _injector_series(R)
        _other_gauge_kinds(R)
        lo._assert_zero_elsewhere(blk, R.named, range(4))
        _transfers(R)
        _gradient(R)
        _frames(R)
        _leave_symmetric_storage(R)
    finally:
        if blk is not None:
            blk.close()


# ---- 1. the hooks ------------------------------------------------------------------------------------------------------------
def _weights(R):
    """complex weights [K, nfreq] as [K, nfreq, 2]: all parts distinct and away from zero"""
    nfreq = spectra_shape(R.row)[1]
    w = R.rng.uniform(0.5, 2.0, (K, nfreq, 2)) * R.rng.choice([-1.0, 1.0], (K, nfreq, 2))
    assert len(set(np.abs(w).ravel())) == w.size
    return w


def _hooks_while_stepping(R):
    from seigen_amd import _lib
    blk, sh = R.blk, R.sh
    fset, nfreq = spectra_shape(R.row)
    wu, ws = _weights(R), _weights(R)
    blk.set_peaks(3, 1, K)
    blk.set_spectra(wu if 0 in fset else None, ws, every=1)
    assert blk.set_gauges(R.pts, 3, 1, K).all()
    assert blk.set_receivers(R.pts, 3, 1, K).all()
    R.us, R.ss = _two_steps(R)
    assert blk.is_sym() == R.row.sym
    assert blk.peaks_samples() == K and blk.spectra_samples() == K
    for hw, st, u, s in zip(R.hws, R.state, R.us, R.ss):      # the steps moved the data, and differently
        assert lo.rel_err(u[0], st["u"]) > 1e-4 and lo.rel_err(u[1], u[0]) > 1e-4 and lo.rel_err(s[1], s[0]) > 1e-4
    _peaks(R)
    _spectra(R, (wu, ws))
    _gauges(R, 3, blk.get_gauges())
    _receivers(R, blk.get_receivers())
    blk.set_receivers(np.zeros((0, sh.dim)))
    blk.set_gauges(np.zeros((0, sh.dim)))
    # the gauges' arithmetic once, on the other velocity field
    uh = _down(R, _lib.FIELD_UH)
    got, owned = blk.probe_gradient(_lib.FIELD_UH, 0, R.pts)
    assert owned.all()
    _gauge_compare(R, 0, got, uh, "probe_gradient UH")


def _peaks(R):
    """get_peaks of both fields against peak_reference of the two downloaded samples, bit for bit; initial outside;
    get_peaks_dev of the stress against get_peaks"""
    import torch
    from tests.test_peaks_host import peak_reference
    blk, sh = R.blk, R.sh
    for k, samples in ((0, R.us), (1, R.ss)):
        value, sample = blk.get_peaks(k)
        for hw, x in zip(R.hws, samples):
            wv, wsmp = peak_reference(x, sh.dim, blk.is_sym(), stress=bool(k))
            ok = np.array_equal(value[hw.cells].view(np.int64), wv.view(np.int64)) and np.array_equal(sample[hw.cells], wsmp)
            _say(R, hw, "peaks field %d" % k, "equal bits" if ok else "DIFFER: %d values, %d samples"
                 % ((value[hw.cells] != wv).sum(), (sample[hw.cells] != wsmp).sum()))
            assert ok
            assert {0, 1} <= set(np.unique(wsmp[hw.data]))          # both samples hold maxima
        for a, b in R.outside + R.named:
            assert not value[a:b].any() and (sample[a:b] == -1).all(), "peak maps of field %d written in cells [%d, %d)" % (k, a, b)
        if k == 1:
            for dtype, want in ((torch.float64, value), (torch.float32, value.astype(np.float32))):
                dv, ds = blk.get_peaks_dev(k, dtype=dtype)
                ok = np.array_equal(dv.cpu().numpy(), want) and np.array_equal(ds.cpu().numpy(), sample)
                _say(R, None, "get_peaks_dev %s" % str(dtype).split(".")[-1], "equal bits" if ok else "DIFFER")
                assert ok
                del dv, ds
        del value, sample
    blk.set_peaks(0)


def _spectra(R, weights):
    """every part of every accumulator through sg_get_spectrum_dev into one tensor; the windows against _check_transform's
    restatement and bound, zero outside by reductions on the device"""
    import torch
    from seigen_amd import _lib
    from tests.test_spectra_gpu import _check_transform
    blk, sh = R.blk, R.sh
    fset, nfreq = spectra_shape(R.row)
    shapes = {0: blk.field_shape(_lib.FIELD_U), 1: blk.field_shape(_lib.FIELD_S)}
    flat = torch.empty(int(np.prod(shapes[1])), dtype=torch.float64, device="cuda")
    for k in fset:
        n = int(np.prod(shapes[k]))
        t = flat[:n].view(shapes[k])
        got = [np.zeros((nfreq,) + (hw.ncells,) + shapes[k][1:], dtype=complex) for hw in R.hws]
        for f in range(nfreq):
            for part in range(2):
                flat.fill_(SENTINEL)
                blk._on_stream(t, lambda: _lib.check(blk.lib.sg_get_spectrum_dev(blk.h, k, f, part, C.c_void_p(t.data_ptr()), 0, n * 8), blk.h))
                _zero_on_device(t, R.outside + R.named, "part %d of accumulator %d of field %d" % (part, f, k))
                for i, hw in enumerate(R.hws):
                    x = t[hw.cell0:hw.cell0 + hw.ncells].cpu().numpy()
                    if part:
                        got[i][f] += 1j * x
                    else:
                        got[i][f] += x
        for i, hw in enumerate(R.hws):
            _check_transform("large hooks %s [%s] field %d" % (R.row.name, hw.w.what, k), got[i], (R.us, R.ss)[k][i], weights[k])
    del t, flat
    blk.set_spectra(None, None)


def _gauge_compare(R, kind, got, u_windows, what):
    """rows [npts, ncomp] against gauge_cases' restatement on the windows' downloaded velocity, at test_gauges_gpu.py's bound"""
    from tests import gauge_cases as gk
    sh = R.sh
    for hw, cfg, u in zip(R.hws, R.wcfg, u_windows):
        mine = _local(R, hw, R.cell)
        ratio, factor, exact = gk.ratio_and_factor(cfg, R.pts[mine], u, kind, got[mine], sh.nd)
        _say(R, hw, "%s kind %d" % (what, kind), "|device - restatement| / (2^-53 A) %.2f, bound %d" % (ratio, factor))
        assert ratio <= factor and exact and np.abs(got[mine]).max() > 0


def _gauges(R, kind, tr):
    assert tr.shape[:2] == (K, len(R.pts))
    for j in range(K):
        _gauge_compare(R, kind, tr[j], [u[j] for u in R.us], "gauges sample %d" % j)


def _receivers(R, rec):
    """as lo._source_sponge_receivers: against the host evaluation of the block's own downloaded fields"""
    from tests import grad_cases as gc
    sh, d = R.sh, R.sh.dim
    assert rec.shape == (K, len(R.pts), d + d * d)
    phi = gc.tabulate_cell(1 if sh.tensor else 0, d, sh.P, R.xi)
    for hw, u, s in zip(R.hws, R.us, R.ss):
        mine = _local(R, hw, R.cell)
        for j in range(K):
            own = np.array([np.concatenate([phi[k] @ u[j][R.cell[k] - hw.cell0],
                                            np.tensordot(phi[k], s[j][R.cell[k] - hw.cell0], axes=(0, 0)).reshape(-1)]) for k in mine])
            scale = np.abs(own).max()
            e = np.abs(rec[j, mine] - own).max() / scale
            _say(R, hw, "receivers sample %d" % j, "%.3e" % e)
            assert scale > 0 and e <= (1e-6 if sh.dtype == "f32" else 1e-14)


def _other_gauge_kinds(R):
    """grad, div and curl: each armed on the re-uploaded data and run through the same two steps - stepping is bitwise
    deterministic, so the samples downloaded in part 1 are these runs' too (asserted on the last run's fields)"""
    from seigen_amd import _lib
    blk = R.blk
    for kind in (0, 1, 2):
        _upload(R)
        assert blk.set_gauges(R.pts, kind, 1, K).all()
        blk.step(K)
        _gauges(R, kind, blk.get_gauges())
    blk.set_gauges(np.zeros((0, R.sh.dim)))
    for f, want in ((_lib.FIELD_U, R.us), (_lib.FIELD_S, R.ss)):
        for got, x in zip(_down(R, f), want):
            assert np.array_equal(got, x[K - 1]), "a re-run of the two steps gave other bits"


# ---- 2. the injectors --------------------------------------------------------------------------------------------------------
def _injector_points(R):
    """(points, the window of each): every window's points with the first one listed twice and once more a little aside - a
    cell with several points, between the others"""
    pts, owner = [], []
    for i, hw in enumerate(R.hws):
        p = [R.pts[k] for k in _local(R, hw, R.cell)]
        pts += p[:1] + p + [p[0] + 1e-3 * np.array(R.sh.h)]
        owner += [i] * (len(p) + 2)
    return np.array(pts), np.array(owner)


def _injection_deltas(R, pts, owner, amp):
    """per window (du, ds): the exactly rounded sum of fma(amp, psi, v) from zero over a cell's points in the order listed
    (test_injectors_gpu.py _expected, on the window's cells)"""
    from seigen_amd.backend import injector_weights
    from tests.test_injectors_gpu import _exact_sum
    sh, d = R.sh, R.sh.dim
    out = []
    for i, (hw, cfg) in enumerate(zip(R.hws, R.wcfg)):
        rows = np.flatnonzero(owner == i)
        cell, psi = injector_weights(cfg, pts[rows], sh.nd)
        assert (cell >= 0).all() and cell[0] == cell[1] and len(set(cell)) < len(rows)      # a cell with several points
        du, ds = np.zeros((hw.ncells, sh.nd, d)), np.zeros((hw.ncells, sh.nd, d, d))
        for c in np.unique(cell):
            here = [r for r in range(len(rows)) if cell[r] == c]
            for a in range(sh.nd):
                for q in range(d + d * d):
                    v = _exact_sum([(float(amp[rows[r], q]), float(psi[r, a])) for r in here])
                    if q < d:
                        du[c, a, q] = v
                    else:
                        ds[c, a, (q - d) // d, (q - d) % d] = v
        assert np.abs(du).max() > 0 and np.abs(ds).max() > 0
        out.append((du, ds))
    return out


def _assert_added(R, what, before, after, deltas):
    """after = before + delta, one add (rounded to float on an FP32 block), bit for bit, in every window"""
    for i, hw in enumerate(R.hws):
        for k, name in enumerate("us"):
            want = _f32(R, before[k][i] + deltas[i][k])
            ok = np.array_equal(after[k][i], want)
            _say(R, hw, "%s %s" % (what, name), "equal bits" if ok else "DIFFER in %d words, largest %.3e"
                 % ((after[k][i] != want).sum(), np.abs(after[k][i] - want).max()))
            assert ok and (after[k][i] != before[k][i]).any()


def _one_shot_injection(R):
    """sg_inject (what = 3) into the re-uploaded data: after = before + the exactly rounded same-order sum of amp psi, one add,
    bit for bit (test_injectors_gpu.py: _expected, and the addition on top of what the fields hold)"""
    from seigen_amd import _lib
    from tests.test_injectors_gpu import _amplitudes
    blk = R.blk
    _upload(R)
    pts, owner = _injector_points(R)
    amp = _amplitudes(R.rng, len(pts), R.sh.dim, R.row.sym)
    before = (_down(R, _lib.FIELD_U), _down(R, _lib.FIELD_S))
    blk.inject(pts, amp, 3)
    assert blk.is_sym() == R.row.sym
    after = (_down(R, _lib.FIELD_U), _down(R, _lib.FIELD_S))
    _assert_added(R, "inject", before, after, _injection_deltas(R, pts, owner, amp))
    lo._assert_zero_elsewhere(blk, R.named, range(4))


def _injector_series(R):
    """a two-entry series armed on the re-uploaded data, step(1) twice.  Entry 0 goes in at the end of step 1: the fields are
    part 1's first sample (the twin without injectors: stepping is bitwise deterministic) + entry 0.  Entry 1 goes in at the
    end of step 2, propagated by nothing: with the series run out, the state after step 1 is uploaded again and stepped once
    without injectors - the fields after step 2 are that twin's + entry 1.  Both bit for bit, as one-shots are compared."""
    from seigen_amd import _lib
    from tests.test_injectors_gpu import _amplitudes
    blk = R.blk
    _upload(R)
    pts, owner = _injector_points(R)
    series = _amplitudes(R.rng, len(pts), R.sh.dim, R.row.sym, lead=(K,))
    assert blk.set_injectors(pts, series, 3).all()
    blk.step(1)
    one = (_down(R, _lib.FIELD_U), _down(R, _lib.FIELD_S))
    twin = ([u[0] for u in R.us], [s[0] for s in R.ss])
    _assert_added(R, "series entry 0", twin, one, _injection_deltas(R, pts, owner, series[0]))
    blk.step(1)
    two = (_down(R, _lib.FIELD_U), _down(R, _lib.FIELD_S))
    assert blk.injector_entries_left() == 0 and blk.is_sym() == R.row.sym
    lo._assert_zero_elsewhere(blk, R.named, range(4))
    blk.set_injectors(np.zeros((0, R.sh.dim)), None)
    for hw, u, s in zip(R.hws, *one):
        blk.set_field_range(_lib.FIELD_U, hw.cell0, u)
        blk.set_field_range(_lib.FIELD_S, hw.cell0, s)
    blk.step(1)
    twin = (_down(R, _lib.FIELD_U), _down(R, _lib.FIELD_S))
    _assert_added(R, "series entry 1", twin, two, _injection_deltas(R, pts, owner, series[1]))


# ---- 3. the read-outs ----------------------------------------------------------------------------------------------------------
def _transfers(R):
    import torch
    from seigen_amd import _lib
    blk, sh, row = R.blk, R.sh, R.row
    f32_block = sh.dtype == "f32"
    for f in (_lib.FIELD_U, _lib.FIELD_S):
        for hw in R.hws:
            want = blk.get_field_range(f, hw.cell0, hw.ncells)
            t = blk.get_field_dev(f, cell0=hw.cell0, ncells=hw.ncells)
            t32 = blk.get_field_dev(f, dtype=torch.float32, cell0=hw.cell0, ncells=hw.ncells)
            ok = np.array_equal(t.cpu().numpy(), want) and np.array_equal(t32.cpu().numpy(), want.astype(np.float32))
            _say(R, hw, "get_field_dev field %d" % f, "equal bits" if ok else "DIFFER")
            assert ok and np.abs(want).max() > 0
            if f == _lib.FIELD_S and sh.dim > 1:
                asym = np.abs(want - np.swapaxes(want, -1, -2)).max()
                assert (asym == 0) == row.sym          # full storage: the (j, i) lines are their own data
    # the whole stress field: the caller's side passes 2^32 bytes
    if row.tier in WHOLE_FIELD or row.name in WHOLE_FIELD:
        t = blk.get_field_dev(_lib.FIELD_S, dtype=torch.float32 if f32_block else torch.float64)
        _zero_on_device(t, R.outside + R.named, "the whole stress field on the device")
        for hw in R.hws:
            want = blk.get_field_range(_lib.FIELD_S, hw.cell0, hw.ncells)
            ok = np.array_equal(t[hw.cell0:hw.cell0 + hw.ncells].cpu().numpy(), want)
            _say(R, hw, "whole-field get_field_dev S", "equal bits" if ok else "DIFFER")
            assert ok
        del t
    # set: fresh data into the mark windows' data layers, symmetric where the storage is
    for f in (_lib.FIELD_U, _lib.FIELD_S):
        for hw in R.hws:
            x = R.rng.uniform(-1, 1, (hw.ncells,) + blk.field_shape(f)[1:])
            if f == _lib.FIELD_S and row.sym:
                x = lo._sym(x)
            for tdt in (torch.float64, torch.float32):
                xs = x.astype(np.float32).astype(np.float64) if (tdt == torch.float32 or f32_block) else x
                blk.set_field_dev(f, torch.from_numpy(xs).to("cuda", dtype=tdt), cell0=hw.cell0)
                ok = np.array_equal(blk.get_field_range(f, hw.cell0, hw.ncells), xs)
                _say(R, hw, "set_field_dev field %d %s" % (f, str(tdt).split(".")[-1]), "equal bits" if ok else "DIFFER")
                assert ok
            assert blk.is_sym() == row.sym
    lo._assert_zero_elsewhere(blk, R.named, (_lib.FIELD_U, _lib.FIELD_S))


def _leave_symmetric_storage(R):
    """last, on a row in symmetric storage: one (i, j) != (j, i) word uploaded from the device into the last mark window - the
    block leaves symmetric storage as test_device_transfer_gpu.py requires, and every window keeps its stress"""
    import torch
    from seigen_amd import _lib
    blk, sh, row = R.blk, R.sh, R.row
    if row.sym and sh.dim > 1:
        keep = _down(R, _lib.FIELD_S)
        hw = R.hws[-2]
        x = keep[-2].copy()
        x[hw.ncells // 2, sh.nd // 2, 1, 0] += 0.5
        x = _f32(R, x)
        blk.set_field_dev(_lib.FIELD_S, torch.from_numpy(x).cuda(), cell0=hw.cell0)
        assert not blk.is_sym()
        now = _down(R, _lib.FIELD_S)
        for i, h2 in enumerate(R.hws):
            ok = np.array_equal(now[i], x if h2 is hw else keep[i])
            _say(R, h2, "stress after leaving symmetric storage", "equal bits" if ok else "DIFFER")
            assert ok
        t = blk.get_field_dev(_lib.FIELD_S, cell0=hw.cell0, ncells=hw.ncells)
        assert np.array_equal(t.cpu().numpy(), x)
        lo._assert_zero_elsewhere(blk, R.named, (_lib.FIELD_S, _lib.FIELD_SH))


def _gradient(R):
    import torch
    from seigen_amd import _lib
    from tests import grad_cases as gc
    from tests.test_grad_gpu import EPS
    blk, sh = R.blk, R.sh
    tab = gc.tables_of(R.cfg)
    factor = 4 * (sh.nd + sh.dim)
    refs = []
    for hw in R.hws:
        u = blk.get_field_range(_lib.FIELD_U, hw.cell0, hw.ncells)
        want, A = gc.grad_reference(tab, u), gc.grad_scale(tab, u)
        G = blk.get_gradient_dev(_lib.FIELD_U, "grad", cell0=hw.cell0, ncells=hw.ncells).cpu().numpy()
        pos = A > 0
        ratio = float((np.abs(G - want)[pos] / (EPS * A[pos])).max())
        _say(R, hw, "gradient", "|device - restatement| / (2^-53 A) %.2f, bound %d" % (ratio, factor))
        assert ratio <= factor and np.array_equal(G[~pos], want[~pos]) and np.abs(want).max() > 0
        E = blk.get_gradient_dev(_lib.FIELD_U, "strain", cell0=hw.cell0, ncells=hw.ncells).cpu().numpy()
        ok = np.array_equal(E, gc.kind_of(G, 3))
        _say(R, hw, "strain", "equal bits" if ok else "DIFFER")
        assert ok
        refs.append(G)
    # the whole block in float32: the caller's side is as large as a stress in the caller's layout
    t = blk.get_gradient_dev(_lib.FIELD_U, "grad", dtype=torch.float32)
    _zero_on_device(t, R.outside + R.named, "the whole block's gradient")
    for hw, G in zip(R.hws, refs):
        ok = np.array_equal(t[hw.cell0:hw.cell0 + hw.ncells].cpu().numpy(), G.astype(np.float32))
        _say(R, hw, "whole-block gradient float32", "equal bits" if ok else "DIFFER")
        assert ok
    del t


def _frames(R):
    import torch
    from seigen_amd import _lib
    from tests import frame_cases as fc
    from tests.test_frame_gpu import _squeeze
    blk, sh, d = R.blk, R.sh, R.sh.dim
    tol = 1e-6 if sh.dtype == "f32" else 1e-14
    last = d - 1
    for f in (_lib.FIELD_U, _lib.FIELD_S):
        values = _down(R, f)
        # a slice through the middle data layer of every mark window: the cubes on both sides of the mark
        for hw, cfg, v in zip(R.hws[:-1], R.wcfg[:-1], values[:-1]):
            z = (hw.d0 + 1 + 0.4) * sh.h[last]
            want, px = fc.host_frame(cfg, sh.P, sh.tensor, 3, {last: z}, v)
            assert px["plan"]["layer"][last] == hw.d0 + 1 - hw.k0
            want = _squeeze(want, d, {last: z})
            got = blk.get_frame_dev(f, m=3, slice={last: z}).cpu().numpy()
            assert got.shape == want.shape
            scale = np.abs(want).max()
            e = np.abs(got - want).max() / scale
            _say(R, hw, "slice frame field %d" % f, "%.3e" % e)
            assert scale > 0 and e <= tol
        # the volume frame, one pixel a cube
        t = blk.get_frame_dev(f, m=1)
        assert tuple(t.shape[-d:]) == tuple(reversed(sh.n(R.Z)))
        tl = t.movedim(-d, 0)                                       # [layer, comps..., (P1,) P0]
        for a, b in R.outside + R.named:
            la, lb = -(-a // sh.per), b // sh.per                   # whole layers of the range
            assert not bool(tl[la:lb].any()), "the volume frame of field %d is not zero in layers [%d, %d)" % (f, la, lb)
        for hw, cfg, v in zip(R.hws, R.wcfg, values):
            want, _ = fc.host_frame(cfg, sh.P, sh.tensor, 1, None, v)
            want = _squeeze(want, d, None)
            got = t[(Ellipsis, slice(hw.k0, hw.k1)) + (slice(None),) * (d - 1)].cpu().numpy()
            scale = np.abs(want).max()
            e = np.abs(got - want).max() / scale
            _say(R, hw, "volume frame field %d" % f, "%.3e" % e)
            assert got.shape == want.shape and scale > 0 and e <= tol
        del t, tl
    if R.row.name == STRIDED:
        # the volume frame of the stress into a strided float32 view: component (i, j) starts at (3 i + j) 2^28 words
        npix = int(np.prod(sh.n(R.Z)))
        assert npix <= STRIDE_J and 8 * STRIDE_J == lo.ELEMS_2_31
        whole = torch.full((9 * STRIDE_J,), SENTINEL, dtype=torch.float32, device="cuda")
        n = sh.n(R.Z)
        view = torch.as_strided(whole, (3, 3, n[2], n[1], n[0]), (3 * STRIDE_J, STRIDE_J, n[1] * n[0], n[0], 1))
        assert blk.get_frame_dev(_lib.FIELD_S, m=1, out=view) is view
        dense = blk.get_frame_dev(_lib.FIELD_S, m=1, dtype=torch.float32)          # (held to the host path above)
        ok = bool(torch.equal(view, dense))
        assert int((whole.view(9, STRIDE_J)[:, npix:] != SENTINEL).sum()) == 0, "the strided frame wrote past its pixels"
        assert int((whole.view(9, STRIDE_J)[:, :npix] == SENTINEL).sum()) == 0, "the strided frame left pixels unwritten"
        for a, b in R.outside + R.named:
            assert not bool(view[:, :, -(-a // sh.per):b // sh.per].any()), "the strided frame is not zero outside the windows"
        values = _down(R, _lib.FIELD_S)
        for hw, cfg, v in zip(R.hws, R.wcfg, values):
            want, _ = fc.host_frame(cfg, sh.P, sh.tensor, 1, None, v)
            got = view[:, :, hw.k0:hw.k1].cpu().numpy().astype(np.float64)
            scale = np.abs(want).max()
            e = np.abs(got - want).max() / scale
            _say(R, hw, "strided volume frame", "%.3e" % e)
            assert scale > 0 and e <= 1e-6
        _say(R, None, "strided volume frame against the dense one", "equal bits" if ok else "DIFFER")
        assert ok
        del whole, view, dense
