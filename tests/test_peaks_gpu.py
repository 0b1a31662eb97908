"""The peak maps: per node the maximum of |u|^2 and of s:s over the samples of a run and the sample that reached it, kept on the
device inside the time loop (include/seigen_hip.h sg_set_peaks / sg_get_peaks / sg_get_peaks_dev / sg_peaks_samples;
kernels_peak.hip, peak.cpp).

Rows: the nine of tests/gradient_loop.py ROWS - all five kernel families, symmetric and full storage, FP32, gw = 16 / 64 / 1 -
and a 1-D lane row (P2, 7 cells); the set-up of tests/test_spectra_gpu.py _block; K = 6 steps in 3-D and 12 otherwise, a
sample after every second step, both fields.

1. bitwise against a twin: step(K) on an armed handle against tests/test_peaks_host.py peak_reference of the (u, s) a twin
   downloads after each of K calls of step(1): value equal bit for bit, sample equal, every row, both fields.
2. against the oracle: a constant-sigma sponge strip and a source on the nodes of a box, OracleLF4 given the same inputs, its
   states through peak_reference.  With delta = 10 tol_of() max |field| (5e-5 max |field| for the FP32 row: the per-word
   parity margins of tests/test_spectra_gpu.py) and W the weighted number of terms (off-diagonals count twice: dim for the
   velocity, dim^2 for the stress), B = W (2 max |x| delta + delta^2) bounds the change of m when every word moves by delta:
   |value - oracle| <= B; the oracle's own m at the device's sample is at least the oracle's maximum - 2 B, for every node;
   nodes with sample = -1 have an oracle maximum <= B.
3. bitwise invariance: graph replay, SEIGEN_HIP_GRAPH=0, K calls of step(1), host-driven stages with end_step, timing on, a
   caller's non-blocking stream.
4. symmetric storage left half-way through the samples: within one storage mode the bits of 1., across the switch the twin's
   restatement with the formula switched at the same step, within B.
5. the lifecycle: nothing recorded after nsamples, re-arming, disarming, the failing calls, a wrong nvalues, the injectors'
   entry, arming between graph replays, and all five hooks armed together.
6. a block split over two ranks (tests/fake_rccl, tests/peaks_exchange_worker.py).
7. the device getter.
8. the solver class on a small explosive-source run.

Measured on an MI355X (profiles/r13/peaks.txt).  1., 3., 5., 6., 7.: equal bits and equal samples.  2.: |value - oracle|
9e-14 .. 1.8e-12 against B of 3e-9 .. 5e-8 in double, 1.9e-6 against 1.5e-3 .. 4.9e-3 in FP32; the oracle's m at the device's
sample is the oracle's maximum at every node.  4.: equal bits on both sides of the switch (the bound asked is B, 6e-8 .. 1.5e-7)."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle.lf4 import OracleLF4  # noqa: E402
from seigen_amd import _lib  # noqa: E402
from tests import gradient_loop as gl  # noqa: E402
from tests.test_parity_gpu import tol_of  # noqa: E402
from tests.test_peaks_host import peak_reference, peak_terms  # noqa: E402
from tests.test_spectra_gpu import SWITCHES, _block, _fields, _initial, _twin_samples  # noqa: E402
from tests.util import oracle_mesh  # noqa: E402

ROWS = list(gl.ROWS) + [("lane-1d-P2", 1, 2, (7,), "left", "f64", "lane")]
BY_NAME = {r[0]: r for r in ROWS}
EVERY = 2
FIELDS = (_lib.FIELD_U, _lib.FIELD_S)


def _steps(dim):
    return 6 if dim == 3 else 12


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _maps(blk):
    """[(value, sample) of the velocity, of the stress]"""
    return [blk.get_peaks(k) for k in range(2)]


def _same_maps(a, b):
    return all(np.array_equal(_bits(a[k][0]), _bits(b[k][0])) and np.array_equal(a[k][1], b[k][1]) for k in range(len(a)))


def _reference(su, ss, dim, sym, start=None, j0=0):
    """the maps of the twin's samples: the velocity's, and the stress's by the formula of the storage mode"""
    start = start or [(None, None), (None, None)]
    return [peak_reference(su, dim, False, start[0][0], start[0][1], j0, stress=False),
            peak_reference(ss, dim, sym, start[1][0], start[1][1], j0, stress=True)]


def _bound(x, dim, stress, factor):
    """B of the module's docstring for the samples x"""
    top = float(np.abs(x).max())
    delta = factor * top
    return (dim * dim if stress else dim) * (2.0 * top * delta + delta * delta)


# ---- 1. bitwise against a twin ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_bitwise_against_a_twin(gpu, monkeypatch, row):
    name, dim = row[0], row[1]
    K = _steps(dim)
    blk, dt = _block(row, monkeypatch)
    twin, _ = _block(row, monkeypatch)
    assert blk.peaks_samples() == 0
    blk.set_peaks(3, EVERY, K // EVERY)
    blk.step(K)
    assert blk.peaks_samples() == K // EVERY and blk.counters()["steps"] == K
    su, ss = _twin_samples(twin, K)
    got = _maps(blk)
    if name.startswith("mfma"):
        assert blk.is_sym()
    elif dim > 1:
        assert np.abs(ss[..., 0, 1] - ss[..., 1, 0]).max() > 1e-3 * np.abs(ss).max(), "full storage must hold s_ij != s_ji"
    want = _reference(su, ss, dim, blk.is_sym())
    for k, tag in enumerate(("velocity", "stress")):
        value, sample = got[k]
        assert value.shape == (blk.ncells, blk.nd) and value.dtype == np.float64 and sample.dtype == np.int32
        assert np.array_equal(_bits(value), _bits(want[k][0])), (name, tag, float(np.abs(value - want[k][0]).max()))
        assert np.array_equal(sample, want[k][1]), (name, tag)
        # the case shows something: every node moved, and not all nodes peak in one sample
        assert (sample >= 0).all() and (value > 0).all() and len(np.unique(sample)) > 1, (name, tag, np.unique(sample))
    # the fields are read, not written: the armed handle holds the twin's bits
    ua, sa = _fields(blk)
    ub, sb = _fields(twin)
    assert np.array_equal(ua, ub) and np.array_equal(sa, sb)
    blk.close()
    twin.close()


# ---- 2. against the oracle -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["tile-tri-P3", "mfma-P4-sym", "tile-tri-P3-f32"])
def test_against_the_oracle_with_a_sponge_and_a_source(gpu, monkeypatch, name):
    row = BY_NAME[name]
    _, dim, degree, n, diagonal, dtype, path = row
    K = _steps(dim)
    blk, dt = _block(row, monkeypatch, sym=True)
    m = oracle_mesh(dim, n, (1.0,) * dim, diagonal)
    Xq = m.node_coords(1)
    sigma = np.where(Xq[..., 0].min(axis=1, keepdims=True) >= 1.0 / n[0] - 1e-9, 25.0, 0.0) * np.ones_like(Xq[..., 0])
    blk.set_absorption(sigma, 1)
    X = blk.node_coords()
    nodes = np.nonzero(np.all((X >= 0.3) & (X <= 0.7), axis=-1).reshape(-1))[0]
    assert 0 < len(nodes) < X.shape[0] * X.shape[1]
    rng = np.random.default_rng(41)
    pat = rng.uniform(-1.0, 1.0, (len(nodes), dim, dim))
    pat = 0.5 * (pat + np.swapaxes(pat, -1, -2))
    vals = np.cos(0.8 * np.arange(K) + 0.3)[:, None, None, None] * pat[None] * 5.0
    blk.set_source(nodes, vals)
    blk.set_peaks(3, EVERY, K // EVERY)
    u0, s0 = _fields(blk) if dtype == "f64" else _initial(X, dim, True, 11)
    blk.step(K)
    sym = blk.is_sym()
    got = _maps(blk)
    blk.close()
    orc = OracleLF4(m, degree)
    lam, mu, _ = gl.material(m.ncells, 10 * dim + degree)
    orc.dt, orc.l, orc.mu, orc.density = dt, lam, mu, 1.0
    orc.E.set_absorption(sigma, 1)
    orc.u0, orc.s0 = u0.copy(), s0.copy()
    su, ss = [], []
    for k in range(K):
        S = np.zeros((X.shape[0] * X.shape[1], dim, dim))
        S[nodes] = vals[k]
        orc.source = lambda t, S=S: S.reshape(X.shape[:2] + (dim, dim))
        orc.step((k + 1) * dt)
        if (k + 1) % EVERY == 0:
            su.append(orc.u1.copy())
            ss.append(orc.s1.copy())
    factor = 5e-5 if dtype == "f32" else 10 * tol_of(degree, diagonal)
    for k, (tag, x) in enumerate((("velocity", np.array(su)), ("stress", np.array(ss)))):
        stress = k == 1
        value, sample = got[k]
        B = _bound(x, dim, stress, factor)
        ms = np.array([peak_terms(x[j], dim, sym and stress, stress) for j in range(len(x))])     # the oracle's own m, per sample
        top = ms.max(axis=0)
        err = float(np.abs(value - top).max())
        moved = sample >= 0
        at = np.take_along_axis(ms, np.maximum(sample, 0)[None].astype(np.int64), axis=0)[0]
        short = float((top - at)[moved].max()) if moved.any() else 0.0
        print("peaks against the oracle %s %s: |value - oracle| %.3e, oracle max - oracle m at the device's sample %.3e, B %.3e, "
              "max m %.3e, %d nodes never moved" % (name, tag, err, short, B, top.max(), int((~moved).sum())))
        assert top.max() > 100 * B, "the bound must be small against the maps"
        assert err <= B, (name, tag, err, B)
        assert np.all(at[moved] >= top[moved] - 2 * B), (name, tag, short, B)
        assert np.all(top[~moved] <= B), (name, tag)
        assert (sample < len(x)).all() and len(np.unique(sample[moved])) > 1


# ---- 3. bitwise invariance -------------------------------------------------------------------------------------------------

WAYS = ("graph", "eager", "single", "stages", "timing", "stream")


def _armed_run(blk, way, K):
    blk.set_peaks(3, EVERY, K // EVERY)
    if way == "timing":
        blk.enable_timing(True)
    if way == "single":
        for _ in range(K):
            blk.step(1)
    elif way == "stages":
        for _ in range(K):
            for st in range(6):
                blk.run_stage(st)
            blk.end_step()
    else:
        blk.step(K)
    assert blk.peaks_samples() == K // EVERY
    return _maps(blk)


def _run_way(row, monkeypatch, way, K):
    from tests.test_caller_stream_gpu import caller_stream
    if way == "stream":
        with caller_stream("hip-nonblocking") as st:
            blk, _ = _block(row, monkeypatch, stream=st.ptr)
            assert blk.stream_ptr() == st.ptr
            out = _armed_run(blk, way, K)
            blk.close()
            return out
    blk, _ = _block(row, monkeypatch, SEIGEN_HIP_GRAPH="0" if way == "eager" else None)
    out = _armed_run(blk, way, K)
    blk.close()
    return out


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_bits_do_not_depend_on_the_way_of_stepping(gpu, monkeypatch, row):
    K = _steps(row[1])
    want = _run_way(row, monkeypatch, "graph", K)
    assert all((v > 0).any() and (s >= 0).any() for v, s in want)
    for way in WAYS[1:]:
        assert _same_maps(_run_way(row, monkeypatch, way, K), want), (row[0], way)


# ---- 4. symmetric storage left mid-run -------------------------------------------------------------------------------------

def test_symmetric_storage_left_half_way(gpu, monkeypatch):
    """mfma-P4-sym, four samples: after two of them a stress upload that is not symmetric makes the block leave symmetric
    storage; val needs no fix-up, and from that step on the full-storage formula runs."""
    row = BY_NAME["mfma-P4-sym"]
    dim, degree, diagonal = row[1], row[2], row[4]
    K = 8
    blk, dt = _block(row, monkeypatch)
    twin, _ = _block(row, monkeypatch)
    blk.set_peaks(3, EVERY, K // EVERY)
    blk.step(K // 2)
    su, ss = _twin_samples(twin, K // 2)
    assert blk.is_sym() and blk.peaks_samples() == 2
    first = _reference(su, ss, dim, True)
    assert _same_maps(_maps(blk), first)
    s = blk.get_field(_lib.FIELD_S)
    s[..., 0, 1] += 0.3 * np.abs(s).max() * np.cos(np.arange(s.shape[1]))[None, :]
    for x in (blk, twin):
        x.set_field(_lib.FIELD_S, s)
        assert not x.is_sym()
    # leaving changes nothing the maps hold
    assert _same_maps(_maps(blk), first) and blk.peaks_samples() == 2
    blk.step(K // 2)
    su2, ss2 = _twin_samples(twin, K // 2)
    assert np.abs(ss2[..., 0, 1] - ss2[..., 1, 0]).max() > 1e-2 * np.abs(ss2).max()
    want = _reference(su2, ss2, dim, False, first, 2)
    got = _maps(blk)
    assert blk.peaks_samples() == 4
    factor = 10 * tol_of(degree, diagonal)
    for k, (tag, x) in enumerate((("velocity", np.concatenate([su, su2])), ("stress", np.concatenate([ss, ss2])))):
        B = _bound(x, dim, k == 1, factor)
        err = float(np.abs(got[k][0] - want[k][0]).max())
        print("peaks, symmetric storage left half-way, %s: |value - restatement| %.3e (B %.3e), bits %s, samples %s"
              % (tag, err, B, "equal" if np.array_equal(_bits(got[k][0]), _bits(want[k][0])) else "differ",
                 "equal" if np.array_equal(got[k][1], want[k][1]) else "differ"))
        assert err <= B, (tag, err, B)
        ms = np.array([peak_terms(x[j], dim, (j < 2) and k == 1, k == 1) for j in range(len(x))])
        at = np.take_along_axis(ms, np.maximum(got[k][1], 0)[None].astype(np.int64), axis=0)[0]
        assert (got[k][1] >= 0).all() and np.all(at >= ms.max(axis=0) - 2 * B), tag
    # the second half shows: some node of the stress peaks in it, by the full-storage formula
    assert (got[1][1] >= 2).any()
    blk.close()
    twin.close()


# ---- 5. the lifecycle ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["tile-tri-P3", "mfma-P3-f32"])
def test_lifecycle(gpu, monkeypatch, name):
    row = BY_NAME[name]
    K = _steps(row[1])
    blk, dt = _block(row, monkeypatch)
    n = K // EVERY
    nv = blk.ncells * blk.nd
    bv, bs = np.zeros(nv), np.zeros(nv, dtype=np.int32)

    def raw_get(field, nvalues=nv):
        return blk.lib.sg_get_peaks(blk.h, field, bv.ctypes.data, bs.ctypes.data, nvalues)

    # nothing armed
    assert raw_get(0) == -3 and raw_get(1) == -3 and blk.peaks_samples() == 0
    blk.set_peaks(3, EVERY, n)
    blk.step(K)
    assert blk.peaks_samples() == n
    armed = _maps(blk)
    assert all((v > 0).all() for v, _ in armed)
    # nothing is recorded after nsamples, nothing is refused
    blk.step(EVERY + 1)
    blk.step(1)

    def intact():
        return blk.peaks_samples() == n and _same_maps(_maps(blk), armed)

    assert intact()
    # the failing calls of the header
    for args in ((-1, EVERY, n), (4, EVERY, n), (3, 0, n), (3, -1, n), (3, EVERY, 0), (3, EVERY, -5), (1, EVERY, 2 ** 31), (2, 1, 2 ** 40)):
        assert blk.lib.sg_set_peaks(blk.h, *args) == -1, args
        assert blk.lib.sg_last_error(blk.h)
        assert intact(), args
    # the read-out's refusals
    assert raw_get(0, nv - 1) == -1 and raw_get(1, nv + 1) == -1 and raw_get(0, 0) == -1 and raw_get(2) == -1 and raw_get(-1) == -1
    assert blk.lib.sg_get_peaks_dev(blk.h, 0, None, 2, None, nv) == -1 and blk.lib.sg_get_peaks_dev(blk.h, 0, None, 0, None, nv - 1) == -1
    assert not bv.any() and not bs.any() and intact()
    # either pointer may be NULL
    assert blk.lib.sg_get_peaks(blk.h, 0, bv.ctypes.data, None, nv) == 0 and np.array_equal(bv.reshape(armed[0][0].shape), armed[0][0])
    assert blk.lib.sg_get_peaks(blk.h, 1, None, bs.ctypes.data, nv) == 0 and np.array_equal(bs.reshape(armed[1][1].shape), armed[1][1])
    # arming again zeroes the maps and restarts the count; the velocity alone: the stress is not selected
    blk.set_peaks(1, 1, 2)
    assert blk.peaks_samples() == 0
    v, s = blk.get_peaks(0)
    assert not v.any() and (s == -1).all()
    assert raw_get(1) == -3
    blk.step(1)
    v, s = blk.get_peaks(0)
    assert blk.peaks_samples() == 1 and (v > 0).all() and (s == 0).all()
    # what = 0 disarms
    blk.set_peaks(0)
    assert raw_get(0) == -3 and blk.lib.sg_get_peaks_dev(blk.h, 0, None, 0, None, nv) == -3 and blk.peaks_samples() == 0
    blk.step(2)
    blk.close()


@pytest.mark.parametrize("name", ["tile-tri-P3", "mfma-P4-sym"])
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_a_sample_excludes_the_injectors_entry_of_its_step(gpu, monkeypatch, name, graph):
    """Injectors armed beside the maps, a sample after every step, large entries: the maps are, bit for bit, those of what a
    twin driven by stages holds BEFORE sg_end_step adds the step's entry - the entry is absent from that sample and present
    in the next - and not those of what it holds after."""
    row = BY_NAME[name]
    dim = row[1]
    K = 6
    env = dict(SEIGEN_HIP_GRAPH=None if graph else "0")
    blk, dt = _block(row, monkeypatch, **env)
    twin, _ = _block(row, monkeypatch, **env)
    pts = np.array([[0.41, 0.57, 0.33][:dim], [0.8, 0.7, 0.2][:dim]])
    rng = np.random.default_rng(9)
    au = rng.uniform(-1.0, 1.0, (K, len(pts), dim))
    a = rng.uniform(-1.0, 1.0, (K, len(pts), dim, dim))
    a = np.triu(a) + np.swapaxes(np.triu(a, 1), -1, -2)
    series = 50.0 * np.concatenate([au, a.reshape(K, len(pts), dim * dim)], axis=-1)
    for x in (blk, twin):
        assert x.set_injectors(pts, series, 3).all()
    blk.set_peaks(3, 1, K)
    blk.step(K)
    before, after = ([], []), ([], [])
    for _ in range(K):
        for st in range(6):
            twin.run_stage(st)
        for k, f in enumerate(FIELDS):
            before[k].append(twin.get_field(f))
        twin.end_step()
        for k, f in enumerate(FIELDS):
            after[k].append(twin.get_field(f))
    sym = blk.is_sym()
    got = _maps(blk)
    assert _same_maps(got, _reference(np.array(before[0]), np.array(before[1]), dim, sym)), name
    assert not _same_maps(got, _reference(np.array(after[0]), np.array(after[1]), dim, sym)), "the entries must show"
    # (entry k went into the twin behind the `before` of step k + 1: the `before` of step k + 2 is computed from it)
    assert np.abs(after[0][0] - before[0][0]).max() > 1e-3 * np.abs(before[0][0]).max()
    ua, sa = _fields(blk)
    ub, sb = _fields(twin)
    assert np.array_equal(ua, ub) and np.array_equal(sa, sb)
    blk.close()
    twin.close()


@pytest.mark.parametrize("name", ["tile-tri-P3", "mfma-P4-sym"])
def test_arming_between_graph_replays(gpu, monkeypatch, name):
    """step(4) by replay with nothing armed, armed, armed again with another every, disarmed: each captured graph is the one
    of what is armed, the maps are the twin's restatement, the fields the twin's bits."""
    row = BY_NAME[name]
    dim = row[1]
    blk, dt = _block(row, monkeypatch, SEIGEN_HIP_GRAPH="1")
    twin, _ = _block(row, monkeypatch, SEIGEN_HIP_GRAPH="1")
    blk.step(4)
    _twin_samples(twin, 4, 1)
    blk.set_peaks(3, 1, 3)
    blk.step(4)                                     # the fourth step is beyond the series
    su, ss = _twin_samples(twin, 4, 1)
    assert blk.peaks_samples() == 3 and _same_maps(_maps(blk), _reference(su[:3], ss[:3], dim, blk.is_sym()))
    blk.set_peaks(2, 2, 5)
    blk.step(4)
    blk.step(3)
    su, ss = _twin_samples(twin, 7, 2)
    want = _reference(su, ss, dim, blk.is_sym())
    assert blk.peaks_samples() == 3 and _same_maps([blk.get_peaks(1)], [want[1]])
    assert blk.lib.sg_get_peaks(blk.h, 0, None, None, blk.ncells * blk.nd) == -3
    blk.set_peaks(0)
    blk.step(4)
    _twin_samples(twin, 4, 1)
    ua, sa = _fields(blk)
    ub, sb = _fields(twin)
    assert np.array_equal(ua, ub) and np.array_equal(sa, sb) and blk.counters()["steps"] == 19
    blk.close()
    twin.close()


@pytest.mark.parametrize("name", ["tile-tri-P3", "mfma-P4-sym"])
def test_all_five_hooks_together(gpu, monkeypatch, name):
    """Receivers, monitor, spectra and injectors armed with and without the maps: their results are bitwise what they are
    without the maps; and the maps bitwise what they are alone - beside the injectors only, which are part of the fields'
    history."""
    from seigen_amd.elastic import spectra_weights
    row = BY_NAME[name]
    dim = row[1]
    K = _steps(dim)
    pts = np.array([[0.41, 0.57, 0.33][:dim], [0.8, 0.7, 0.2][:dim]])
    rng = np.random.default_rng(19)
    au = rng.uniform(-1.0, 1.0, (K, len(pts), dim))
    a = rng.uniform(-1.0, 1.0, (K, len(pts), dim, dim))
    a = np.triu(a) + np.swapaxes(np.triu(a, 1), -1, -2)
    series = 5.0 * np.concatenate([au, a.reshape(K, len(pts), dim * dim)], axis=-1)

    def run(others, peaks):
        blk, dt = _block(row, monkeypatch)
        assert blk.set_injectors(pts, series, 3).all()
        if others:
            assert blk.set_receivers(pts, 3, EVERY, K // EVERY).all()
            blk.set_monitor(EVERY, K // EVERY, (1.0, 0.5, 0.25))
            w = spectra_weights([0.0, 1.0 / (K * dt)], dt, EVERY, K // EVERY)
            blk.set_spectra(w, w, EVERY)
        if peaks:
            blk.set_peaks(3, EVERY, K // EVERY)
        blk.step(K)
        out = {"fields": _fields(blk)}
        if others:
            out["rec"], out["mon"] = blk.get_receivers(), blk.get_monitor()
            out["spc"] = [blk.get_spectrum(k, f) for k in range(2) for f in range(2)]
        if peaks:
            out["peaks"] = _maps(blk)
        blk.close()
        return out

    both, others, alone = run(True, True), run(True, False), run(False, True)
    assert len(both["rec"]) == K // EVERY and both["rec"].any() and both["mon"].any()
    assert np.array_equal(both["rec"], others["rec"]) and np.array_equal(both["mon"], others["mon"])
    assert all(np.array_equal(x, y) for x, y in zip(both["spc"], others["spc"]))
    assert all(np.array_equal(x, y) for x, y in zip(both["fields"], others["fields"]))
    assert all(np.array_equal(x, y) for x, y in zip(both["fields"], alone["fields"]))
    assert _same_maps(both["peaks"], alone["peaks"]) and all((v > 0).all() for v, _ in alone["peaks"])


# ---- 6. a split block ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fake():
    from fake_rccl.build import build
    return build()


def test_peaks_on_a_split_block(gpu, fake, tmp_path):
    """Two ranks over the transport double, the exchange inside the library, ONE sg_step(n) with a source and a sponge: the
    blocks' maps put together equal the single block's bit for bit."""
    from native_exchange_worker import setup_block
    from peaks_exchange_worker import peaks_of, EVERY as W_EVERY
    from seigen_amd.backend import HipBlock
    grid, n, degree, steps, world = (1, 1, 2), (16, 4, 4), 4, 6, 2
    env = dict(os.environ, SEIGEN_RCCL_LIB=fake, FAKE_RCCL_TIMEOUT_S="60", FAKE_RCCL_LOG=str(tmp_path / "fake"),
               HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2", FAKE_RCCL_ASYNC="1", FAKE_RCCL_SLOT_BYTES="1048576")
    env.pop("FAKE_RCCL_HOST", None)
    for var in SWITCHES:
        env.pop(var, None)
    logs = [open(tmp_path / ("rank%d.log" % r), "w") for r in range(world)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "peaks_exchange_worker.py"), str(tmp_path), str(world),
                               str(r), ",".join(map(str, grid)), ",".join(map(str, n)), str(degree), str(steps)],
                              cwd=ROOT, env=env, stdout=logs[r], stderr=subprocess.STDOUT) for r in range(world)]
    deadline = time.time() + 300
    errs = []
    for r, p in enumerate(procs):
        try:
            p.wait(timeout=max(1.0, deadline - time.time()))
        except subprocess.TimeoutExpired:
            p.kill()
            p.wait()
        logs[r].close()
        if p.returncode != 0:
            errs.append("rank %d: exit %r\n%s" % (r, p.returncode, open(tmp_path / ("rank%d.log" % r)).read()[-3000:]))
    assert not errs, "\n-----\n".join(errs)
    blk = HipBlock(3, degree, n, [1.0 / n[a] for a in range(3)], [0.0] * 3, "left", 0)
    setup_block(blk, n, degree, "source")
    blk.set_peaks(3, W_EVERY, steps // W_EVERY)
    blk.step(steps)
    whole = peaks_of(blk)
    blk.close()
    assert (whole["uv"] > 0).any() and (whole["sv"] > 0).any() and len(np.unique(whole["ss"])) > 1
    seen = np.zeros(whole["uv"].shape[0], dtype=int)
    for r in range(world):
        d = np.load(tmp_path / ("rank%d.npz" % r))
        assert int(d["steps"]) == steps and int(d["samples"]) == steps // W_EVERY
        seen[d["cells"]] += 1
        for key in ("uv", "sv"):
            assert np.array_equal(_bits(d[key]), _bits(whole[key][d["cells"]])), "rank %d %s" % (r, key)
        for key in ("us", "ss"):
            assert np.array_equal(d[key], whole[key][d["cells"]]), "rank %d %s" % (r, key)
    assert np.all(seen == 1)


# ---- 7. the device getter --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["mfma-P4-sym", "lane-2d-P2", "generic-2d-P2", "tile-tri-P3-f32"])
def test_device_getter(gpu, monkeypatch, name):
    """get_peaks_dev queued between two step calls without a host wait: a float64 tensor equals get_peaks of a twin stopped
    there bit for bit, a float32 tensor its rounding, the samples are equal; the steps behind it do not show in it."""
    import torch
    row = BY_NAME[name]
    K = _steps(row[1])
    blk, dt = _block(row, monkeypatch)
    twin, _ = _block(row, monkeypatch)
    for x in (blk, twin):
        x.set_peaks(3, EVERY, K // EVERY)
    blk.step(K // 2)
    dev = [blk.get_peaks_dev(k) for k in range(2)]
    dev32 = [blk.get_peaks_dev(k, dtype=torch.float32) for k in range(2)]
    blk.step(K - K // 2)
    twin.step(K // 2)
    half = _maps(twin)
    twin.step(K - K // 2)
    torch.cuda.synchronize()
    for k in range(2):
        v, s = dev[k]
        assert v.dtype == torch.float64 and s.dtype == torch.int32 and tuple(v.shape) == (blk.ncells, blk.nd) == tuple(s.shape)
        assert np.array_equal(_bits(v.cpu().numpy()), _bits(half[k][0])) and np.array_equal(s.cpu().numpy(), half[k][1]), (name, k)
        v32, s32 = dev32[k]
        assert v32.dtype == torch.float32
        assert np.array_equal(v32.cpu().numpy(), half[k][0].astype(np.float32)) and np.array_equal(s32.cpu().numpy(), half[k][1]), (name, k)
        assert (half[k][0] > 0).all()
    # ... and the whole run is the twin's
    full = _maps(twin)
    assert _same_maps(_maps(blk), full) and not _same_maps(full, half)
    blk.close()
    twin.close()


# ---- 8. the solver class ---------------------------------------------------------------------------------------------------

def test_solver_class_on_the_explosive_source(gpu, monkeypatch):
    """ElasticLF4.set_peaks / run / peak_map on the explosive-source set-up (DG4 sponge, box-Ricker stress source) on a reduced
    domain: amplitude^2, sample and time against the block-level getters and (sample + 1) * every * dt (+ dt / 2 for the
    stress); peak_map_torch against peak_map."""
    from seigen_amd.harness.explosive_source import ExplosiveSourceLF4
    for var in SWITCHES:
        monkeypatch.delenv(var, raising=False)
    Lx, Ly, h, dt, every = 100.0, 50.0, 2.5, 1e-3, 3
    T = 60 * dt
    el = ExplosiveSourceLF4().setup(Lx=Lx, Ly=Ly, h=h, dt=dt, source_x=45.0)
    nsteps = len(el.step_times(T))
    assert 59 <= nsteps <= 61
    with pytest.raises(RuntimeError):
        el.peak_map("velocity")
    with pytest.raises(ValueError):
        el.set_peaks(fields=("pressure",))
    el.set_peaks(fields=("velocity", "stress"), every=every)
    el.run(T)
    blk = el.block
    assert blk.counters()["steps"] == nsteps and blk.peaks_samples() == nsteps // every
    for k, field in enumerate(("velocity", "stress")):
        pm = el.peak_map(field)
        value, sample = blk.get_peaks(k)
        nodes = el.u1.dat.data.shape[0]
        assert pm["amplitude"].shape == pm["time"].shape == pm["sample"].shape == (nodes,)
        assert np.array_equal(pm["sample"], sample.ravel()) and np.array_equal(pm["amplitude"], np.sqrt(value.ravel()))
        assert np.allclose(pm["amplitude"] ** 2, value.ravel(), rtol=1e-15, atol=0.0)
        moved = pm["sample"] >= 0
        assert moved.any() and pm["amplitude"].max() > 0 and len(np.unique(pm["sample"][moved])) > 1
        want = (pm["sample"][moved] + 1.0) * every * dt + (0.5 * dt if k else 0.0)
        assert np.array_equal(pm["time"][moved], want) and np.isnan(pm["time"][~moved]).all()
        assert not value.ravel()[~moved].any()
        pt = el.peak_map_torch(field)
        for key in ("time", "sample"):
            assert np.array_equal(pt[key].cpu().numpy(), pm[key], equal_nan=True), (field, key)
        # (the square roots are taken by two libraries: equal to within an ulp)
        assert np.allclose(pt["amplitude"].cpu().numpy(), pm["amplitude"], rtol=4e-16, atol=0.0), field
    # no fields: the next run disarms
    el.set_peaks(fields=())
    el.run(2 * dt)
    with pytest.raises(RuntimeError):
        el.peak_map("velocity")
    assert el.block.peaks_samples() == 0
