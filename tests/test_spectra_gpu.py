"""The spectra: running Fourier transforms of the wavefield accumulated on the device inside the time loop
(include/seigen_hip.h sg_set_spectra / sg_get_spectrum / sg_spectra_samples / sg_correlate_spectra; kernels_spectra.hip).

Rows: the nine of tests/gradient_loop.py ROWS, K = 6 steps in 3-D and 12 in 2-D, three frequencies with f = 0 among them, a
sample after every second step, both fields, smooth fields with random phases and per-cell lambda, mu.  The matrix-pipe rows
hold a symmetric stress and stay in symmetric storage (the i > j lines are skipped), the others hold s_ij != s_ji.

1. the transform: step(K) on an armed handle against numpy's transform (in long double) of the fields a twin downloads after
   each of K calls of step(1).  Per word and part |device - reference| <= 2 (n + 2) 2^-53 sum_j |w_j x_j|, n the number of
   samples: the bound of a length-n dot product evaluated with fma, twice - once for the device's sum, once for headroom
   against the reference's own rounding; FP32 rows alike, the conversion being exact.  With one frequency and the weights
   (1, 0) the real part is the samples' sum in the order taken, bit for bit, and the imaginary part is zero.
2. against the oracle: a constant-sigma sponge strip and a source on the nodes of a box, OracleLF4 given the same inputs and
   transformed by numpy, within 10 tol_of() sum_j |w_j| max |field| (5e-5 for the FP32 row).
3. bitwise invariance: graph replay, SEIGEN_HIP_GRAPH=0, K calls of step(1), host-driven stages with end_step, timing on, a
   caller's non-blocking stream.
4. symmetric storage left half-way through the samples.
5. the lifecycle: nothing added after nsamples, re-arming, the failing calls, the read-out's refusals, the injectors' entry.
6. a block split over two ranks (tests/fake_rccl, tests/spectra_exchange_worker.py).
7. sg_correlate_spectra against Geometry.forms of the downloaded spectra, in sg_correlate's accumulator.

Measured on an MI355X (profiles/r10/spectra.txt).  1. and 4.: the largest |device - reference| / bound over words and parts
0.11 .. 0.22 in every row, FP32 rows included.  2.: |device - oracle| 2e-16 .. 4e-15 against bounds of 2e-11 .. 3e-11 in
double, 1e-8 .. 2e-8 against 1.1e-5 .. 1.4e-5 in FP32.  3., 5., 6.: equal bits.  7.: |device - host| / scale 3e-16 .. 1.4e-15
(bound 1e-11) with the accumulator at 0.15 .. 0.52 of its scale."""
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
from seigen_amd.backend import HipBlock  # noqa: E402
from seigen_amd.elastic import spectra_weights  # noqa: E402
from tests import gradient_loop as gl  # noqa: E402
from tests.test_parity_gpu import tol_of  # noqa: E402
from tests.util import oracle_mesh  # noqa: E402

ROWS = gl.ROWS
BY_NAME = {r[0]: r for r in ROWS}
SWITCHES = ("SEIGEN_HIP_PATH", "SEIGEN_HIP_GRAPH", "SEIGEN_HIP_SPONGE_AFFINE", "SEIGEN_HIP_SYM", "SEIGEN_HIP_SOURCE_LAUNCH",
            "SEIGEN_HIP_XCORR")
EVERY = 2
U53 = 2.0 ** -53
FIELDS = (_lib.FIELD_U, _lib.FIELD_S)


def _steps(dim):
    return 6 if dim == 3 else 12


def _freqs(dt, K):
    """f = 0, one period over the run, and a quarter of the sampling rate"""
    return np.array([0.0, 1.0 / (K * dt), 0.25 / (EVERY * dt)])


def _env(monkeypatch, path, **kw):
    for var in SWITCHES:
        monkeypatch.delenv(var, raising=False)
    if path:
        monkeypatch.setenv("SEIGEN_HIP_PATH", path)
    for k, v in kw.items():
        if v is not None:
            monkeypatch.setenv(k, v)


def _initial(X, dim, sym, seed):
    """smooth fields with phases from `seed`; sym: a symmetric stress, else s_ij != s_ji"""
    ph = np.random.default_rng(seed).uniform(0.0, 2.0 * np.pi, dim + dim * dim)
    u = np.stack([np.cos(3 * X[..., 0] + ph[i]) * np.sin(2 * X[..., -1] + 0.5 * i + 1.0) for i in range(dim)], axis=-1)
    s = np.zeros(X.shape[:-1] + (dim, dim))
    for i in range(dim):
        for j in range(dim):
            k = (min(i, j) * dim + max(i, j)) if sym else i * dim + j
            s[..., i, j] = np.sin(2 * X[..., 0] + ph[dim + k]) * (1.5 - X[..., -1])
    return u, s


def _block(row, monkeypatch, seed=11, stream=None, sym=None, **env):
    """(block, dt) of a row on the unit box: per-cell lambda, mu (gradient_loop.material), smooth fields"""
    name, dim, degree, n, diagonal, dtype, path = row
    _env(monkeypatch, path, **env)
    h = [1.0 / k for k in n]
    blk = HipBlock(dim, degree, n, h, [0.0] * dim, diagonal, stream=stream, dtype=dtype)
    dt = gl.DT_FACTOR * min(h) / degree ** 2
    lam, mu, _ = gl.material(blk.ncells, 10 * dim + degree)
    blk.set_params(1.0, dt, lam, mu)
    sym = name.startswith("mfma") if sym is None else sym
    u0, s0 = _initial(blk.node_coords(), dim, sym, seed)
    blk.set_field(_lib.FIELD_U, u0)
    blk.set_field(_lib.FIELD_S, s0)
    if name.startswith("mfma"):
        assert blk.is_sym() == sym
    blk._row, blk._dt, blk._hh = row, dt, h
    return blk, dt


def _weights(dt, K, every=EVERY, nsamples=None):
    n = K // every if nsamples is None else nsamples
    f = _freqs(dt, K)
    return spectra_weights(f, dt, every, n), spectra_weights(f, dt, every, n, stagger=0.5 * dt)


def _fields(blk):
    return blk.get_field(_lib.FIELD_U), blk.get_field(_lib.FIELD_S)


def _spectra(blk, nfreq=3, fields=(0, 1)):
    """[field][nfreq] complex arrays"""
    return [np.array([blk.get_spectrum(k, f) for f in range(nfreq)]) for k in fields]


def _twin_samples(twin, K, every=EVERY):
    """the twin's fields after every `every`-th of K calls of step(1): ([n, ...] velocity, [n, ...] stress)"""
    us, ss = [], []
    for k in range(1, K + 1):
        twin.step(1)
        if k % every == 0:
            u, s = _fields(twin)
            us.append(u)
            ss.append(s)
    return np.array(us), np.array(ss)


def _check_transform(tag, got, samples, w):
    """got [nfreq] complex, samples [n, ...], w [n, nfreq, 2]: the bound of the module's docstring, per word and part"""
    n = len(samples)
    x = np.asarray(samples, dtype=np.longdouble)
    worst = 0.0
    for f in range(w.shape[1]):
        for part, g in ((0, got[f].real), (1, got[f].imag)):
            wj = w[:n, f, part].astype(np.longdouble)
            ref = sum(wj[j] * x[j] for j in range(n))
            mag = np.asarray(sum(abs(wj[j]) * np.abs(x[j]) for j in range(n)), dtype=np.float64)
            bound = 2 * (n + 2) * U53 * mag
            err = np.abs(np.asarray(g - ref, dtype=np.float64))
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
            assert np.isfinite(g).all() and np.all(err <= bound), (tag, f, part, float((err / np.maximum(mag, 1e-300)).max()))
            if part == 0 or f > 0:
                assert np.abs(np.asarray(ref, dtype=np.float64)).max() > 0, (tag, f, part, "an empty transform shows nothing")
    print("spectra %s: largest |device - reference| / bound %.3f" % (tag, worst))


# ---- 1. the transform ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_transform_of_every_row(gpu, monkeypatch, row):
    name, dim = row[0], row[1]
    K = _steps(dim)
    blk, dt = _block(row, monkeypatch)
    twin, _ = _block(row, monkeypatch)
    wu, ws = _weights(dt, K)
    assert blk.spectra_samples() == 0
    blk.set_spectra(wu, ws, EVERY)
    blk.step(K)
    assert blk.spectra_samples() == K // EVERY and blk.counters()["steps"] == K
    su, ss = _twin_samples(twin, K)
    gu, gs = _spectra(blk)
    if name.startswith("mfma"):
        assert blk.is_sym()
    else:
        assert np.abs(ss[..., 0, 1] - ss[..., 1, 0]).max() > 1e-3 * np.abs(ss).max(), "full storage must hold s_ij != s_ji"
    _check_transform(name + " velocity", gu, su, wu)
    _check_transform(name + " stress", gs, ss, ws)
    # the fields are read, not written: the armed handle holds the twin's bits
    ua, sa = _fields(blk)
    ub, sb = _fields(twin)
    assert np.array_equal(ua, ub) and np.array_equal(sa, sb)
    # one frequency, weights (1, 0): the samples' sum in the order taken, bit for bit; re-arming has restarted the count
    n = K // EVERY
    ones = np.zeros((n, 1, 2))
    ones[..., 0] = 1.0
    blk.set_spectra(ones, ones, EVERY)
    assert blk.spectra_samples() == 0
    blk.step(K)
    su, ss = _twin_samples(twin, K)
    for k, x in ((0, su), (1, ss)):
        got = blk.get_spectrum(k, 0)
        want = np.zeros(x.shape[1:])
        for j in range(n):
            want = want + x[j]
        assert np.array_equal(got.real, want) and not got.imag.any() and np.abs(want).max() > 0, (name, k)
    blk.close()
    twin.close()


# ---- 2. against the oracle -----------------------------------------------------------------------------------------------

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
    wu, ws = _weights(dt, K)
    blk.set_spectra(wu, ws, EVERY)
    u0, s0 = _fields(blk) if dtype == "f64" else _initial(X, dim, True, 11)
    blk.step(K)
    gu, gs = _spectra(blk)
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
    for tag, got, x, w in (("velocity", gu, np.array(su), wu), ("stress", gs, np.array(ss), ws)):
        wc = w[..., 0] + 1j * w[..., 1]
        want = np.einsum("jf,j...->f...", wc, x)
        for f in range(3):
            bound = factor * np.abs(wc[:, f]).sum() * np.abs(x).max()
            err = np.abs(got[f] - want[f]).max()
            print("spectra against the oracle %s %s f%d: |device - oracle| %.3e, bound %.3e, max |transform| %.3e"
                  % (name, tag, f, err, bound, np.abs(want[f]).max()))
            assert np.abs(want[f]).max() > 10 * bound and err <= bound, (name, tag, f, err, bound)


# ---- 3. bitwise invariance -----------------------------------------------------------------------------------------------

WAYS = ("graph", "eager", "single", "stages", "timing", "stream")


def _run_way(row, monkeypatch, way, K):
    from tests.test_caller_stream_gpu import caller_stream
    if way == "stream":
        with caller_stream("hip-nonblocking") as st:
            blk, dt = _block(row, monkeypatch, stream=st.ptr)
            assert blk.stream_ptr() == st.ptr
            out = _armed_run(blk, dt, way, K)
            blk.close()
            return out
    blk, dt = _block(row, monkeypatch, SEIGEN_HIP_GRAPH="0" if way == "eager" else None)
    out = _armed_run(blk, dt, way, K)
    blk.close()
    return out


def _armed_run(blk, dt, way, K):
    wu, ws = _weights(dt, K)
    blk.set_spectra(wu, ws, EVERY)
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
    assert blk.spectra_samples() == K // EVERY
    return _spectra(blk)


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_bits_do_not_depend_on_the_way_of_stepping(gpu, monkeypatch, row):
    K = _steps(row[1])
    want = _run_way(row, monkeypatch, "graph", K)
    assert all(np.abs(x).max() > 0 for x in want)
    for way in WAYS[1:]:
        got = _run_way(row, monkeypatch, way, K)
        for k in range(2):
            assert np.array_equal(got[k], want[k]), (row[0], way, "velocity stress".split()[k])


# ---- 4. symmetric storage left mid-run -----------------------------------------------------------------------------------

def test_symmetric_storage_left_half_way(gpu, monkeypatch):
    """mfma-P4-sym, four samples: after two of them a stress upload that is not symmetric makes the block leave symmetric
    storage; the accumulators' i > j lines are then filled from their mirrors and accumulated from there on."""
    row = BY_NAME["mfma-P4-sym"]
    K = 8
    blk, dt = _block(row, monkeypatch)
    twin, _ = _block(row, monkeypatch)
    wu, ws = _weights(dt, K)
    blk.set_spectra(wu, ws, EVERY)
    blk.step(K // 2)
    su, ss = _twin_samples(twin, K // 2)
    assert blk.is_sym() and blk.spectra_samples() == 2
    gu, gs = _spectra(blk)
    _check_transform("before leaving: velocity", gu, su, wu)
    _check_transform("before leaving: stress", gs, ss, ws)
    assert np.array_equal(gs, np.swapaxes(gs, -1, -2))
    s = blk.get_field(_lib.FIELD_S)
    s[..., 0, 1] += 0.3 * np.abs(s).max() * np.cos(np.arange(s.shape[1]))[None, :]
    for x in (blk, twin):
        x.set_field(_lib.FIELD_S, s)
        assert not x.is_sym()
    # the mirror has filled the i > j lines: the read-out is what it was
    gs2 = _spectra(blk)[1]
    assert np.array_equal(gs2, gs) and blk.spectra_samples() == 2
    blk.step(K // 2)
    su2, ss2 = _twin_samples(twin, K // 2)
    gu, gs = _spectra(blk)
    su, ss = np.concatenate([su, su2]), np.concatenate([ss, ss2])
    assert np.abs(ss[2:, ..., 0, 1] - ss[2:, ..., 1, 0]).max() > 1e-2 * np.abs(ss).max()
    _check_transform("after leaving: velocity", gu, su, wu)
    _check_transform("after leaving: stress", gs, ss, ws)
    assert np.abs(gs[..., 0, 1] - gs[..., 1, 0]).max() > 1e-3 * np.abs(gs).max()
    blk.close()
    twin.close()


# ---- 5. the lifecycle ------------------------------------------------------------------------------------------------------

def _raw_set(blk, nfreq, what, every, nsamples, wu, ws):
    return blk.lib.sg_set_spectra(blk.h, nfreq, what, every, nsamples, None if wu is None else wu.ctypes.data,
                                  None if ws is None else ws.ctypes.data)


@pytest.mark.parametrize("name", ["tile-tri-P3", "mfma-P3-f32"])
def test_lifecycle(gpu, monkeypatch, name):
    row = BY_NAME[name]
    K = _steps(row[1])
    blk, dt = _block(row, monkeypatch)
    n = K // EVERY
    wu, ws = _weights(dt, K)
    bu, bs = np.zeros(blk.field_shape(_lib.FIELD_U)), np.zeros(blk.field_shape(_lib.FIELD_S))
    # nothing armed
    assert blk.lib.sg_get_spectrum(blk.h, 0, 0, 0, bu.ctypes.data, bu.nbytes) == -3
    assert blk.lib.sg_get_spectrum(blk.h, 1, 0, 0, bs.ctypes.data, bs.nbytes) == -3
    assert blk.spectra_samples() == 0
    blk.set_spectra(wu, ws, EVERY)
    blk.step(K)
    assert blk.spectra_samples() == n
    armed = _spectra(blk)
    assert all(np.abs(x).max() > 0 for x in armed)
    # nothing is added after nsamples, nothing is refused
    blk.step(EVERY + 1)
    blk.step(1)
    assert blk.spectra_samples() == n

    def intact():
        now = _spectra(blk)
        return blk.spectra_samples() == n and all(np.array_equal(now[k], armed[k]) for k in range(2))

    assert intact()
    # the failing calls
    big = np.zeros((n, _lib.SPECTRA_MAX_FREQ + 1, 2))
    for rc, args in ((-1, (_lib.SPECTRA_MAX_FREQ + 1, 3, EVERY, n, big, big)), (-1, (-1, 3, EVERY, n, wu, ws)),
                     (-1, (3, 3, 0, n, wu, ws)), (-1, (3, 0, EVERY, n, wu, ws)), (-1, (3, 4, EVERY, n, wu, ws)),
                     (-1, (3, 3, EVERY, n, wu, None)), (-1, (3, 3, EVERY, n, None, ws)), (-1, (3, 1, EVERY, n, None, ws)),
                     (-1, (3, 3, EVERY, 0, wu, ws)),
                     # out of memory: a weight table of 2^32 samples x 8 frequencies is 512 GiB, refused before anything is read
                     (-4, (_lib.SPECTRA_MAX_FREQ, 3, EVERY, 2 ** 32, big, big))):
        assert _raw_set(blk, *args) == rc, args[:4]
        assert blk.lib.sg_last_error(blk.h)
        assert intact(), args[:4]
    # the read-out's refusals
    assert blk.lib.sg_get_spectrum(blk.h, 0, 0, 0, bu.ctypes.data, bu.nbytes - 8) == -1
    assert blk.lib.sg_get_spectrum(blk.h, 0, 0, 0, bs.ctypes.data, bs.nbytes) == -1
    assert blk.lib.sg_get_spectrum(blk.h, 0, 3, 0, bu.ctypes.data, bu.nbytes) == -1
    assert blk.lib.sg_get_spectrum(blk.h, 0, -1, 0, bu.ctypes.data, bu.nbytes) == -1
    assert blk.lib.sg_get_spectrum(blk.h, 0, 0, 2, bu.ctypes.data, bu.nbytes) == -1
    assert blk.lib.sg_get_spectrum(blk.h, 2, 0, 0, bu.ctypes.data, bu.nbytes) == -1
    assert blk.lib.sg_get_spectrum(blk.h, 0, 0, 0, None, bu.nbytes) == -1
    assert not bu.any() and not bs.any() and intact()
    # re-arming zeroes the accumulators and restarts the count; the velocity alone: the stress is not selected
    blk.set_spectra(wu, None, EVERY)
    assert blk.spectra_samples() == 0
    assert not any(blk.get_spectrum(0, f).any() for f in range(3))
    assert blk.lib.sg_get_spectrum(blk.h, 1, 0, 0, bs.ctypes.data, bs.nbytes) == -3
    blk.step(EVERY)
    assert blk.spectra_samples() == 1 and blk.get_spectrum(0, 1).any()
    # nfreq = 0 disarms
    blk.set_spectra(None, None)
    assert blk.lib.sg_get_spectrum(blk.h, 0, 0, 0, bu.ctypes.data, bu.nbytes) == -3 and blk.spectra_samples() == 0
    blk.step(2)
    blk.close()


@pytest.mark.parametrize("name", ["tile-tri-P3", "mfma-P4-sym"])
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_a_sample_excludes_the_injectors_entry_of_its_step(gpu, monkeypatch, name, graph):
    """Injectors armed beside the spectra, a sample after every step with the weights (1, 0): the accumulator is the sum, bit
    for bit, of what a twin driven by stages holds BEFORE sg_end_step adds the step's entry - and not of what it holds after."""
    row = BY_NAME[name]
    _, dim, degree, n, diagonal, dtype, path = row
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
    ones = np.zeros((K, 1, 2))
    ones[..., 0] = 1.0
    for x in (blk, twin):
        assert x.set_injectors(pts, series, 3).all()
    blk.set_spectra(ones, ones, 1)
    blk.step(K)
    before, after = [np.zeros(blk.field_shape(f)) for f in FIELDS], [np.zeros(blk.field_shape(f)) for f in FIELDS]
    for _ in range(K):
        for st in range(6):
            twin.run_stage(st)
        for k, f in enumerate(FIELDS):
            before[k] = before[k] + twin.get_field(f)
        twin.end_step()
        for k, f in enumerate(FIELDS):
            after[k] = after[k] + twin.get_field(f)
    for k in range(2):
        got = blk.get_spectrum(k, 0)
        assert np.array_equal(got.real, before[k]) and not got.imag.any(), (name, k)
        assert np.abs(after[k] - before[k]).max() > 1e-3 * np.abs(before[k]).max(), "the entries must show"
    ua, sa = _fields(blk)
    ub, sb = _fields(twin)
    assert np.array_equal(ua, ub) and np.array_equal(sa, sb)
    blk.close()
    twin.close()


# ---- 6. a split block ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fake():
    from fake_rccl.build import build
    return build()


def test_spectra_on_a_split_block(gpu, fake, tmp_path):
    """Two ranks over the transport double, the exchange inside the library, ONE sg_step(n) with a source and a sponge: every
    rank's spectra equal the single block's cells bit for bit."""
    from native_exchange_worker import setup_block
    from spectra_exchange_worker import spectra_of, weights_of, EVERY as W_EVERY
    grid, n, degree, steps, world = (1, 1, 2), (16, 4, 4), 4, 6, 2
    env = dict(os.environ, SEIGEN_RCCL_LIB=fake, FAKE_RCCL_TIMEOUT_S="60", FAKE_RCCL_LOG=str(tmp_path / "fake"),
               HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2", FAKE_RCCL_ASYNC="1", FAKE_RCCL_SLOT_BYTES="1048576")
    env.pop("FAKE_RCCL_HOST", None)
    for var in SWITCHES:
        env.pop(var, None)
    logs = [open(tmp_path / ("rank%d.log" % r), "w") for r in range(world)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "spectra_exchange_worker.py"), str(tmp_path), str(world),
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
    dt = setup_block(blk, n, degree, "source")
    wu, ws = weights_of(dt, steps)
    blk.set_spectra(wu, ws, W_EVERY)
    blk.step(steps)
    whole = spectra_of(blk)
    blk.close()
    assert np.abs(whole["u"]).max() > 0 and np.abs(whole["s"]).max() > 0
    seen = np.zeros(whole["u"].shape[1], dtype=int)
    for r in range(world):
        d = np.load(tmp_path / ("rank%d.npz" % r))
        assert int(d["steps"]) == steps and int(d["samples"]) == steps // W_EVERY
        seen[d["cells"]] += 1
        assert np.array_equal(d["u"], whole["u"][:, d["cells"]]) and np.array_equal(d["s"], whole["s"][:, d["cells"]]), "rank %d" % r
    assert np.all(seen == 1)


# ---- 7. sg_correlate_spectra -------------------------------------------------------------------------------------------------

def _host_correlation(geo, A, fa, B, fb, w, z):
    """w_k |det J| Re(z conj(A_fa) . B_fb)_k per cell from Geometry.forms of the real and imaginary parts"""
    (au, as_), (bu, bs) = A, B
    ar, ai = (au[fa].real, as_[fa].real), (au[fa].imag, as_[fa].imag)
    br, bi = (bu[fb].real, bs[fb].real), (bu[fb].imag, bs[fb].imag)
    z = complex(z)
    out = z.real * (geo.forms(ar, br) + geo.forms(ai, bi)) - z.imag * geo.forms(ar, bi) + z.imag * geo.forms(ai, br)
    return np.asarray(w)[None, :] * out


def _scale(row, A, fa, B, fb, w, z):
    """the scale of tests/test_correlate_gpu.py (host_forms of the absolute values), summed over the launches"""
    from tests.test_correlate_gpu import host_forms
    (au, as_), (bu, bs) = A, B
    z = complex(z)
    S = 0.0
    for pa, pb, zw in ((np.real, np.real, z.real), (np.imag, np.imag, z.real), (np.real, np.imag, z.imag), (np.imag, np.real, z.imag)):
        S = S + abs(zw) * host_forms(row, (pa(au[fa]), pa(as_[fa])), (pb(bu[fb]), pb(bs[fb])))[1]
    return np.abs(np.asarray(w))[None, :] * S


@pytest.mark.parametrize("name", ["mfma-P4-sym", "tile-tri-P3", "mfma-P3-f32"])
def test_correlate_spectra_against_the_host_s_forms(gpu, monkeypatch, name):
    """Two handles with different fields, both armed: the calls with z = 1 (two launches), a complex z and two different
    frequencies (four), then sg_correlate of the fields themselves, all into one accumulator, against Geometry.forms of the
    downloaded spectra within the bound of tests/test_correlate_gpu.py; reset zeroes it."""
    from tests.test_correlate_gpu import BOUND, host_forms
    row = BY_NAME[name]
    _, dim, degree, n, diagonal, dtype, path = row
    K = _steps(dim)
    a, dt = _block(row, monkeypatch, seed=11)
    b, _ = _block(row, monkeypatch, seed=5)
    wu, ws = _weights(dt, K)
    for x in (a, b):
        x.set_spectra(wu, ws, EVERY)
        x.step(K)
    geo = gl.Geometry(dim, degree, n, diagonal)
    A, B = _spectra(a), _spectra(b)
    buf = np.zeros((a.ncells, 3))
    assert a.lib.sg_get_correlation(a.h, buf.ctypes.data, buf.nbytes) == -3
    W = np.array([0.7, -1.3, 2.1])
    calls = [(1, 1, W, 1.0), (1, 2, np.array([1.0, 0.5, -2.0]), 0.3 - 0.8j), (2, 2, W, 1j), (0, 0, None, 1.0)]
    want, scale = np.zeros((a.ncells, 3)), np.zeros((a.ncells, 3))
    for fa, fb, w, z in calls:
        a.correlate_spectra(b, fa, fb, w, z)
        w1 = np.ones(3) if w is None else w
        want += _host_correlation(geo, A, fa, B, fb, w1, z)
        scale += _scale(row, A, fa, B, fb, w1, z)
    got = a.get_correlation()
    err = np.abs(got - want) / np.maximum(scale, 1e-300)
    print("correlate_spectra %s: largest |device - host| / scale per entry %s (bound %.1e); max |acc| / scale %s"
          % (name, err.max(axis=0), BOUND, (np.abs(want) / np.maximum(scale, 1e-300)).max(axis=0)))
    assert np.isfinite(got).all() and np.all(scale.max(axis=0) > 0) and np.abs(want).max() > 0
    assert np.all(np.abs(got - want) <= BOUND * scale), (name, err.max())
    # z = NULL is z = (1, 0)
    a.reset_correlation()
    a.correlate_spectra(b, 1, 2, W, 1.0)
    first = a.get_correlation()
    a.reset_correlation()
    _lib.check(a.lib.sg_correlate_spectra(a.h, 1, b.h, 2, W.ctypes.data, None), a.h)
    assert np.array_equal(first, a.get_correlation()) and first.any()
    # the accumulator is sg_correlate's: the fields' own correlation adds to it
    fa_, fb_ = _fields(a), _fields(b)
    a.correlate(b, W)
    B1, S1 = host_forms(row, fa_, fb_)
    w12 = _host_correlation(geo, A, 1, B, 2, W, 1.0)
    s12 = _scale(row, A, 1, B, 2, W, 1.0)
    both = a.get_correlation()
    assert np.all(np.abs(both - (w12 + W * B1)) <= BOUND * (s12 + np.abs(W) * S1))
    assert np.abs(both - first).max() > 0
    a.reset_correlation()
    assert not a.get_correlation().any()
    # b = a
    a.correlate_spectra(a, 1, 1, W, 1.0)
    own = _host_correlation(geo, A, 1, A, 1, W, 1.0)
    assert np.all(np.abs(a.get_correlation() - own) <= BOUND * _scale(row, A, 1, A, 1, W, 1.0))
    # refusals leave the accumulator alone
    keep = a.get_correlation()
    assert a.lib.sg_correlate_spectra(a.h, 3, b.h, 0, W.ctypes.data, None) == -1
    assert a.lib.sg_correlate_spectra(a.h, 0, b.h, -1, W.ctypes.data, None) == -1
    assert a.lib.sg_correlate_spectra(a.h, 0, None, 0, W.ctypes.data, None) == -1
    assert np.array_equal(a.get_correlation(), keep)
    a.close()
    b.close()


def test_correlate_spectra_needs_the_fields_a_weight_asks_for(gpu, monkeypatch):
    """a has armed the stress alone, b both fields: a weight on uu is refused (SG_ERR_STATE, no accumulator yet), the
    weights (0, ws, wt) give ss and tt and exactly nothing in uu; b against b with (wu, 0, 0) gives uu alone; a handle
    with nothing armed is refused."""
    from tests.test_correlate_gpu import BOUND
    row = BY_NAME["tile-tri-P3"]
    _, dim, degree, n, diagonal, dtype, path = row
    K = _steps(dim)
    a, dt = _block(row, monkeypatch, seed=11)
    b, _ = _block(row, monkeypatch, seed=5)
    c, _ = _block(row, monkeypatch, seed=7)
    wu, ws = _weights(dt, K)
    a.set_spectra(None, ws, EVERY)
    b.set_spectra(wu, ws, EVERY)
    for x in (a, b):
        x.step(K)
    geo = gl.Geometry(dim, degree, n, diagonal)
    W = np.array([0.7, -1.3, 2.1])
    buf = np.zeros((a.ncells, 3))
    for first, second in ((a, b), (b, a), (a, c), (c, a)):
        assert first.lib.sg_correlate_spectra(first.h, 1, second.h, 1, W.ctypes.data, None) == -3
        assert first.lib.sg_get_correlation(first.h, buf.ctypes.data, buf.nbytes) == -3
    zero_u = np.zeros((3,) + a.field_shape(_lib.FIELD_U), dtype=complex)
    A, B = (zero_u, _spectra(a, fields=(1,))[0]), _spectra(b)
    w0 = np.array([0.0, -1.3, 2.1])
    a.correlate_spectra(b, 1, 2, w0, 0.3 - 0.8j)
    got = a.get_correlation()
    assert not got[:, 0].any() and got[:, 1].any() and got[:, 2].any()
    assert np.all(np.abs(got - _host_correlation(geo, A, 1, B, 2, w0, 0.3 - 0.8j)) <= BOUND * _scale(row, A, 1, B, 2, w0, 0.3 - 0.8j))
    w1 = np.array([0.7, 0.0, 0.0])
    b.correlate_spectra(b, 1, 2, w1, 1j)
    got = b.get_correlation()
    assert got[:, 0].any() and not got[:, 1].any() and not got[:, 2].any()
    assert np.all(np.abs(got - _host_correlation(geo, B, 1, B, 2, w1, 1j)) <= BOUND * _scale(row, B, 1, B, 2, w1, 1j))
    for x in (a, b, c):
        x.close()


# ---- the solver class ------------------------------------------------------------------------------------------------------

def test_solver_class_on_the_eigenmode(gpu, monkeypatch):
    """Two ElasticLF4 on the reference's 2-D eigenmode (N = 8, P2), the second started at another phase: set_spectra, run,
    spectrum and correlate_spectra against numpy's transform of a twin's downloaded fields with the weights of
    spectra_weights (stagger dt / 2 for the stress) and the host's forms of the spectra."""
    from seigen_amd import Function
    from seigen_amd.harness.eigenmode import Eigenmode2DLF4
    from tests.test_correlate_gpu import BOUND
    _env(monkeypatch, None)
    N, P, dt, K, every = 8, 2, 0.25 / 8, 12, 3
    freqs = [0.0, 0.7, 2.0]
    row = ("eigenmode", 2, P, (N, N), "left")
    ems = [Eigenmode2DLF4(N, P, dt, output=False) for _ in range(3)]
    for em, t0 in zip(ems, (0.0, 0.4, 0.0)):
        el = em.elastic
        el.u0.assign(Function(el.U).interpolate(em._u(t0)))
        el.s0.assign(Function(el.S).interpolate(em._s(t0 + dt / 2.0)))
    fwd, adj, twin = (em.elastic for em in ems)
    with pytest.raises(RuntimeError):
        fwd.spectrum("velocity", 0.7)
    with pytest.raises(ValueError):
        fwd.set_spectra(np.arange(9.0))
    for el in (fwd, adj):
        el.set_spectra(freqs, every=every)
        el.run(K * dt * (1 + 1e-9))
        assert el.block.counters()["steps"] == K and el.block.spectra_samples() == K // every
    twin.setup()
    su, ss = _twin_samples(twin.block, K, every)
    wu = spectra_weights(freqs, dt, every, K // every)
    ws = spectra_weights(freqs, dt, every, K // every, stagger=0.5 * dt)
    gu = np.array([fwd.spectrum("velocity", f) for f in freqs])
    gs = np.array([fwd.spectrum("stress", f) for f in freqs])
    assert gu.shape[1:] == fwd.u1.dat.data.shape and gs.shape[1:] == fwd.s1.dat.data.shape
    _check_transform("eigenmode velocity", gu.reshape((3,) + su.shape[1:]), su, wu)
    _check_transform("eigenmode stress", gs.reshape((3,) + ss.shape[1:]), ss, ws)
    with pytest.raises(ValueError):
        fwd.spectrum("velocity", 0.5)
    geo = gl.Geometry(2, P, (N, N), "left")
    A, B = _spectra(adj.block), _spectra(fwd.block)
    adj.correlate_spectra(fwd, 0.7, weights=(1.0, 0.5, -2.0))
    adj.correlate_spectra(fwd, 2.0, 0.7, z=0.3 - 0.8j)
    want = _host_correlation(geo, A, 1, B, 1, (1.0, 0.5, -2.0), 1.0) + _host_correlation(geo, A, 2, B, 1, np.ones(3), 0.3 - 0.8j)
    scale = _scale(row, A, 1, B, 1, (1.0, 0.5, -2.0), 1.0) + _scale(row, A, 2, B, 1, np.ones(3), 0.3 - 0.8j)
    corr = adj.correlation()
    got = np.stack([corr["uu"], corr["ss"], corr["tt"]], axis=-1)
    assert np.abs(want).max() > 0 and np.all(np.abs(got - want) <= BOUND * scale)
    # no frequencies: the next run disarms
    fwd.set_spectra(None)
    fwd.run(2 * dt * (1 + 1e-9))
    with pytest.raises(RuntimeError):
        fwd.spectrum("velocity", 0.7)
    assert fwd.block.spectra_samples() == 0
