"""Handles that launch on a stream of the caller's (sg_config::stream; include/seigen_hip.h), against the oracle and bit
for bit against the same handle on a stream of its own.

Every other module leaves sg_config::stream NULL: the library then makes a non-blocking stream, and destroys it.  Here the
caller makes the stream - a HIP stream with default flags (blocking: it also synchronises with the legacy stream, which the
library's set-up paths use through hipMemset and hipMemcpy), a HIP stream with hipStreamNonBlocking, one of torch's - and
hands it to sg_create.  On it run: the scripted lifetime of tests/lifetime_script.py (graph capture and replay, eager and
timed steps, host-driven stages, uploads, sources, receivers) per kernel family and number type; what that script does not
arm (a monitor, an injector series, sg_inject, sg_measure); teardown, after which the stream is the caller's to use and to
destroy; three handles of different elements on one stream; sg_correlate of two handles on one stream and on two; and the
multi-block exchange of tests/test_harness_gpu.py with every block on one torch stream and no host synchronisation between
pack, copy and stage - the stream alone orders them, and SECOND launches run on the blocks' second streams beside it.

Every test asserts first that the handle reports the caller's stream (sg_get_stream) and that a handle created without one
reports another.  Every comparison is bitwise against that twin and within the suite's bounds against the oracle; no
tolerance is new: tests/test_lifetime_gpu.py's for the lifetime (FP64 max(10 tol_of, 10 x the committed floor), float
5e-5 ceil(k / 3)), 10 tol_of / 5e-5 ceil(k / 3) for whole steps as tests/test_injectors_gpu.py has them,
tests/test_correlate_gpu.py's 1e-11 x scale.

The ordering rule behind all of it: a non-blocking stream - the library's own, torch's - is not ordered against the legacy
stream, a blocking one is.  Two fills broke it and went onto the handle's stream with this module: the zeroing of
sg_correlate's fresh accumulator (hipMemset, then the launch that adds to it) and the fills that end sg_comm_selftest
(they could land on the first traces of the run behind it: tests/test_native_exchange_gpu.py's eight ranks at production
width failed on that now and then, by 1e-4).

Whether graph replay survives on a blocking stream cannot be seen from here: a handle whose capture fails launches the same
kernels one by one, with the same results.

Largest relative error against the oracle on an MI355X (a record, not a bound; the same figure on all three kinds of
stream, as the bitwise comparison with the twin demands):
  lifetime: generic-1d-P2 1.6e-15   lane-2d-P2 4.1e-15   tile-tri-P3 7.3e-15   mfma-P4-sym 6.9e-14   hexm-DQ3 2.0e-14
            mfma-P4-f32 5.9e-7 (FP64 bound 1e-10, float 5e-5 .. 3.5e-4)
  monitor / injectors / sg_measure, 11 steps: mfma-P4-sym 1.2e-14   tile-tri-P3 9.1e-15 (bound 1e-10)   mfma-P4-f32 2.1e-7 (2e-4)
  sg_correlate: mfma-P4-sym 2.3e-16   tile-tri-P3 8.5e-16 of the scale (bound 1e-11)
Seeded in a scratch build: sg_run_stage(SG_REGION_SECOND) without its wait for ev_stage - the second stream then starts
ahead of what the main stream still holds - passes the 32 multi-block rows of tests/test_harness_gpu.py that synchronise the
host after every stage and fails the 3d-P4-pipelined row here (velocity differs from the single block)."""
import contextlib
import ctypes as C
import json
import math

import numpy as np
import pytest

from oracle.lf4 import OracleLF4
from seigen_amd import _lib
from seigen_amd.backend import HipBlock, injector_weights
from tests import lifetime_script as ls
from tests.test_correlate_gpu import BOUND, ROW, W, _other_fields, host_forms
from tests.test_injectors_gpu import _add, _amplitudes
from tests.test_injectors_host import make_cfg
from tests.test_lifetime_gpu import FIELDS, FLOOR_FILE, _environment, compare, moved
from tests.test_parity_gpu import tol_of
from tests.test_receivers_gpu import make_case, receiver_points
from tests.util import oracle_mesh, rel_err

pytestmark = pytest.mark.gpu

KINDS = ("hip-blocking", "hip-nonblocking", "torch")
HIP_STREAM_NON_BLOCKING = 0x01
MW = np.array([0.55, 0.5, -0.1])        # the monitor's weights (wk, ws, wt): without any, EK = ES = 0


def _hip():
    hip = C.CDLL("libamdhip64.so")
    hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    hip.hipStreamQuery.argtypes = [C.c_void_p]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return hip


class CallerStream(object):
    """A stream the test owns.  ptr: the hipStream_t as an integer; torch: the torch.cuda.Stream behind it, or None;
    destroy(): hipStreamDestroy's return value (a torch stream is torch's to destroy: None)."""

    def __init__(self, kind):
        self.kind, self.torch, self.hip = kind, None, _hip()
        if kind == "torch":
            torch = pytest.importorskip("torch")
            if not torch.cuda.is_available():
                pytest.skip("torch sees no GPU")
            self.torch = torch.cuda.Stream()
            self.ptr = int(self.torch.cuda_stream)
        else:
            s = C.c_void_p()
            flags = {"hip-blocking": 0, "hip-nonblocking": HIP_STREAM_NON_BLOCKING}[kind]
            assert self.hip.hipStreamCreateWithFlags(C.byref(s), flags) == 0
            self.ptr = int(s.value)
        assert self.ptr != 0

    def query(self):
        return self.hip.hipStreamQuery(C.c_void_p(self.ptr))

    def destroy(self):
        ptr, self.ptr = self.ptr, 0
        if self.kind == "torch" or not ptr:
            self.torch = None
            return None
        return self.hip.hipStreamDestroy(C.c_void_p(ptr))


@contextlib.contextmanager
def caller_stream(kind):
    s = CallerStream(kind)
    try:
        yield s
    finally:
        s.destroy()


def _on_the_callers_stream(st, *blocks):
    """the handles report the caller's stream; a handle created without one, alive beside them (an address is not handed out
    twice at a time; a destroyed twin's could be), reports another"""
    for blk in blocks:
        assert blk.stream_ptr() == st.ptr
    twin = HipBlock(1, 1, (2,), [0.5], [0.0])
    try:
        assert twin.stream_ptr() not in (0, st.ptr)
    finally:
        twin.close()


# ---- a. a lifetime on a caller's stream ----------------------------------------------------------------------------------

LIFETIME_CASES = ("generic-1d-P2", "lane-2d-P2", "tile-tri-P3", "mfma-P4-sym", "hexm-DQ3", "mfma-P4-f32")
_MIRROR, _TWIN = {}, {}


def _lifetime_block(case, stream=None):
    return HipBlock(case.dim, case.degree, case.n, [1.0 / k for k in case.n], [0.0] * case.dim, case.cell, stream=stream,
                    dtype=case.dtype)


def _mirror(case):
    """(script, the oracle mirror's observations, floor) of a case, once per module"""
    if case.name not in _MIRROR:
        script, want = ls.mirror_run(case)
        floor = None
        if case.dtype == "f64":
            with open(FLOOR_FILE) as f:
                floor = json.load(f)[case.name]
            assert len(floor) == moved(want)
        else:
            moved(want)
        _MIRROR[case.name] = (script, want, floor)
    return _MIRROR[case.name]


def _own_stream_run(case, script):
    """the observations of the script on a handle with a stream of its own, once per module and process"""
    if case.name not in _TWIN:
        twin = _lifetime_block(case)
        try:
            _TWIN[case.name] = ls.run_script(twin, script)
        finally:
            twin.close()
    return _TWIN[case.name]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", LIFETIME_CASES)
def test_a_lifetime_on_a_callers_stream(gpu, monkeypatch, name, kind):
    """The 111 steps of the lifetime script, graph replay on, on a handle created on the caller's stream: every observation
    against the oracle mirror within tests/test_lifetime_gpu.py's bounds, fields and traces bit for bit those of the same
    script on a handle with a stream of its own."""
    case = ls.case_by_name(name)
    script, want, floor = _mirror(case)
    _environment(monkeypatch, case, None)
    own = _own_stream_run(case, script)
    with caller_stream(kind) as st:
        blk = _lifetime_block(case, st.ptr)
        try:
            _on_the_callers_stream(st, blk)
            got = ls.run_script(blk, script)
            assert blk.stream_ptr() == st.ptr
        finally:
            blk.close()
        assert st.query() == 0
    print("LIFETIME-WORST %s %s: %.4f of its bound, %.2e" % ((case.name, kind) + compare(case, kind, got, want, floor)))
    assert len(got) == len(own)
    for a, b in zip(got, own):
        for k in FIELDS + ("traces",):
            if k in b:
                assert np.array_equal(a[k], b[k]), (case.name, kind, b["i"], b["op"], k)


# ---- b. what the lifetime script does not arm: monitor, injector series, sg_inject, sg_measure -------------------------------

ARMED_ROWS = [("mfma-P4-sym", ROW["mfma-P4-sym"]), ("tile-tri-P3", ROW["tile-tri-P3"]), ("mfma-P4-f32", ROW["mfma-P4-f32"])]
ARMED_STEPS = 11
_ARMED = {}


def _spec_env(monkeypatch, spec):
    for var in ls.SWITCHES:
        monkeypatch.delenv(var, raising=False)
    if spec[6]:
        monkeypatch.setenv("SEIGEN_HIP_PATH", spec[6])


def _armed_points(dim, n):
    """an injection point inside a cell of the middle cube, one on a cube face, one next to the first; the receivers"""
    h = [1.0 / k for k in n]
    cube, c = int(np.prod(n)) // 2, []
    for a in range(dim):
        c.append(cube % n[a])
        cube //= n[a]
    p0 = np.array([(c[a] + (0.31, 0.57, 0.23)[a]) * h[a] for a in range(dim)])
    face = p0.copy()
    face[0] = h[0]
    return np.array([p0, face, p0 + 1e-3 * np.array(h)]), receiver_points(dim, n)[0]


def _armed_run(spec, st=None):
    """monitor (every = 1) and a series of four entries armed, sg_inject, step(10), sg_measure, step(1)"""
    name, dim, degree, n, diagonal, dtype, path, sym = spec
    rng = np.random.default_rng(31)
    pts, recv = _armed_points(dim, n)
    # (an injector's weights are Mhat^-1 phi / |det J|, some 1e3 .. 1e4 here: amplitudes that leave the fields at their size)
    series = 1e-3 * _amplitudes(rng, len(pts), dim, sym, (4,))
    shot = 1e-3 * _amplitudes(rng, len(pts), dim, sym)
    blk, dt = make_case(dim, degree, n, diagonal, dtype, sym, stream=st.ptr if st else None)
    out = dict(ptr=blk.stream_ptr(), dt=dt, pts=pts, series=series, shot=shot)
    try:
        if st is not None:
            _on_the_callers_stream(st, blk)
        else:                   # what the oracle starts from and is told: read from the twin before anything is queued
            out["u0"], out["s0"] = blk.get_field(_lib.FIELD_U), blk.get_field(_lib.FIELD_S)
            out["X"], out["Xq"] = blk.node_coords(), blk.node_coords(2)
        blk.set_monitor(1, ARMED_STEPS, MW)
        assert blk.set_receivers(recv, 3, 1, ARMED_STEPS).all()
        assert blk.set_injectors(pts, series, 3).all()
        blk.inject(pts, shot, 3)
        blk.step(10)
        out["measure"] = blk.measure(MW)
        blk.step(1)
        out["monitor"] = blk.get_monitor()
        out["traces"] = blk.get_receivers()
        out["u"], out["s"] = blk.get_field(_lib.FIELD_U), blk.get_field(_lib.FIELD_S)
        assert blk.counters()["steps"] == ARMED_STEPS and blk.stream_ptr() == out["ptr"]
    finally:
        blk.close()
    return out


def _armed_oracle(spec, twin):
    """OracleLF4 told what make_case and _armed_run tell the handle: the box-Ricker source at the nodes of the closed box
    (include/seigen_hip.h sg_set_source_box_ricker), the sponge, the one-shot injection before the first step and entry k of
    the series behind step k + 1"""
    name, dim, degree, n, diagonal, dtype, path, sym = spec
    dt = twin["dt"]
    orc = OracleLF4(oracle_mesh(dim, n, (1.0,) * dim, diagonal), degree)
    orc.dt, orc.l, orc.mu, orc.density = dt, 0.5, 0.25, 1.0
    Xq = twin["Xq"]
    orc.E.set_absorption(np.where(Xq[..., 0] >= 0.6, 20.0 + 30.0 * Xq[..., 0], 0.0).reshape(len(Xq), -1), 2)
    inside = np.all((twin["X"] >= 0.3) & (twin["X"] <= 0.6), axis=-1)
    assert inside.any()
    a, t0 = 400.0, 3 * dt

    def source(t):
        S = np.zeros(inside.shape + (dim, dim))
        w = (-1.0 + 2 * a * (t - t0) ** 2) * math.exp(-a * (t - t0) ** 2)
        for i in range(dim):
            S[..., i, i] = np.where(inside, w, 0.0)
        return S
    orc.source = source
    h = [1.0 / k for k in n]
    cell, psi = injector_weights(make_cfg(dim, degree, n, h, diagonal == "quadrilateral"), twin["pts"], orc.E.nd)
    assert (cell >= 0).all()
    u, s = twin["u0"].copy(), twin["s0"].copy()
    _add(u, s, cell, psi, twin["shot"], dim)
    orc.u0, orc.s0 = u, s
    for step in range(1, ARMED_STEPS + 1):
        orc.step(step * dt)
        if step <= len(twin["series"]):
            u, s = orc.u1.copy(), orc.s1.copy()
            _add(u, s, cell, psi, twin["series"][step - 1], dim)
            orc.u0 = orc.u1 = u
            orc.s0 = orc.s1 = s
    return orc.u1, orc.s1


def _armed_reference(spec):
    """(the twin's run on a stream of its own, the oracle's fields), once per module"""
    if spec[0] not in _ARMED:
        twin = _armed_run(spec)
        _ARMED[spec[0]] = (twin, _armed_oracle(spec, twin))
    return _ARMED[spec[0]]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,spec", ARMED_ROWS, ids=[r[0] for r in ARMED_ROWS])
def test_monitor_injectors_and_measure_on_a_callers_stream(gpu, monkeypatch, name, spec, kind):
    _spec_env(monkeypatch, spec)
    twin, (ou, os_) = _armed_reference(spec)
    with caller_stream(kind) as st:
        got = _armed_run(spec, st)
        assert got["ptr"] == st.ptr
        assert st.query() == 0
    assert got["monitor"].shape == (ARMED_STEPS, 5) and got["monitor"].all()
    assert got["traces"].shape[0] == ARMED_STEPS and np.abs(got["traces"]).max() > 0
    for k in ("monitor", "measure", "u", "s", "traces"):
        assert np.array_equal(got[k], twin[k]), (name, kind, k)
    assert np.array_equal(got["measure"], got["monitor"][9])       # sg_measure behind step 10 is the monitor's sample of it
    bound = 5e-5 * math.ceil(ARMED_STEPS / 3.0) if spec[5] == "f32" else 10 * tol_of(spec[2], spec[4])
    eu, es = rel_err(got["u"], ou), rel_err(got["s"], os_)
    print("CALLER-STREAM-WORST armed %s %s: rel err u %.2e s %.2e (bound %.1e)" % (name, kind, eu, es, bound))
    assert eu < bound and es < bound, (name, kind, eu, es)


# ---- c. teardown and reuse -----------------------------------------------------------------------------------------------

def _three_steps(spec, st=None):
    blk, dt = make_case(*spec[1:6], spec[7], stream=st.ptr if st else None)
    try:
        if st is not None:
            _on_the_callers_stream(st, blk)
        blk.step(3)
        return blk.get_field(_lib.FIELD_U), blk.get_field(_lib.FIELD_S)
    finally:
        blk.close()


@pytest.mark.parametrize("kind", KINDS)
def test_destroy_leaves_the_callers_stream_alive(gpu, monkeypatch, kind):
    """After sg_destroy the stream is idle and alive (hipStreamQuery: hipSuccess).  Only then: the caller's own work runs
    on it, a second handle created on it gives the first one's three steps bit for bit, and the caller destroys it."""
    spec = ROW["tile-tri-P3"]
    _spec_env(monkeypatch, spec)
    tu, ts = _three_steps(spec)
    st = CallerStream(kind)
    try:
        u1, s1 = _three_steps(spec, st)
        assert st.query() == 0, "sg_destroy left the caller's stream busy, or destroyed it"
        hip, buf, host = st.hip, C.c_void_p(), (C.c_ubyte * 256)()
        assert hip.hipMalloc(C.byref(buf), 256) == 0
        try:
            assert hip.hipMemsetAsync(buf, 0x5a, 256, C.c_void_p(st.ptr)) == 0
            assert hip.hipStreamSynchronize(C.c_void_p(st.ptr)) == 0
            assert hip.hipMemcpy(host, buf, 256, 2) == 0 and bytes(host) == b"\x5a" * 256      # 2: device to host
        finally:
            hip.hipFree(buf)
        u2, s2 = _three_steps(spec, st)
        assert st.query() == 0
        assert np.array_equal(u2, u1) and np.array_equal(s2, s1)
        assert np.array_equal(u1, tu) and np.array_equal(s1, ts) and np.abs(u1).max() > 0
    finally:
        rc = st.destroy()
    assert rc == (None if kind == "torch" else 0)


# ---- d. several handles on one stream --------------------------------------------------------------------------------------

SHARED = ("mfma-P4-sym", "tile-tri-P3-f32", "hexm-DQ3")


def _rounds(blocks):
    """step(3) each in turn, twice round; (u, s, monitor samples) per block"""
    for _ in range(2):
        for b in blocks:
            b.step(3)
    return [(b.get_field(_lib.FIELD_U), b.get_field(_lib.FIELD_S), b.get_monitor()) for b in blocks]


def test_three_handles_of_different_elements_on_one_stream(gpu, monkeypatch):
    """Each handle's graphs are captured on the stream the others launch on; each gives what it gives alone."""
    for var in ls.SWITCHES:
        monkeypatch.delenv(var, raising=False)
    alone = []
    for name in SHARED:
        spec = ROW[name]
        blk, _ = make_case(*spec[1:6], spec[7])
        blk.set_monitor(1, 6, MW)
        alone.append(_rounds([blk])[0])
        blk.close()
    with caller_stream("torch") as st:
        blocks = []
        try:
            for name in SHARED:
                spec = ROW[name]
                blk, _ = make_case(*spec[1:6], spec[7], stream=st.ptr)
                blk.set_monitor(1, 6, MW)
                blocks.append(blk)
            _on_the_callers_stream(st, *blocks)
            assert len({blk.stage_kernel_name(0) for blk in blocks}) == 3
            got = _rounds(blocks)
        finally:
            for blk in blocks:
                blk.close()
        assert st.query() == 0
    for name, g, w in zip(SHARED, got, alone):
        assert g[2].shape == (6, 5) and g[2].all(), name
        for k in range(3):
            assert np.array_equal(g[k], w[k]), (name, ("u", "s", "monitor")[k])


# ---- e. sg_correlate across caller streams -------------------------------------------------------------------------------

def _pair(spec, stream_a, stream_b):
    name, dim, degree, n, diagonal, dtype, path, sym = spec
    a, _ = make_case(dim, degree, n, diagonal, dtype, sym, stream=stream_a)
    b, _ = make_case(dim, degree, n, diagonal, dtype, sym, stream=stream_b)
    u, s = _other_fields(b, dim, sym, 5)
    b.set_field(_lib.FIELD_U, u)
    b.set_field(_lib.FIELD_S, s)
    return a, b


def _correlate_twice(a, b, download=False):
    """correlate, two steps of b, correlate; download: b's fields as each call must see them (a synchronising read between
    the calls: the twin's business only)"""
    fields = lambda x: (x.get_field(_lib.FIELD_U), x.get_field(_lib.FIELD_S))      # noqa: E731
    a.step(3)
    seen = [fields(a), fields(b)] if download else None
    a.correlate(b, W)
    b.step(2)
    if download:
        seen.append(fields(b))
    a.correlate(b, W)
    return a.get_correlation(), fields(b), seen


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("streams", ["one-stream", "two-streams"])
@pytest.mark.parametrize("name", ["mfma-P4-sym", "tile-tri-P3"])
def test_correlate_across_caller_streams(gpu, monkeypatch, name, streams, kind):
    """b's stream waits for a's launch and a's for what b had queued (api.cpp sg_correlate): with both handles on one
    caller's stream, and on two.  b's two steps between the calls must reach the second call and not the first."""
    spec = ROW[name]
    _spec_env(monkeypatch, spec)
    ta, tb = _pair(spec, None, None)
    want_acc, want_b, (fa, fb0, fb2) = _correlate_twice(ta, tb, download=True)
    ta.close()
    tb.close()
    with caller_stream(kind) as s1, caller_stream(kind) as s2:
        pa, pb = (s1.ptr, s1.ptr) if streams == "one-stream" else (s1.ptr, s2.ptr)
        a, b = _pair(spec, pa, pb)
        try:
            _on_the_callers_stream(s1, a)
            _on_the_callers_stream(s1 if streams == "one-stream" else s2, b)
            assert s1.ptr != s2.ptr
            got_acc, got_b, _ = _correlate_twice(a, b)
        finally:
            a.close()
            b.close()
        assert s1.query() == 0 and s2.query() == 0
    assert np.array_equal(got_acc, want_acc), (name, streams, kind)
    assert np.array_equal(got_b[0], want_b[0]) and np.array_equal(got_b[1], want_b[1])
    (B0, S0), (B2, S2) = host_forms(spec, fa, fb0), host_forms(spec, fa, fb2)
    want, scale = W * (B0 + B2), np.abs(W) * (S0 + S2)
    assert np.max(np.abs(B2[:, 1] - B0[:, 1]) / S0[:, 1]) > 1e-6, "b's two steps change nothing: the test shows nothing"
    err = np.abs(got_acc - want) / np.maximum(scale, 1e-300)
    print("CALLER-STREAM-WORST correlate %s %s %s: %.2e of scale (bound %.1e)" % (name, streams, kind, err.max(), BOUND))
    assert np.isfinite(got_acc).all() and np.all(np.abs(got_acc - want) <= BOUND * scale), (name, err.max())


# ---- f. stream-ordered exchange with no host synchronisation -----------------------------------------------------------------

EXCHANGE_ROWS = [
    ("3d-P4-pipelined", 3, 4, (4, 2, 4), (2, 1, 2), True, "left"),
    ("2d-P3-pipelined", 2, 3, (10, 9), (1, 3), True, "left"),
    ("hex-DQ3-unpipelined", 3, 3, (4, 2, 3), (2, 1, 3), False, "quadrilateral"),
]


@pytest.mark.parametrize("row", EXCHANGE_ROWS, ids=[r[0] for r in EXCHANGE_ROWS])
def test_exchange_ordered_by_the_callers_stream_alone(gpu, monkeypatch, row):
    """Every block of the grid and the single block on one torch stream; packs, the copies between the blocks and the
    stages are queued without the host waiting in between; a sponge and a source are on.  Bitwise the single block
    (asserted inside _multiblock_case).  The pipelined rows run SECOND on each block's second stream beside the caller's."""
    from tests.test_harness_gpu import _multiblock_case
    name, dim, degree, n, grid, pipelined, diagonal = row
    for var in ls.SWITCHES:
        monkeypatch.delenv(var, raising=False)
    with caller_stream("torch") as st:
        _on_the_callers_stream(st)
        res = _multiblock_case(dim, degree, n, grid, pipelined, extras=True, diagonal=diagonal, stream=st.torch, host_sync=False)
        assert len(res["streams"]) == int(np.prod(grid)) + 1
        assert all(main == st.ptr for main, _ in res["streams"])
        seconds = [second for _, second in res["streams"][:-1]]
        assert all(s not in (0, st.ptr) for s in seconds) and len(set(seconds)) == len(seconds)
        assert res["streams"][-1][1] == 0          # the single block has no neighbours: no second stream
        assert np.abs(res["u"]).max() > 0
