"""Device transfers on the GPU (include/seigen_hip.h sg_get_field_dev / sg_set_field_dev / sg_get_spectrum_dev;
seigen_amd/csrc/kernels_xfer.hip): fields and spectra between a handle and torch tensors on its device.

Everything here is data movement and is compared BITWISE; the yardstick is the existing host path - sg_set_field*, sg_get_field*,
sg_get_spectrum - never the new calls against themselves.  ROWS: the nine rows of tests/gradient_loop.py (one group with
padding lanes each; every family, f32, symmetric storage) and four rows of several groups with a partial last one, among them
the hexahedral DQ_2 item of 243 x 64 words on the lane family, which the plan must slice.

1 get, 2 set, 3 ranges: test_get_set_and_ranges.  4 the field has really been written (write counts, sponge pre-pass):
test_set_is_seen_by_the_next_steps and test_asymmetric_stress_then_steps.  5 queued-only ordering on a torch stream.
6 hand-over of a state from handle A to handle B.  7 spectra.  8 the Python layer."""
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
from tests import gradient_loop as gl  # noqa: E402

SWITCHES = ("SEIGEN_HIP_PATH", "SEIGEN_HIP_GRAPH", "SEIGEN_HIP_SPONGE_AFFINE", "SEIGEN_HIP_SYM", "SEIGEN_HIP_SOURCE_LAUNCH",
            "SEIGEN_HIP_XCORR", "SEIGEN_HIP_OVERLAP", "SEIGEN_HIP_PLAIN_COPY")
# (name, dim, degree, cubes, diagonal, dtype, SEIGEN_HIP_PATH)
GROUP_ROWS = [
    ("mfma-P4-groups", 3, 4, (5, 3, 3), "left", "f64", None),                 # 45 cubes: 3 groups of 16
    ("lane-2d-P2-groups", 2, 2, (9, 8), "left", "f64", "lane"),               # 72 cubes: 2 groups of 64
    ("tile-tri-P3-f32-groups", 2, 3, (7, 5), "left", "f32", None),            # 35 cubes: 3 groups of 16
    ("hex-DQ2-lane", 3, 2, (5, 4, 4), "quadrilateral", "f64", "lane"),        # 80 cubes: 2 groups of 64, 243 rows: sliced
]
ROWS = list(gl.ROWS) + GROUP_ROWS
ROW = {r[0]: r for r in ROWS}
IDS = [r[0] for r in ROWS]
FIELDS = (_lib.FIELD_U, _lib.FIELD_S, _lib.FIELD_UH, _lib.FIELD_SH)
STRESS = (_lib.FIELD_S, _lib.FIELD_SH)
STAGES = (_lib.STAGE_UH1, _lib.STAGE_STEMP, _lib.STAGE_U1, _lib.STAGE_SH1, _lib.STAGE_UTEMP, _lib.STAGE_S1)
GUARD = 64


def _torch():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no GPU")
    return torch


def _env(monkeypatch, row, graph=None):
    for var in SWITCHES:
        monkeypatch.delenv(var, raising=False)
    if row[6]:
        monkeypatch.setenv("SEIGEN_HIP_PATH", row[6])
    if graph is not None:
        monkeypatch.setenv("SEIGEN_HIP_GRAPH", graph)


def _block(row, stream=None):
    name, dim, degree, n, diagonal, dtype, path = row
    blk = HipBlock(dim, degree, n, [1.0 / k for k in n], [0.0] * dim, diagonal, stream=stream, dtype=dtype)
    blk.set_params(1.0, 0.1 * min(1.0 / k for k in n) / degree ** 2, 0.5, 0.25)
    return blk


def _interleaved(row):
    return row[6] != "generic"


def _random(blk, field, rng, sym=True):
    x = rng.uniform(-1, 1, blk.field_shape(field))
    if field in STRESS and sym:
        x = 0.5 * (x + np.swapaxes(x, -1, -2))
    return x


def _guarded(torch, shape, dtype):
    """a tensor of `shape` inside an allocation with GUARD words of a pattern in front and behind: (tensor, check)"""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), -7.25, dtype=dtype, device="cuda")
    t = whole[GUARD:GUARD + n].view(shape)

    def intact():
        g = torch.cat([whole[:GUARD], whole[GUARD + n:]]).cpu().numpy()
        return bool((g == -7.25).all())
    return t, intact


def _ranges(blk, gw):
    """(cell0, ncells): start and end inside a cube; across the first group boundary where the block has one"""
    ncls, n = blk.ncls, blk.ncells
    r = [(1, min(n - 2, 2 * ncls + 1)), (n - ncls - 1, ncls + 1)]
    if gw > 1 and n > gw * ncls + ncls + 2:
        r.append((gw * ncls - ncls - 1, 2 * ncls + 3))
    return [(c0, k) for c0, k in r if c0 >= 0 and k > 0 and c0 + k <= n]


def _gw(row):
    if row[6] == "generic":
        return 1
    return 64 if row[6] == "lane" else 16


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_get_set_and_ranges(gpu, monkeypatch, row):
    """1, 2 and 3 of the module's docstring on one block of the row"""
    torch = _torch()
    _env(monkeypatch, row)
    rng = np.random.default_rng(5)
    blk = _block(row)
    lib = blk.lib
    f32_block = row[5] == "f32"
    try:
        assert blk.is_sym() == _interleaved(row)
        # ---- 1. get: all four fields uploaded through sg_set_field, then again after two steps, when the (i > j) lines of a
        # block in symmetric storage are stale and the mirrors must be delivered
        for f in FIELDS:
            blk.set_field(f, _random(blk, f, rng))
        for state in ("uploaded", "stepped"):
            assert blk.is_sym() == _interleaved(row)
            for f in FIELDS:
                want = blk.get_field(f)
                t, intact = _guarded(torch, want.shape, torch.float64)
                assert blk.get_field_dev(f, out=t) is t
                assert np.array_equal(t.cpu().numpy(), want), (state, f)
                assert intact()
                t32, intact32 = _guarded(torch, want.shape, torch.float32)
                blk.get_field_dev(f, out=t32)
                assert np.array_equal(t32.cpu().numpy(), want.astype(np.float32)), (state, f, "float")
                assert intact32()
                # 3. ranges
                for c0, k in _ranges(blk, _gw(row)):
                    tr, intact_r = _guarded(torch, (k,) + want.shape[1:], torch.float64)
                    blk.get_field_dev(f, out=tr, cell0=c0, ncells=k)
                    assert np.array_equal(tr.cpu().numpy(), want[c0:c0 + k]), (state, f, c0, k)
                    assert intact_r()
            blk.step(2)
        # ---- 2. set, against what sg_set_field makes of the same doubles
        for f in FIELDS:
            x = _random(blk, f, rng)
            for tensor_dtype in (torch.float64, torch.float32):
                xs = x if tensor_dtype == torch.float64 else x.astype(np.float32).astype(np.float64)
                blk.set_field(f, xs)
                want = blk.get_field(f)
                if not f32_block:
                    assert np.array_equal(want, xs)
                blk.set_field(f, np.zeros_like(x))
                t = torch.from_numpy(xs).to("cuda", dtype=tensor_dtype)
                assert np.array_equal(t.cpu().numpy().astype(np.float64), xs)
                blk.set_field_dev(f, t)
                assert np.array_equal(blk.get_field(f), want), (f, tensor_dtype)
                assert blk.is_sym() == _interleaved(row)
            # 3. ranges: the cells outside keep their old bits
            for c0, k in _ranges(blk, _gw(row)):
                old = blk.get_field(f)
                new = _random(blk, f, rng)[c0:c0 + k]
                blk.set_field_range(f, c0, new)
                twin = blk.get_field(f)
                assert np.array_equal(twin[:c0], old[:c0]) and np.array_equal(twin[c0 + k:], old[c0 + k:])
                blk.set_field(f, old)
                blk.set_field_dev(f, torch.from_numpy(np.ascontiguousarray(new)).cuda(), cell0=c0)
                assert np.array_equal(blk.get_field(f), twin), (f, c0, k)
            # a tensor of another size: SG_ERR_ARG, nothing changes
            old = blk.get_field(f)
            t = torch.from_numpy(_random(blk, f, rng)).cuda()
            nbytes = t.numel() * 8
            for bad in (nbytes - 8, nbytes + 8, nbytes // 2):
                assert lib.sg_set_field_dev(blk.h, f, 0, blk.ncells, C.c_void_p(t.data_ptr()), 0, bad) == -1
                assert lib.sg_get_field_dev(blk.h, f, 0, blk.ncells, C.c_void_p(t.data_ptr()), 0, bad) == -1
            assert lib.sg_set_field_dev(blk.h, f, 0, blk.ncells, C.c_void_p(t.data_ptr()), 1, nbytes) == -1
            assert lib.sg_set_field_dev(blk.h, f, 1, blk.ncells, C.c_void_p(t.data_ptr()), 0, nbytes) == -1
            assert lib.sg_set_field_dev(blk.h, f, 0, blk.ncells, C.c_void_p(t.data_ptr()), 2, nbytes) == -1
            assert lib.sg_set_field_dev(blk.h, f, 0, blk.ncells, None, 0, nbytes) == -1
            assert lib.sg_get_field_dev(blk.h, f, 0, blk.ncells, None, 0, nbytes) == -1
            assert np.array_equal(blk.get_field(f), old)
            assert blk.is_sym() == _interleaved(row)
        with pytest.raises(ValueError):
            blk.set_field_dev(_lib.FIELD_U, torch.zeros(blk.field_shape(_lib.FIELD_U), dtype=torch.float16, device="cuda"))
        with pytest.raises(ValueError):
            blk.set_field_dev(_lib.FIELD_U, torch.zeros(blk.field_shape(_lib.FIELD_U), dtype=torch.float64))
        with pytest.raises(ValueError):
            blk.set_field_dev(_lib.FIELD_S, torch.zeros(blk.field_shape(_lib.FIELD_S), dtype=torch.float64, device="cuda").transpose(-1, -2))
        # ---- 2. a stress with one (i, j) != (j, i) word: the block leaves symmetric storage, all d^2 lines are right
        if blk.dim > 1:
            blk.step(1)     # (the (i > j) lines of both stress buffers are stale again)
            keep = blk.get_field(_lib.FIELD_SH)
            x = _random(blk, _lib.FIELD_S, rng)
            x[blk.ncells // 2, blk.nd // 2, 1, 0] += 0.5
            if f32_block:
                x = x.astype(np.float32).astype(np.float64)
            blk.set_field_dev(_lib.FIELD_S, torch.from_numpy(x).cuda())
            assert not blk.is_sym()
            assert np.array_equal(blk.get_field(_lib.FIELD_S), x)
            assert np.array_equal(blk.get_field(_lib.FIELD_SH), keep)     # the other buffer's mirrors were made valid
            t = blk.get_field_dev(_lib.FIELD_S)
            assert np.array_equal(t.cpu().numpy(), x)
    finally:
        blk.close()


# ---- 4. the field has really been written -------------------------------------------------------------------------------------

def _sponge_block(row, stream=None, source_steps=0):
    """a block of the row with smooth fields and a sponge (the set-up of tests/test_receivers_gpu.py make_case), and a
    box-Ricker source for the first `source_steps` steps"""
    name, dim, degree, n, diagonal, dtype, path = row
    blk = _block(row, stream)
    dt = 0.1 * min(1.0 / k for k in n) / degree ** 2
    X = blk.node_coords()
    u = np.stack([np.sin(2 * X[..., 0] + i) * np.cos(X[..., -1] - i) for i in range(dim)], axis=-1)
    s = np.zeros(X.shape[:-1] + (dim, dim))
    for i in range(dim):
        for j in range(dim):
            s[..., i, j] = np.cos(X[..., 0] + 0.5 * (i + j)) * (1 + X[..., -1])
    blk.set_field(_lib.FIELD_U, u)
    blk.set_field(_lib.FIELD_S, s)
    if source_steps:
        blk.set_source_box_ricker([0.3] * dim, [0.6] * dim, 400.0, 3 * dt, dt, dt, source_steps)
    Xq = blk.node_coords(2)
    blk.set_absorption(np.where(Xq[..., 0] >= 0.6, 20.0 + 30.0 * Xq[..., 0], 0.0), 2)
    return blk


PREPASS_ROWS = ("mfma-P4-sym", "hexm-DQ3", "lane-2d-P2")     # the families whose F stages read the sponge from a pre-pass


@pytest.mark.parametrize("graph", ["1", "0"])
@pytest.mark.parametrize("name", PREPASS_ROWS)
def test_set_is_seen_by_the_next_steps(gpu, monkeypatch, name, graph):
    """step 2, set u through the device path, step 2 more: bitwise the twin that got the same values through sg_set_field.
    A write the library did not count would leave the sponge's pre-pass of the old u in place."""
    torch = _torch()
    row = ROW[name]
    _env(monkeypatch, row, graph)
    rng = np.random.default_rng(11)
    out = []
    for device_path in (False, True):
        blk = _sponge_block(row)
        try:
            blk.step(2)
            if not out:
                new = 0.5 * rng.uniform(-1, 1, blk.field_shape(_lib.FIELD_U))
            if device_path:
                blk.set_field_dev(_lib.FIELD_U, torch.from_numpy(new).cuda())
            else:
                blk.set_field(_lib.FIELD_U, new)
            blk.step(2)
            out.append((blk.get_field(_lib.FIELD_U), blk.get_field(_lib.FIELD_S), blk.is_sym()))
        finally:
            blk.close()
    assert out[0][2] and out[1][2]
    assert np.abs(out[0][0] - new).max() > 1e-6          # the steps moved the field
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


@pytest.mark.parametrize("name", ["mfma-P4-sym", "tile-tri-P3", "lane-2d-P2"])
def test_asymmetric_stress_then_steps(gpu, monkeypatch, name):
    """an asymmetric stress through the device path, then two steps, against the twin that got it through sg_set_field"""
    torch = _torch()
    row = ROW[name]
    _env(monkeypatch, row)
    rng = np.random.default_rng(13)
    out = []
    for device_path in (False, True):
        blk = _sponge_block(row)
        try:
            blk.step(2)
            if not out:
                new = rng.uniform(-1, 1, blk.field_shape(_lib.FIELD_S))
            assert blk.is_sym()
            if device_path:
                blk.set_field_dev(_lib.FIELD_S, torch.from_numpy(new).cuda())
            else:
                blk.set_field(_lib.FIELD_S, new)
            assert not blk.is_sym()
            blk.step(2)
            out.append((blk.get_field(_lib.FIELD_U), blk.get_field(_lib.FIELD_S)))
        finally:
            blk.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


# ---- 5. queued-only ordering ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["mfma-P4-sym", "tile-tri-P3-f32", "generic-2d-P2"])
def test_get_is_ordered_on_the_callers_stream(gpu, monkeypatch, name):
    """on a torch stream given as sg_config::stream: six stages, sg_end_step, sg_get_field_dev, a torch operation on the
    tensor on that stream - one synchronisation at the end - equals the sequential path"""
    torch = _torch()
    row = ROW[name]
    _env(monkeypatch, row)
    twin = _sponge_block(row)
    try:
        for st in STAGES:
            twin.run_stage(st)
        twin.end_step()
        want = {f: 2.0 * twin.get_field(f) + 1.0 for f in (_lib.FIELD_U, _lib.FIELD_S)}
    finally:
        twin.close()
    ts = torch.cuda.Stream()
    blk = _sponge_block(row, stream=int(ts.cuda_stream))
    try:
        assert blk.stream_ptr() == int(ts.cuda_stream)
        got = {}
        with torch.cuda.stream(ts):
            outs = {f: torch.empty(blk.field_shape(f), dtype=torch.float64, device="cuda") for f in want}
            for st in STAGES:
                blk.run_stage(st)
            blk.end_step()
            for f in want:
                blk.get_field_dev(f, out=outs[f])
                got[f] = 2.0 * outs[f] + 1.0
        ts.synchronize()
        for f in want:
            assert np.array_equal(got[f].cpu().numpy(), want[f]), f
    finally:
        blk.close()


# ---- 6. hand-over ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("streams", ["own", "two-torch-streams"])
@pytest.mark.parametrize("name", ["mfma-P4-sym", "lane-2d-P2", "mfma-P3-f32"])
def test_hand_over_to_a_second_handle(gpu, monkeypatch, name, streams):
    """A steps 2k, its source running out after k; after k steps its (u, s) go through two tensors into B - the same
    configuration and sponge, no source - which steps k: A and B are bitwise equal"""
    torch = _torch()
    row = ROW[name]
    _env(monkeypatch, row)
    k = 3
    sa = sb = None
    if streams != "own":
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    a = _sponge_block(row, stream=int(sa.cuda_stream) if sa else None, source_steps=k)
    b = _sponge_block(row, stream=int(sb.cuda_stream) if sb else None)
    try:
        a.step(k)
        tdt = torch.float32 if row[5] == "f32" else torch.float64
        u = a.get_field_dev(_lib.FIELD_U, dtype=tdt)
        s = a.get_field_dev(_lib.FIELD_S, dtype=tdt)
        b.set_field_dev(_lib.FIELD_U, u)
        b.set_field_dev(_lib.FIELD_S, s)
        a.step(k)
        b.step(k)
        assert a.is_sym() and b.is_sym()
        for f in (_lib.FIELD_U, _lib.FIELD_S):
            fa, fb = a.get_field(f), b.get_field(f)
            assert np.isfinite(fa).all() and np.abs(fa).max() > 1e-3
            assert np.array_equal(fa, fb), f
    finally:
        a.close()
        b.close()


# ---- 7. spectra -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["mfma-P3-sym", "tile-tri-P3-f32", "generic-2d-P2", "hex-DQ2-lane"])
def test_spectra(gpu, monkeypatch, name):
    torch = _torch()
    row = ROW[name]
    _env(monkeypatch, row)
    rng = np.random.default_rng(17)
    blk = _sponge_block(row)
    try:
        nbytes = {k: int(np.prod(blk.field_shape(f))) * 8 for k, f in ((0, _lib.FIELD_U), (1, _lib.FIELD_S))}
        buf = torch.zeros(blk.field_shape(_lib.FIELD_S), dtype=torch.float64, device="cuda")
        for k in (0, 1):
            assert blk.lib.sg_get_spectrum_dev(blk.h, k, 0, 0, C.c_void_p(buf.data_ptr()), 0, nbytes[k]) == -3     # SG_ERR_STATE
        nsamples, nfreq = 4, 2
        w = rng.uniform(-1, 1, (2, nsamples, nfreq)) + 1j * rng.uniform(-1, 1, (2, nsamples, nfreq))
        blk.set_spectra(w[0], w[1])
        blk.step(nsamples)
        for state in ("symmetric", "full"):
            assert blk.is_sym() == (state == "symmetric" and _interleaved(row))
            for k in (0, 1):
                for fr in range(nfreq):
                    want = blk.get_spectrum(k, fr)
                    got = blk.get_spectrum_dev(k, fr)
                    assert got.dtype == torch.complex128 and np.abs(want).max() > 0
                    assert np.array_equal(got.cpu().numpy(), want), (state, k, fr)
                    # into a float buffer: one rounding of each part
                    t32 = torch.empty(want.shape, dtype=torch.float32, device="cuda")
                    assert blk.lib.sg_get_spectrum_dev(blk.h, k, fr, 1, C.c_void_p(t32.data_ptr()), 1, nbytes[k] // 2) == 0
                    blk.sync()
                    assert np.array_equal(t32.cpu().numpy(), want.imag.astype(np.float32))
                assert blk.lib.sg_get_spectrum_dev(blk.h, k, nfreq, 0, C.c_void_p(buf.data_ptr()), 0, nbytes[k]) == -1
                assert blk.lib.sg_get_spectrum_dev(blk.h, k, 0, 2, C.c_void_p(buf.data_ptr()), 0, nbytes[k]) == -1
                assert blk.lib.sg_get_spectrum_dev(blk.h, k, 0, 0, C.c_void_p(buf.data_ptr()), 0, nbytes[k] - 8) == -1
            blk.leave_sym()
    finally:
        blk.close()


# ---- 8. the Python layer --------------------------------------------------------------------------------------------------------

def test_functions_and_spectrum_torch(gpu, monkeypatch):
    torch = _torch()
    import seigen_amd
    import seigen_amd.helpers as helpers
    from seigen_amd import ElasticLF4, RectangleMesh
    from seigen_amd.functionspace import Function
    row = ROW["tile-tri-P3"]
    _env(monkeypatch, row)
    monkeypatch.setattr(helpers, "log", lambda s: None)
    monkeypatch.setattr(seigen_amd.elastic, "log", lambda s: None)
    mesh = RectangleMesh(5, 3, 1.0, 1.0, diagonal="left")
    el = ElasticLF4.create(mesh, "DG", 3, dimension=2, solver="explicit", output=False)
    el.l, el.mu, el.density = 0.5, 0.25, 1.0
    el.dt = 1e-3
    rng = np.random.default_rng(19)
    blk = el.block
    u = rng.uniform(-1, 1, blk.field_shape(_lib.FIELD_U))
    s = rng.uniform(-1, 1, blk.field_shape(_lib.FIELD_S))
    s = 0.5 * (s + np.swapaxes(s, -1, -2))
    assert el.u0.from_torch(torch.from_numpy(u).cuda()) is el.u0
    el.s0.from_torch(torch.from_numpy(s).cuda())
    assert np.array_equal(blk.get_field(_lib.FIELD_U), u) and np.array_equal(blk.get_field(_lib.FIELD_S), s)
    tu, ts = el.u1.to_torch(), el.s1.to_torch(dtype=torch.float32)
    assert tu.is_cuda and tu.dtype == torch.float64 and np.array_equal(tu.cpu().numpy(), u)
    assert ts.dtype == torch.float32 and np.array_equal(ts.cpu().numpy(), s.astype(np.float32))
    out = torch.empty_like(tu)
    assert el.u1.to_torch(out=out) is out and np.array_equal(out.cpu().numpy(), u)
    free = Function(el.U)
    with pytest.raises(ValueError):
        free.to_torch()
    with pytest.raises(ValueError):
        free.from_torch(tu)
    freqs = [3.0, 7.0]
    el.set_spectra(freqs)
    el.run(6 * el.dt * (1 + 1e-9))
    for field in ("velocity", "stress"):
        for f in freqs:
            want = el.spectrum(field, f)
            got = el.spectrum_torch(field, f)
            assert got.dtype == torch.complex128 and tuple(got.shape) == want.shape and np.abs(want).max() > 0
            assert np.array_equal(got.cpu().numpy(), want)
