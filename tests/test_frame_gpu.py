"""Frames on the GPU (include/seigen_hip.h sg_get_frame_dev; seigen_amd/csrc/frame.cpp, kernels_frame.hip): a field rastered on
a pixel lattice aligned with the block's cubes, into torch tensors on the block's device.

The yardstick is the host path - sg_get_field and the weights of sg_frame_weights, whose cells tests/test_frame_host.py has
compared with sg_locate_points on the CPU - never the new call against itself.  ROWS: the nine rows of tests/gradient_loop.py
(one group with padding lanes each; every family, f32, symmetric storage) and the four group rows of
tests/test_device_transfer_gpu.py restated (several groups, a partial last one, groups that straddle rows of cubes).

1 value against the host path: test_value_against_the_host_path.  2 the order of the sum, bitwise: test_the_sum_bitwise.
3 families agree.  4 strides: a split block into views of one image, gaps untouched.  5 slices.  6 queued-only ordering on a
torch stream.  7 ElasticLF4.set_frames."""
import ctypes as C
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from seigen_amd import _lib  # noqa: E402
from seigen_amd.backend import HipBlock, make_frame  # noqa: E402
from tests import frame_cases as fc  # noqa: E402
from tests import gradient_loop as gl  # noqa: E402

SWITCHES = ("SEIGEN_HIP_PATH", "SEIGEN_HIP_GRAPH", "SEIGEN_HIP_SPONGE_AFFINE", "SEIGEN_HIP_SYM", "SEIGEN_HIP_SOURCE_LAUNCH",
            "SEIGEN_HIP_XCORR", "SEIGEN_HIP_OVERLAP", "SEIGEN_HIP_PLAIN_COPY")
# (name, dim, degree, cubes, diagonal, dtype, SEIGEN_HIP_PATH): the group rows of tests/test_device_transfer_gpu.py
GROUP_ROWS = [
    ("mfma-P4-groups", 3, 4, (5, 3, 3), "left", "f64", None),                 # 45 cubes: 3 groups of 16
    ("lane-2d-P2-groups", 2, 2, (9, 8), "left", "f64", "lane"),               # 72 cubes: 2 groups of 64
    ("tile-tri-P3-f32-groups", 2, 3, (7, 5), "left", "f32", None),            # 35 cubes: 3 groups of 16
    ("hex-DQ2-lane", 3, 2, (5, 4, 4), "quadrilateral", "f64", "lane"),        # 80 cubes: 2 groups of 64
]
ROWS = list(gl.ROWS) + GROUP_ROWS
ROW = {r[0]: r for r in ROWS}
IDS = [r[0] for r in ROWS]
FIELDS = (_lib.FIELD_U, _lib.FIELD_S)
STAGES = (_lib.STAGE_UH1, _lib.STAGE_STEMP, _lib.STAGE_U1, _lib.STAGE_SH1, _lib.STAGE_UTEMP, _lib.STAGE_S1)
GUARD = 64


def _torch():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no GPU")
    return torch


def _env(monkeypatch, row):
    for var in SWITCHES:
        monkeypatch.delenv(var, raising=False)
    if row[6]:
        monkeypatch.setenv("SEIGEN_HIP_PATH", row[6])


def _block(row, stream=None, n=None, cube0=None, mesh_n=None):
    name, dim, degree, n0, diagonal, dtype, path = row
    n = n0 if n is None else n
    mesh_n = n if mesh_n is None else mesh_n
    blk = HipBlock(dim, degree, n, [1.0 / k for k in mesh_n], [0.0] * dim, diagonal, stream=stream, dtype=dtype, cube0=cube0)
    blk.set_params(1.0, 0.1 * min(1.0 / k for k in mesh_n) / degree ** 2, 0.5, 0.25)
    return blk


def _cfg(row, n=None, cube0=None, mesh_n=None):
    return fc.block_cfg(row[1], row[2], row[3] if n is None else n, row[4], cube0=cube0, mesh_n=mesh_n)


def _gw(row):
    if row[6] == "generic":
        return 1
    return 64 if row[6] == "lane" else 16


def _random(blk, field, rng):
    x = rng.uniform(-1, 1, blk.field_shape(field))
    if field == _lib.FIELD_S:
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


def _squeeze(img, dim, slice):
    """comps + (P2, P1, P0) of frame_cases.host_frame -> the shape of get_frame_dev: axes beyond dim and sliced axes dropped"""
    nv = img.ndim - 3
    drop = tuple(nv + (2 - a) for a in range(3) if a >= dim or (slice and a in slice))
    return img.reshape([s for k, s in enumerate(img.shape) if k not in drop])


def _upload(blk, rng):
    for f in (_lib.FIELD_U, _lib.FIELD_S, _lib.FIELD_UH, _lib.FIELD_SH):
        blk.set_field(f, _random(blk, _lib.FIELD_S if f in (_lib.FIELD_S, _lib.FIELD_SH) else _lib.FIELD_U, rng))


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_value_against_the_host_path(gpu, monkeypatch, row):
    """1: phi[q] @ get_field(f)[cell] on every frame of the host test's list, for u and s, as uploaded and again after two
    steps (the (i > j) lines of symmetric storage stale), within the receivers' tolerance; the guard words intact"""
    torch = _torch()
    _env(monkeypatch, row)
    name, dim, degree, n, diagonal, dtype, path = row
    quad = diagonal == "quadrilateral"
    cfg = _cfg(row)
    rng = np.random.default_rng(23)
    blk = _block(row)
    try:
        _upload(blk, rng)
        for state in ("uploaded", "stepped"):
            assert blk.is_sym() == (path != "generic")
            for f in FIELDS:
                values = blk.get_field(f)
                for m, slice in fc.frames_of(dim, n):
                    want, px = fc.host_frame(cfg, degree, quad, m, slice, values)
                    want = _squeeze(want, dim, slice)
                    scale = np.abs(want).max()
                    tol = (1e-6 if dtype == "f32" else 1e-14) * scale
                    assert tuple(want.shape) == blk.frame_shape(f, m, slice)
                    t, intact = _guarded(torch, want.shape, torch.float64)
                    assert blk.get_frame_dev(f, m=m, slice=slice, out=t) is t
                    got = t.cpu().numpy()
                    err = np.abs(got - want).max()
                    print("%s %s field %d m %r slice %r: err / scale %.3e" % (name, state, f, m, slice, err / scale))
                    assert scale > 0 and err <= tol, (name, state, f, m, slice, err / scale)
                    assert intact()
                    t32, intact32 = _guarded(torch, want.shape, torch.float32)
                    blk.get_frame_dev(f, m=m, slice=slice, out=t32)
                    assert np.array_equal(t32.cpu().numpy(), got.astype(np.float32)), (name, state, f, m, slice)
                    assert intact32()
            blk.step(2)
    finally:
        blk.close()


def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_the_sum_bitwise(gpu, monkeypatch, row):
    """2: on >= 200 pixels (all where there are fewer) - every in-cube pixel, cubes of the first group, of the partial last
    one and of a group that straddles two rows of cubes among them - the double frame is v <- fma(phi[q][a], x[a], v) over a
    ascending from zero, in exact arithmetic rounded once per step, on the downloaded field; the float frame its rounding"""
    torch = _torch()
    _env(monkeypatch, row)
    name, dim, degree, n, diagonal, dtype, path = row
    quad = diagonal == "quadrilateral"
    gw = _gw(row)
    cfg = _cfg(row)
    m = {1: 4, 2: (2, 3), 3: (2, 2, 2)}[dim]
    rng = np.random.default_rng(29)
    blk = _block(row)
    try:
        _upload(blk, rng)
        blk.step(2)
        ncube = int(np.prod(n))
        Q = int(np.prod(m))
        # the cubes: the first group's, the last group's, both sides of the first group boundary and of a row end, then random ones
        pick = [0, 1, ncube - 1, ncube // 2, n[0] - 1, n[0] % ncube, (gw - 1) % ncube, gw % ncube]
        straddlers = [g for g in range(-(-ncube // gw)) if gw > 1 and (g * gw) // n[0] != (min((g + 1) * gw, ncube) - 1) // n[0]]
        if gw > 1:
            assert straddlers, "no group of this row straddles two rows of cubes"
            pick += [straddlers[-1] * gw, min((straddlers[-1] + 1) * gw, ncube) - 1]
        want_cubes = min(ncube, -(-200 // Q))
        pick = sorted(set(pick))
        rest = [c for c in rng.permutation(ncube) if c not in pick]
        pick = sorted(pick + [int(c) for c in rest[:max(0, want_cubes - len(pick))]])
        groups = {c // gw for c in pick}
        assert 0 in groups and (ncube - 1) // gw in groups and (gw == 1 or groups & set(straddlers))
        assert ncube % gw != 0 or gw == 1, "the last group of this row is not a partial one"
        for f in FIELDS:
            values = blk.get_field(f)
            _, px = fc.host_frame(cfg, degree, quad, m, None, values)
            got = blk.get_frame_dev(f, m=m).cpu().numpy()
            got32 = blk.get_frame_dev(f, m=m, dtype=torch.float32).cpu().numpy()
            assert np.array_equal(got32, got.astype(np.float32))
            nv = got.ndim - dim
            got = got.reshape((-1,) + got.shape[nv:])
            v = values.reshape(values.shape[0], values.shape[1], -1)
            sel = np.nonzero(np.isin(px["cube"], pick))[0]
            assert len(sel) >= min(200, ncube * Q) and set(px["q"][sel]) == set(range(Q))
            bad = 0
            for p in sel:
                q, cell = px["q"][p], px["cell"][p]
                idx = tuple(px["index"][p][a] for a in reversed(range(dim)))
                for c in range(v.shape[2]):
                    acc = 0.0
                    for a in range(v.shape[1]):
                        acc = _fma(px["phi"][q, a], v[cell, a, c], acc)
                    bad += acc != got[(c,) + idx]
            assert bad == 0, (name, f, bad, len(sel))
    finally:
        blk.close()


FAMILY_PAIRS = [
    ("tile-lane-2d-P2", (2, 2, (9, 8), "left"), (None, "lane")),
    ("tile-lane-2d-P3", (2, 3, (7, 5), "left"), (None, "lane")),
    ("mfma-generic-3d-P3", (3, 3, (4, 3, 2), "left"), (None, "generic")),
]


@pytest.mark.parametrize("pair", FAMILY_PAIRS, ids=[p[0] for p in FAMILY_PAIRS])
def test_families_agree_bitwise(gpu, monkeypatch, pair):
    """3: the same fields in blocks of two kernel families (layouts gw = 16 / 64 / 1) give bitwise equal frames"""
    torch = _torch()
    name, (dim, degree, n, diagonal), paths = pair
    rng = np.random.default_rng(31)
    fields, out = None, []
    for path in paths:
        row = (name, dim, degree, n, diagonal, "f64", path)
        _env(monkeypatch, row)
        blk = _block(row)
        try:
            if fields is None:
                fields = {f: _random(blk, f, rng) for f in FIELDS}
            for f in FIELDS:
                blk.set_field(f, fields[f])
            frames = []
            for m, slice in fc.frames_of(dim, n):
                for f in FIELDS:
                    frames.append(blk.get_frame_dev(f, m=m, slice=slice).cpu().numpy())
                    frames.append(blk.get_frame_dev(f, m=m, slice=slice, dtype=torch.float32).cpu().numpy())
            out.append((blk.stage_kernel_name(0), frames))
        finally:
            blk.close()
    assert out[0][0] != out[1][0], "both blocks ran the same kernel family"
    assert len(out[0][1]) == len(out[1][1])
    for a, b in zip(out[0][1], out[1][1]):
        assert np.abs(a).max() > 0 and np.array_equal(a, b)


def test_split_block_writes_views_of_one_image(gpu, monkeypatch):
    """4: the four blocks of a 2 x 2 split of the (8, 6) block, holding the fields of the single block's cells, write into views
    of one image: bitwise the single block's frame.  A strided `out` leaves the gaps untouched."""
    torch = _torch()
    row = ("tile-tri-P2", 2, 2, (8, 6), "left", "f64", None)
    _env(monkeypatch, row)
    rng = np.random.default_rng(37)
    m = (2, 3)
    one = _block(row)
    try:
        fields = {f: _random(one, f, rng) for f in FIELDS}
        for f in FIELDS:
            one.set_field(f, fields[f])
        whole = {f: one.get_frame_dev(f, m=m) for f in FIELDS}
        # a strided out: every second row, every third column from the second of a larger buffer
        shape = one.frame_shape(_lib.FIELD_U, m)
        big = torch.full((shape[0], 2 * shape[1], 3 * shape[2] + 1), -7.25, dtype=torch.float64, device="cuda")
        view = big[:, ::2, 1::3]
        assert tuple(view.shape) == shape and not view.is_contiguous()
        one.get_frame_dev(_lib.FIELD_U, m=m, out=view)
        assert np.array_equal(view.cpu().numpy(), whole[_lib.FIELD_U].cpu().numpy())
        mask = torch.ones_like(big, dtype=torch.bool)
        mask[:, ::2, 1::3] = False
        assert bool((big[mask] == -7.25).all())
        # an out whose value axes are not row-major, on the wrong device, of the wrong shape
        with pytest.raises(ValueError):
            one.get_frame_dev(_lib.FIELD_S, m=m, out=torch.empty(one.frame_shape(_lib.FIELD_S, m), dtype=torch.float64, device="cuda").transpose(0, 1))
        with pytest.raises(ValueError):
            one.get_frame_dev(_lib.FIELD_U, m=m, out=torch.empty(shape, dtype=torch.float64))
        with pytest.raises(ValueError):
            one.get_frame_dev(_lib.FIELD_U, m=m, out=torch.empty(shape[:-1] + (shape[-1] + 1,), dtype=torch.float64, device="cuda"))
        # nbytes one element short of the largest index touched: SG_ERR_ARG, nothing written
        t, intact = _guarded(torch, shape, torch.float64)
        t.fill_(-7.25)
        fr = make_frame(2, m)
        assert one.lib.sg_get_frame_dev(one.h, _lib.FIELD_U, C.byref(fr), C.c_void_p(t.data_ptr()), 0, None, t.numel() * 8 - 8) == -1
        stride = (C.c_int64 * 4)(t.stride(0), 0, t.stride(1), t.stride(2) + 1)
        assert one.lib.sg_get_frame_dev(one.h, _lib.FIELD_U, C.byref(fr), C.c_void_p(t.data_ptr()), 0, stride, t.numel() * 8) == -1
        stride = (C.c_int64 * 4)(t.stride(0), 0, t.stride(1), -1)
        assert one.lib.sg_get_frame_dev(one.h, _lib.FIELD_U, C.byref(fr), C.c_void_p(t.data_ptr()), 0, stride, t.numel() * 8) == -1
        one.sync()
        assert bool((t == -7.25).all()) and intact()
    finally:
        one.close()
    image = {f: torch.full(tuple(whole[f].shape), -7.25, dtype=torch.float64, device="cuda") for f in FIELDS}
    for by in range(2):
        for bx in range(2):
            blk = _block(row, n=(4, 3), cube0=(4 * bx, 3 * by), mesh_n=(8, 6))
            try:
                # the single block's cells of this quarter: cube (i, j) of the quarter is cube (4 bx + i, 3 by + j) there
                j, i = np.meshgrid(np.arange(3), np.arange(4), indexing="ij")
                cubes = ((4 * bx + i) + 8 * (3 * by + j)).ravel()
                cells = (cubes[:, None] * blk.ncls + np.arange(blk.ncls)[None, :]).ravel()
                for f in FIELDS:
                    blk.set_field(f, fields[f][cells])
                    view = image[f][..., 3 * by * m[1]:3 * (by + 1) * m[1], 4 * bx * m[0]:4 * (bx + 1) * m[0]]
                    blk.get_frame_dev(f, m=m, out=view)
                blk.sync()
            finally:
                blk.close()
    for f in FIELDS:
        assert np.array_equal(image[f].cpu().numpy(), whole[f].cpu().numpy()), f


def test_slices(gpu, monkeypatch):
    """5: a z slice at the fraction of a volume pixel equals that plane of the volume bitwise (h = 1/2 along z: the fraction
    is exact); the slice on the interior grid plane reads the lower layer; a block that does not hold the layer writes nothing"""
    torch = _torch()
    row = ("mfma-P2", 3, 2, (5, 3, 2), "left", "f64", None)
    _env(monkeypatch, row)
    rng = np.random.default_rng(41)
    cfg = _cfg(row)
    blk = _block(row)
    try:
        fields = {f: _random(blk, f, rng) for f in FIELDS}
        for f in FIELDS:
            blk.set_field(f, fields[f])
        for f in FIELDS:
            vol = blk.get_frame_dev(f, m=(2, 3, 2)).cpu().numpy()
            for layer in range(2):
                for j in range(2):
                    z = (layer + (j + 0.5) / 2) * 0.5
                    got = blk.get_frame_dev(f, m=(2, 3, 5), slice={2: z}).cpu().numpy()
                    assert np.array_equal(got, vol[..., 2 * layer + j, :, :]), (f, layer, j)
            # the grid plane z = 1/2: layer 0 at fraction 1, not layer 1 at fraction 0
            got = blk.get_frame_dev(f, m=(2, 3, 1), slice={2: 0.5}).cpu().numpy()
            values = blk.get_field(f)
            want, px = fc.host_frame(cfg, 2, False, (2, 3, 1), {2: 0.5}, values)
            assert px["plan"]["layer"] == (-1, -1, 0) and px["cube"].max() < 15
            assert np.abs(got - _squeeze(want, 3, {2: 0.5})).max() <= 1e-14 * np.abs(want).max()
            upper = values.copy()
            upper[:15 * 6] = 0.0            # the same field with the lower layer's cells zeroed: another frame altogether
            other, _ = fc.host_frame(cfg, 2, False, (2, 3, 1), {2: 0.5 + 1e-6}, upper)
            assert np.abs(got - _squeeze(other, 3, {2: 0.5})).max() > 1e-3
    finally:
        blk.close()
    # the upper half of a mesh of four layers: a slice through the lower half is another block's
    top = _block(row, n=(5, 3, 2), cube0=(0, 0, 2), mesh_n=(5, 3, 4))
    try:
        top.set_field(_lib.FIELD_U, rng.uniform(-1, 1, top.field_shape(_lib.FIELD_U)))
        t, intact = _guarded(torch, top.frame_shape(_lib.FIELD_U, 2, {2: 0.3}), torch.float64)
        t.fill_(-7.25)
        top.get_frame_dev(_lib.FIELD_U, m=2, slice={2: 0.3}, out=t)
        top.sync()
        assert bool((t == -7.25).all()) and intact()
        top.get_frame_dev(_lib.FIELD_U, m=2, slice={2: 0.8}, out=t)
        top.sync()
        assert not bool((t == -7.25).any()) and intact()
    finally:
        top.close()


def _smooth_block(row, stream=None):
    """a block of the row with smooth fields, a source and a sponge (the set-up of tests/test_device_transfer_gpu.py)"""
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
    blk.set_source_box_ricker([0.3] * dim, [0.6] * dim, 400.0, 3 * dt, dt, dt, 4)
    Xq = blk.node_coords(2)
    blk.set_absorption(np.where(Xq[..., 0] >= 0.6, 20.0 + 30.0 * Xq[..., 0], 0.0), 2)
    return blk


@pytest.mark.parametrize("name", ["mfma-P4-sym", "tile-tri-P3-f32", "generic-2d-P2"])
def test_frame_is_ordered_on_the_callers_stream(gpu, monkeypatch, name):
    """6: on a torch stream given as sg_config::stream: six stages, sg_end_step, sg_get_frame_dev, a torch operation on the
    tensor on that stream - one synchronisation at the end - equals the sequential path; twice, the second time with the
    handle's tables cached"""
    torch = _torch()
    row = ROW[name]
    _env(monkeypatch, row)
    m = {2: (2, 3), 3: (2, 2, 2)}[row[1]]
    twin = _smooth_block(row)
    try:
        want = []
        for rep in range(2):
            for st in STAGES:
                twin.run_stage(st)
            twin.end_step()
            twin.sync()
            want.append({f: 2.0 * twin.get_frame_dev(f, m=m).cpu().numpy() + 1.0 for f in FIELDS})
    finally:
        twin.close()
    ts = torch.cuda.Stream()
    blk = _smooth_block(row, stream=int(ts.cuda_stream))
    try:
        assert blk.stream_ptr() == int(ts.cuda_stream)
        got = []
        with torch.cuda.stream(ts):
            for rep in range(2):
                outs = {f: torch.empty(blk.frame_shape(f, m), dtype=torch.float64, device="cuda") for f in FIELDS}
                for st in STAGES:
                    blk.run_stage(st)
                blk.end_step()
                g = {}
                for f in FIELDS:
                    blk.get_frame_dev(f, m=m, out=outs[f])
                    g[f] = 2.0 * outs[f] + 1.0
                got.append(g)
        ts.synchronize()
        for rep in range(2):
            for f in FIELDS:
                assert np.abs(want[rep][f]).max() > 1 and np.array_equal(got[rep][f].cpu().numpy(), want[rep][f]), (rep, f)
    finally:
        blk.close()


def test_set_frames(gpu, monkeypatch):
    """7: the 2-D explosive-source set-up at (12, 6) P2, every = 3 over 10 steps: run(T) returns bitwise the (u1, s1) and the
    receiver traces of a run without frames; frame j equals Function.frame of a twin advanced (j + 1) * 3 steps; with no
    frames set the launches of run are those of a solver that never heard of frames"""
    torch = _torch()
    import seigen_amd
    import seigen_amd.helpers as helpers
    from seigen_amd.harness.explosive_source import ExplosiveSourceLF4
    for var in SWITCHES:
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setattr(helpers, "log", lambda s: None)
    monkeypatch.setattr(seigen_amd.elastic, "log", lambda s: None)
    monkeypatch.setattr(seigen_amd.harness.explosive_source, "log", lambda s: None)
    dt, steps, every, m = 1e-3, 10, 3, (2, 3)
    recv = ((45.0, 149.0), (90.0, 149.0), (140.0, 149.0))

    def solver():
        # (the L2 projection of the source box: its nodal interpolant is zero on a mesh this coarse)
        el = ExplosiveSourceLF4().setup(h=25.0, degree=2, dt=dt, source_mode="project")
        assert tuple(el.block.n) == (12, 6)
        el.set_receivers(recv, every=1)
        return el

    def state(el):
        return (el.block.get_field(_lib.FIELD_U), el.block.get_field(_lib.FIELD_S), el.receiver_traces()[1]["velocity"],
                list(el.block.counters()["launches"]))

    plain = solver()
    plain.run(steps * dt * (1 + 1e-9))
    want = state(plain)
    assert np.abs(want[0]).max() > 0 and want[2].shape[0] == steps
    for function, func_of in (("velocity", lambda el: el.u1), ("stress", lambda el: el.s1)):
        el = solver()
        el.set_frames(function, m=m, every=every, dtype=torch.float32 if function == "stress" else None)
        with pytest.raises(RuntimeError):
            el.frames()
        u1, s1 = el.run(steps * dt * (1 + 1e-9))
        got = state(el)
        for a, b in zip(want[:3], got[:3]):
            assert np.array_equal(a, b)
        frames = el.frames()
        value = (2,) if function == "velocity" else (2, 2)
        assert tuple(frames.shape) == (steps // every,) + value + (6 * m[1], 12 * m[0])
        assert frames.dtype == (torch.float32 if function == "stress" else torch.float64)
        for j in range(steps // every):
            twin = solver()
            twin.run((j + 1) * every * dt * (1 + 1e-9))
            t = func_of(twin).frame(m=m, dtype=frames.dtype)
            assert np.abs(t.cpu().numpy()).max() > 0
            assert np.array_equal(frames[j].cpu().numpy(), t.cpu().numpy()), (function, j)
        # no frames set any more: today's path, and the launches of a solver that never had any
        el2 = solver()
        el2.set_frames(function, m=m, every=every)
        el2.set_frames(None)
        el2.run(steps * dt * (1 + 1e-9))
        again = state(el2)
        assert again[3] == want[3] and np.array_equal(again[0], want[0]) and np.array_equal(again[1], want[1])
        with pytest.raises(RuntimeError):
            el2.frames()
    with pytest.raises(ValueError):
        plain.set_frames("pressure")
    with pytest.raises(ValueError):
        plain.set_frames("velocity", every=0)
