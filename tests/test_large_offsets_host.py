"""What tests/test_large_offsets_gpu.py rests on, without a GPU: the mark helper against the layout formula evaluated cube by
cube in Python integers, the device-free host logic (sg_locate_points, sg_region_boxes) on the largest block configuration
of that file, and the reach rule its window margins come from, on the oracle."""
import ctypes as C

import numpy as np
import pytest

from oracle import mesh as omesh
from oracle.lf4 import OracleLF4
from seigen_amd import _lib
from seigen_amd.backend import locate_points
from tests import test_large_offsets_gpu as lo

_Q = "quadrilateral"

# first cubes as the proportional estimate ceil(mark / bytes per cube) gives them (FP64): the helper's cube lies in the same
# group of gw cubes, since every cube of the group that holds the mark has lines past it from some class on
QUOTED = [
    (lo.Shape(3, "left", 4), "S", "B", 1 << 32, 284059),
    (lo.Shape(3, "left", 4), "U", "B", 1 << 32, 852177),
    (lo.Shape(3, "left", 4), "S", "el", 1 << 31, 1136235),
    (lo.Shape(3, _Q, 4), "S", "B", 1 << 32, 477219),
    (lo.Shape(3, _Q, 4), "S", "el", 1 << 31, 1908875),
    (lo.Shape(3, _Q, 2, lane=True), "S", "B", 1 << 32, 2209346),
    (lo.Shape(2, "left", 4), "S", "B", 1 << 32, 4473925),
    (lo.Shape(2, _Q, 4), "S", "B", 1 << 32, 5368710),
]


def _largest_offset(sh, ncomp, cube):
    return max(lo.device_offset(sh, ncomp, cube, k, b, c) for k in range(sh.ncls) for b in range(sh.nd) for c in range(ncomp))


@pytest.mark.parametrize("sh,field,unit,value,quoted", QUOTED, ids=lambda v: None)
def test_first_cube_past_a_mark_by_brute_force(sh, field, unit, value, quoted):
    ncomp, mark = sh.ncomp(field), lo.mark_elements(sh, unit, value)
    cube = lo.first_cube_past(sh, ncomp, mark)
    per_cube = sh.ncls * sh.nd * ncomp
    assert quoted == -(-mark // per_cube)
    assert cube // sh.gw == quoted // sh.gw
    # every offset of every cube of the three groups around it, in Python integers
    first = None
    for c in range((cube // sh.gw - 1) * sh.gw, (cube // sh.gw + 2) * sh.gw):
        if _largest_offset(sh, ncomp, c) >= mark:
            first = c
            break
    assert first == cube
    assert _largest_offset(sh, ncomp, cube - 1) < mark


@pytest.mark.parametrize("gw,ncls,nd,ncomp", [(16, 6, 4, 9), (64, 1, 8, 3), (16, 2, 3, 4), (1, 1, 2, 1)])
def test_first_cube_past_every_mark_of_small_layouts(gw, ncls, nd, ncomp):
    sh = lo.Shape(3, "left", 1)
    sh.gw, sh.ncls, sh.nd = gw, ncls, nd
    ncube = 3 * gw + 5
    largest = [_largest_offset(sh, ncomp, c) for c in range(ncube)]
    for mark in range(0, 3 * gw * ncls * nd * ncomp):
        want = next(c for c in range(ncube) if largest[c] >= mark)
        assert lo.first_cube_past(sh, ncomp, mark) == want, mark


def test_plans_hold_their_marks_and_stay_disjoint():
    for row in lo.ROWS:
        sh = row.sh
        Z, wins = lo.plan(sh, row.tier, row.ghost)
        assert wins[-1].k0 + sh.W == Z and wins[0].k0 >= sh.W
        for a, b in zip(wins, wins[1:]):
            assert a.k0 + sh.W <= b.k0
        end = lo.mark_layer(sh, *lo.TIER_END[row.tier])
        assert any(w.mark == lo.TIER_END[row.tier] and w.k0 + w.d0 + 1 == end for w in wins)
        if row.tier == "B":
            assert {w.mark for w in wins[:-1]} >= {("S", "B", 1 << 32), ("S", "el", 1 << 31)}
        ranges = lo.elsewhere(sh, wins)
        assert ranges and all(0 <= a < b <= Z * sh.per for a, b in ranges)
        for a, b in ranges:
            assert all(b <= w.cell0 or a >= w.cell0 + w.ncells for w in wins)
        # the cells 2^32 bytes below the first window's stress lines are among them
        w = wins[0]
        s_lo, s_hi = lo.offset_range(sh, sh.ncomp("S"), w)
        shift = (1 << 32) // sh.itemsize
        if s_lo - shift >= 0:
            cube = (s_lo - shift) // (sh.ncls * sh.nd * sh.ncomp("S") * sh.gw) * sh.gw
            assert any(a <= cube * sh.ncls < b for a, b in ranges)
    assert lo.field_bytes(lo.ROWS[3].sh, lo.plan(lo.ROWS[3].sh, "A")[0]) < 12e9            # P4 tets, tier A: 11.5 GB
    assert 44e9 < lo.field_bytes(lo.ROWS[15].sh, lo.plan(lo.ROWS[15].sh, "B")[0]) < 47e9   # tier B, FP64: 46 GB


def _config(sh, Z, mask=0):
    cfg = _lib.SgConfig()
    cfg.dim, cfg.degree, cfg.diagonal, cfg.nbr_mask = sh.dim, sh.P, 2 if sh.tensor else 0, mask
    for a in range(3):
        cfg.n[a] = sh.n(Z)[a] if a < sh.dim else 1
        cfg.h[a] = sh.h[a] if a < sh.dim else 1.0
    return cfg


@pytest.mark.parametrize("name", ["B-tets-P4", "B-hexm-DQ4"])
def test_locate_points_on_the_tier_b_block(name):
    """points in the last cube and in the mark cubes: the expected 64-bit cell index (cube 6 + class; the class from the
    order of the fractions for a Kuhn tetrahedron is not assumed - the cell's cube is checked, and xi against the point)"""
    row = next(r for r in lo.ROWS if r.name == name)
    sh = row.sh
    Z, wins = lo.plan(sh, row.tier)
    cubes = [Z * 6 - 1] + [lo.first_cube_past(sh, sh.ncomp(w.mark[0]), lo.mark_elements(sh, *w.mark[1:])) for w in wins[:-1]]
    frac = np.array([0.31, 0.52, 0.73])
    pts = np.array([[(c % 3 + frac[0]) * sh.h[0], (c // 3 % 2 + frac[1]) * sh.h[1], (c // 6 + frac[2]) * sh.h[2]] for c in cubes])
    cell, xi = locate_points(_config(sh, Z), pts)
    assert cell.dtype == np.int64
    assert list(cell // sh.ncls) == cubes
    assert max(cubes) * sh.ncls * sh.nd * 9 > 1 << 31           # the last cell's stress lines lie past 2^31 elements
    if sh.tensor:
        assert np.abs(xi - frac).max() < 1e-9
    else:
        # the Kuhn tetrahedron of the point: the class is the same in every cube, as in the first
        c0, _ = locate_points(_config(sh, 4), frac[None] * np.array(sh.h))
        assert list(cell % sh.ncls) == [int(c0[0])] * len(cubes)
    outside, _ = locate_points(_config(sh, Z), np.array([[0.5, 0.3, Z * sh.h[2] + 0.1]]))
    assert outside[0] == -1


def test_region_boxes_on_the_tier_b_block_with_a_neighbour_above():
    row = next(r for r in lo.ROWS if r.name == "B-tets-P4")
    sh = row.sh
    Z, _ = lo.plan(sh, row.tier)
    lib = _lib.load()
    cover = {}
    for region in range(5):
        buf = (C.c_int32 * (6 * 16))()
        cnt = lib.sg_region_boxes(C.byref(_config(sh, Z, 1 << 5)), region, buf, 16)
        assert 0 <= cnt <= 7
        boxes = [tuple(buf[6 * i + k] for k in range(6)) for i in range(cnt)]
        layers = np.zeros(Z, dtype=np.int64)                  # cubes covered per layer
        for o0, o1, o2, n0, n1, n2 in boxes:
            assert n0 > 0 and n1 > 0 and n2 > 0 and o0 + n0 <= 3 and o1 + n1 <= 2 and o2 + n2 <= Z
            layers[o2:o2 + n2] += n0 * n1
        cover[region] = layers
    assert (cover[0] == 6).all()                                # ALL
    assert (cover[1] + cover[2] == 6).all() and (cover[3] + cover[4] == 6).all()
    assert cover[2][Z - 1] == 6 and cover[2][:Z - 1].sum() == 0  # BOUNDARY: the top layer, whose cubes face the neighbour
    assert cover[1][:Z - 1].min() == 6                          # INTERIOR: everything below


@pytest.mark.parametrize("cell,reach1,reach2", [("left", 2, 4), (_Q, 6, 12)])
def test_reach_of_one_and_two_steps(cell, reach1, reach2):
    """P2, a 3 x 2 x 40 mesh, one data layer: how many layers away from the data a stage field of one and of two LF4 steps
    is nonzero.  Tetrahedra: at most 2 and 4 (u1 after one step: 1) - margin 4 of the windows covers one step; hexahedra: 6
    per step - margin 7.  A change to the oracle or the scheme that widens the reach fails here, not silently in the windows."""
    Z, k0 = 40, 20
    quad = cell == _Q
    m = omesh.structured(3, (3, 2, Z), (3 * 0.4, 2 * 0.3, Z * 0.5), quadrilateral=quad)
    orc = OracleLF4(m, 2)
    per = m.ncells // Z
    rng = np.random.default_rng(1)
    sl = slice(k0 * per, (k0 + 1) * per)
    orc.u0[sl] = rng.uniform(-1, 1, orc.u0[sl].shape)
    s = rng.uniform(-1, 1, orc.s0[sl].shape)
    orc.s0[sl] = 0.5 * (s + np.swapaxes(s, -1, -2))
    orc.dt, orc.l, orc.mu = 0.01, rng.uniform(0.4, 0.8, m.ncells), rng.uniform(0.2, 0.4, m.ncells)
    orc.density = rng.uniform(0.9, 1.1, m.ncells)

    def reach(a):
        nz = np.flatnonzero(np.abs(a.reshape(Z, -1)).max(axis=1) > 0)
        return max(k0 - nz.min(), nz.max() - k0)

    assert reach(orc.E.apply_F(orc.s0, orc.u0)) == 1 and reach(orc.E.apply_G(orc.u0, orc.l, orc.mu)) == 1
    orc.step(orc.dt)
    one = {k: reach(v) for k, v in dict(orc.last, u1=orc.u1, s1=orc.s1).items()}
    assert max(one.values()) <= reach1, one
    if not quad:
        assert one["u1"] == 1 and one["s1"] == 2 and one["sh1"] == 2 and one["utemp"] == 2, one
    orc.step(2 * orc.dt)
    two = {k: reach(v) for k, v in dict(orc.last, u1=orc.u1, s1=orc.s1).items()}
    assert max(two.values()) <= reach2, two
    sh = lo.Shape(3, cell, 2)
    assert sh.margin > reach1


def test_reach_in_two_dimensions():
    """triangles: a step reaches 3 rows (margin 4); quadrilaterals: 6 (margin 7)"""
    for cell, want in (("left", 3), (_Q, 6)):
        Z, k0 = 24, 12
        m = omesh.structured(2, (3, Z), (3 * 0.4, Z * 0.5), quadrilateral=cell == _Q)
        orc = OracleLF4(m, 2)
        per = m.ncells // Z
        rng = np.random.default_rng(2)
        sl = slice(k0 * per, (k0 + 1) * per)
        orc.u0[sl] = rng.uniform(-1, 1, orc.u0[sl].shape)
        s = rng.uniform(-1, 1, orc.s0[sl].shape)
        orc.s0[sl] = 0.5 * (s + np.swapaxes(s, -1, -2))
        orc.dt, orc.l, orc.mu = 0.01, 0.5, 0.25
        orc.step(orc.dt)
        reach = 0
        for a in list(orc.last.values()) + [orc.u1, orc.s1]:
            nz = np.flatnonzero(np.abs(a.reshape(Z, -1)).max(axis=1) > 0)
            reach = max(reach, k0 - nz.min(), nz.max() - k0)
        assert reach <= want < lo.Shape(2, cell, 2).margin, (cell, reach)


# ---- what tests/test_large_offsets_hooks_gpu.py rests on ---------------------------------------------------------------------
from tests import test_large_offsets_hooks_gpu as hk  # noqa: E402


@pytest.mark.parametrize("dim,cell,P", [(2, "left", 1), (3, "left", 1), (2, _Q, 1), (3, _Q, 1)])
def test_reach_of_two_whole_steps_from_three_data_layers(dim, cell, P):
    """R = hk.step_reach(): two whole steps of OracleLF4 from data in three layers leave every field of every stage exactly zero
    outside 3 + 2 * 2 * R layers, and u1 or s1 nonzero in the outermost layer inside, on both sides - degree 1 shows it"""
    sh = lo.Shape(dim, cell, P)
    R = hk.step_reach(sh)
    assert R == (6 if cell == _Q else (3 if dim == 2 else 2)) and hk.K == 2
    reach = hk.K * R
    Z = lo.DATA + 2 * reach + 6
    k0 = reach + 3
    m = omesh.structured(dim, sh.n(Z), tuple(sh.h[a] * k for a, k in enumerate(sh.n(Z))), "left", quadrilateral=sh.tensor)
    orc = OracleLF4(m, P)
    per = m.ncells // Z
    assert per == sh.per
    rng = np.random.default_rng(3)
    sl = slice(k0 * per, (k0 + lo.DATA) * per)
    orc.u0[sl] = rng.uniform(-1, 1, orc.u0[sl].shape)
    s = rng.uniform(-1, 1, orc.s0[sl].shape)
    orc.s0[sl] = 0.5 * (s + np.swapaxes(s, -1, -2))
    orc.dt, orc.l, orc.mu = 0.04 * min(sh.h) / P ** 2, 0.5, 0.25
    seen = []
    for step in range(hk.K):
        orc.step((step + 1) * orc.dt)
        seen += [np.abs(a.reshape(Z, -1)).max(axis=1) for a in list(orc.last.values()) + [orc.u1, orc.s1]]
    rows = np.max(seen, axis=0)
    assert not rows[:k0 - reach].any() and not rows[k0 + lo.DATA + reach:].any(), np.flatnonzero(rows)
    state = np.maximum(np.abs(orc.u1.reshape(Z, -1)).max(axis=1), np.abs(orc.s1.reshape(Z, -1)).max(axis=1))
    assert state[k0 - reach] > 0 and state[k0 + lo.DATA + reach - 1] > 0, np.flatnonzero(state)


@pytest.mark.parametrize("row", hk.ROWS, ids=[r.name for r in hk.ROWS])
def test_hook_window_plans_are_not_vacuous(row):
    """every mark window's hook window keeps its K R layers on both sides and holds lines on both sides of its mark; the hook
    windows are disjoint and ascending (the top window's alone may start where the one below ends); the accumulator of the last
    part lies past 2^32 bytes (tier B: past 2^31 elements) at every window; the caller's side of the whole-field transfer and
    of the whole-block gradient passes the marks the GPU module's docstring claims; the memory figures of that docstring"""
    sh = row.sh
    Z, wins = lo.plan(sh, row.tier, row.ghost)
    hws = hk.hook_windows(sh, Z, wins)
    reach = hk.K * hk.step_reach(sh)
    assert [hw.w for hw in hws] == wins
    for a, b in zip(hws, hws[1:]):
        assert a.k1 <= b.k0
    for hw in hws[:-1]:
        assert hw.k0 == hw.d0 - reach and hw.k1 == hw.d0 + lo.DATA + reach and hw.k0 >= 0 and hw.k1 <= Z
        field, unit, value = hw.w.mark
        ncomp, mark = sh.ncomp(field), lo.mark_elements(sh, unit, value)
        cube = lo.first_cube_past(sh, ncomp, mark)
        assert cube // sh.cubes_per_layer == hw.d0 + 1                  # the middle data layer
        c0, c1 = hw.k0 * sh.cubes_per_layer, hw.k1 * sh.cubes_per_layer - 1
        assert lo.device_offset(sh, ncomp, c0, 0, 0, 0) < mark <= lo.device_offset(sh, ncomp, c1, sh.ncls - 1, sh.nd - 1, ncomp - 1)
    top = hws[-1]
    assert top.k1 == Z and top.d0 + lo.DATA == Z and top.k0 <= top.d0 - hk.step_reach(sh)
    assert top.k0 == max(top.d0 - reach, hws[-2].k1)
    # the ranges that must stay initial lie outside every hook window and cover the cells 2^32 bytes below the first one
    outside = hk.complement(hws, Z * sh.per)
    named = hk.elsewhere_outside(sh, wins, hws)
    assert named and all(any(a >= c and b <= d for c, d in outside) for a, b in named)
    assert sum(b - a for a, b in outside) + sum(hw.ncells for hw in hws) == Z * sh.per
    # spectra: accumulator (2 f + part) n + idx, n the field's padded word count, in doubles
    fset, nfreq = hk.spectra_shape(row)
    ncube_pad = -(-Z * sh.cubes_per_layer // sh.gw) * sh.gw
    for k in fset:
        ncomp = sh.ncomp("US"[k])
        n = ncube_pad * sh.ncls * sh.nd * ncomp
        for hw in hws[:-1]:
            first = (2 * nfreq - 1) * n + lo.device_offset(sh, ncomp, hw.k0 * sh.cubes_per_layer // sh.gw * sh.gw, 0, 0, 0)
            assert first * 8 > lo.BYTES_2_32
            if row.tier == "B":
                assert first > lo.ELEMS_2_31
    # the caller's side, buf + rel * rows: the stress window's first cell against the marks
    s_windows = [hw for hw in hws[:-1] if hw.w.mark[0] == "S"]
    assert s_windows
    row_values = sh.nd * sh.ncomp("S")
    last = s_windows[-1]
    if row.tier in hk.WHOLE_FIELD or row.name in hk.WHOLE_FIELD:
        out_bytes = 4 if sh.dtype == "f32" else 8                       # the whole-field transfer: the block's own type
        assert (last.cell0 + last.ncells) * row_values * out_bytes > lo.BYTES_2_32
    grad_words = (last.cell0 + last.ncells) * row_values                # the whole-block gradient in float32: dim * dim values a node
    if sh.dtype == "f32":
        assert grad_words * 4 > lo.BYTES_2_32
    if row.tier == "B":
        assert last.cell0 * row_values < lo.ELEMS_2_31 < grad_words     # lines on both sides of 2^31 elements
    if row.name == hk.STRIDED:
        assert Z * sh.cubes_per_layer <= hk.STRIDE_J and 8 * hk.STRIDE_J == lo.ELEMS_2_31
    need = hk.need(row, Z)
    quoted = {"A-tets-P4": 40.1, "A-tets-P4-full": 40.1, "A-tets-P4-f32": 68.7, "A-hexlane-DQ2": 40.1, "A-tri-P4-f32": 79.5,
              "B-tets-P4": 103.1, "B-tets-P4-f32": 80.2}
    print("%s needs %.1f GB: %r" % (row.name, need["total"] / 1e9, {k: round(v / 1e9, 1) for k, v in need.items()}))
    assert abs(need["total"] / 1e9 - quoted[row.name]) < 0.1, need
