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
