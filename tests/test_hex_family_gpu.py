"""Every instantiation of the two hexahedral families - sg::hexm_stage (kernels_hexm.hip, DQ_3 / DQ_4 at every size) and
sg::hex_stage (kernels_lane.hip, DQ_1 / DQ_2 from SG_HEX_LANE_MIN_CELLS cubes; here through SEIGEN_HIP_PATH=lane) -
against the FP64 oracle on hexahedra.

HEXM_KERNELS and HEX_LANE_KERNELS list what launch_hexm_p / launch_hex_p can dispatch; test_host_logic.py holds them equal
to the kernel objects the built library exports.  Each row of ROWS - (degree, symmetric stress, block,
SEIGEN_HIP_SPONGE_AFFINE) - pins its six stage kernels by name, then runs the checks of tests/test_tile2d_family_gpu.py
(check_block): one application of F and G, and three whole LF4 steps with per-cell material, a density (scalar, per cell,
per cell physical in turn), a nodal source with a node listed twice and a DG4 sponge with cells of the four kinds of
test_mfma_family_gpu._sponge (none, constant, general nodal, affine) side by side; full-tensor rows start from a
non-symmetric stress and add non-symmetric source values.  Both families read the sponge term from a pre-pass; hexm_stage's
takes affine cells by four numbers by default, the lane kernels' only under SEIGEN_HIP_SPONGE_AFFINE=1, which one DQ_2 row
sets.  SPLITS run every (degree, symmetry) as blocks with neighbours against the single block, bitwise; the families have
no instantiation of their own for such blocks, so the kernels a split names are its row's, which the rows compare with
the oracle.  test_rows_name_every_stage_kernel checks that the rows reach all 36 instantiations.

The oracle's cost grows steeply with the degree (DQ_4: 125 nodes and a 25 x 25 x 25-point sponge quadrature per cube), so
the DQ_4 blocks stay at or under 70 cubes.  Tolerances: tol_of() per application, 10 tol_of() for the steps (test_parity_gpu.py)."""
import pytest

from oracle import mesh as omesh
from tests.test_mfma_family_gpu import _sponge
from tests.test_tile2d_family_gpu import check_block

pytestmark = pytest.mark.gpu

_Q = "quadrilateral"

# hexm_stage<P, KIND, MODE, SYM> as launch_stage_hexm / launch_hexm_p dispatch them: P = 3, 4; KIND 0 = F in three modes (0:
# UH1 / apply_F, 1: U1, 2: UTEMP), KIND 1 = G in two (0: STEMP, SH1 / apply_G, 1: S1); SYM 1 = symmetric-stress storage.
HEXM_KERNELS = frozenset("sg::hexm_stage<%d, %d, %d, %d>" % (P, kind, mode, sym) for P in (3, 4)
                         for kind, mode in ((0, 0), (0, 1), (0, 2), (1, 0), (1, 1)) for sym in (0, 1))
# hex_stage<P, KIND, MODE, SYM> as launch_stage_lane / launch_hex_p dispatch them: P = 1, 2; F and G in modes 0 and 1 only -
# stage UTEMP (mode 2 elsewhere) runs the F MODE 1 object with c_self = 0 (hostlogic.hpp lf4_stage).
HEX_LANE_KERNELS = frozenset("sg::hex_stage<%d, %d, %d, %d>" % (P, kind, mode, sym) for P in (1, 2) for kind in (0, 1)
                             for mode in (0, 1) for sym in (0, 1))

# degree, symmetric stress, block, SEIGEN_HIP_SPONGE_AFFINE.  Blocks: one cube; (16, 2, 1) one hexm group per x row; (17, 2, 2)
# hexm groups of 16 straddle rows and layers, a second lane group of 4 cubes; (3, 4, 5)-like: rows narrower than a group.
ROWS = [
    (1, True, (17, 2, 2), None),
    (1, False, (3, 4, 5), None),
    (1, False, (1, 1, 1), None),
    (2, True, (16, 2, 1), None),
    (2, False, (17, 2, 2), "1"),
    (2, True, (3, 4, 5), None),
    (3, True, (17, 2, 2), None),
    (3, False, (16, 2, 1), None),
    (3, True, (1, 1, 1), None),
    (3, False, (3, 4, 5), None),
    (4, True, (3, 4, 5), None),
    (4, False, (17, 2, 2), None),
    (4, False, (1, 1, 1), None),
    (4, True, (16, 2, 1), None),
]

# one split per (degree, symmetry): degree, symmetric stress, mesh, block grid, pipelined
SPLITS = [
    (1, True, (6, 3, 5), (3, 1, 2), True),
    (1, False, (4, 4, 4), (2, 2, 2), False),
    (2, True, (4, 4, 4), (2, 2, 2), True),
    (2, False, (70, 3, 2), (2, 1, 1), True),
    (3, True, (36, 4, 2), (2, 2, 1), True),
    (3, False, (4, 2, 3), (2, 1, 3), False),
    (4, True, (2, 4, 2), (1, 2, 2), False),
    (4, False, (6, 2, 2), (2, 1, 1), True),
]


def _stage_names(P, sym):
    """the instantiation each of the six stages launches (hostlogic.hpp lf4_stage)"""
    fmt = "sg::hex%s_stage<%d, %%d, %%d, %d>" % ("" if P <= 2 else "m", P, int(sym))
    utemp = 1 if P <= 2 else 2
    return [fmt % km for km in ((0, 0), (1, 0), (0, 1), (1, 0), (0, utemp), (1, 1))]


def _row_id(r):
    return "DQ%d-%s-%s%s" % (r[0], "sym" if r[1] else "full", "x".join(map(str, r[2])), "" if r[3] is None else "-affine" + r[3])


def _split_id(s):
    return "%s-on-%s-%s" % (_row_id(s[:3] + (None,)), "x".join(map(str, s[3])), "pipelined" if s[4] else "unpipelined")


def _environment(monkeypatch, P, affine=None):
    """the family under test, and nothing else that picks an instantiation, the sponge's form or a source path"""
    for var in ("SEIGEN_HIP_SPONGE_AFFINE", "SEIGEN_HIP_SYM", "SEIGEN_HIP_PATH", "SEIGEN_HIP_SOURCE_LAUNCH", "SEIGEN_HIP_GRAPH"):
        monkeypatch.delenv(var, raising=False)
    if P <= 2:
        monkeypatch.setenv("SEIGEN_HIP_PATH", "lane")
    if affine is not None:
        monkeypatch.setenv("SEIGEN_HIP_SPONGE_AFFINE", affine)


def _block(P, n, L):
    from seigen_amd.backend import HipBlock
    return HipBlock(3, P, n, [L[a] / n[a] for a in range(3)], [0.0] * 3, _Q)


def _size(n):
    return (0.4 * n[0], 0.3 * n[1], 0.35 * n[2])


@pytest.mark.parametrize("row", ROWS, ids=_row_id)
def test_row_against_the_oracle(gpu, monkeypatch, row):
    P, sym, n, affine = row
    _environment(monkeypatch, P, affine)
    L = _size(n)
    check_block("hexm" if P >= 3 else "hex_lane", lambda: _block(P, n, L), omesh.structured(3, n, L, quadrilateral=True), 0.3,
                P, _Q, "f64", sym, _stage_names(P, sym), ("scalar", "cell", "physical")[ROWS.index(row) % 3], _sponge,
                2000 * P + 10 * n[0] + n[2])


@pytest.mark.parametrize("split", SPLITS, ids=_split_id)
def test_split_row_is_bitwise_the_single_block(gpu, monkeypatch, split):
    """blocks with neighbours through the host-driven exchange (test_harness_gpu._LocalExchange), sponge and source
    included, bitwise equal to the single block; the kernels they name are the six of the rows of their (degree, symmetry)"""
    from tests.test_harness_gpu import _multiblock_case
    P, sym, n, grid, pipelined = split
    _environment(monkeypatch, P)
    res = _multiblock_case(3, P, n, grid, pipelined, extras=True, diagonal=_Q, sym=sym)
    assert res["names"] == sorted(set(_stage_names(P, sym))), res["names"]


def test_the_lists_cover_what_they_claim():
    kinds = {(P, sym) for P in (1, 2, 3, 4) for sym in (False, True)}
    assert {r[:2] for r in ROWS} == kinds
    assert sorted(s[:2] for s in SPLITS) == sorted(kinds)
    for degrees in ((1, 2), (3, 4)):           # each family meets each kind of block
        blocks = [r[2] for r in ROWS if r[0] in degrees]
        assert (1, 1, 1) in blocks and (16, 2, 1) in blocks and any(b[0] == 17 for b in blocks) and any(b[0] == 3 for b in blocks)
    assert [r[:2] for r in ROWS if r[3] == "1"] == [(2, False)]
    assert all(r[2][0] * r[2][1] * r[2][2] <= 70 for r in ROWS if r[0] == 4)


def test_rows_name_every_stage_kernel(gpu, monkeypatch):
    """ROWS launch every hexm_stage and hex_stage instantiation and nothing else: each row's block is set up as its test sets
    it up and asked for its six kernels."""
    seen = set()
    for P, sym, n, affine in ROWS:
        _environment(monkeypatch, P, affine)
        blk = _block(P, n, _size(n))
        blk.set_params(1.0, 0.01, 0.5, 0.25)
        if not sym:
            blk.leave_sym()
        names = [blk.stage_kernel_name(st) for st in range(6)]
        assert names == _stage_names(P, sym), names
        seen.update(names)
        blk.close()
    listed = HEXM_KERNELS | HEX_LANE_KERNELS
    assert len(HEXM_KERNELS) == 20 and len(HEX_LANE_KERNELS) == 16
    assert listed <= seen, sorted(listed - seen)
    assert seen <= listed, sorted(seen - listed)
