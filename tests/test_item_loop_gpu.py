"""The persistent-grid kernels when a wave runs many items back to back.

mfma_stage_F / mfma_stage_G (kernels_mfma.hip), hexm_stage (kernels_hexm.hip) and the two affine-sigma sponge pre-passes
(sponge_affine_mfma, sponge_pre_affine_kernel) take a first item, finish it and go round the item loop again with the same
registers, the same wave-private LDS and the same operator tiles.  The family rows (test_mfma_family_gpu.py,
test_hex_family_gpu.py) hand each wave at most one item: the library shrinks the grid to the items.  Here
SEIGEN_HIP_GRID_BLOCKS=8 forces the smallest grid - 8 blocks, 32 waves, 64 in the stash form of the degree-4 G stages - and
caps the grid of the affine pre-passes at 8 blocks, so that a second and third trip through every loop is checked:

  tier A  block (15, 4, 3) (72 items: 2 or 3 per wave) against the FP64 oracle, the whole check of
          test_mfma_family_gpu._check_row, for every (dtype, degree, storage), FACT 0 and 1, both forms of the degree-4 G
          stages, and SEIGEN_HIP_ORDER_CHUNK=5 (a ragged last chunk: waves meet a past-the-end index after their items);
          the two rows of the stash form again on (15, 5, 5) (144 items: 2 or 3 for each of its 64 waves);
  tier B  blocks (15, 8, 8) and (15, 7, 9) (360 items: 11 or 12 per wave, 5 or 6 in the stash form): the item split only
          changes speed, so the bits of a run must not depend on the grid - forced grid, chunked or not, against the
          library's own grid of one item per wave, which is the path the family rows hold to the oracle;
  tier C  blocks with neighbours: the listed items of INTERIOR / SECOND launches and remote traces (GHOST = 1) on the
          forced grid, bitwise against the single block, and that against the single block on the library's own grid;
  tier D  hexm_stage on (13, 9, 11) hexahedra (81 items: 2 or 3 per wave), bitwise against the library's own grid and
          against the generic kernels at twice the row tolerances (each side is within one of the same oracle in
          test_hex_family_gpu.py; the oracle itself is far too slow at DQ_4 for this size).

tests/test_item_loop_host.py restates who runs which item and proves, without a GPU, that these shapes loop as said.
Tolerances are the suite's own (test_mfma_family_gpu._tolerances, test_parity_gpu.tol_of); every figure is printed before
it is asserted.

Shown to bite, once, with a library built aside whose mfma_stage_G zeroes its accumulators Sd / So in front of the item
loop instead of inside it (wrong numbers from a wave's second item on, nothing else): all 22 tier A tests failed on the one
application of G, relative error 2.0 (the stash form on (15, 4, 3), one second trip per label) to 6.6 (the same on
(15, 5, 5)) against 1e-11 and 2e-5, F at 6e-15; all 20 tier B tests failed on the G array, forced grid against the library's
own, relative difference 82 to 3.2e4.  All 24 rows of test_mfma_family_gpu.py::test_row_against_the_oracle passed with that
library, and so did its split rows: they never go round the loop."""
import functools

import numpy as np
import pytest

from oracle import mesh as omesh
from tests.test_item_loop_host import TIER_A, TIER_A_CHUNK, TIER_A_STASH, TIER_B, TIER_B_CHUNKS, TIER_B_RAGGED, TIER_C, TIER_D
from tests.test_mfma_family_gpu import SharedOracle, _block, _check_row, _environment, _fact, _sponge, _stage_names, _stress
from tests.test_parity_gpu import tol_of
from tests.util import oracle_mesh, rel_err

pytestmark = pytest.mark.gpu

_GRID, _CHUNK, _STASH = "SEIGEN_HIP_GRID_BLOCKS", "SEIGEN_HIP_ORDER_CHUNK", "SEIGEN_HIP_GSTASH"
_DENSITIES = ("scalar", "cell", "physical")

# dtype, degree, symmetric stress, SEIGEN_HIP_GQ, SEIGEN_HIP_GSTASH, SEIGEN_HIP_ORDER_CHUNK (None: unset)
ROWS = [
    ("f64", 1, True, None, None, None),
    ("f64", 1, False, None, None, "5"),
    ("f64", 2, True, None, None, None),
    ("f64", 2, False, None, None, None),
    ("f64", 3, True, "0", None, None),
    ("f64", 3, False, "1", None, None),
    ("f64", 3, True, "1", None, None),
    ("f64", 4, True, "1", None, None),
    ("f64", 4, False, "1", None, None),
    ("f64", 4, False, "1", "0", None),
    ("f64", 4, True, "0", None, "5"),
    ("f64", 4, False, "0", None, None),
    ("f32", 1, True, None, None, None),
    ("f32", 1, False, None, None, None),
    ("f32", 2, True, None, None, None),
    ("f32", 2, False, None, None, None),
    ("f32", 3, True, None, None, "5"),
    ("f32", 3, False, None, None, None),
    ("f32", 4, True, None, None, None),
    ("f32", 4, False, None, None, "5"),
]
assert all(r[5] in (None, str(TIER_A_CHUNK)) for r in ROWS)
# the stash form (the default of the degree-4 G stages with FACT = 1) has 64 waves on 8 blocks: (15, 4, 3) gives one wave
# of a label a second item; these rows run on (15, 5, 5), where every wave runs two or three
STASH_ROWS = [r for r in ROWS if r[:2] == ("f64", 4) and r[3] == "1" and r[4] is None]
assert len(STASH_ROWS) == 2 and {r[2] for r in STASH_ROWS} == {True, False}
# tier B: the combinations of tier A (the chunk override is part of its own sequence of runs)
COMBOS = list(dict.fromkeys(r[:5] for r in ROWS))


def _row_id(r):
    return "%s-P%d-%s%s%s%s" % (r[0], r[1], "sym" if r[2] else "full", "" if r[3] is None else "-gq" + r[3],
                                "" if r[4] is None else "-gstash" + r[4], "" if len(r) < 6 or r[5] is None else "-chunk" + r[5])


def _launch(grid, chunk=None, gstash=None):
    return {_GRID: grid, _CHUNK: chunk, _STASH: gstash}


@functools.lru_cache(maxsize=None)
def _oracle(P, n=TIER_A):
    """the oracle of a tier A block at one degree, with one sponge: built once (11 + 5 s at degree 4 on (15, 4, 3), twice
    that on (15, 5, 5)), lent to every row"""
    return SharedOracle(n, P, 4000 + P)


# ---------------------------------------------------------------------------------------------------------------------------
#  tier A
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ROWS, ids=_row_id)
def test_forced_grid_row_against_the_oracle(gpu, monkeypatch, row):
    dtype, P, sym, gq, gstash, chunk = row
    _environment(monkeypatch, "mfma", gq, _launch("8", chunk, gstash))
    _check_row(dtype, P, sym, TIER_A, gq, _DENSITIES[ROWS.index(row) % 3], oracle=_oracle(P))


@pytest.mark.parametrize("row", STASH_ROWS, ids=_row_id)
def test_forced_grid_stash_form_row_against_the_oracle(gpu, monkeypatch, row):
    dtype, P, sym, gq, gstash, chunk = row
    _environment(monkeypatch, "mfma", gq, _launch("8", chunk, gstash))
    _check_row(dtype, P, sym, TIER_A_STASH, gq, _DENSITIES[1 + STASH_ROWS.index(row)], oracle=_oracle(P, TIER_A_STASH))


def _parse(name):
    """('F' or 'G', type, degree, mode, sym, ghost or fact) of a reported stage kernel"""
    head, args = name[:-1].split("<")
    assert head in ("sg::mfma_stage_F", "sg::mfma_stage_G"), name
    t, P, mode, sym, last = [a.strip() for a in args.split(",")]
    return head[-1], {"double": "f64", "float": "f32"}[t], int(P), int(mode), int(sym), int(last)


def test_rows_reach_what_they_claim(gpu, monkeypatch):
    """By the names the library reports for each row's block, set up under the row's switches: every (dtype, degree) in
    both stress storages; FACT 0 and 1 at degrees 3 and 4 in double; the chunk override on rows of both dtypes, of different
    degree and storage.  The two launch forms at degree 4 with FACT = 1 share one kernel object, so no name tells them
    apart: that both are listed is read from the rows' own SEIGEN_HIP_GSTASH, a guard on the table and no more."""
    reached, facts, forms, chunked = set(), set(), set(), set()
    for row in ROWS:
        dtype, P, sym, gq, gstash, chunk = row
        _environment(monkeypatch, "mfma", gq, _launch("8", chunk, gstash))
        blk = _block(dtype, P, TIER_A, tuple(0.4 * k for k in TIER_A))
        blk.set_params(1.0, 0.01, 0.5, 0.25)
        if not sym:
            blk.leave_sym()
        names = [blk.stage_kernel_name(st) for st in range(6)]
        blk.close()
        assert names == _stage_names(dtype, P, sym, _fact(dtype, P, gq)), names
        for kind, t, p, mode, s, last in map(_parse, names):
            assert (t, p, s) == (dtype, P, int(sym))
            reached.add((t, p, s))
            if kind == "G":
                facts.add((t, p, last))
                if (t, p, last) == ("f64", 4, 1):
                    forms.add("from memory" if gstash == "0" else "stash")
            else:
                assert last == 0          # GHOST = 1 is tier C's
        if chunk is not None:
            chunked.add((dtype, P, sym))
    assert reached == {(t, P, s) for t in ("f64", "f32") for P in (1, 2, 3, 4) for s in (0, 1)}
    assert {f for f in facts if f[0] == "f64" and f[1] >= 3} == {("f64", P, fact) for P in (3, 4) for fact in (0, 1)}
    assert {f[2] for f in facts if f[0] == "f32" or f[1] <= 2} == {0}
    assert forms == {"stash", "from memory"}
    assert {c[0] for c in chunked} == {"f64", "f32"}
    assert len({c[1] for c in chunked}) >= 2 and {c[2] for c in chunked} == {True, False}


# ---------------------------------------------------------------------------------------------------------------------------
#  tier B
# ---------------------------------------------------------------------------------------------------------------------------
def _unique_source_nodes(n, nd, rng):
    """scattered nodes and nodes of the last cube in x of three rows, each once: a node listed twice may add in either order"""
    ncube = n[0] * n[1] * n[2]
    last = (np.arange(n[1] * n[2]) * n[0] + n[0] - 1)[:3]
    nodes = np.concatenate([rng.integers(0, 6 * ncube * nd, size=10), (6 * last + 5) * nd + rng.integers(0, nd, size=len(last)),
                            [6 * ncube * nd - 1]])          # ... and the last node of the last (ragged) group
    return np.unique(nodes)


def _tet_inputs(n, P, sym, density):
    """what a tier B sequence starts from: built once per test, shared, unchanged, by every run of its combination"""
    rng = np.random.default_rng(7000 + 100 * P + 10 * n[1] + int(sym))
    L = tuple(0.4 * k for k in n)
    m = oracle_mesh(3, n, L)
    nc, nd = m.ncells, m.node_coords(P).shape[1]
    I = dict(L=L, lam=rng.uniform(0.4, 0.8, nc), mu=rng.uniform(0.2, 0.4, nc), dt=0.04 * 0.4 / P ** 2,
             T=_stress((nc, nd, 3, 3), rng, sym), u=rng.uniform(-1, 1, (nc, nd, 3)),
             s0=_stress((nc, nd, 3, 3), rng, sym), u0=rng.uniform(-1, 1, (nc, nd, 3)),
             rho=1.1 if density == "scalar" else (rng.uniform(0.9, 1.1, nc) if density == "cell" else rng.uniform(0.8, 1.5, nc)),
             sigma=_sponge(m, rng), nodes=_unique_source_nodes(n, nd, rng))
    I["vals"] = _stress((3, len(I["nodes"]), 3, 3), rng, sym)
    for a in I.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return I


def _sequence(make_block, I, density, sym, names=None):
    """apply_F, apply_G, then three steps with all extras; the six arrays it leaves: UH, SH of the applications, then U, S,
    UH, SH after the last step"""
    from seigen_amd import _lib
    blk = make_block()
    blk.set_params(1.0, 0.01, I["lam"], I["mu"])
    blk.set_field(_lib.FIELD_S, I["T"])
    blk.set_field(_lib.FIELD_U, I["u"])
    if sym is not None:
        assert blk.is_sym() == sym
    if names is not None:
        assert [blk.stage_kernel_name(st) for st in range(6)] == names
    blk.apply_F(_lib.FIELD_S, _lib.FIELD_U, _lib.FIELD_UH)
    out = [blk.get_field(_lib.FIELD_UH)]
    blk.apply_G(_lib.FIELD_U, _lib.FIELD_SH)
    out.append(blk.get_field(_lib.FIELD_SH))
    blk.close()
    blk = make_block()
    if density == "scalar":
        blk.set_params(I["rho"], I["dt"], I["lam"], I["mu"])
    else:
        blk.set_params(1.0, I["dt"], I["lam"], I["mu"])
        blk.set_density(I["rho"], physical=density == "physical")
    blk.set_absorption(I["sigma"], 4)
    blk.set_source(I["nodes"], I["vals"])
    blk.set_field(_lib.FIELD_U, I["u0"])
    blk.set_field(_lib.FIELD_S, I["s0"])
    if sym is not None:
        assert blk.is_sym() == sym
    blk.step(3)
    out += [blk.get_field(f) for f in (_lib.FIELD_U, _lib.FIELD_S, _lib.FIELD_UH, _lib.FIELD_SH)]
    blk.close()
    return out


_ARRAYS = ("F", "G", "u", "s", "uh", "sh")


def _assert_same_bits(what, got, want):
    for k, a, b in zip(_ARRAYS, got, want):
        assert np.array_equal(a, b), (what, k, rel_err(a, b))


def _assert_alive(out, u0):
    for k, a in zip(_ARRAYS, out):
        assert np.isfinite(a).all(), k
    moved = rel_err(out[2], u0)
    print("MOVED %.3e" % moved)
    assert moved > 1e-4


@pytest.mark.parametrize("combo", COMBOS, ids=_row_id)
def test_the_bits_do_not_depend_on_the_grid(gpu, monkeypatch, combo):
    """(15, 8, 8): the forced grid - as it is, with SEIGEN_HIP_ORDER_CHUNK 0 and 7 (7 does not divide 360) - against the
    library's own grid; (15, 7, 9), whose last group holds one cube: the forced grid in chunks of 7 against the library's own"""
    dtype, P, sym, gq, gstash = combo
    density = _DENSITIES[COMBOS.index(combo) % 3]
    names = _stage_names(dtype, P, sym, _fact(dtype, P, gq))
    for n, chunks in ((TIER_B, (None,) + tuple(str(c) for c in TIER_B_CHUNKS)), (TIER_B_RAGGED, ("7",))):
        I = _tet_inputs(n, P, sym, density)

        def run(grid, chunk):
            _environment(monkeypatch, "mfma", gq, _launch(grid, chunk, gstash))
            return _sequence(lambda: _block(dtype, P, n, I["L"]), I, density, sym, names)

        own = run(None, None)
        _assert_alive(own, I["u0"])
        for chunk in chunks:
            _assert_same_bits((n, "forced grid, chunk %s" % chunk), run("8", chunk), own)


# ---------------------------------------------------------------------------------------------------------------------------
#  tier C
# ---------------------------------------------------------------------------------------------------------------------------
def _case_id(c):
    return "%s-P%d-%s-%s-on-%s-%s" % (c[1], c[0], "sym" if c[2] else "full", "x".join(map(str, c[3])), "x".join(map(str, c[4])),
                                      "pipelined" if c[5] else "unpipelined")


@pytest.mark.parametrize("case", TIER_C, ids=_case_id)
def test_region_launches_on_the_forced_grid(gpu, monkeypatch, case):
    """INTERIOR / SECOND launches take the overridden grid and walk a list of items; BOUNDARY / FIRST keep the full one.
    _multiblock_case holds the blocks to the single block bitwise; the single block itself - 8 blocks for the whole mesh -
    must equal the single block on the library's own grid."""
    from tests.test_harness_gpu import _multiblock_case
    P, dtype, sym, n, grid, pipelined = case
    _environment(monkeypatch, "mfma", None, _launch("8"))
    forced = _multiblock_case(3, P, n, grid, pipelined, extras=True, dtype=dtype, sym=sym)
    assert forced["names"] == sorted(set(_stage_names(dtype, P, sym, _fact(dtype, P, None), ghost=1))), forced["names"]
    _environment(monkeypatch, "mfma", None, _launch(None))
    own = _multiblock_case(3, P, n, grid, pipelined, extras=True, dtype=dtype, sym=sym)
    for k in ("u", "s"):
        assert np.isfinite(forced[k]).all()
        assert np.array_equal(forced[k], own[k]), (k, rel_err(forced[k], own[k]))
    assert rel_err(forced["u"], forced["u0"]) > 1e-4


# ---------------------------------------------------------------------------------------------------------------------------
#  tier D
# ---------------------------------------------------------------------------------------------------------------------------
_Q = "quadrilateral"
HEX_ROWS = [(3, True), (3, False), (4, True), (4, False)]


def _hex_inputs(P, sym, density):
    """check_block's inputs (test_tile2d_family_gpu.py) on (13, 9, 11) hexahedra, the source nodes each once; built once per
    test and unchanged by its runs"""
    n = TIER_D
    L = (0.4 * n[0], 0.3 * n[1], 0.35 * n[2])
    rng = np.random.default_rng(9000 + 10 * P + int(sym))
    m = omesh.structured(3, n, L, quadrilateral=True)
    nc, nd = m.ncells, (P + 1) ** 3
    I = dict(L=L, lam=rng.uniform(0.4, 0.8, nc), mu=rng.uniform(0.2, 0.4, nc), dt=0.04 * 0.3 / P ** 2,
             T=_stress((nc, nd, 3, 3), rng, sym), u=rng.uniform(-1, 1, (nc, nd, 3)),
             s0=_stress((nc, nd, 3, 3), rng, sym), u0=rng.uniform(-1, 1, (nc, nd, 3)),
             rho=1.1 if density == "scalar" else (rng.uniform(0.9, 1.1, nc) if density == "cell" else rng.uniform(0.8, 1.5, nc)),
             sigma=_sponge(m, rng))
    I["nodes"] = np.unique(np.concatenate([rng.integers(0, nc * nd, size=10), np.array([nc - 1, nc - 2]) * nd + rng.integers(0, nd, size=2)]))
    I["vals"] = _stress((3, len(I["nodes"]), 3, 3), rng, sym)
    for a in I.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return I


@pytest.mark.parametrize("row", HEX_ROWS, ids=lambda r: "DQ%d-%s" % (r[0], "sym" if r[1] else "full"))
def test_hexm_stage_on_the_forced_grid(gpu, monkeypatch, row):
    from seigen_amd.backend import HipBlock
    from tests.test_hex_family_gpu import _stage_names as hex_names
    from tests.test_lane_generic_family_gpu import _stage_names as family_names
    P, sym = row
    density = _DENSITIES[HEX_ROWS.index(row) % 3]
    I = _hex_inputs(P, sym, density)
    n, L = TIER_D, I["L"]

    def run(path, grid, sym_is, names):
        for var in ("SEIGEN_HIP_SPONGE_AFFINE", "SEIGEN_HIP_SYM", "SEIGEN_HIP_PATH", "SEIGEN_HIP_SOURCE_LAUNCH", "SEIGEN_HIP_GRAPH",
                    _GRID, _CHUNK, _STASH):
            monkeypatch.delenv(var, raising=False)
        if path:
            monkeypatch.setenv("SEIGEN_HIP_PATH", path)
        if grid:
            monkeypatch.setenv(_GRID, grid)
        return _sequence(lambda: HipBlock(3, P, n, [L[a] / n[a] for a in range(3)], [0.0] * 3, _Q), I, density, sym_is, names)

    forced = run(None, "8", sym, hex_names(P, sym))
    _assert_alive(forced, I["u0"])
    _assert_same_bits("the library's own grid", forced, run(None, None, sym, hex_names(P, sym)))
    # the generic kernels: another family on the same inputs (by the names its stages report - were the switch ignored, this
    # would compare hexm_stage with itself); it never enters symmetric storage - full tensors on both sides
    generic_names = family_names("generic", 3, P, _Q, False)
    assert not any(name.startswith("sg::hexm_stage") for name in generic_names), generic_names
    generic = run("generic", None, False, generic_names)
    tol = tol_of(P, _Q)
    errs = [rel_err(a, b) for a, b in zip(forced, generic)]
    print("ERR hexm against generic", dict(zip(_ARRAYS, ["%.3e" % e for e in errs])))
    assert max(errs[:2]) < 2 * tol, errs
    assert max(errs[2:]) < 20 * tol, errs
