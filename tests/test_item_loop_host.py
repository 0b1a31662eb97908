"""Who runs which item of a persistent-grid launch, restated on the host, and the proof that the shapes of
tests/test_item_loop_gpu.py make waves go round the item loop as that module says (no GPU).

items_per_wave() restates the launch sizing of launch_stage_mfma (kernels_mfma.hip) and launch_stage_hexm
(kernels_hexm.hip) and the split of item_range / item_of (kernels_mfma.hip; hexm_stage has the same contiguous split inline)
for launches that are not `spread`: a map from (items, SEIGEN_HIP_GRID_BLOCKS or None, waves per block, items per XCD chunk)
to the list of items each wave visits, -1 where the loop index falls past the end of the last chunk.  region_item_count()
restates the boxes of a region of a block with neighbours (hostapi.cpp region_boxes, hostlogic.hpp shell_width_x) down to
the number of (cell group, class) items the launch lists.  affine_mfma_trips() and pre_affine_trips() restate the two
affine-sigma pre-passes of sg_set_absorption - the items plan_sponge lists for the sigma of test_mfma_family_gpu._sponge, the
grid cap (hostlogic.hpp affine_grid_cap) and the loops of sponge_affine_mfma and sponge_pre_affine_kernel.

The stage kernels have a second `continue`, `if (!__any(L.active)) continue;`.  No launch of these tests reaches it: a
whole-block launch has a real cube in every group, and a region launch lists only the groups its boxes touch (hostapi.cpp
region_items), so every listed item has an active lane.

A shape that stops meeting these conditions - because the launch sizing changed - is to be replaced by one that does."""
import numpy as np

# blocks of four waves an MI355X holds of a stage kernel (256 CUs, one or two per CU): the library's own grid before it is
# shrunk to the items.  Every condition below holds for both.
SLOTS = (256, 512)

# tests/test_item_loop_gpu.py
TIER_A = (15, 4, 3)       # 180 cubes, 12 groups (the last: 4 of 16 lanes), 72 items
TIER_A_CHUNK = 5
TIER_A_STASH = (15, 5, 5)     # 375 cubes, 24 groups (the last: 7 of 16 lanes), 144 items: two or three for each of 64 waves
TIER_B = (15, 8, 8)       # 960 cubes, 60 whole groups, 360 items
TIER_B_RAGGED = (15, 7, 9)    # 945 cubes, 60 groups (the last: 1 of 16 lanes), 360 items: the same split, a ragged end
TIER_B_CHUNKS = (0, 7)
TIER_D = (13, 9, 11)      # hexahedra: 1287 cubes, 81 groups (the last: 7 lanes) = 81 items
# tier C: degree, dtype, symmetric stress, mesh, block grid, pipelined
TIER_C = [
    (1, "f64", True, (30, 4, 10), (1, 1, 2), True),
    (2, "f32", False, (64, 4, 14), (2, 1, 2), True),
    (3, "f64", False, (30, 4, 10), (1, 1, 2), False),
    (3, "f32", True, (20, 5, 12), (1, 1, 2), True),
    (4, "f64", True, (30, 4, 10), (1, 1, 2), True),
    (4, "f32", False, (30, 4, 6), (1, 1, 2), False),
]


def tet_items(n):
    return (n[0] * n[1] * n[2] + 15) // 16 * 6


def hex_items(n):
    return (n[0] * n[1] * n[2] + 15) // 16


def mfma_grid(nitems, grid_blocks, wpb, slots=512):
    """blocks of launch_stage_mfma (not spread): grid_blocks counts slots of four waves, an eight-wave block takes two"""
    nblk = grid_blocks if grid_blocks else slots
    if wpb == 8:
        nblk = max(nblk // 16 * 8, 8)
    need = ((nitems + wpb - 1) // wpb + 7) // 8 * 8
    return min(need, nblk)


def hexm_grid(nitems, grid_blocks, degree, slots=None):
    """blocks of launch_stage_hexm: four-wave blocks, HXW<P>::WPE per CU"""
    cap = grid_blocks if grid_blocks else (slots if slots else 256 * (2 if degree <= 3 else 1))
    return (min((nitems + 3) // 4, cap) + 7) // 8 * 8


def items_per_wave(nitems, nblk, wpb, chunk=0):
    """{(block, wave): [item, ...]} of a launch of nblk blocks: item_range and item_of, one loop trip per entry"""
    out = {}
    for blk in range(nblk):
        xcd, slot = blk % 8, blk // 8
        blocks_here = (nblk - xcd + 7) // 8
        step = blocks_here * wpb
        for wave in range(wpb):
            if chunk > 0:
                nchunks = (nitems + chunk - 1) // chunk
                mine = (nchunks - xcd + 7) // 8
                lo, hi = slot * wpb + wave, max(mine, 0) * chunk
                its = []
                for it in range(lo, hi, step):
                    c = it // chunk
                    item = (c * 8 + xcd) * chunk + (it - c * chunk)
                    its.append(item if item < nitems else -1)
            else:
                ipx = (nitems + 7) // 8
                lo, hi = xcd * ipx + slot * wpb + wave, min((xcd + 1) * ipx, nitems)
                its = list(range(lo, hi, step))
            out[(blk, wave)] = its
    return out


def affine_grid_cap(prepared, value):
    """hostlogic.hpp affine_grid_cap: what SEIGEN_HIP_GRID_BLOCKS=value leaves of the grid prepared for an affine pre-pass"""
    return min(prepared, max(8, value // 8 * 8))


def affine_items(n, ncls, gw=16):
    """the items (cube group, class) plan_sponge lists for the affine pre-pass under test_mfma_family_gpu._sponge: kind =
    cell % 4 with cell = ncls * cube + class, kind 3 affine.  (Among tetrahedra kind = (2 cube + class) % 4: the items of an
    odd class hold kinds 1 and 3, those of an even class 0 and 2 - half the items are listed.  Kind 1, one value per cell,
    shares its items with kind 3: whether it counts as affine does not change the list.)"""
    cells = np.arange(n[0] * n[1] * n[2] * ncls)
    hit = cells[cells % 4 == 3]
    return len(np.unique(hit // ncls // gw * ncls + hit % ncls))


def affine_mfma_trips(nitems, grid):
    """loop trips of every wave of sponge_affine_mfma (the 3-D matrix-pipe family in double): a unit is one velocity
    component of an item, blocks of eight waves, min(ceil(units / 8), grid) of them"""
    units = 3 * nitems
    blocks = min((units + 7) // 8, grid)
    return [len(range(b * 8 + w, units, blocks * 8)) for b in range(blocks) for w in range(8)]


def pre_affine_trips(nitems, grid):
    """loop trips of every block of sponge_pre_affine_kernel (every other family, and float): a block per item"""
    blocks = min(grid, nitems)
    return [len(range(b, nitems, blocks)) for b in range(blocks)]


# grids prepared for the affine pre-passes on 256 CUs: one to four blocks per CU
AFFINE_PREPARED = (256, 512, 1024)


def _every_item_once(per_wave, nitems):
    seen = sorted(i for its in per_wave.values() for i in its if i >= 0)
    return seen == list(range(nitems))


def _labels_with_items(per_wave):
    return {blk % 8 for (blk, _), its in per_wave.items() if any(i >= 0 for i in its)}


def region_item_count(n, has_nbr, region, ncls=6, gw=16):
    """items that the launch of a region of a 3-D block lists: region_boxes' interior (one cube peeled off every side with a
    neighbour block, a whole group of gw cubes along x where shell_width_x says so), cut in two along z for SECOND"""
    assert region in ("interior", "second")
    lo, hi = [0, 0, 0], list(n)
    sides = int(has_nbr[0]) + int(has_nbr[1])
    xw = gw if 2 * (n[0] - sides * gw) >= n[0] else 1
    for a in range(3):
        w = xw if a == 0 else 1
        if has_nbr[2 * a]:
            lo[a] = min(w, n[a])
        if has_nbr[2 * a + 1]:
            hi[a] = max(n[a] - w, 0)
        hi[a] = max(hi[a], lo[a])
    if region == "second":
        lo[2] = lo[2] + (hi[2] - lo[2]) // 2
    ci, cj, ck = np.meshgrid(np.arange(lo[0], hi[0]), np.arange(lo[1], hi[1]), np.arange(lo[2], hi[2]), indexing="ij")
    groups = np.unique((ci + n[0] * (cj + n[1] * ck)) // gw)
    return len(groups) * ncls


def test_the_model_deals_every_item_once():
    for nitems in (1, 5, 6, 48, 71, 72, 81, 360, 1000):
        for wpb in (4, 8):
            for gb in (None, 8, 16, 96):
                nblk = mfma_grid(nitems, gb, wpb)
                assert nblk % 8 == 0 and nblk >= 8
                for chunk in (0, 1, 5, 7, 6, 400):
                    assert _every_item_once(items_per_wave(nitems, nblk, wpb, chunk), nitems), (nitems, wpb, gb, chunk)
        for P in (3, 4):
            for gb in (None, 8):
                assert _every_item_once(items_per_wave(nitems, hexm_grid(nitems, gb, P), 4), nitems)


def test_tier_a_shape_loops_on_the_forced_grid():
    """(15, 4, 3): on 8 blocks of four waves ipx = 9 and step 4 - wave 0 of every label runs 3 items, waves 1 to 3 run 2"""
    nitems = tet_items(TIER_A)
    assert nitems == 72 and TIER_A[0] * TIER_A[1] * TIER_A[2] % 16 == 4
    assert mfma_grid(nitems, 8, 4) == 8
    pw = items_per_wave(nitems, 8, 4)
    assert _labels_with_items(pw) == set(range(8))
    assert all(len(its) >= 2 for its in pw.values()) and max(len(its) for its in pw.values()) >= 3
    assert all(len(pw[(b, 0)]) == 3 and [len(pw[(b, w)]) for w in (1, 2, 3)] == [2, 2, 2] for b in range(8))
    # the library's own grid: no wave runs more than one item (what the family rows of test_mfma_family_gpu.py exercise)
    for slots in SLOTS:
        nblk = mfma_grid(nitems, None, 4, slots)
        assert nblk == 24
        assert max(len(its) for its in items_per_wave(nitems, nblk, 4).values()) == 1


def test_tier_a_stash_form_on_the_forced_grid():
    """The eight-wave blocks of the stash form (mfma_stage_G<double, 4, *, *, 1> by default) on (15, 4, 3): 8 blocks hold 64
    waves for 72 items, so only wave 0 of every label goes round twice.  Tier A holds that form to the oracle with this
    one second trip; tier B's (15, 8, 8) gives every one of its waves 5 or 6 items, and tests/test_g_stash_gpu.py six."""
    pw = items_per_wave(tet_items(TIER_A), mfma_grid(72, 8, 8), 8)
    assert len(pw) == 64
    assert all(len(pw[(b, 0)]) == 2 and all(len(pw[(b, w)]) == 1 for w in range(1, 8)) for b in range(8))


def test_tier_a_stash_block_makes_every_wave_of_the_stash_form_loop():
    """(15, 5, 5), the block of tier A's two extra rows of the stash form: 144 items on 8 eight-wave blocks, ipx = 18 and
    step 8 - waves 0 and 1 of every label run 3 items, waves 2 to 7 run 2; the library's own grid is 24 blocks, one item per
    wave.  Its affine pre-pass (sponge_affine_mfma, 72 items listed) runs 3 or 4 units per wave under the cap."""
    nitems = tet_items(TIER_A_STASH)
    assert nitems == 144 and TIER_A_STASH[0] * TIER_A_STASH[1] * TIER_A_STASH[2] % 16 == 7
    assert mfma_grid(nitems, 8, 8) == 8
    pw = items_per_wave(nitems, 8, 8)
    assert len(pw) == 64 and _labels_with_items(pw) == set(range(8))
    assert all([len(pw[(b, w)]) for w in range(8)] == [3, 3, 2, 2, 2, 2, 2, 2] for b in range(8))
    for slots in SLOTS:
        nblk = mfma_grid(nitems, None, 8, slots)
        assert nblk == 24
        assert max(len(its) for its in items_per_wave(nitems, nblk, 8).values()) == 1
    # the F stages of these rows, four-wave blocks: 4 or 5 items per wave
    assert {len(its) for its in items_per_wave(nitems, mfma_grid(nitems, 8, 4), 4).values()} == {4, 5}
    assert affine_items(TIER_A_STASH, 6) == 72
    assert set(affine_mfma_trips(72, affine_grid_cap(512, 8))) == {3, 4} and max(affine_mfma_trips(72, 256)) == 1


def _past_the_end_after_real(per_wave):
    return [k for k, its in per_wave.items() if any(a >= 0 > b for a, b in zip(its, its[1:]))]


def test_tier_a_chunk_override_meets_a_past_the_end_index_after_real_items():
    """SEIGEN_HIP_ORDER_CHUNK=5 on 72 items: 15 chunks, chunk 14 holds items 70 to 74 of which 72 to 74 do not exist.  It
    is the second chunk of label 6: its waves 0 and 1 run two items and then meet -1 (item_of's `continue` path), wave 3 one."""
    nitems = tet_items(TIER_A)
    pw = items_per_wave(nitems, 8, 4, TIER_A_CHUNK)
    assert (nitems + TIER_A_CHUNK - 1) // TIER_A_CHUNK == 15
    assert sum(its.count(-1) for its in pw.values()) == 3
    assert _past_the_end_after_real(pw) == [(6, 0), (6, 1), (6, 3)]
    assert pw[(6, 0)] == [30, 34, -1] and pw[(6, 2)] == [32, 71] and pw[(6, 3)] == [33, -1]
    # labels 0 to 5 hold two whole chunks: ten items, two or three per wave (label 7 holds one chunk)
    assert all(sorted(len(pw[(b, w)]) for w in range(4)) == [2, 2, 3, 3] for b in range(6))
    assert all(min(pw[(b, w)]) >= 0 for b in range(6) for w in range(4))


def test_a_past_the_end_index_is_never_followed_by_a_real_item():
    """Whatever the shape: the indices past the end are the tail of the last chunk, that chunk is the last of its label, and
    a wave walks its label's indices upwards - so `item_of(...) < 0` is only ever met after a wave's last real item."""
    for nitems in (1, 7, 72, 81, 360, 1001):
        for wpb in (4, 8):
            for nblk in (8, 16, 24, 96):
                for chunk in (1, 5, 6, 7, 13, 400):
                    pw = items_per_wave(nitems, nblk, wpb, chunk)
                    assert not any(a < 0 <= b for its in pw.values() for a, b in zip(its, its[1:])), (nitems, wpb, nblk, chunk)


def test_tier_b_shape_loops_on_the_forced_grid_and_not_on_the_librarys_own():
    """(15, 8, 8) and its ragged sibling (15, 7, 9): 360 items, 45 per label; 11 or 12 per wave on 8 four-wave blocks, 5 or
    6 on 8 eight-wave blocks; one per wave on the library's own grid in both forms; chunks of 7 do not divide 360"""
    nitems = tet_items(TIER_B)
    assert nitems == 360 == tet_items(TIER_B_RAGGED)
    assert TIER_B[0] * TIER_B[1] * TIER_B[2] % 16 == 0 and TIER_B_RAGGED[0] * TIER_B_RAGGED[1] * TIER_B_RAGGED[2] % 16 == 1
    assert TIER_B[2] < 16 and TIER_B_RAGGED[2] < 16        # the library's own item order is unchunked here
    for wpb, counts in ((4, {11, 12}), (8, {5, 6})):
        assert mfma_grid(nitems, 8, wpb) == 8
        pw = items_per_wave(nitems, 8, wpb)
        assert {len(its) for its in pw.values()} == counts
        for slots in SLOTS:
            own = items_per_wave(nitems, mfma_grid(nitems, None, wpb, slots), wpb)
            assert max(len(its) for its in own.values()) == 1, (wpb, slots)
    assert mfma_grid(nitems, None, 4) == 96 and mfma_grid(nitems, None, 8) == 48
    for chunk in TIER_B_CHUNKS:
        pw = items_per_wave(nitems, 8, 4, chunk)
        assert _every_item_once(pw, nitems) and min(sum(i >= 0 for i in its) for its in pw.values()) >= 2
    assert nitems % 7 != 0
    assert _past_the_end_after_real(items_per_wave(nitems, 8, 4, 7))


def test_tier_c_regions_list_well_over_32_items():
    """every block of every tier C case: the launch that takes the overridden grid - SECOND of a pipelined step, INTERIOR
    of an unpipelined one - lists at least 64 items, so on 8 blocks every wave of a four-wave kernel loops"""
    seen = set()
    for P, dtype, sym, n, grid, pipelined in TIER_C:
        assert all(n[a] % grid[a] == 0 for a in range(3))
        nb = tuple(n[a] // grid[a] for a in range(3))
        for bx in range(grid[0]):
            for bz in range(grid[2]):
                has = [bx > 0, bx < grid[0] - 1, False, False, bz > 0, bz < grid[2] - 1]
                cnt = region_item_count(nb, has, "second" if pipelined else "interior")
                assert cnt >= 64, (n, grid, bx, bz, cnt)
                pw = items_per_wave(cnt, mfma_grid(cnt, 8, 4), 4)
                assert max(len(its) for its in pw.values()) >= 3 and min(len(its) for its in pw.values()) >= 1
        seen.add((P, dtype, sym))
    assert len(TIER_C) == 6
    assert {c[0] for c in TIER_C} == {1, 2, 3, 4} and {c[1] for c in TIER_C} == {"f64", "f32"}
    assert {c[2] for c in TIER_C} == {True, False}
    assert any(c[4] == (2, 1, 2) for c in TIER_C) and any(not c[5] for c in TIER_C)


def test_tier_d_shape_loops_on_the_forced_grid_and_not_on_the_librarys_own():
    """(13, 9, 11) hexahedra: 81 items, ipx = 11 - three waves of a label run 3 items and one runs 2 (the last label: 4
    items); the library's own grid is 24 blocks with one item per wave"""
    nitems = hex_items(TIER_D)
    assert nitems == 81 and TIER_D[0] * TIER_D[1] * TIER_D[2] % 16 == 7
    for P in (3, 4):
        assert hexm_grid(nitems, 8, P) == 8
        pw = items_per_wave(nitems, 8, 4)
        assert all(sorted(len(pw[(b, w)]) for w in range(4)) == [2, 3, 3, 3] for b in range(7))
        assert sorted(len(pw[(7, w)]) for w in range(4)) == [1, 1, 1, 1]
        own = hexm_grid(nitems, None, P)
        assert own == 24
        assert max(len(its) for its in items_per_wave(nitems, own, 4).values()) == 1


def test_the_affine_pre_passes_loop_under_the_cap_and_not_without_it():
    """SEIGEN_HIP_GRID_BLOCKS=8 leaves 8 blocks of either affine pre-pass.  Tier A lists 36 of its 72 items: in double 108
    units on 64 waves - every wave runs one, 44 of them a second; in float 36 items on 8 blocks, 4 or 5 each.  Tier B lists
    180 (178 with the ragged end): 8 or 9 units per wave, 22 or 23 items per block.  Tier D, hexahedra, lists all 81 groups:
    10 or 11 per block of sponge_pre_affine_kernel<double, 3>.  On the prepared grids no wave or block goes round twice."""
    assert [affine_grid_cap(p, 8) for p in AFFINE_PREPARED] == [8, 8, 8]
    assert affine_grid_cap(256, 4) == 8 and affine_grid_cap(4, 8) == 4 and affine_grid_cap(256, 4096) == 256
    for n, ncls, listed, mfma, pre in ((TIER_A, 6, 36, {1, 2}, {4, 5}), (TIER_B, 6, 180, {8, 9}, {22, 23}),
                                       (TIER_B_RAGGED, 6, 178, {8, 9}, {22, 23}), (TIER_D, 1, 81, None, {10, 11})):
        nitems = affine_items(n, ncls)
        assert nitems == listed, (n, nitems)
        for prepared in AFFINE_PREPARED:
            grid = affine_grid_cap(prepared, 8)
            if mfma:
                trips = affine_mfma_trips(nitems, grid)
                assert len(trips) == 64 and set(trips) == mfma and sum(trips) == 3 * nitems, (n, sorted(set(trips)))
                assert max(affine_mfma_trips(nitems, prepared)) == 1
            trips = pre_affine_trips(nitems, grid)
            assert len(trips) == 8 and set(trips) == pre and sum(trips) == nitems and min(trips) >= 4, (n, sorted(set(trips)))
            assert max(pre_affine_trips(nitems, prepared)) == 1
