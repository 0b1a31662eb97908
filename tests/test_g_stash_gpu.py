"""The G stage kernels of degree 4 in double whose lifts take their OWN traces out of a wave-private LDS stash
(kernels_mfma.hip mfma_stage_G<double, 4, MODE, SYM, 1> launched with 512 threads: one block of eight waves per CU, the
4-row operator tiles stored compact; the default) against the oracle and, bit for bit, against the form before it, which the
same kernel objects run when launched with 256 threads (SEIGEN_HIP_GSTASH=0: four-wave blocks, own traces from memory).

Shapes, each the smallest at which a part can go wrong:
  3 x 2 x 2   12 cubes: one ragged cell group, 6 items - fewer than the waves of the one block that has items of its XCD
              label; idle waves must not touch the stash;
  5 x 3 x 3   45 cubes: the last group holds 13 of 16 lanes;
  8 x 4 x 4   128 cubes, 48 items, the persistent grid forced to its smallest (SEIGEN_HIP_GRID_BLOCKS=8).  The grid
              never has fewer than eight blocks - an item range belongs to an XCD label, blockIdx % 8 - so this shape gives
              every label one block and six of its waves one item each;
  16 x 8 x 8  1024 cubes, 384 items on that smallest grid: every wave of every block runs six items back to back and
              overwrites its stash five times (what the shape above cannot show with eight blocks).  Bitwise against the
              form without a stash only: the oracle takes a minute to set up 6144 cells.
On each: one plain G, one fused S1 (s = s + G(w)) and three whole LF4 steps from a smooth non-zero state, with symmetric
and full stress storage and with per-cell lambda / mu; tolerances as tests/test_parity_gpu.py has them for the same
quantities (1e-11 for one operator, ten times that after three steps)."""
import contextlib
import functools
import os

import numpy as np
import pytest

from oracle.lf4 import OracleLF4
from tests.util import oracle_mesh, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-11
DEGREE = 4
SHAPES = {
    "3x2x2": ((3, 2, 2), None),
    "5x3x3": ((5, 3, 3), None),
    "8x4x4-smallest-grid": ((8, 4, 4), "8"),
    "16x8x8-smallest-grid": ((16, 8, 8), "8"),
}
VARIANTS = {"sym": (True, False), "full": (False, False), "sym-percell": (True, True)}
CASES = [(s, v) for s in SHAPES for v in VARIANTS if not (s.startswith("16") and v == "sym-percell")]


@contextlib.contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


LENGTHS = (1.0, 0.8, 0.9)
ORACLE_SHAPES = [s for s in SHAPES if not s.startswith("16")]     # the oracle's set-up of 6144 cells takes a minute


@functools.lru_cache(maxsize=None)
def _oracle(shape):
    """The oracle's operators of a shape (seconds to set up): built once, shared by every variant and test."""
    return OracleLF4(oracle_mesh(3, SHAPES[shape][0], LENGTHS), DEGREE)


@functools.lru_cache(maxsize=None)
def _inputs(shape, variant):
    """Smooth fields on the node coordinates, per-cell material, and what the oracle makes of them (computed once)."""
    n, _ = SHAPES[shape]
    sym, per_cell = VARIANTS[variant]
    L = LENGTHS
    m = oracle_mesh(3, n, L)
    x = m.node_coords(DEGREE)                                   # [cell][node][3]
    ph = 2.0 * np.pi * (x[..., 0] / L[0] + 0.5 * x[..., 1] / L[1] + 0.25 * x[..., 2] / L[2])
    u = np.stack([np.sin(ph) + 0.3, np.cos(1.5 * ph) - 0.2, np.sin(0.5 * ph + 1.0)], axis=-1)
    w = np.stack([np.cos(ph), 0.5 + np.sin(2.0 * ph), np.cos(0.5 * ph - 0.3)], axis=-1)
    s = np.stack([np.stack([np.sin(ph + 0.1 * (3 * i + j)) + 0.05 * (i - j) for j in range(3)], axis=-1) for i in range(3)], axis=-2)
    if sym:
        s = 0.5 * (s + np.swapaxes(s, -1, -2))
    r = np.random.default_rng(9)
    lam = r.uniform(0.4, 0.8, m.ncells) if per_cell else 0.7
    mu = r.uniform(0.2, 0.4, m.ncells) if per_cell else 0.3
    dt = 0.05 * min(L[a] / n[a] for a in range(3)) / DEGREE ** 2
    ref = None
    if shape in ORACLE_SHAPES:
        orc = _oracle(shape)
        orc.dt, orc.l, orc.mu, orc.density = dt, lam, mu, 1.0
        orc.u0, orc.s0 = u, s
        for k in range(3):
            orc.step((k + 1) * dt)
        ref = dict(G=orc.E.apply_G(u, lam, mu), S1=s + orc.E.apply_G(w, lam, mu), u3=orc.u1, s3=orc.s1)
    for a in (u, w, s) + tuple((ref or {}).values()):
        a.setflags(write=False)
    return dict(n=n, L=L, u=u, w=w, s=s, lam=lam, mu=mu, dt=dt, sym=sym, ref=ref)


@functools.lru_cache(maxsize=None)
def _gpu_results(shape, variant, stash):
    from seigen_amd import _lib
    from seigen_amd.backend import HipBlock
    I = _inputs(shape, variant)
    n, L = I["n"], I["L"]
    with _env(SEIGEN_HIP_GSTASH=None if stash else "0", SEIGEN_HIP_GRID_BLOCKS=SHAPES[shape][1]):
        blk = HipBlock(3, DEGREE, n, [L[a] / n[a] for a in range(3)], [0.0] * 3, "left")
        blk.set_params(1.0, I["dt"], I["lam"], I["mu"])
        blk.set_field(_lib.FIELD_S, I["s"])
        assert blk.is_sym() == I["sym"]
        names = [blk.stage_kernel_name(st) for st in (_lib.STAGE_STEMP, _lib.STAGE_SH1, _lib.STAGE_S1)]      # one kernel object holds both forms
        assert names == ["sg::mfma_stage_G<double, 4, %d, %d, 1>" % (mode, int(I["sym"])) for mode in (0, 0, 1)], names
        out = {}
        blk.set_field(_lib.FIELD_U, I["u"])
        blk.apply_G(_lib.FIELD_U, _lib.FIELD_SH)
        out["G"] = blk.get_field(_lib.FIELD_SH)
        blk.set_field(_lib.FIELD_UH, I["w"])
        blk.run_stage(_lib.STAGE_S1)
        out["S1"] = blk.get_field(_lib.FIELD_S)
        blk.set_field(_lib.FIELD_U, I["u"])
        blk.set_field(_lib.FIELD_S, I["s"])
        blk.step(3)
        out["u3"] = blk.get_field(_lib.FIELD_U)
        out["s3"] = blk.get_field(_lib.FIELD_S)
        blk.close()
    return out


@pytest.mark.parametrize("shape,variant", [c for c in CASES if c[0] in ORACLE_SHAPES])
def test_stash_kernels_vs_oracle(gpu, shape, variant):
    ref = _inputs(shape, variant)["ref"]
    got = _gpu_results(shape, variant, True)
    errs = {k: rel_err(got[k], ref[k]) for k in ref}
    print(shape, variant, errs)
    assert errs["G"] < TOL and errs["S1"] < TOL, errs
    assert errs["u3"] < 10 * TOL and errs["s3"] < 10 * TOL, errs


@pytest.mark.parametrize("shape,variant", CASES)
def test_stash_kernels_bitwise_equal_to_own_traces_from_memory(gpu, shape, variant):
    on, off = _gpu_results(shape, variant, True), _gpu_results(shape, variant, False)
    for k in on:
        assert np.isfinite(on[k]).all(), k
        assert np.array_equal(on[k], off[k]), (k, rel_err(on[k], off[k]))


def test_stash_block_with_neighbour_blocks_bitwise(gpu):
    """2 x 1 x 2 blocks on one device: block (0, 0, 1) has a neighbour block on its +x and its -z side, the others on other
    pairs of sides; interior, shell and whole-block launches of the stash kernels, remote traces on the neighbour side
    only.  Equal to the single block bit for bit, in both stress storages."""
    from tests.test_harness_gpu import _multiblock_case
    for sym in (True, False):
        res = _multiblock_case(3, DEGREE, (4, 2, 4), (2, 1, 2), True, sym=sym)
        names = res["names"]
        assert any(nm.startswith("sg::mfma_stage_G<double, 4, ") and nm.endswith(", 1>") for nm in names), names
