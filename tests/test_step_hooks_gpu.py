"""All four end-of-step hooks - receivers, monitor, spectra, injectors (seigen_amd/csrc/stages.cpp hooks) - and a
time-dependent source armed on ONE handle, at different steps, so that their clocks and their device-side step counters all
differ: every way of driving the steps leaves the same bits.  The per-feature files make these claims one feature at a time
(test_receivers_gpu, test_monitor_gpu, test_spectra_gpu, test_injectors_gpu, test_graph_source_gpu); nothing is compared
against a tolerance here.

The run, 15 steps:
  step 0        a source with a value table of 9 steps: its last slice goes into step 9, steps 10 .. 15 add nothing
  1 step
  after step 1  receivers, every 2, capacity 7: 14 steps follow the arming, samples after steps 3, 5, .. 15 = 14 // 2 = 7 <= 7
                monitor, every 3, capacity 5: samples after steps 4, 7, 10, 13 = 14 // 3 = 4 <= 5
                (neither trace refuses a step; a call of 11 steps at 3 completed: (3 + 11) // 2 = 7 and (3 + 11) // 3 = 4 fit)
  3 steps
  after step 4  spectra, every 2, 3 samples, 2 frequencies, velocity and stress: samples after steps 6, 8, 10 - run out after
                6 of the 11 steps that follow
                injectors, 5 entries, velocity and a symmetric stress (the storage mode stays): entries at the end of steps
                5 .. 9 - run out after 5 of the 11
  11 steps      in the pattern of the way
so the last 11 steps begin with everything active and run past the end of the source, the spectra and the injectors: eager
launches stop, replayed launches go on and must add nothing, and the graphs are captured anew after each arming.

Shapes: the smallest that reach each stepping path - the 2-D tile kernels (the source fused into the G stages, its counter
bumped by the launch that opens a step), the 3-D matrix-pipe kernels at P4 (source launches; the separate G stash form), the
lane-per-cell kernels on the smallest mesh tests/test_lane_generic_family_gpu.py gives them in 3-D."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (name, dim, degree, cubes, SEIGEN_HIP_PATH, expected kernel-name prefix)
CASES = [
    ("tile-tri-P3", 2, 3, (6, 5), None, "sg::tile2d_stage<"),
    ("mfma-P4", 3, 4, (3, 2, 2), None, "sg::mfma_stage_"),
    ("lane-3d-P1", 3, 1, (1, 1, 1), "lane", "sg::lane_"),
]
# way -> (SEIGEN_HIP_GRAPH, the calls of the last 11 steps; None: host-driven stages with sg_end_step, every step of the run)
WAYS = {
    "eager": ("0", (11,)),
    "graph": ("1", (11,)),          # one eight-step graph and three one-step graphs
    "graph-2-1-8": ("1", (2, 1, 8)),  # two one-step graphs, an eager step, one eight-step graph
    "stages": (None, None),
}
SWITCHES = ("SEIGEN_HIP_PATH", "SEIGEN_HIP_GRAPH", "SEIGEN_HIP_SPONGE_AFFINE", "SEIGEN_HIP_SYM", "SEIGEN_HIP_SOURCE_LAUNCH")


def _run(monkeypatch, case, way):
    from seigen_amd import _lib
    from seigen_amd.backend import HipBlock
    from tests.util import seeded
    name, dim, degree, n, path, prefix = case
    graph, calls = WAYS[way]
    for var in SWITCHES:
        monkeypatch.delenv(var, raising=False)
    if path:
        monkeypatch.setenv("SEIGEN_HIP_PATH", path)
    if graph is not None:
        monkeypatch.setenv("SEIGEN_HIP_GRAPH", graph)
    h = [1.0 / k for k in n]
    blk = HipBlock(dim, degree, n, h, [0.0] * dim, "left")
    assert blk.stage_kernel_name(0).startswith(prefix), blk.stage_kernel_name(0)
    blk.set_params(1.0, 0.05 * min(h) / degree ** 2, 0.5, 0.25)
    blk.set_field(_lib.FIELD_U, seeded(blk.field_shape(_lib.FIELD_U), 1))
    s0 = seeded(blk.field_shape(_lib.FIELD_S), 2)
    blk.set_field(_lib.FIELD_S, 0.5 * (s0 + np.swapaxes(s0, -1, -2)))
    Xq = blk.node_coords(2)
    blk.set_absorption(np.where(Xq[..., 0] >= 0.5, 10.0 + 20.0 * Xq[..., 0], 0.0), 2)
    rng = np.random.default_rng(41)
    nodes = np.unique(rng.integers(0, blk.ncells * blk.nd, size=12))
    sv = rng.uniform(-1, 1, size=(9, len(nodes), dim, dim))
    rec_pts = rng.uniform(0.05, 0.95, size=(3, dim))
    inj_pts = rng.uniform(0.05, 0.95, size=(3, dim))
    inj_pts[1] = inj_pts[0] + 0.01          # two points of one cell (or of neighbours): the order of the kernel's sum
    au = rng.uniform(-1, 1, size=(5, 3, dim))
    as_ = rng.uniform(-1, 1, size=(5, 3, dim, dim))
    series = np.concatenate([au, (0.5 * (as_ + np.swapaxes(as_, -1, -2))).reshape(5, 3, dim * dim)], axis=-1)
    w = rng.uniform(-1, 1, size=(2, 3, 2)) + 1j * rng.uniform(-1, 1, size=(2, 3, 2))

    def step(calls_):
        if calls is None:
            for _ in range(sum(calls_)):
                for st in range(6):
                    blk.run_stage(st)
                blk.end_step()
        else:
            for c in calls_:
                blk.step(c)

    was_sym = blk.is_sym()
    blk.set_source(nodes, 0.5 * (sv + np.swapaxes(sv, -1, -2)))
    step((1,))
    assert blk.set_receivers(rec_pts, 3, 2, 7).all()
    blk.set_monitor(3, 5)
    step((3,))
    blk.set_spectra(w[0], w[1], every=2)
    assert blk.set_injectors(inj_pts, series, 3).all()
    step(calls if calls is not None else (11,))
    assert blk.is_sym() == was_sym
    out = {
        "steps": blk.counters()["steps"],
        "u1": blk.get_field(_lib.FIELD_U),
        "s1": blk.get_field(_lib.FIELD_S),
        "receivers": blk.get_receivers(),
        "monitor": blk.get_monitor(),
        "spectra_samples": blk.spectra_samples(),
    }
    for f in range(2):
        out["spectrum-u-%d" % f] = blk.get_spectrum(0, f)
        out["spectrum-s-%d" % f] = blk.get_spectrum(1, f)
    blk.close()
    return out


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_all_hooks_on_one_handle_bitwise_across_the_ways_of_stepping(gpu, monkeypatch, case):
    """SEIGEN_HIP_GRAPH=0 in one call, graph replay in one call, graph replay in calls of 2, 1 and 8, and sg_run_stage x 6 +
    sg_end_step: the same final u1 and s1, receiver traces, monitor trace and spectra, bit for bit, with the same counts."""
    out = {way: _run(monkeypatch, case, way) for way in WAYS}
    ref = out["eager"]
    assert ref["receivers"].shape[0] == 7 and ref["monitor"].shape[0] == 4 and ref["spectra_samples"] == 3
    assert np.abs(ref["receivers"][-1]).max() > 0
    assert np.abs(ref["monitor"][-1]).max() > 0 and np.abs(ref["spectrum-u-1"]).max() > 0 and np.abs(ref["spectrum-s-1"]).max() > 0
    assert np.isfinite(ref["u1"]).all() and np.isfinite(ref["s1"]).all()
    for way, got in out.items():
        assert got["steps"] == 15, way
        assert got["spectra_samples"] == ref["spectra_samples"], way
        for key in ref:
            if key not in ("steps", "spectra_samples"):
                assert got[key].shape == ref[key].shape and np.array_equal(got[key], ref[key]), (way, key)
