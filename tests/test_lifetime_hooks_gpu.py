"""One handle whose monitor, spectra and injectors are armed, re-armed and disarmed, whose fields are written by sg_inject, by
an injector series and by sg_set_field_dev, and which is read through the device readers - all between stepping calls on a
handle that already holds graphs, a sponge pre-pass, running counters and the other hooks - against the oracle after every
stepping call.

tests/test_lifetime_gpu.py does this for the setters of the first script; this module runs the second script of
tests/lifetime_script.py (make_hooks_script, 78 steps) on the same fifteen cases: the three hooks armed one after the other
behind a capture, a step that all of them and the receivers sample while a large injector entry lands at its end, series that
run out inside a replay, the velocity written from a device buffer and by an injection under the sponge, symmetric-stress
storage left with stress spectra armed (by a few stress cells from a device buffer, by a stress series, by sg_leave_sym, in
turn over the cases), a source and sg_set_params in mid-run, host-driven and timed steps, sg_get_field_dev,
sg_get_spectrum_dev, sg_get_frame_dev and sg_measure between two replays.  The mirror says what every observation must be.
Each case runs twice, with graph replay and with SEIGEN_HIP_GRAPH=0: both against the mirror, and against each other bit for
bit in fields, traces, monitor samples, spectra, downloads and frames.

Bounds, all from tests/test_lifetime_gpu.py _bounds - b(c, k): FP64 max(10 tol_of, 10 x the floor of checkpoint c in
tests/golden/lifetime_hooks_floor.json), float 5e-5 ceil(k / 3) for the k steps since both fields were last handed over whole
(by sg_set_field or by sg_set_field_dev; an injection or a few cells do not restart the count).
  fields at a checkpoint        b, relative to the field's largest value
  receiver sample               b at the sample's step x max_k sum_a |phi_a(xi_k)|, relative to the field's largest value then
  spectrum (either reader)      sum_j |w_j| b_j max |field_j| over the samples taken, absolute
  monitor sample, sg_measure    (2 b + 1e-11) x the same sample taken with |w| (the samples are quadratic in the state; 1e-11 is
                                the summation term of tests/test_monitor_gpu.py; |w| because wt < 0 cancels in ES)
  sg_get_field_dev              b; and bitwise sg_get_field_range of the same cells on the same handle
  sg_get_frame_dev              b x max_pixel sum_a |phi_a| x the field's largest value

Every figure is printed before it is asserted on (LIFETIME-HOOKS ...).  Largest relative error of the fields over all
checkpoints of a case on an MI355X, and in brackets the largest error / bound over ALL its observations (a record, not a
bound; the replay and the eager run agree to the bit; FP64 bound 1e-10, DQ_4 5e-10, float 5e-5 .. 4.5e-4):
  generic-1d-P2 1.8e-15 (2.0e-5)   generic-2d-P2 6.0e-15 (6.0e-5)   lane-2d-P2 3.9e-15 (4.1e-5)     lane-hex-DQ2 4.9e-15 (4.9e-5)
  tile-tri-P3 1.0e-14 (1.0e-4)     tile-quad-P2 3.2e-15 (3.2e-5)    mfma-P3-sym 1.6e-14 (1.6e-4)    mfma-P3-full 1.3e-14 (1.3e-4)
  mfma-P4-sym 2.0e-13 (2.0e-3)     mfma-P4-full 2.1e-13 (2.8e-3)    mfma-P4-f32 6.9e-7 (4.3e-3)     hexm-DQ3 1.7e-14 (1.7e-4)
  hexm-DQ4 1.9e-13 (4.3e-4)        tile-tri-P3-f32 7.3e-7 (5.3e-3)  lane-hex-DQ2-affine 4.8e-15 (5.3e-5)
Seeded in a scratch build, case mfma-P3-sym (mfma-P4-sym fails at the same checkpoints): sg_set_field_dev without its
Fields::write fails the replay run at checkpoint 15 (dev.range, step 57, the eager step behind the few velocity cells: 0.020);
queue_inject taking the velocity with Fields::read instead of write fails the replay run at checkpoint 8 (size.classes, step
36, the call behind the eager step at whose end the large entry landed: 3.0e-4) - and passed while the injectors' cells had
no sponge, which is why the script gives those cells one (tests/test_lifetime_oracle.py asserts it)."""
import json
import os

import numpy as np
import pytest

from tests import lifetime_script as ls
from tests.lifetime_script import CASES, rel_field_error
from tests.test_lifetime_gpu import FIELDS, _block, _bounds, _environment, moved

pytestmark = pytest.mark.gpu

FLOOR_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lifetime_hooks_floor.json")
BITWISE = FIELDS + ("traces", "samples", "sample", "acc", "dev", "range", "frame", "taken", "owned")


def compare(case, mode, got, want, floor):
    """every observation of a run against the mirror's; returns the largest error / bound and the largest field error"""
    assert [(o["i"], o["op"]) for o in got] == [(o["i"], o["op"]) for o in want]
    bound_at, _ = _bounds(case, floor)
    worst, worst_err, c, last = 0.0, 0.0, 0, None

    def report(where, err, bound):
        print("LIFETIME-HOOKS %s: %.3e of %.1e" % (where, err, bound))
        return max(worst, err / bound if bound > 0 else 0.0)

    for g, w in zip(got, want):
        where = "%s %s op %d %s (%s)" % (case.name, mode, w["i"], w["op"], w["tag"])
        op = w["op"]
        if op == "kernels":
            assert g["names"] == w["names"], where
        elif op in ("set_receivers", "set_injectors"):
            assert np.array_equal(g["owned"], w["owned"]), where
        elif op == "spectra_samples":
            assert g["taken"] == w["taken"], where
        elif op == "get_receivers":
            assert g["traces"].shape == w["traces"].shape, where
            nu = case.dim if w["what"] & 1 else 0
            for j in range(len(w["traces"])):
                diff = np.abs(g["traces"][j] - w["traces"][j])
                eu = diff[:, :nu].max() / w["scales"][j][0] if nu else 0.0
                es = diff[:, nu:].max() / w["scales"][j][1] if diff.shape[1] > nu else 0.0
                bound = bound_at(*w["log"][j]) * w["lebesgue"]
                worst = report("%s sample %d" % (where, j), max(eu, es), bound)
                assert max(eu, es) < bound, (where, j)
            assert len(w["traces"]) == 0 or np.abs(w["traces"]).max() > 0
        elif op in ("get_monitor", "measure"):
            gs, ws = (g["samples"], w["samples"]) if op == "get_monitor" else (g["sample"][None], w["sample"][None])
            scale = np.reshape(w["abs"], (-1, 5)) if len(ws) else np.zeros((0, 5))
            assert gs.shape == ws.shape, where
            for j in range(len(ws)):
                b = bound_at(*w["log"][j]) if op == "get_monitor" else last
                allow = (2.0 * b + 1e-11) * scale[j]
                err = np.abs(gs[j] - ws[j])
                rel = float((err[scale[j] > 0] / scale[j][scale[j] > 0]).max())
                worst = report("%s sample %d" % (where, j), rel, 2.0 * b + 1e-11)
                assert np.all(err <= allow) and scale[j][:3].min() > 0, (where, j, gs[j], ws[j])
        elif op in ("get_spectrum", "get_spectrum_dev"):
            assert g["acc"].shape == w["acc"].shape and g["acc"].dtype == np.complex128, where
            bound = sum(aw * bound_at(cc, k) * scale for aw, cc, k, scale in w["terms"])
            err = float(np.abs(g["acc"] - w["acc"]).max())
            worst = report("%s %d samples" % (where, len(w["terms"])), err, bound)
            assert err <= bound and (len(w["terms"]) == 0 or np.abs(w["acc"]).max() > 0), where
        elif op == "get_field_dev":
            assert np.array_equal(g["dev"], g["range"]), where
            err = rel_field_error(g["dev"], w["dev"])
            worst = report(where, err, last)
            assert g["dev"].shape == w["dev"].shape and err < last, where
        elif op == "get_frame_dev":
            assert g["frame"].shape == w["frame"].shape, where
            bound = last * w["lebesgue"] * w["scale"]
            err = float(np.abs(g["frame"] - w["frame"]).max())
            worst = report(where, err, bound)
            assert err < bound and np.abs(w["frame"]).max() > 0, where
        else:
            assert op in ls.STEPPING, op
            assert (g["steps"], g["launches"]) == (w["steps"], w["launches"]), where
            assert g["sym"] == w["sym"], where
            bound = last = bound_at(c, w["stretch"])
            errs = [rel_field_error(g[k], w[k]) for k in FIELDS]
            print("LIFETIME-HOOKS %s checkpoint %d, step %d: %s of %.1e" % (where, c, w["steps"], " ".join("%.3e" % e for e in errs), bound))
            assert max(errs) < bound, (where, c, errs)
            worst, worst_err = max(worst, max(errs) / bound), max(worst_err, max(errs))
            c += 1
    return worst, worst_err


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_a_lifetime_of_hooks_against_the_oracle(gpu, monkeypatch, case):
    script, want = ls.hooks_mirror_run(case)
    floor = None
    if case.dtype == "f64":
        with open(FLOOR_FILE) as f:
            floor = json.load(f)[case.name]
        assert len(floor) == moved(want)
    else:
        moved(want)
    runs = {}
    for mode, graph in (("replay", None), ("eager", "0")):
        _environment(monkeypatch, case, graph)
        blk = _block(case)
        try:
            runs[mode] = ls.run_script(blk, script)
        finally:
            blk.close()
        print("LIFETIME-HOOKS-WORST %s %s: %.2e of its bound, fields %.2e" % ((case.name, mode) + compare(case, mode, runs[mode], want, floor)))
    for a, b in zip(runs["replay"], runs["eager"]):
        for k in BITWISE:
            if k in a:
                assert np.array_equal(a[k], b[k]), (case.name, a["i"], a["op"], k)
