"""The scripted lifetime of a handle (tests/lifetime_script.py), without a GPU: that the generated script reaches every
transition it is there for, that its mirror means what include/seigen_hip.h says, and the round-off floor between the two
CPU statements of the step (numpy oracle, plain-C port) that tests/test_lifetime_gpu.py builds its FP64 bound from.

The floor - the largest relative difference of the four fields at every checkpoint - is committed as
tests/golden/lifetime_floor.json (numbers only; `python tests/golden/make_lifetime_floor.py` writes it) and recomputed here:
the committed figures must be within a factor 2 of what this machine measures.  It is measured between two references, never
against the library.  The mirrors of all FP64 cases together, both engines, take about a minute on 8 threads (the numpy one
alone, which the GPU module runs, half of that)."""
import json
import os

import numpy as np
import pytest

from oracle.lf4 import OracleLF4
from tests import lifetime_script as ls
from tests.lifetime_script import CASES, FIELD_S, FIELD_U, SETTERS

FLOOR_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lifetime_floor.json")
FP64 = [c for c in CASES if c.dtype == "f64"]
SIZE_CLASSES = ("1", "2..7", "8", ">=9")


def _size_class(n):
    return "1" if n == 1 else ("2..7" if n < 8 else ("8" if n == 8 else ">=9"))


def _walk(script):
    """The script seen by a plain state machine (no fields): per operation what the handle holds when it runs -
    {"i", "op", "args", "capture": a graph has been captured before, "replayed": a sg_step that replays graphs, "source":
    a source is active when the call starts, "runs_out": it ends inside the call, "sponge", "receivers", "timing"}."""
    out = []
    capture = timing = sponge = False
    src_left = 0            # steps the source still has (None: static)
    rec = None              # [every, capacity, steps]
    for i, (op, a) in enumerate(script):
        row = dict(i=i, op=op, args=a, capture=capture, timing=timing, sponge=sponge, receivers=rec is not None,
                   source=src_left is None or src_left > 0, replayed=False, runs_out=False)
        if op == "enable_timing":
            timing = a["on"]
        elif op == "set_absorption":
            sponge = a["sigma"] is not None
        elif op == "set_source":
            src_left = 0 if len(a["nodes"]) == 0 else (None if a["static"] else len(a["values"]))
        elif op == "set_source_separable":
            src_left = len(a["weights"])
        elif op == "set_receivers":
            rec = [a["every"], a["capacity"], 0] if len(a["points"]) else None
        elif op in ls.STEPPING:
            n = a["n"]
            row["replayed"] = op == "step" and n >= 2 and not timing
            capture = capture or row["replayed"]
            if src_left is not None and src_left > 0:
                row["runs_out"] = src_left < n
                src_left = max(src_left - n, 0)
            if rec is not None:
                rec[2] += n
                row["samples"], row["capacity"] = rec[2] // rec[0], rec[1]
        out.append(row)
    return out


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_the_script_reaches_every_transition(case):
    script = ls.make_script(case)
    again = ls.make_script(case)
    assert [op for op, _ in script] == [op for op, _ in again]
    for (_, a), (_, b) in zip(script, again):                  # generated from the seed alone
        assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a if a[k] is not None)
    rows = _walk(script)
    steps = [r for r in rows if r["op"] in ls.STEPPING]
    calls = [r for r in rows if r["op"] == "step"]
    omitted = ls.OMITTED.get(case.name, {})

    # 1. the four ways sg_step splits a call, on the fresh handle: eager, the first capture, graph8 + graph1, graph8 alone
    assert [r["args"]["n"] for r in calls[:4]] == [1, 2, 9, 8] and not calls[0]["capture"] and calls[2]["capture"]
    # every setter is called after a capture exists and the next stepping call is a replay
    for setter in SETTERS:
        hit = False
        for r in rows:
            if r["op"] == setter and r["capture"]:
                nxt = next((s for s in steps if s["i"] > r["i"]), None)
                hit = hit or (nxt is not None and nxt["replayed"])
        assert hit, setter
    # every size class with and without a source, a sponge, receivers
    for what in ("source", "sponge", "receivers"):
        for on in (False, True):
            seen = {_size_class(r["args"]["n"]) for r in calls if r[what] == on and not r["timing"]}
            assert seen == set(SIZE_CLASSES), (what, on, seen)
    # a velocity upload between two stepping calls while a sponge is set: the whole field between two replays, a few cells
    # between two eager steps
    for op, replayed in (("set_field", True), ("set_field_range", False)):
        hit = False
        for k, r in enumerate(rows):
            if r["op"] == op and r["args"]["field"] == FIELD_U and r["sponge"] and r["args"]["tag"].startswith("sponge."):
                hit = hit or (rows[k - 1]["op"] == "step" and rows[k + 1]["op"] == "step"
                              and rows[k - 1]["replayed"] == rows[k + 1]["replayed"] == replayed)
        assert hit or ("sponge.upload" if op == "set_field" else "sponge.range") in omitted, op
    # a source that runs out inside a stepping call, and a replay without a source right after it
    k = next(k for k, r in enumerate(steps) if r["runs_out"])
    assert steps[k]["replayed"] and steps[k + 1]["replayed"] and not steps[k + 1]["source"]
    # the ways of stepping while a source is active: timed eager, replay, host-driven, replay
    assert any(r["timing"] and r["source"] and r["op"] == "step" for r in rows)
    k = next(k for k, r in enumerate(steps) if r["op"] == "host_steps")
    assert steps[k - 1]["replayed"] and steps[k + 1]["replayed"] and steps[k]["source"] and steps[k]["args"]["n"] == 2
    # receivers: the first trace exactly full, a host-driven step among the replays of the second
    full = [r for r in steps if r.get("samples") is not None]
    assert any(r["samples"] == r["capacity"] for r in full) and all(r["samples"] <= r["capacity"] for r in full)
    assert any(r["op"] == "host_steps" and r["receivers"] for r in steps)
    # float bounds count the steps of a stretch between two uploads of the whole state
    total = sum(r["args"]["n"] for r in steps)
    assert total > 3 * ls.MAX_STRETCH
    # what a case leaves out
    assert len(omitted) <= 2 and set(omitted) <= set(ls.TAGS)
    assert {a["tag"] for _, a in script} == set(ls.TAGS) - set(omitted)


def test_every_operation_runs_in_at_least_ten_cases():
    assert len(CASES) == 15 and len({c.name for c in CASES}) == 15
    assert set(ls.OMITTED) <= {c.name for c in CASES}
    for tag in ls.TAGS:
        assert sum(tag not in ls.OMITTED.get(c.name, {}) for c in CASES) >= 10, tag
    # symmetric-stress storage is left by the stress in some cases and by the source in the others
    first = {}
    for c in CASES:
        if c.sym and ls.sym_storage(c):
            first[c.name] = next(a["tag"] for _, a in ls.make_script(c) if a["tag"].startswith("sym."))
    assert sorted(set(first.values())) == ["sym.source", "sym.stress"], first
    assert sum(not c.sym for c in CASES) >= 2 and sum(c.dtype == "f32" for c in CASES) == 2


def test_the_mirror_means_what_the_header_says():
    """The mirror against an OracleLF4 driven by hand, on the smallest case: sg_set_params ends a density override, a source
    counts its steps from its own call and is silent once it has run out, a repeated node gets the sum, re-armed receivers
    count from the arming call, a non-symmetric stress ends symmetric-stress storage."""
    case = ls.case_by_name("lane-2d-P2")
    mir = ls.Mirror(case)
    rng = np.random.default_rng(1)
    nc, nd, d = mir.ncells, mir.nd, 2
    u0, s0 = rng.uniform(-1, 1, (nc, nd, d)), rng.uniform(-1, 1, (nc, nd, d, d))
    s0 = s0 + np.swapaxes(s0, -1, -2)
    nodes = np.array([5, 17, 5])
    vals = rng.uniform(-1, 1, (2, 3, d, d))
    vals = vals + np.swapaxes(vals, -1, -2)
    rho = rng.uniform(0.8, 1.2, nc)
    mir.set_params(1.1, 1e-3, 0.5, 0.25)
    mir.set_field(FIELD_U, u0)
    mir.set_field(FIELD_S, s0)
    mir.set_density(rho, physical=True)
    mir.step(1)
    mir.set_params(0.9, 2e-3, 0.6, 0.3)              # the override ends here
    mir.set_source(nodes, vals)
    assert mir.is_sym()
    mir.set_receivers(np.array([[0.31, 0.42]]), 1, 2, 4)
    mir.step(3)                                      # the source covers two of them

    orc = OracleLF4(ls.case_mesh(case), case.degree)
    orc.u0, orc.s0 = u0, s0
    orc.dt, orc.l, orc.mu, orc.density, orc.density_physical = 1e-3, 0.5, 0.25, rho, True
    orc.step(None)
    orc.dt, orc.l, orc.mu, orc.density, orc.density_physical = 2e-3, 0.6, 0.3, 0.9, False
    for k in range(3):
        S = np.zeros((nc * nd, d, d))
        if k < 2:
            S[5] = vals[k, 0] + vals[k, 2]
            S[17] = vals[k, 1]
        orc.source = lambda t, S=S: S.reshape(nc, nd, d, d)
        orc.step(None)
        if k == 1:
            u_at_2 = orc.u1
    assert np.array_equal(mir.get_field(FIELD_U), orc.u1) and np.array_equal(mir.get_field(FIELD_S), orc.s1)
    assert mir.counters() == dict(steps=4, launches=[4] * 6)
    tr = mir.get_receivers()
    cell, phi = ls.receiver_basis(case, np.array([[0.31, 0.42]]))
    assert tr.shape == (1, 1, 2) and np.array_equal(tr[0, 0], phi[0] @ u_at_2[cell[0]])      # after step 2 of the arming
    mir.set_field_range(FIELD_S, 3, rng.uniform(-1, 1, (1, nd, d, d)))
    assert not mir.is_sym()


def measure_floor(case):
    _, a = ls.mirror_run(case, "numpy")
    _, b = ls.mirror_run(case, "cport")
    return ls.floor_of(a, b)


def committed_floor():
    with open(FLOOR_FILE) as f:
        return json.load(f)


@pytest.mark.parametrize("case", FP64, ids=[c.name for c in FP64])
def test_the_committed_floor_is_what_two_references_differ_by(case):
    want = committed_floor()[case.name]
    got = measure_floor(case)
    assert len(got) == len(want) and min(got) > 0
    for k, (g, w) in enumerate(zip(got, want)):
        assert 0.5 * g <= w <= 2.0 * g, (case.name, k, g, w)
    # round-off, growing no faster than the steps: far below the suite's own figure for three steps
    assert max(want) < 1e-12
