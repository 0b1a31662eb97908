"""The scripted lifetime of a handle (tests/lifetime_script.py), without a GPU: that the generated script reaches every
transition it is there for, that its mirror means what include/seigen_hip.h says, and the round-off floor between the two
CPU statements of the step (numpy oracle, plain-C port) that tests/test_lifetime_gpu.py builds its FP64 bound from.

The floor - the largest relative difference of the four fields at every checkpoint - is committed as
tests/golden/lifetime_floor.json (numbers only; `python tests/golden/make_lifetime_floor.py` writes it) and recomputed here:
the committed figures must be within a factor 2 of what this machine measures.  It is measured between two references, never
against the library.  The mirrors of all FP64 cases together, both engines, take about a minute on 8 threads (the numpy one
alone, which the GPU module runs, half of that).

The same three for the second script (make_hooks_script: monitor, spectra, injectors, device transfers; run by
tests/test_lifetime_hooks_gpu.py): its walker, its mirror operations against an oracle stepped by hand, and its floor,
tests/golden/lifetime_hooks_floor.json (`python tests/golden/make_lifetime_floor.py hooks`), half a minute more."""
import json
import os

import numpy as np
import pytest

from oracle.lf4 import OracleLF4
from tests import lifetime_script as ls
from tests.lifetime_script import CASES, FIELD_S, FIELD_U, SETTERS

FLOOR_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lifetime_floor.json")
HOOKS_FLOOR_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lifetime_hooks_floor.json")
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


# ---- the second script: hooks, injections, device transfers (lifetime_script.make_hooks_script) -------------------------------

READERS = ("measure", "get_field_dev", "get_spectrum_dev", "get_frame_dev")


def _whole(case, a):
    return a["cell0"] == 0 and len(a["values"]) == int(np.prod(case.n)) * ls.ncls_of(case)


def _walk_hooks(case, script):
    """The second script seen by a plain state machine: per operation what the handle holds when it runs.  A hook is "on"
    while armed with something left to do: room in the monitor's trace, rows of the spectra's table, entries of the series."""
    out = []
    capture = timing = sponge = False
    src_left = 0
    rec = mon = spc = inj = None        # [every, capacity, steps] / [every, capacity, steps] / [every, nsamples, steps] / [entries, steps, series]
    fresh, stretch = set(), 0
    for i, (op, a) in enumerate(script):
        row = dict(i=i, op=op, args=a, capture=capture, timing=timing, sponge=sponge, receivers=rec is not None,
                   source=src_left > 0, replayed=False,
                   monitor=mon is not None and mon[2] // mon[0] < mon[1], monitor_armed=mon is not None,
                   spectra=spc is not None and spc[2] // spc[0] < spc[1], spectra_armed=spc is not None,
                   spectra_stress=spc is not None and spc[3], injectors=inj is not None and inj[1] < inj[0],
                   injectors_armed=inj is not None, mon_every=mon[0] if mon else None, spc_every=spc[0] if spc else None,
                   inj_entries=inj[0] if inj else None)
        if op == "enable_timing":
            timing = a["on"]
        elif op == "set_absorption":
            sponge = a["sigma"] is not None
        elif op == "set_source":
            src_left = 0 if len(a["nodes"]) == 0 else len(a["values"])
        elif op == "set_receivers":
            rec = [a["every"], a["capacity"], 0] if len(a["points"]) else None
        elif op == "set_monitor":
            mon = [a["every"], a["capacity"], 0] if a["every"] else None
            row["arms"] = mon is not None
        elif op == "set_spectra":
            w = a["wu"] if a["wu"] is not None else a["ws"]
            spc = [a["every"], len(w), 0, a["ws"] is not None] if w is not None else None
            row["arms"] = spc is not None
            assert w is None or w.shape[1] <= 2                       # at most two frequencies
        elif op == "set_injectors":
            inj = [len(a["series"]), 0, a["series"]] if len(a["points"]) else None
            row["arms"] = inj is not None
        elif op in ("set_field", "set_field_dev"):
            if op == "set_field" or _whole(case, a):
                fresh.add(a["field"])
        elif op in ls.STEPPING:
            n = a["n"]
            row["replayed"] = op == "step" and n >= 2 and not timing
            capture = capture or row["replayed"]
            if {FIELD_U, FIELD_S} <= fresh:
                stretch = 0
            fresh = set()
            stretch += n
            row["stretch"] = stretch
            src_left = max(src_left - n, 0)
            if rec is not None:
                row["rec_sample_last"] = (rec[2] + n) % rec[0] == 0
                rec[2] += n
                assert rec[2] // rec[0] <= rec[1]
            if mon is not None:
                row["mon_sample_last"] = (mon[2] + n) % mon[0] == 0
                mon[2] += n
                assert mon[2] // mon[0] <= mon[1], "a stepping call the library refuses"
                row["mon_full"] = mon[2] == mon[0] * mon[1]
            if spc is not None:
                row["spc_sample_last"] = (spc[2] + n) % spc[0] == 0 and (spc[2] + n) // spc[0] <= spc[1]
                row["spc_runs_out"] = spc[2] < spc[0] * spc[1] < spc[2] + n
                spc[2] += n
            if inj is not None:
                row["inj_entry_last"] = inj[2][inj[1] + n - 1] if inj[1] + n <= inj[0] else None
                row["inj_runs_out"] = inj[1] < inj[0] < inj[1] + n
                inj[1] += n
        out.append(row)
    return out


def _is_disarm(r):
    return r["op"] in ("set_monitor", "set_spectra", "set_injectors") and not r["arms"]


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_the_hooks_script_reaches_every_transition(case):
    from seigen_amd.backend import injector_weights
    script = ls.make_hooks_script(case)
    again = ls.make_hooks_script(case)
    assert [op for op, _ in script] == [op for op, _ in again]
    for (_, a), (_, b) in zip(script, again):                  # generated from the seed alone
        assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a if a[k] is not None and not isinstance(a[k], dict))
    rows = _walk_hooks(case, script)
    steps = [r for r in rows if r["op"] in ls.STEPPING]
    calls = [r for r in rows if r["op"] == "step"]
    hooks = ("monitor", "spectra", "injectors")
    setter_of = dict(monitor="set_monitor", spectra="set_spectra", injectors="set_injectors")
    nc, ncls = int(np.prod(case.n)) * ls.ncls_of(case), ls.ncls_of(case)

    def nxt(r):
        return next((s for s in steps if s["i"] > r["i"]), None)

    def prv(r):
        return next((s for s in reversed(steps) if s["i"] < r["i"]), None)

    def between_replays(r, replayed=True):
        p, n = prv(r), nxt(r)
        return p is not None and n is not None and p["op"] == n["op"] == "step" and p["replayed"] == n["replayed"] == replayed \
            and (replayed or p["args"]["n"] == n["args"]["n"] == 1)

    # about 70 steps, stretches of the float bound within MAX_STRETCH
    total = sum(r["args"]["n"] for r in steps)
    assert 60 <= total <= 80 and max(r["stretch"] for r in steps) <= ls.MAX_STRETCH
    # the fresh handle: every size class with no hook, the first capture among them
    assert [r["args"]["n"] for r in calls[:4]] == [1, 2, 9, 8] and not calls[0]["capture"] and calls[2]["capture"]
    # every new setter after a capture with a replay as the next stepping call; the same for disarming each hook
    for setter in ls.HOOK_SETTERS:
        assert any(r["op"] == setter and r["capture"] and r.get("arms", True) and nxt(r) is not None and nxt(r)["replayed"]
                   for r in rows), setter
    for hook in hooks:
        others = [h for h in hooks if h != hook]
        mine = [r for r in rows if r["op"] == setter_of[hook]]
        # armed while the other two and the receivers are armed and running
        assert any(r["arms"] and r["receivers"] and all(r[o] for o in others) for r in mine), hook
        # armed again while armed, with another `every` (the injectors: another number of entries)
        key = dict(monitor="mon_every", spectra="spc_every", injectors="inj_entries")[hook]
        new = lambda r: r["args"]["every"] if hook != "injectors" else len(r["args"]["series"])      # noqa: E731
        assert any(r["arms"] and r[hook + "_armed"] and r[key] != new(r) for r in mine), hook
        # disarmed while the others keep running, behind a capture, a replay next
        assert any(_is_disarm(r) and r[hook + "_armed"] and r["capture"] and all(r[o] for o in others) and r["receivers"]
                   and nxt(r)["replayed"] for r in mine), hook
        # every size class with the hook on and off
        for on in (False, True):
            seen = {_size_class(r["args"]["n"]) for r in calls if r[hook] == on and not r["timing"]}
            assert seen == set(SIZE_CLASSES), (hook, on, seen)
    # the monitor with one weight triple, with weights per cell and with none
    shapes = {np.shape(r["args"]["w"]) for r in rows if r["op"] == "set_monitor" and r["arms"]}
    assert {(3,), (nc, 3), ()} <= shapes, shapes
    # series that run out: the monitor's trace exactly full; the spectra's table and the injectors' series end inside a
    # replayed call, and the next call is a replay with the hook still armed, which must add nothing
    assert any(r.get("mon_full") for r in steps)
    for hook, key in (("spectra", "spc_runs_out"), ("injectors", "inj_runs_out")):
        k = next(k for k, r in enumerate(steps) if r.get(key))
        assert steps[k]["replayed"] and steps[k + 1]["replayed"] and steps[k + 1][hook + "_armed"] and not steps[k + 1][hook], hook
    # under the sponge: the whole velocity from a device buffer between two replays, a few cells from the middle of a cube
    # between two eager single steps, a velocity injection between two eager single steps
    dev_u = [r for r in rows if r["op"] == "set_field_dev" and r["args"]["field"] == FIELD_U and r["sponge"]]
    assert any(_whole(case, r["args"]) and between_replays(r) for r in dev_u)
    assert any(not _whole(case, r["args"]) and (ncls == 1 or r["args"]["cell0"] % ncls) and 0 < len(r["args"]["values"]) <= 3
               and between_replays(r, False) for r in dev_u)
    assert any(r["op"] == "inject" and r["args"]["what"] & 1 and r["sponge"] and between_replays(r, False) for r in rows)
    # leaving symmetric storage: stress spectra armed and running, graphs captured, kernel names pinned around the call,
    # the stress spectrum read before the call and after the next stepping call
    k = next(k for k, r in enumerate(rows) if r["args"]["tag"] == "sym.leave" and r["op"] in ls.SYM_LEAVERS)
    r = rows[k]
    assert r["op"] == ls.SYM_LEAVERS[CASES.index(case) % 3] and r["capture"] and r["spectra"] and r["spectra_stress"]
    assert rows[k - 1]["op"] == rows[k + 1]["op"] == "kernels" and nxt(r)["replayed"]
    spectrum_s = lambda x: x["op"] == "get_spectrum" and x["args"]["field"] == 1      # noqa: E731
    assert spectrum_s(rows[k - 2]) and any(spectrum_s(x) for x in rows[nxt(r)["i"] + 1:nxt(nxt(r))["i"]])
    if r["op"] == "set_field_dev":
        v = r["args"]["values"]
        assert r["args"]["field"] == FIELD_S and not _whole(case, r["args"]) and (case.dim == 1 or np.any(v != np.swapaxes(v, -1, -2)))
    if r["op"] == "set_injectors":
        d = case.dim
        v = r["args"]["series"].reshape(-1, 3, d, d)
        assert r["args"]["what"] == 2 and (case.dim == 1 or np.any(v != np.swapaxes(v, -1, -2)))
    if case.sym:
        for x in rows[:k]:            # nothing before it is asymmetric
            for key in ("values", "series"):
                v = x["args"].get(key)
                if v is not None and (x["args"].get("field") in (FIELD_S,) or (key == "series" and x["args"]["what"] == 2)):
                    v = v.reshape(v.shape[:-1] + (case.dim, case.dim)) if key == "series" else v
                    assert np.array_equal(v, np.swapaxes(v, -1, -2)), x["i"]
    # the clocks: a source set while the injectors run; sg_set_params with another dt while every hook runs
    assert any(r["op"] == "set_source" and len(r["args"]["nodes"]) and r["injectors"] for r in rows)
    dts = [r["args"]["dt"] for r in rows if r["op"] == "set_params"]
    assert any(r["op"] == "set_params" and all(r[h] for h in hooks) and r["receivers"] and r["args"]["dt"] != dts[0] for r in rows)
    # the other ways of stepping among the replays, every hook running
    k = next(k for k, r in enumerate(steps) if r["op"] == "host_steps")
    assert steps[k]["args"]["n"] == 2 and steps[k - 1]["replayed"] and steps[k + 1]["replayed"]
    assert all(steps[k][h] for h in hooks) and steps[k]["receivers"]
    assert any(r["timing"] and r["op"] == "step" and all(r[h] for h in hooks) and r["receivers"] for r in rows)
    # the order inside a step: receivers, monitor and spectra all sample the step at whose end the large entry lands
    r = next(r for r in steps if r["args"]["tag"] == "order")
    assert r["rec_sample_last"] and r["mon_sample_last"] and r["spc_sample_last"] and r["inj_entry_last"] is not None
    series = next(x["args"]["series"] for x in rows if x["op"] == "set_injectors")
    sizes = np.sort(np.abs(series).reshape(len(series), -1).max(axis=1))
    assert np.abs(r["inj_entry_last"]).max() == sizes[-1] > 0.5 * ls.LARGE_ENTRY * sizes[-2]
    # the readers between two replays, nothing else between them
    k = next(k for k, r in enumerate(rows) if r["op"] in READERS)
    block = rows[prv(rows[k])["i"] + 1:nxt(rows[k])["i"]]
    assert {x["op"] for x in block} == set(READERS) and between_replays(rows[k])
    assert any(x["op"] == "get_field_dev" and 0 < x["args"]["ncells"] < nc for x in block)
    frames = [x["args"] for x in block if x["op"] == "get_frame_dev"]
    if case.dim == 3:
        at = [a["slice"][ax] * case.n[ax] for a in frames for ax in a["slice"]]
        assert any(abs(t - round(t)) < 1e-9 for t in at) and any(abs(t - round(t)) > 0.1 for t in at)
    else:
        assert frames and all(a["slice"] is None for a in frames)
    # the points: the receivers of the first script; three injector points, two in one cell, one on a grid line
    assert all(np.array_equal(x["args"]["points"], ls.receiver_points(case)) for x in rows if x["op"] == "set_receivers")
    ipts = ls.injector_points(case)
    cell, _ = injector_weights(ls.case_cfg(case), ipts, ls.nnodes(case.dim, case.degree, case.cell))
    assert len(ipts) == 3 and cell[0] == cell[1] >= 0 and cell[2] >= 0 and abs(ipts[2, 0] * case.n[0] - 2.0) < 1e-12
    assert all(len(x["args"]["points"]) in (0, 3) for x in rows if x["op"] in ("set_injectors", "inject"))
    # ... in cells that absorb, as some of the few velocity cells handed over between the eager steps do: what is written
    # there makes the pre-pass of the step before stale
    sigma = next(x["args"]["sigma"] for x in rows if x["op"] == "set_absorption")
    assert all(np.abs(sigma[c]).min() > 0 for c in cell)
    few = next(x["args"] for x in dev_u if not _whole(case, x["args"]))
    assert np.abs(sigma[few["cell0"]:few["cell0"] + len(few["values"])]).max() > 0
    # what a case leaves out
    omitted = ls.HOOKS_OMITTED.get(case.name, {})
    assert len(omitted) <= 2 and set(omitted) <= set(ls.HOOK_TAGS)
    assert {a["tag"] for _, a in script} == set(ls.HOOK_TAGS) - set(omitted)


def test_every_hooks_operation_runs_in_at_least_ten_cases():
    assert set(ls.HOOKS_OMITTED) <= {c.name for c in CASES}
    for tag in ls.HOOK_TAGS:
        assert sum(tag not in ls.HOOKS_OMITTED.get(c.name, {}) for c in CASES) >= 10, tag
    # symmetric-stress storage is left in each of the three ways by at least three cases that hold it
    how = {}
    for c in CASES:
        if c.sym and ls.sym_storage(c):
            how[c.name] = next(op for op, a in ls.make_hooks_script(c) if a["tag"] == "sym.leave" and op in ls.SYM_LEAVERS)
    for op in ls.SYM_LEAVERS:
        assert sum(v == op for v in how.values()) >= 3, (op, how)
    # the first script is what it was: the second draws from a generator of its own
    assert [op for op, _ in ls.make_script(CASES[0])][:3] == ["set_params", "kernels", "set_field"]


def test_the_mirror_of_the_hooks_means_what_the_header_says():
    """The new mirror operations against an OracleLF4 stepped by hand on the smallest case: injector entry k goes in at the
    END of step k + 1 counted from the arming call, behind that step's samples, and nothing after the last; the spectra and the
    monitor count from their own arming calls and restart when armed again; sg_set_params and a source reset no clock; two
    points of one cell add up; a stress series that is not symmetric ends symmetric storage at the call."""
    case = ls.case_by_name("lane-2d-P2")
    mir = ls.Mirror(case)
    rng = np.random.default_rng(2)
    nc, nd, d = mir.ncells, mir.nd, 2
    u0, s0 = rng.uniform(-1, 1, (nc, nd, d)), rng.uniform(-1, 1, (nc, nd, d, d))
    s0 = s0 + np.swapaxes(s0, -1, -2)
    ipts = ls.injector_points(case)
    from seigen_amd.backend import injector_weights
    cell, psi = injector_weights(ls.case_cfg(case), ipts, nd)
    assert cell[0] == cell[1] != cell[2]
    series = rng.uniform(-1, 1, (2, 3, d))                          # two velocity entries
    wu = rng.uniform(-1, 1, (2, 1)) + 1j * rng.uniform(-1, 1, (2, 1))
    w3 = np.array([0.5, 1.0, -0.25])
    mir.set_params(1.0, 1e-3, 0.5, 0.25)
    mir.set_field(FIELD_U, u0)
    mir.set_field(FIELD_S, s0)
    mir.step(1)
    mir.set_monitor(2, 4, w3)                                        # armed after step 1: samples after steps 3, 5
    mir.step(1)
    mir.set_injectors(ipts, series, 1)                               # armed after step 2: entries at the end of steps 3, 4
    mir.set_spectra(wu, None, 2)                                     # armed after step 2: samples after steps 4, 6 - two rows
    mir.set_params(1.0, 2e-3, 0.5, 0.25)                             # no clock restarts
    mir.set_source(np.array([3]), np.zeros((1, 1, d, d)))
    mir.step(5)                                                      # steps 3 .. 7

    orc = OracleLF4(ls.case_mesh(case), case.degree)
    orc.u0, orc.s0, orc.l, orc.mu, orc.density, orc.density_physical = u0, s0, 0.5, 0.25, 1.0, False
    add = lambda amp: sum(psi[r][None, :, None] * amp[r][None, None, :] * (np.arange(nc) == cell[r])[:, None, None] for r in range(3))  # noqa: E731
    state, acc = {}, 0.0
    for step in range(1, 8):
        orc.dt = 1e-3 if step <= 2 else 2e-3
        orc.step(None)
        state[step] = (orc.u1.copy(), orc.s1.copy())
        if step in (4, 6):
            acc = acc + wu[step // 2 - 2, 0] * orc.u1                # ... before the entry of step 4 goes in
        if step in (3, 4):
            orc.u0 = orc.u1 = orc.u1 + add(series[step - 3])
    assert np.allclose(mir.get_field(FIELD_U), orc.u1, rtol=0, atol=1e-15) and np.allclose(mir.get_field(FIELD_S), orc.s1, rtol=0, atol=1e-15)
    assert mir.spectra_samples() == 2 and np.allclose(mir.get_spectrum(0, 0), acc, rtol=0, atol=1e-15)
    got = mir.get_monitor()
    assert got.shape == (3, 5)                                       # after steps 3, 5, 7
    for j, step in enumerate((3, 5, 7)):
        u, s = state[step]                                           # the sample of step 3 does not hold entry 0
        from tests.test_monitor_gpu import host_sample
        want = host_sample(d, case.degree, case.n, case.cell, u, s, w3)
        assert np.allclose(got[j], want, rtol=1e-12, atol=0), (j, got[j], want)
    # armed again: the counts restart, the accumulators are zeroed
    mir.set_spectra(wu, None, 1)
    mir.set_monitor(1, 2, None)
    mir.set_injectors(ipts, series[:1], 1)
    assert mir.spectra_samples() == 0 and not mir.get_spectrum(0, 0).any() and len(mir.get_monitor()) == 0
    before = mir.get_field(FIELD_U)
    orc.dt = 2e-3
    orc.step(None)
    mir.step(1)
    assert np.array_equal(mir.get_spectrum(0, 0), wu[0, 0] * orc.u1) and mir.spectra_samples() == 1
    assert np.allclose(mir.get_field(FIELD_U), orc.u1 + add(series[0]), rtol=0, atol=1e-15) and not np.array_equal(before, orc.u1)
    assert np.array_equal(mir.get_monitor()[0, 3:], [0.0, 0.0])
    # a one-shot injection adds at once; a stress table that is symmetric keeps the storage, one that is not ends it
    sym = rng.uniform(-1, 1, (3, 3, d, d))
    sym = sym + np.swapaxes(sym, -1, -2)
    mir.set_injectors(ipts, sym.reshape(3, 3, d * d), 2)
    assert mir.is_sym()
    s_was = mir.get_field(FIELD_S)
    mir.inject(ipts, sym[0].reshape(3, d * d), 2)
    assert mir.is_sym() and np.abs(mir.get_field(FIELD_S) - s_was)[cell[0]].max() > 0
    mir.set_injectors(ipts, rng.uniform(-1, 1, (3, 3, d * d)), 2)
    assert not mir.is_sym()


def measure_floor(case):
    _, a = ls.mirror_run(case, "numpy")
    _, b = ls.mirror_run(case, "cport")
    return ls.floor_of(a, b)


def measure_hooks_floor(case):
    _, a = ls.hooks_mirror_run(case, "numpy")
    _, b = ls.hooks_mirror_run(case, "cport")
    return ls.floor_of(a, b)


def committed_hooks_floor():
    with open(HOOKS_FLOOR_FILE) as f:
        return json.load(f)


@pytest.mark.parametrize("case", FP64, ids=[c.name for c in FP64])
def test_the_committed_hooks_floor_is_what_two_references_differ_by(case):
    want = committed_hooks_floor()[case.name]
    got = measure_hooks_floor(case)
    assert len(got) == len(want) and min(got) > 0
    for k, (g, w) in enumerate(zip(got, want)):
        assert 0.5 * g <= w <= 2.0 * g, (case.name, k, g, w)
    assert max(want) < 1e-12


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
