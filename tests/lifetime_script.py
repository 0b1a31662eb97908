"""The scripted lifetime of one handle, and its CPU mirror (tests/test_lifetime_oracle.py, tests/test_lifetime_gpu.py).

Every oracle row of the suite makes a handle, configures it once and steps it three times.  What decides, ACROSS calls on a
living handle, what a launch reads - the graph cache and its epoch, the split of a stepping call into replays of the graphs of
eight steps and of one, the reuse of the sponge pre-pass, the step counters of the source and the receivers, leaving
symmetric-stress storage in mid-run, the documented semantics of the setters - is reached by a SCRIPT here: a list of
operations as plain data, (name, arguments), generated from a seed (make_script).  run_script applies it to anything with
HipBlock's method names and collects what can be observed after every stepping call (a checkpoint).  Mirror has those method
names and keeps an OracleLF4 told the same thing at every call, with the semantics of include/seigen_hip.h - not of
api.cpp: sg_set_params drops the density override, every source counts its steps from its own call, re-arming the receivers
counts steps from the arming call, a non-symmetric stress or source ends symmetric-stress storage.  Its steps run through
the numpy oracle (oracle/lf4.py) or through the plain-C port (oracle/cport.py so_step_ex): two statements of the same forms
with different summation orders, whose difference per checkpoint is the round-off floor of tests/golden/lifetime_floor.json.
The C port has no un-fused operator with a sponge, so the apply_F / apply_G operations are mirrored with numpy in both (they
write the two work fields only, which every step overwrites: the state and the floor do not depend on them).

A second script (make_hooks_script; tests/test_lifetime_hooks_gpu.py) reaches what the first stops short of: the other three
end-of-step hooks - monitor, spectra, injectors - armed, re-armed and disarmed beside the receivers, the writers of the fields
outside the stages (sg_inject, an injector series, sg_set_field_dev, sg_leave_sym) and the readers queued on the stream
(sg_measure, sg_get_field_dev, sg_get_spectrum_dev, sg_get_frame_dev).  The mirror takes their meaning from the header as
well: an injection adds amp * psi to the owning cells, summed per cell in the order listed; entry k of a series goes in at the
END of step k + 1 counted from the arming call, behind that step's receiver, monitor and spectra samples; a monitor sample
is { U2, S2, T2, EK, ES } as tests/test_monitor_gpu.py host_sample states it; the spectra add w[j][f] * field after step
(j + 1) * every; every clock counts from its own arming call and no other call resets it; a frame is tests/frame_cases.py
host_frame of the field.  Injections are applied in numpy between the steps of either engine.  Its round-off floor is
tests/golden/lifetime_hooks_floor.json.

Nothing here needs a GPU or torch (a device tensor is made only where the target is a HipBlock).  Point location, the basis
at a receiver and the weights of an injector are the library's device-free entry points (sg_locate_points, sg_tabulate_cell,
sg_injector_weights - checked on its own in tests/test_injectors_host.py), the first two through tests/test_receivers_gpu.py
_locate_on as in its host_samples."""
import collections
import types

import numpy as np

from oracle.lf4 import OracleLF4
from tests.util import oracle_mesh

FIELD_U, FIELD_UH, FIELD_S, FIELD_SH = 0, 1, 2, 3        # enum sg_field (include/seigen_hip.h)
_Q = "quadrilateral"

# name, dim, degree, cubes, cell, dtype, SEIGEN_HIP_PATH, symmetric initial stress, further switches, kernel family.
# The thirteen specs of tests/test_receivers_gpu.py FAMILIES, one tile case in float, one lane case whose affine sponge cells
# take dim + 1 numbers (SEIGEN_HIP_SPONGE_AFFINE=1).
Case = collections.namedtuple("Case", "name dim degree n cell dtype path sym env family")
CASES = [
    Case("generic-1d-P2", 1, 2, (7,), "left", "f64", None, True, {}, "generic"),
    Case("generic-2d-P2", 2, 2, (4, 3), "left", "f64", "generic", True, {}, "generic"),
    Case("lane-2d-P2", 2, 2, (5, 3), "left", "f64", "lane", True, {}, "lane"),
    Case("lane-hex-DQ2", 3, 2, (3, 2, 2), _Q, "f64", "lane", True, {}, "hex_lane"),
    Case("tile-tri-P3", 2, 3, (5, 3), "left", "f64", None, True, {}, "tile"),
    Case("tile-quad-P2", 2, 2, (5, 3), _Q, "f64", None, True, {}, "tile"),
    Case("mfma-P3-sym", 3, 3, (4, 3, 2), "left", "f64", None, True, {}, "mfma"),
    Case("mfma-P3-full", 3, 3, (4, 3, 2), "left", "f64", None, False, {}, "mfma"),
    Case("mfma-P4-sym", 3, 4, (4, 3, 2), "left", "f64", None, True, {}, "mfma"),
    Case("mfma-P4-full", 3, 4, (4, 3, 2), "left", "f64", None, False, {}, "mfma"),
    Case("mfma-P4-f32", 3, 4, (4, 3, 2), "left", "f32", None, True, {}, "mfma"),
    Case("hexm-DQ3", 3, 3, (3, 2, 2), _Q, "f64", None, True, {}, "hexm"),
    Case("hexm-DQ4", 3, 4, (3, 2, 2), _Q, "f64", None, True, {}, "hexm"),
    Case("tile-tri-P3-f32", 2, 3, (5, 3), "left", "f32", None, True, {}, "tile"),
    Case("lane-hex-DQ2-affine", 3, 2, (3, 2, 2), _Q, "f64", "lane", True, {"SEIGEN_HIP_SPONGE_AFFINE": "1"}, "hex_lane"),
]
# every switch that picks a kernel instantiation, the sponge's form, the source path or the way of stepping: unset before a
# case sets its own
SWITCHES = ("SEIGEN_HIP_PATH", "SEIGEN_HIP_SPONGE_AFFINE", "SEIGEN_HIP_SYM", "SEIGEN_HIP_GQ", "SEIGEN_HIP_SOURCE_LAUNCH",
            "SEIGEN_HIP_TILE_GRID", "SEIGEN_HIP_GRAPH", "SEIGEN_HIP_OVERLAP", "SEIGEN_HIP_GRID_BLOCKS")

# The transitions of the script, by tag.  OMITTED: case name -> {tag: reason} for what a case cannot take; a case may leave
# out at most two, every tag must run in at least ten cases (tests/test_lifetime_oracle.py).  Nothing but the planning of the
# sponge's cell kinds and the number type depends on the family (hostlogic.hpp, api.cpp), and neither makes an operation of
# this script impossible: the tile family takes affine cells through their matrices, float exists on every family a float
# case names.  The table is empty.
TAGS = ("fresh", "density.cell", "density.scalar", "params.cell", "params.scalar", "sponge.set", "sponge.upload", "sponge.range",
        "sponge.apply", "sponge.second", "sponge.off", "source.table", "source.separable", "source.static", "source.twice",
        "source.empty", "sym.stress", "sym.source", "step.timing", "step.host", "recv.arm", "recv.rearm", "recv.disarm")
OMITTED = {}

SETTERS = ("set_params", "set_density", "set_absorption", "set_source", "set_source_separable", "set_receivers", "set_field",
           "set_field_range")
STEPPING = ("step", "host_steps")
# a stretch between two full uploads of both fields: the float bound of tests/test_lifetime_gpu.py counts its steps
MAX_STRETCH = 30


def case_by_name(name):
    return next(c for c in CASES if c.name == name)


def ncls_of(case):
    return 1 if case.cell == _Q else {1: 1, 2: 2, 3: 6}[case.dim]


def nnodes(dim, degree, cell):
    if cell == _Q:
        return (degree + 1) ** dim
    return {1: degree + 1, 2: (degree + 1) * (degree + 2) // 2, 3: (degree + 1) * (degree + 2) * (degree + 3) // 6}[dim]


def case_mesh(case):
    return oracle_mesh(case.dim, case.n, (1.0,) * case.dim, case.cell)


def sym_storage(case):
    """the generic kernels have no symmetric-stress storage: such a handle never reports it"""
    return case.family != "generic"


def kernel_names(case, sym):
    """the six instantiations a case must run (hostlogic.hpp lf4_stage), in the words of sg_stage_kernel_name; sym: what
    is_sym() says at that moment"""
    T = {"f64": "double", "f32": "float"}[case.dtype]
    d, P, s = case.dim, case.degree, int(bool(sym))
    lane_like = ((0, 0), (1, 0), (0, 1), (1, 0), (0, 1), (1, 1))        # UTEMP on the F MODE 1 object with c_self = 0
    own_utemp = ((0, 0), (1, 0), (0, 1), (1, 0), (0, 2), (1, 1))
    if case.family == "generic":
        fmt = "sg::stage_kernel<%d, %d, %%d, %d>" % (d, P, d - 1 if case.cell == _Q else 0)
        return [fmt % kind for kind in (0, 1, 0, 1, 0, 1)]
    if case.family == "lane":
        return ["sg::lane_stage<%d, %d, %d, %d, %d>" % (d, P, k, m, s) for k, m in lane_like]
    if case.family == "hex_lane":
        return ["sg::hex_stage<%d, %d, %d, %d>" % (P, k, m, s) for k, m in lane_like]
    if case.family == "hexm":
        return ["sg::hexm_stage<%d, %d, %d, %d>" % (P, k, m, s) for k, m in own_utemp]
    if case.family == "tile":
        return ["sg::tile2d_stage<%d, %d, %d, %d, 0, %d, %s>" % (P, k, m, s, int(case.cell == _Q), T) for k, m in own_utemp]
    fact = int(T == "double" and P >= 4)                                # the factorised volume term: on from degree 4, double
    return ["sg::mfma_stage_F<%s, %d, %d, %d, 0>" % (T, P, m, s) if k == 0 else "sg::mfma_stage_G<%s, %d, %d, %d, %d>" % (T, P, m, s, fact)
            for k, m in own_utemp]


def receiver_points(case):
    """points of every kind inside the mesh (cells, cube faces, edges, vertices, inner simplex faces, the boundary) and the
    ones outside it, which nobody owns: tests/test_receivers_gpu.py receiver_points"""
    from tests.test_receivers_host import point_kinds
    pts = point_kinds(case.n, (1.0,) * case.dim, seed=3)
    inside = np.all((pts >= 0.0) & (pts <= 1.0), axis=1)
    return np.concatenate([pts[inside], pts[~inside][:2]])


def receiver_basis(case, pts):
    """(cell [npts] or -1, phi [npts, nd]) of the receivers: the host evaluation of tests/test_receivers_gpu.py host_samples"""
    from seigen_amd import _lib
    from tests.test_receivers_gpu import _locate_on
    tensor = case.cell == _Q and case.dim > 1
    shape = types.SimpleNamespace(dim=case.dim, degree=case.degree, _n=case.n, nfaces=2 * case.dim if tensor else case.dim + 1)
    cell, xi = _locate_on(shape, pts)
    phi = np.empty((len(pts), nnodes(case.dim, case.degree, case.cell)))
    _lib.check(_lib.load().sg_tabulate_cell(1 if tensor else 0, case.dim, case.degree, len(pts),
                                            np.ascontiguousarray(xi).ctypes.data, phi.ctypes.data))
    return cell, phi


def case_cfg(case):
    """the sg_config of a case's block, for the library's device-free entry points (tests/frame_cases.py block_cfg)"""
    from tests.frame_cases import block_cfg
    return block_cfg(case.dim, case.degree, case.n, case.cell)


def injector_points(case):
    """three points: two inside one cell of the second cube along x, one on the grid line x = 2 h (the lower cell's)"""
    d, n = case.dim, np.array(case.n, dtype=np.float64)
    p0 = (np.array([1.0, 0.0, 0.0])[:d] + np.array([0.35, 0.2, 0.1])[:d]) / n
    p2 = (np.array([2.0, 0.0, 0.0])[:d] + np.array([0.0, 0.45, 0.15])[:d]) / n
    return np.stack([p0, p0 + 0.02 / n, p2])


# ---- the script -----------------------------------------------------------------------------------------------------------

def _stress(shape, rng, sym):
    s = rng.uniform(-1, 1, shape)
    return 0.5 * (s + np.swapaxes(s, -1, -2)) if sym else s


def _sponge(m, ncls, q, rng):
    """DG_q nodal sigma with cells of all four kinds - none, one value, general nodal, affine in x with a gradient of its own -
    in turn along the cubes of every class: tests/test_mfma_family_gpu.py _sponge in any dimension"""
    Xq = m.node_coords(q)
    cell = np.arange(m.ncells)
    kind = (cell // ncls + cell % ncls) % 4
    sigma = np.zeros(Xq.shape[:2])
    c, g, a = kind == 1, kind == 2, kind == 3
    sigma[c] = rng.uniform(2.0, 30.0, size=(c.sum(), 1))
    sigma[g] = rng.uniform(0.0, 30.0, size=(g.sum(), Xq.shape[1]))
    grad = rng.uniform(-20.0, 20.0, size=(a.sum(), 1, Xq.shape[2]))
    sigma[a] = rng.uniform(5.0, 30.0, size=(a.sum(), 1)) + (grad * (Xq[a] - Xq[a][:, :1])).sum(axis=-1)
    return sigma


class _Builder(object):
    def __init__(self, case, rng, omit, tags=None):
        self.case, self.rng, self.omit, self.tags = case, rng, omit, TAGS if tags is None else tags
        self.ops = []
        self.stretch = 0
        self.nc = int(np.prod(case.n)) * ncls_of(case)
        self.nd = nnodes(case.dim, case.degree, case.cell)
        d = case.dim
        self.ushape, self.sshape = (self.nc, self.nd, d), (self.nc, self.nd, d, d)
        self.symmetric = case.sym        # the data handed over so far is symmetric

    def add(self, op, tag, **args):
        assert tag in self.tags, tag
        args["tag"] = tag
        self.ops.append((op, args))

    def wants(self, tag):
        assert tag in self.tags, tag
        return tag not in self.omit

    def step(self, n, tag):
        self.stretch += n
        assert self.stretch <= MAX_STRETCH, (tag, self.stretch)
        self.add("step", tag, n=n)

    def host_steps(self, n, tag):
        self.stretch += n
        assert self.stretch <= MAX_STRETCH, (tag, self.stretch)
        self.add("host_steps", tag, n=n)

    def upload_state(self, tag):
        """both fields anew: the stretch a float bound counts starts here"""
        self.add("set_field", tag, field=FIELD_U, values=self.rng.uniform(-1, 1, self.ushape))
        self.add("set_field", tag, field=FIELD_S, values=_stress(self.sshape, self.rng, self.symmetric))
        self.stretch = 0

    def nodes(self, count, twice=False):
        nodes = self.rng.choice(self.nc * self.nd, size=count, replace=False)
        nodes[-1] = self.nc * self.nd - 1 - int(self.rng.integers(0, self.nd))      # a node of the last cell (the last, ragged group)
        nodes = np.unique(nodes)
        self.rng.shuffle(nodes)
        return np.concatenate([nodes, nodes[:1]]) if twice else nodes


def make_script(case, seed=0):
    """the lifetime of one handle of `case` as a list of (operation, arguments); every stepping operation is a checkpoint"""
    import zlib
    rng = np.random.default_rng([seed, zlib.crc32(case.name.encode())])
    b = _Builder(case, rng, OMITTED.get(case.name, {}))
    m = case_mesh(case)
    assert m.ncells == b.nc
    d, P, nc, nd, ncls = case.dim, case.degree, b.nc, b.nd, ncls_of(case)
    dt = 0.04 * min(1.0 / k for k in case.n) / P ** 2
    lam_c, mu_c = rng.uniform(0.4, 0.8, nc), rng.uniform(0.2, 0.4, nc)
    odd = CASES.index(case) % 2 == 1

    # 1. a fresh handle: scalar density != 1, scalar lambda and mu; one eager step, the first capture and two replays of
    # graph1, graph8 + graph1, graph8 alone
    b.add("set_params", "fresh", density=1.1, dt=dt, lam=0.5, mu=0.25)
    b.add("kernels", "fresh")
    b.upload_state("fresh")
    b.add("kernels", "fresh")
    for n in (1, 2, 9, 8):
        b.step(n, "fresh")
    b.upload_state("fresh")

    # 2. density: per cell and scalar, physical; then sg_set_params, which ends the override, with another dt and per-cell
    # material
    if b.wants("density.cell"):
        b.add("set_density", "density.cell", rho=rng.uniform(0.8, 1.5, nc), physical=True)
        b.step(3, "density.cell")
    if b.wants("density.scalar"):
        b.add("set_density", "density.scalar", rho=1.3, physical=True)
        b.step(2, "density.scalar")
    if b.wants("params.cell"):
        b.add("set_params", "params.cell", density=0.9, dt=0.75 * dt, lam=lam_c, mu=mu_c)
        b.step(3, "params.cell")

    # 3. the sponge: cells of all four kinds; a velocity upload, an upload of a few cells and the un-fused operators between
    # two stepping calls (the pre-pass of the velocity the step before left must not be reused)
    sigma4 = _sponge(m, ncls, 4, rng)
    b.add("set_absorption", "sponge.set", sigma=sigma4, degree=4)
    b.step(3, "sponge.set")
    if b.wants("sponge.upload"):
        b.add("set_field", "sponge.upload", field=FIELD_U, values=rng.uniform(-1, 1, b.ushape))
        b.step(2, "sponge.upload")
    if b.wants("sponge.range"):
        few = min(3, nc)
        # (between two eager steps - what a run that writes output after every step does: the first leaves a pre-pass of
        # its own u1 behind, valid until somebody writes the field)
        b.step(1, "sponge.range")
        b.add("set_field_range", "sponge.range", field=FIELD_U, cell0=(nc - few) // 2, values=rng.uniform(-1, 1, (few,) + b.ushape[1:]))
        b.step(1, "sponge.range")
        b.step(2, "sponge.range")
    if b.wants("sponge.apply"):
        b.add("apply_F", "sponge.apply")
        b.add("apply_G", "sponge.apply")
        b.step(2, "sponge.apply")
    b.upload_state("sponge.apply")

    # 4. sources, each counting its steps from its own call: a table that runs out inside a stepping call, then graphs
    # without a source; a separable one; a static one; a node listed twice; none
    if b.wants("source.table"):
        nodes = b.nodes(9)
        b.add("set_source", "source.table", nodes=nodes, values=_stress((5, len(nodes), d, d), rng, b.symmetric), static=False)
        for n in (3, 4, 2):
            b.step(n, "source.table")
    if b.wants("source.separable"):
        nodes = b.nodes(7)
        b.add("set_source_separable", "source.separable", nodes=nodes, pattern=_stress((len(nodes), d, d), rng, b.symmetric),
              weights=rng.uniform(-2, 2, 12))
        b.step(3, "source.separable")
    if b.wants("source.static"):
        nodes = b.nodes(6)
        b.add("set_source", "source.static", nodes=nodes, values=_stress((1, len(nodes), d, d), rng, b.symmetric), static=True)
        b.step(2, "source.static")
    if b.wants("source.twice"):
        nodes = b.nodes(8, twice=True)
        b.add("set_source", "source.twice", nodes=nodes, values=_stress((6, len(nodes), d, d), rng, b.symmetric), static=False)
        b.step(3, "source.twice")
    if b.wants("source.empty"):
        b.add("set_source", "source.empty", nodes=np.zeros(0, dtype=np.int64), values=None, static=False)
        b.step(2, "source.empty")
    b.upload_state("source.empty")

    # 5. leaving symmetric-stress storage in mid-run: by a few non-symmetric cells of the stress, and by a non-symmetric source
    # (which stays active to the end of the script); whichever comes first - in turn over the cases - is the one that leaves
    def sym_stress():
        few = min(2, nc)
        b.add("set_field_range", "sym.stress", field=FIELD_S, cell0=nc // 2, values=_stress((few,) + b.sshape[1:], rng, False))
        b.symmetric = False

    def sym_source():
        nodes = b.nodes(9)
        b.add("set_source_separable", "sym.source", nodes=nodes, pattern=_stress((len(nodes), d, d), rng, False),
              weights=rng.uniform(-2, 2, 96))
        b.symmetric = False

    for k, (tag, emit) in enumerate((("sym.source", sym_source), ("sym.stress", sym_stress))[::-1 if odd else 1]):
        if b.wants(tag):
            emit()
            b.add("kernels", tag)
            b.step(3 - k, tag)

    # 6. the ways of stepping, mixed on the one handle while the source is active: eager with an event pair per launch,
    # replay, two host-driven steps (six sg_run_stage and sg_end_step each), replay
    if b.wants("step.timing"):
        b.add("enable_timing", "step.timing", on=True)
        b.step(3, "step.timing")
        b.add("enable_timing", "step.timing", on=False)
        b.step(2, "step.timing")
    if b.wants("step.host"):
        b.host_steps(2, "step.host")
        b.step(2, "step.host")
    b.upload_state("step.host")

    # 7. receivers, armed in mid-run with source and sponge on: every stepping size class, the trace exactly full; read out;
    # armed again with another `every` and `what`, a host-driven step among the replays; disarmed
    pts = receiver_points(case)
    if b.wants("recv.arm"):
        b.add("set_receivers", "recv.arm", points=pts, what=3, every=1, capacity=21)
        b.step(1, "recv.arm")
        b.step(3, "recv.arm")
        b.add("get_receivers", "recv.arm")
        b.step(8, "recv.arm")
        b.step(9, "recv.arm")
        b.add("get_receivers", "recv.arm")
        b.upload_state("recv.arm")
    if b.wants("recv.rearm"):
        b.add("set_receivers", "recv.rearm", points=pts[::2], what=2, every=3, capacity=3)
        b.step(4, "recv.rearm")
        b.host_steps(2, "recv.rearm")
        b.step(2, "recv.rearm")
        b.add("get_receivers", "recv.rearm")
    if b.wants("recv.disarm"):
        b.add("set_receivers", "recv.disarm", points=np.zeros((0, d)), what=1, every=1, capacity=0)
        b.step(2, "recv.disarm")
        b.add("get_receivers", "recv.disarm")

    # a second sigma of another degree, no sponge, and back to scalar material (per_cell 1 -> 0)
    if b.wants("sponge.second"):
        b.add("set_absorption", "sponge.second", sigma=_sponge(m, ncls, 2, rng), degree=2)
        b.step(3, "sponge.second")
    if b.wants("sponge.off"):
        b.add("set_absorption", "sponge.off", sigma=None, degree=0)
        b.step(2, "sponge.off")
    if b.wants("params.scalar"):
        b.add("set_params", "params.scalar", density=0.95, dt=dt, lam=0.6, mu=0.3)
        b.step(3, "params.scalar")
    return b.ops


# ---- the second script: the other end-of-step hooks, the injections and the device transfers -------------------------------

# The transitions of make_hooks_script by tag, with the rule of TAGS / OMITTED: nothing in it depends on the family.
HOOK_TAGS = ("fresh", "arm.monitor", "arm.spectra", "arm.injectors", "order", "size.classes", "readers", "runout.spectra",
             "rearm.spectra", "dev.upload", "runout.injectors", "rearm.injectors", "monitor.full", "rearm.monitor", "dev.range",
             "inject.sponge", "sym.leave", "clock.source", "clock.params", "step.host", "sym.again", "inject.replay",
             "step.timing", "disarm.monitor", "disarm.spectra", "disarm.injectors")
HOOKS_OMITTED = {}
HOOK_SETTERS = ("set_monitor", "set_spectra", "set_injectors", "inject", "set_field_dev", "leave_sym")
# how a case leaves symmetric-stress storage in the second script, in turn over the cases
SYM_LEAVERS = ("set_field_dev", "set_injectors", "leave_sym")
LARGE_ENTRY = 10.0          # the factor of the injector entry that lands on the step all hooks sample ("order")


def frames_of(case):
    """(field, m, slice) of the frames read in mid-run: in 3-D a plane slice on a grid plane and one inside a cube, else the
    raster of the mesh"""
    if case.dim == 3:
        return [(FIELD_U, (2, 2, 1), {2: 1.0 / case.n[2]}), (FIELD_S, (1, 2, 2), {0: 2.5 / case.n[0]})]
    m = (2, 3) if case.dim == 2 else 4
    return [(FIELD_U, m, None), (FIELD_S, m, None)]


def make_hooks_script(case, seed=0):
    """The second lifetime of a handle of `case`: monitor, spectra and injectors armed, re-armed and disarmed beside the
    receivers on a handle that holds graphs, a pre-pass and running counters; fields written by sg_inject, an injector series
    and sg_set_field_dev between stepping calls; readers queued on the stream in mid-run.  78 steps; the absolute step at which
    each call is made stands in the comments (tests/test_lifetime_oracle.py walks them)."""
    import zlib
    from seigen_amd.backend import injector_weights
    rng = np.random.default_rng([seed, zlib.crc32(case.name.encode()), 1])
    b = _Builder(case, rng, HOOKS_OMITTED.get(case.name, {}), HOOK_TAGS)
    m = case_mesh(case)
    assert m.ncells == b.nc
    d, P, nc, nd, ncls = case.dim, case.degree, b.nc, b.nd, ncls_of(case)
    dt = 0.04 * min(1.0 / k for k in case.n) / P ** 2
    lam_c, mu_c = rng.uniform(0.4, 0.8, nc), rng.uniform(0.2, 0.4, nc)
    turn = CASES.index(case) % 3
    pts, ipts = receiver_points(case), injector_points(case)
    icell, psi = injector_weights(case_cfg(case), ipts, nd)
    assert icell[0] == icell[1] >= 0 and icell[2] >= 0
    unit = 0.1 / np.abs(psi).max()                        # an entry moves a nodal value by 0.1 at the most, the large one by 1
    mid = (nc // 2) // ncls * ncls + (1 if ncls > 1 else 0)     # a cell in the middle of a cube's classes
    triple = np.array([0.55, 1.0, -0.5 / (d * 0.5 + 0.5)])      # rho / 2, 1 / (4 mu), -lambda / (4 mu (d lambda + 2 mu))
    rho_c = rng.uniform(0.5, 2.0, nc)
    per_cell = np.stack([rho_c / 2.0, 1.0 / (4.0 * mu_c), -lam_c / (4.0 * mu_c * (d * lam_c + 2.0 * mu_c))], axis=-1)

    def amps(entries, what):
        parts = []
        if what & 1:
            parts.append(rng.uniform(-1, 1, (entries, 3, d)))
        if what & 2:
            parts.append(_stress((entries, 3, d, d), rng, b.symmetric).reshape(entries, 3, d * d))
        return unit * np.concatenate(parts, axis=-1)

    def weights(nsamples):
        return rng.uniform(-1, 1, (nsamples, 2)) + 1j * rng.uniform(-1, 1, (nsamples, 2))

    def read_hooks(tag):
        b.add("get_receivers", tag)
        b.add("get_monitor", tag)
        b.add("spectra_samples", tag)
        for field, freq in ((0, 0), (1, 1)):
            b.add("get_spectrum", tag, field=field, freq=freq)

    # 1. a fresh handle with no hook: every size class (eager, the first capture, graph8 + graph1, graph8)        steps 0 .. 20
    b.add("set_params", "fresh", density=1.1, dt=dt, lam=0.5, mu=0.25)
    b.add("kernels", "fresh")
    b.upload_state("fresh")
    for n in (1, 2, 9, 8):
        b.step(n, "fresh")
    b.upload_state("fresh")
    # (the sponge for the rest of the script; the injectors' cells absorb - general nodal sigma - whatever kind their turn
    # gives them: a velocity added there changes what the pre-pass holds)
    sigma = _sponge(m, ncls, 4, rng)
    own = np.unique(icell)
    sigma[own] = rng.uniform(5.0, 30.0, size=(len(own), sigma.shape[1]))
    b.add("set_absorption", "fresh", sigma=sigma, degree=4)

    # 2. the hooks armed one call after the other on the handle that holds those graphs, a replay after each      20 .. 27
    b.add("set_receivers", "arm.monitor", points=pts, what=3, every=2, capacity=40)
    b.add("set_monitor", "arm.monitor", every=1, capacity=35, w=triple)                    # full after step 55
    b.step(2, "arm.monitor")
    b.add("set_spectra", "arm.spectra", wu=weights(18), ws=weights(18), every=1)             # armed at 22: the last sample at 40
    b.step(2, "arm.spectra")
    series = amps(25, 3)                                                                     # armed at 24: the last entry at 49
    series[3] *= LARGE_ENTRY                                                                 # ... and entry 3 at the end of step 28
    b.add("set_injectors", "arm.injectors", points=ipts, series=series, what=3)
    b.step(3, "arm.injectors")

    # 3. the order inside a step: step 28 is a sample step of the receivers (every 2 from 20), the monitor and the spectra,
    # and the large entry lands at its end; then the size classes with every hook running                           27 .. 45
    b.step(1, "order")
    read_hooks("order")
    b.step(8, "size.classes")
    b.step(9, "size.classes")                      # the spectra's series runs out at step 40, inside this call

    # 4. readers queued on the stream between two replays; the second replay must add nothing to the spectra      45 .. 47
    b.add("measure", "readers", w=per_cell)
    b.add("measure", "readers", w=None)
    few = min(3, nc - mid)
    for field in (FIELD_U, FIELD_S):
        b.add("get_field_dev", "readers", field=field, cell0=mid, ncells=few)
    for field, freq in ((0, 1), (1, 0)):
        b.add("get_spectrum_dev", "readers", field=field, freq=freq)
    for field, mm, sl in frames_of(case):
        b.add("get_frame_dev", "readers", field=field, m=mm, slice=sl)
    b.step(2, "runout.spectra")
    read_hooks("runout.spectra")

    # 5. the spectra armed again with another `every` beside the running monitor and injectors; both fields from device
    # buffers between two replays (the sponge is set: a pre-pass of the old velocity must not be reused); the injectors'
    # series runs out at step 49 inside the replay, the next adds nothing                                            47 .. 52
    b.add("set_spectra", "rearm.spectra", wu=weights(20), ws=weights(20), every=2)         # samples after 49, 51, .. 85
    b.add("set_field_dev", "dev.upload", field=FIELD_U, cell0=0, values=rng.uniform(-1, 1, b.ushape))
    b.add("set_field_dev", "dev.upload", field=FIELD_S, cell0=0, values=_stress(b.sshape, rng, b.symmetric))
    b.stretch = 0
    b.step(3, "dev.upload")
    b.step(2, "runout.injectors")

    # 6. a stress series armed beside the running monitor and spectra; the monitor's trace exactly full at step 55, read,
    # and armed again with another `every` and weights per cell                                                      52 .. 55
    b.add("set_injectors", "rearm.injectors", points=ipts, series=amps(30, 2), what=2)
    b.step(3, "rearm.injectors")
    b.add("get_monitor", "monitor.full")
    b.add("set_monitor", "rearm.monitor", every=3, capacity=12, w=per_cell)              # samples after 58, 61, .. 70

    # 7. under the sponge, between eager single steps: a few velocity cells from a device buffer, then a velocity injection -
    # the pre-pass the step before left is stale both times                                                          55 .. 58
    b.step(1, "dev.range")
    b.add("set_field_dev", "dev.range", field=FIELD_U, cell0=mid, values=rng.uniform(-1, 1, (few,) + b.ushape[1:]))
    b.step(1, "dev.range")
    b.add("inject", "inject.sponge", points=ipts, amp=amps(1, 1)[0], what=1)
    b.step(1, "inject.sponge")

    # 8. leaving symmetric-stress storage with stress spectra armed and graphs captured, in turn over the cases by a few
    # stress cells from a device buffer, by a stress series that is not symmetric, by sg_leave_sym                   58 .. 60
    b.add("get_spectrum", "sym.leave", field=1, freq=0)
    b.add("kernels", "sym.leave")
    b.symmetric = False
    if SYM_LEAVERS[turn] == "set_field_dev":
        b.add("set_field_dev", "sym.leave", field=FIELD_S, cell0=mid, values=_stress((min(2, nc - mid),) + b.sshape[1:], rng, False))
    elif SYM_LEAVERS[turn] == "set_injectors":
        b.add("set_injectors", "sym.leave", points=ipts, series=amps(24, 2), what=2)
    else:
        b.add("leave_sym", "sym.leave")
    b.add("kernels", "sym.leave")
    b.step(2, "sym.leave")
    b.add("get_spectrum", "sym.leave", field=1, freq=0)

    # 9. every clock keeps its own count: a source set while the injectors run, sg_set_params with another dt while all
    # hooks run                                                                                                        60 .. 64
    nodes = b.nodes(7)
    b.add("set_source", "clock.source", nodes=nodes, values=_stress((5, len(nodes), d, d), rng, False), static=False)
    b.step(2, "clock.source")
    b.add("set_params", "clock.params", density=0.9, dt=0.8 * dt, lam=lam_c, mu=mu_c)
    b.step(2, "clock.params")

    # 10. the other ways of stepping among the replays, all hooks armed: two host-driven steps, a replay (sg_leave_sym on a
    # block that has left, and an injection of both fields, in front of it), a timed eager call, a replay            64 .. 72
    b.host_steps(2, "step.host")
    b.add("leave_sym", "sym.again")
    b.add("inject", "inject.replay", points=ipts, amp=amps(1, 3)[0], what=3)
    b.step(2, "inject.replay")
    b.add("enable_timing", "step.timing", on=True)
    b.step(2, "step.timing")
    b.add("enable_timing", "step.timing", on=False)
    b.step(2, "step.timing")
    read_hooks("step.timing")
    b.upload_state("step.timing")

    # 11. each hook disarmed while the others keep running, a replay behind it, and armed again                     72 .. 78
    b.add("set_monitor", "disarm.monitor", every=0, capacity=0, w=None)
    b.step(2, "disarm.monitor")
    b.add("get_monitor", "disarm.monitor")
    b.add("set_monitor", "disarm.monitor", every=2, capacity=4, w=None)
    b.add("set_spectra", "disarm.spectra", wu=None, ws=None, every=1)
    b.step(2, "disarm.spectra")
    b.add("spectra_samples", "disarm.spectra")
    b.add("set_spectra", "disarm.spectra", wu=weights(3), ws=None, every=1)
    b.add("set_injectors", "disarm.injectors", points=np.zeros((0, d)), series=None, what=1)
    b.step(2, "disarm.injectors")
    b.add("get_receivers", "disarm.injectors")
    b.add("get_monitor", "disarm.injectors")
    b.add("get_spectrum", "disarm.injectors", field=0, freq=1)
    return b.ops


# ---- applying it ------------------------------------------------------------------------------------------------------------

def _snapshot(target):
    """what a checkpoint observes; a mirror is told that one has been taken (it logs its samples by checkpoint)"""
    getattr(target, "checkpoint", lambda: None)()
    c = target.counters()
    return dict(u=target.get_field(FIELD_U), s=target.get_field(FIELD_S), uh=target.get_field(FIELD_UH),
                sh=target.get_field(FIELD_SH), steps=c["steps"], launches=list(c["launches"]), sym=target.is_sym(),
                stretch=getattr(target, "stretch", None))


def _copy(x):
    return None if x is None else list(x)


def _host(x):
    """a device tensor as a numpy array (the copy runs on torch's current stream, which HipBlock has put behind the
    handle's launch)"""
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _device(target, values):
    """the values as a double tensor on the block's device where the target is a HipBlock - the only place a device tensor
    is made - and as they are for a mirror"""
    if not hasattr(target, "_torch_device"):
        return values
    import torch
    return torch.as_tensor(np.ascontiguousarray(values, dtype=np.float64), device=target._torch_device())


def run_script(target, script):
    """Apply the script to `target` - a HipBlock, or anything with its method names - and return what can be observed, one
    dict per observing operation: {"i": index in the script, "op", "tag"} and, after a stepping call (a checkpoint), the four
    fields, the counters and is_sym(); after apply_F / apply_G the field written; for get_receivers the samples; for
    kernels the six stage kernel names; for the readers of the second script what they return, as numpy arrays (and, from a
    mirror, what the bound of that observation is made from)."""
    seen = []
    for i, (op, a) in enumerate(script):
        obs = None
        if op == "set_params":
            target.set_params(a["density"], a["dt"], a["lam"], a["mu"])
        elif op == "set_density":
            target.set_density(a["rho"], physical=a["physical"])
        elif op == "set_absorption":
            target.set_absorption(a["sigma"], a["degree"])
        elif op == "set_field":
            target.set_field(a["field"], a["values"])
        elif op == "set_field_range":
            target.set_field_range(a["field"], a["cell0"], a["values"])
        elif op == "set_source":
            target.set_source(a["nodes"], a["values"], static=a["static"])
        elif op == "set_source_separable":
            target.set_source_separable(a["nodes"], a["pattern"], a["weights"])
        elif op == "set_receivers":
            obs = dict(owned=np.asarray(target.set_receivers(a["points"], a["what"], a["every"], a["capacity"])))
        elif op == "enable_timing":
            target.enable_timing(a["on"])
        elif op == "step":
            target.step(a["n"])
            obs = _snapshot(target)
        elif op == "host_steps":
            for _ in range(a["n"]):
                for st in range(6):
                    target.run_stage(st)
                target.end_step()
            obs = _snapshot(target)
        elif op == "apply_F":
            target.apply_F(FIELD_S, FIELD_U, FIELD_UH)
            obs = dict(uh=target.get_field(FIELD_UH))
        elif op == "apply_G":
            target.apply_G(FIELD_U, FIELD_SH)
            obs = dict(sh=target.get_field(FIELD_SH))
        elif op == "get_receivers":
            obs = dict(traces=target.get_receivers(), scales=getattr(target, "rec_scales", None),
                       lebesgue=getattr(target, "rec_lebesgue", None), what=getattr(target, "rec_what", None),
                       log=_copy(getattr(target, "rec_log", None)))
        elif op == "kernels":
            obs = dict(names=[target.stage_kernel_name(st) for st in range(6)])
        elif op == "leave_sym":
            target.leave_sym()
        elif op == "inject":
            target.inject(a["points"], a["amp"], a["what"])
        elif op == "set_injectors":
            obs = dict(owned=np.asarray(target.set_injectors(a["points"], a["series"], a["what"])))
        elif op == "set_field_dev":
            target.set_field_dev(a["field"], _device(target, a["values"]), cell0=a["cell0"])
        elif op == "set_monitor":
            target.set_monitor(a["every"], a["capacity"], a["w"])
        elif op == "get_monitor":
            mon = getattr(target, "mon", None) or {}
            obs = dict(samples=target.get_monitor(), abs=_copy(mon.get("abs")), log=_copy(mon.get("log")))
        elif op == "measure":
            obs = dict(sample=target.measure(a["w"]), abs=getattr(target, "measure_abs", None))
        elif op == "set_spectra":
            target.set_spectra(a["wu"], a["ws"], a["every"])
        elif op in ("get_spectrum", "get_spectrum_dev"):
            get = target.get_spectrum if op == "get_spectrum" else target.get_spectrum_dev
            obs = dict(acc=_host(get(a["field"], a["freq"])))
            if hasattr(target, "spectrum_terms"):
                obs["terms"] = target.spectrum_terms(a["field"], a["freq"])
        elif op == "spectra_samples":
            obs = dict(taken=target.spectra_samples())
        elif op == "get_field_dev":
            obs = dict(dev=_host(target.get_field_dev(a["field"], cell0=a["cell0"], ncells=a["ncells"])),
                       range=target.get_field_range(a["field"], a["cell0"], a["ncells"]), field=a["field"])
        elif op == "get_frame_dev":
            obs = dict(frame=_host(target.get_frame_dev(a["field"], a["m"], a["slice"])), field=a["field"],
                       lebesgue=getattr(target, "frame_lebesgue", None), scale=getattr(target, "frame_scale", None))
        else:
            raise ValueError("unknown operation %r" % (op,))
        if obs is not None:
            obs.update(i=i, op=op, tag=a["tag"])
            seen.append(obs)
    return seen


class Mirror(object):
    """An OracleLF4 behind HipBlock's method names, told what include/seigen_hip.h says each call means.  engine "numpy":
    steps through oracle/lf4.py; "cport": through oracle/cport.py so_step_ex (one step per call: the source's step and the
    density rule are the mirror's)."""

    def __init__(self, case, engine="numpy"):
        self.case, self.engine = case, engine
        self.mesh = case_mesh(case)
        self.orc = OracleLF4(self.mesh, case.degree)
        self.cp = None
        if engine == "cport":
            from oracle.cport import CPort
            self.cp = CPort(self.mesh, case.degree)
        elif engine != "numpy":
            raise ValueError(engine)
        d, nd, nc = case.dim, self.orc.E.nd, self.mesh.ncells
        self.dim, self.nd, self.ncells = d, nd, nc
        self.f = {FIELD_U: np.zeros((nc, nd, d)), FIELD_UH: np.zeros((nc, nd, d)), FIELD_S: np.zeros((nc, nd, d, d)),
                  FIELD_SH: np.zeros((nc, nd, d, d))}
        self.rho, self.physical, self.dt, self.lam, self.mu = 1.0, False, None, None, None
        self.sigma = None                 # (nodal values, degree)
        self.src = None                   # (unique nodes, table [nsteps, nnz, d, d], static)
        self.src_step = 0
        self.rec = None
        self.rec_scales, self.rec_lebesgue, self.rec_what = None, None, 0      # per sample (max |u1|, max |s1|); max_k sum_a |phi_a(xi_k)|
        self.sym = sym_storage(case)
        self.steps = 0
        self.stretch, self._fresh = 0, set()
        self._dirty = True
        # the hooks of make_hooks_script: every sample is logged with (stepping calls completed before its own, steps of
        # the stretch), what a bound of the fields at that sample is made from
        self.ncheck = 0
        self.rec_log = None
        self.mon = self.spc = self.inj = None
        self.measure_abs = None
        self.frame_lebesgue = self.frame_scale = None
        self._mass = None

    # ---- setters: include/seigen_hip.h --------------------------------------------------------------------------------
    def set_params(self, density, dt, lam, mu):
        """sg_set_params: the scalar density of the explicit reference's update - and the end of what sg_set_density set
        ("overrides until the next sg_set_params")"""
        self.rho, self.physical = float(density), False
        self.dt = float(dt)
        self.lam = np.array(lam, dtype=np.float64) if np.ndim(lam) else float(lam)
        self.mu = np.array(mu, dtype=np.float64) if np.ndim(mu) else float(mu)
        self._dirty = True

    def set_density(self, rho, physical=False):
        self.rho = np.array(rho, dtype=np.float64) if np.ndim(rho) else float(rho)
        self.physical = bool(physical)
        self._dirty = True

    def set_absorption(self, sigma_nodes, sigma_degree):
        self.sigma = None if sigma_nodes is None else (np.array(sigma_nodes, dtype=np.float64).reshape(self.ncells, -1), int(sigma_degree))
        if self.sigma is None:
            self.orc.E.absorb = None
        else:
            self.orc.E.set_absorption(*self.sigma)
        self._dirty = True

    def _upload(self, field, values):
        if field in (FIELD_S, FIELD_SH) and self.sym and np.any(values != np.swapaxes(values, -1, -2)):
            self.sym = False              # "left automatically when THIS block is handed a non-symmetric stress or source"

    def set_field(self, field, values):
        values = np.array(values, dtype=np.float64).reshape(self.f[field].shape)
        self._upload(field, values)
        self.f[field] = values
        self._fresh.add(field)

    def set_field_range(self, field, cell0, values):
        values = np.asarray(values, dtype=np.float64)
        self._upload(field, values)
        self.f[field] = self.f[field].copy()
        self.f[field][cell0:cell0 + len(values)] = values

    def _set_source(self, nodes, table, static):
        """steps k = 0 .. nsteps-1 "counted from this call; no source afterwards"; a node listed more than once receives the
        sum of its entries"""
        self.src_step = 0
        self._dirty = True
        nodes = np.asarray(nodes, dtype=np.int64).ravel()
        if nodes.size == 0 or table is None or len(table) == 0:
            self.src = None
            return
        uniq, inv = np.unique(nodes, return_inverse=True)
        summed = np.zeros((table.shape[0], len(uniq)) + table.shape[2:])
        for j, slot in enumerate(inv):                      # in the order listed
            summed[:, slot] += table[:, j]
        if self.sym and np.any(table != np.swapaxes(table, -1, -2)):
            self.sym = False
        self.src = (uniq, summed, bool(static))

    def set_source(self, nodes, values, static=False):
        nodes = np.asarray(nodes, dtype=np.int64).ravel()
        table = None if values is None else np.asarray(values, dtype=np.float64).reshape(-1, nodes.size, self.dim, self.dim)
        self._set_source(nodes, table, static)

    def set_source_separable(self, nodes, pattern, weights):
        """S(node, step k) = weights[k] * pattern[node], the product rounded before it is added"""
        nodes = np.asarray(nodes, dtype=np.int64).ravel()
        pattern = np.asarray(pattern, dtype=np.float64).reshape(nodes.size, self.dim, self.dim)
        weights = np.asarray(weights, dtype=np.float64).ravel()
        self._set_source(nodes, weights[:, None, None, None] * pattern[None], False)

    def set_receivers(self, points, what=1, every=1, capacity=0):
        """re-arming discards the old samples and counts steps from the arming call; no points: disarmed"""
        pts = np.asarray(points, dtype=np.float64).reshape(-1, self.dim)
        if len(pts) == 0:
            self.rec, self.rec_what = None, 0
            return np.zeros(0, dtype=bool)
        cell, phi = receiver_basis(self.case, pts)
        self.rec = dict(cell=cell, phi=phi, what=int(what), every=int(every), capacity=int(capacity), steps=0, samples=[])
        self.rec_scales, self.rec_log, self.rec_what = [], [], int(what)
        self.rec_lebesgue = float(np.abs(phi[cell >= 0]).sum(axis=1).max()) if (cell >= 0).any() else 0.0
        return cell >= 0

    def get_receivers(self):
        if self.rec is None:
            return np.zeros((0, 0, 0))
        r = self.rec
        ncomp = (self.dim if r["what"] & 1 else 0) + (self.dim ** 2 if r["what"] & 2 else 0)
        return np.array(r["samples"]).reshape(len(r["samples"]), len(r["cell"]), ncomp)

    def enable_timing(self, on=True):
        pass

    def is_sym(self):
        return self.sym

    def leave_sym(self):
        self.sym = False

    # ---- writers outside the stages ---------------------------------------------------------------------------------------
    def set_field_dev(self, field, values, cell0=0):
        """sg_set_field_dev: the cells from cell0 - the rule of sg_set_field for a stress that is not symmetric; the whole
        field counts as an upload of it"""
        values = np.asarray(values, dtype=np.float64)
        if cell0 == 0 and len(values) == self.ncells:
            self.set_field(field, values)
        else:
            self.set_field_range(field, cell0, values)

    def _injectors(self, points, what):
        from seigen_amd.backend import injector_weights
        pts = np.asarray(points, dtype=np.float64).reshape(-1, self.dim)
        return injector_weights(case_cfg(self.case), pts, self.nd)

    def _amp_leaves_sym(self, cell, amp, what):
        """"a stress table that is symmetric to the bit (the owned points', every entry) writes the i <= j lines only; one
        that is not makes THIS block leave symmetric storage at the call"; amp [entries, npts, ncomp]"""
        if not (what & 2 and self.sym):
            return
        d = self.dim
        t = amp[:, cell >= 0, d if what & 1 else 0:].reshape(len(amp), -1, d, d)
        if np.any(t != np.swapaxes(t, -1, -2)):
            self.sym = False

    def _add(self, cell, psi, amp, what):
        """field[cell][a][c] += sum_r amp[r][c] psi_r[a] over the cell's points r in the order listed; amp [npts, ncomp]"""
        d = self.dim
        nu = d if what & 1 else 0
        for field, lo, hi in ((FIELD_U, 0, nu), (FIELD_S, nu, amp.shape[1])):
            if hi == lo:
                continue
            v = {}
            for r, c in enumerate(cell):
                if c >= 0:
                    v[int(c)] = v.get(int(c), 0.0) + psi[r][:, None] * amp[r, lo:hi][None, :]
            out = self.f[field].copy()
            for c, add in v.items():
                out[c] = out[c] + add.reshape(out[c].shape)
            self.f[field] = out

    def inject(self, points, amp, what=1):
        cell, psi = self._injectors(points, what)
        amp = np.asarray(amp, dtype=np.float64).reshape(len(cell), -1)
        self._amp_leaves_sym(cell, amp[None], what)
        self._add(cell, psi, amp, what)

    def set_injectors(self, points, series, what=1):
        """entry k at the END of step k + 1 counted from this call; re-arming restarts the count; no points or no entries:
        disarmed"""
        pts = np.asarray(points, dtype=np.float64).reshape(-1, self.dim)
        if len(pts) == 0 or series is None or len(series) == 0:
            self.inj = None
            return np.zeros(len(pts), dtype=bool)
        cell, psi = self._injectors(pts, what)
        series = np.asarray(series, dtype=np.float64).reshape(len(series), len(pts), -1)
        self._amp_leaves_sym(cell, series, what)
        self.inj = dict(cell=cell, psi=psi, series=series, what=int(what), steps=0)
        return cell >= 0

    # ---- monitor ------------------------------------------------------------------------------------------------------------
    def _sample(self, u, s, w):
        """{ U2, S2, T2, EK, ES }: tests/test_monitor_gpu.py host_sample, with the forms v^T Mhat v taken cell by cell"""
        if self._mass is None:
            from oracle import refelem
            kind = getattr(self.mesh, "kind", "simplex")
            xq, wq = refelem.el_quadrature(self.dim, 2 * self.case.degree, kind)
            phi, _ = refelem.el_tabulate(self.dim, self.case.degree, xq, kind)
            self._mass = np.einsum('q,qa,qb->ab', wq, phi, phi)
        M, dj = self._mass, np.abs(self.mesh.detJ)
        t = np.einsum('cnii->cn', s)
        s2 = s.reshape(s.shape[0], s.shape[1], -1)
        Qu = np.einsum('cak,ab,cbk->c', u, M, u)
        Qs = np.einsum('cak,ab,cbk->c', s2, M, s2)
        Qt = np.einsum('ca,ab,cb->c', t, M, t)
        out = [np.sum(dj * Qu), np.sum(dj * Qs), np.sum(dj * Qt), 0.0, 0.0]
        if w is not None:
            w = np.broadcast_to(np.asarray(w, dtype=np.float64), (self.ncells, 3))
            out[3:] = [np.sum(dj * w[:, 0] * Qu), np.sum(dj * (w[:, 1] * Qs + w[:, 2] * Qt))]
        return np.array(out)

    def measure(self, w=None):
        """one sample of u and s as they stand now; measure_abs: the same with |w|, the scale of its bound"""
        self.measure_abs = self._sample(self.f[FIELD_U], self.f[FIELD_S], None if w is None else np.abs(w))
        return self._sample(self.f[FIELD_U], self.f[FIELD_S], w)

    def set_monitor(self, every, capacity, w=None):
        """sample j after step (j + 1) * every counted from this call; every = 0 disarms; re-arming discards the samples"""
        if int(every) == 0:
            self.mon = None
            return
        self.mon = dict(every=int(every), capacity=int(capacity), w=None if w is None else np.array(w, dtype=np.float64), steps=0,
                        samples=[], abs=[], log=[])

    def get_monitor(self):
        return np.array(self.mon["samples"]).reshape(-1, 5) if self.mon is not None else np.zeros((0, 5))

    # ---- spectra ------------------------------------------------------------------------------------------------------------
    def set_spectra(self, wu=None, ws=None, every=1):
        """acc[f] += w[j][f] * field after step (j + 1) * every counted from this call, for the nsamples rows of the table;
        arming zeroes the accumulators and restarts the count; no table: disarmed"""
        if wu is None and ws is None:
            self.spc = None
            return
        w = [None if x is None else np.asarray(x, dtype=np.complex128) for x in (wu, ws)]
        nsamples, nfreq = next(x for x in w if x is not None).shape
        shapes = (self.f[FIELD_U].shape, self.f[FIELD_S].shape)
        self.spc = dict(w=w, every=int(every), nsamples=nsamples, steps=0, log=[],
                        acc=[None if w[k] is None else np.zeros((nfreq,) + shapes[k], dtype=np.complex128) for k in range(2)])

    def _spectrum_field(self, field):
        return {0: 0, 1: 1, FIELD_S: 1}[int(field)]

    def get_spectrum(self, field, freq):
        return self.spc["acc"][self._spectrum_field(field)][freq].copy()

    def get_spectrum_dev(self, field, freq):
        return self.get_spectrum(field, freq)

    def spectra_samples(self):
        return len(self.spc["log"]) if self.spc is not None else 0

    def spectrum_terms(self, field, freq):
        """per sample taken (|w[j][freq]|, stepping calls completed, steps of the stretch, max |field|): the terms of the
        bound of an accumulator"""
        k = self._spectrum_field(field)
        return [(abs(self.spc["w"][k][j][freq]), c, n, (su, ss)[k]) for j, (c, n, su, ss) in enumerate(self.spc["log"])]

    # ---- readers ------------------------------------------------------------------------------------------------------------
    def get_field_range(self, field, cell0, ncells):
        return self.f[field][cell0:cell0 + ncells].copy()

    def get_field_dev(self, field, out=None, dtype=None, cell0=0, ncells=None):
        return self.get_field_range(field, cell0, self.ncells - cell0 if ncells is None else ncells)

    def get_frame_dev(self, field, m=1, slice=None):
        """tests/frame_cases.py host_frame of the field, the sliced axes dropped as HipBlock.get_frame_dev drops them;
        frame_lebesgue: the largest sum_a |phi_a| over the pixels; frame_scale: max |field|"""
        from tests.frame_cases import host_frame
        img, px = host_frame(case_cfg(self.case), self.case.degree, self.case.cell == _Q, m, slice, self.f[field])
        self.frame_lebesgue = float(np.abs(px["phi"]).sum(axis=1).max())
        self.frame_scale = float(np.abs(self.f[field]).max())
        free = [a for a in reversed(range(self.dim)) if not px["frame"].fixed[a]]
        return img.reshape(self.f[field].shape[2:] + tuple(px["P"][a] for a in free))

    def stage_kernel_name(self, stage):
        return kernel_names(self.case, self.sym)[stage]

    def counters(self):
        return dict(steps=self.steps, launches=[self.steps] * 6)      # six launches, one per stage, per step

    def get_field(self, field):
        return self.f[field].copy()

    # ---- the operators and the step -------------------------------------------------------------------------------------
    def apply_F(self, s_in, u_abs, u_out):
        self.f[u_out] = self.orc.E.apply_F(self.f[s_in], self.f[u_abs])

    def apply_G(self, u_in, s_out, use_source=False):
        assert not use_source
        self.f[s_out] = self.orc.E.apply_G(self.f[u_in], self.lam, self.mu)

    def _source_now(self):
        """(nodes, values [nnz, d, d]) of the step about to run, or None"""
        if self.src is None:
            return None
        nodes, table, static = self.src
        if static:
            return nodes, table[0]
        return (nodes, table[self.src_step]) if self.src_step < len(table) else None

    def _cport_extra(self):
        from oracle.cport import sponge_blocks
        src = self.src
        self.cp.set_extra(lam=self.lam if np.ndim(self.lam) else None, mu=self.mu if np.ndim(self.mu) else None,
                          rho=self.rho if np.ndim(self.rho) else None, rho_physical=self.physical,
                          sponge=sponge_blocks(self.mesh, self.case.degree, *self.sigma) if self.sigma is not None else None,
                          src_nodes=src[0] if src is not None else None, src_values=src[1] if src is not None else None)
        self._dirty = False

    def _one_step(self):
        dt = self.dt
        now = self._source_now()
        if self.engine == "numpy":
            orc = self.orc
            orc.u0, orc.s0, orc.dt, orc.l, orc.mu = self.f[FIELD_U], self.f[FIELD_S], dt, self.lam, self.mu
            orc.density, orc.density_physical = self.rho, self.physical
            S = None
            if now is not None:
                S = np.zeros((self.ncells * self.nd, self.dim, self.dim))
                S[now[0]] = now[1]
                S = S.reshape(self.f[FIELD_S].shape)
            orc.source = (lambda t: S) if S is not None else None
            orc.step(None)
            u1, s1, utemp, sh1 = orc.u1, orc.s1, orc.last["utemp"], orc.last["sh1"]
        else:
            if self._dirty:
                self._cport_extra()
            static = self.src is not None and self.src[2]
            scalar = lambda v: 0.0 if np.ndim(v) else float(v)      # noqa: E731  (an array went through set_extra)
            u1, s1 = self.cp.step_ex(self.f[FIELD_U], self.f[FIELD_S], scalar(self.rho), dt, scalar(self.lam), scalar(self.mu), 1,
                                     step0=0 if static else self.src_step)
            utemp, sh1 = self.cp.work[0], self.cp.work[1].copy()
        # what a step leaves in the work fields: w = dt u1 + dt^3/24 utemp (stage UTEMP) and sh1 = G(u1) + S (stage SH1)
        self.f = {FIELD_U: u1, FIELD_S: s1, FIELD_UH: dt * u1 + dt ** 3 / 24.0 * utemp, FIELD_SH: sh1}
        self.src_step += 1
        self.steps += 1
        r = self.rec
        if r is not None:
            r["steps"] += 1
            if r["steps"] % r["every"] == 0:
                assert len(r["samples"]) < r["capacity"], "the script overfills the trace"
                rows = []
                for k, c in enumerate(r["cell"]):
                    uu = r["phi"][k] @ u1[c] if c >= 0 else np.zeros(self.dim)
                    ss = np.tensordot(r["phi"][k], s1[c], axes=(0, 0)).reshape(-1) if c >= 0 else np.zeros(self.dim ** 2)
                    rows.append(np.concatenate(([uu] if r["what"] & 1 else []) + ([ss] if r["what"] & 2 else [])))
                r["samples"].append(rows)
                self.rec_scales.append((np.abs(u1).max(), np.abs(s1).max()))
                self.rec_log.append((self.ncheck, self.stretch))
        # the other hooks of the one clock, in its order: monitor, spectra, and last the injectors' entry, which belongs to
        # the step that follows - no sample of this step contains it
        where = (self.ncheck, self.stretch)
        m = self.mon
        if m is not None:
            m["steps"] += 1
            if m["steps"] % m["every"] == 0:
                assert len(m["samples"]) < m["capacity"], "the script overfills the monitor's trace"
                m["samples"].append(self._sample(u1, s1, m["w"]))
                m["abs"].append(self._sample(u1, s1, None if m["w"] is None else np.abs(m["w"])))
                m["log"].append(where)
        p = self.spc
        if p is not None:
            p["steps"] += 1
            j = p["steps"] // p["every"] - 1
            if p["steps"] % p["every"] == 0 and j < p["nsamples"]:
                for k, fld in enumerate((u1, s1)):
                    if p["w"][k] is not None:
                        p["acc"][k] = p["acc"][k] + p["w"][k][j].reshape((-1,) + (1,) * fld.ndim) * fld[None]
                p["log"].append(where + (np.abs(u1).max(), np.abs(s1).max()))
        q = self.inj
        if q is not None:
            k, q["steps"] = q["steps"], q["steps"] + 1
            if k < len(q["series"]):
                self._add(q["cell"], q["psi"], q["series"][k], q["what"])

    def _stepped(self, n):
        if {FIELD_U, FIELD_S} <= self._fresh:
            self.stretch = 0
        self._fresh = set()
        for _ in range(n):
            self.stretch += 1
            self._one_step()

    def step(self, nsteps=1):
        self._stepped(int(nsteps))

    def run_stage(self, stage):
        """the six stages of a host-driven step: the mirror takes the whole step at sg_end_step"""
        assert 0 <= stage < 6

    def end_step(self):
        self._stepped(1)

    def checkpoint(self):
        self.ncheck += 1


def mirror_run(case, engine="numpy", seed=0):
    """(script, what the mirror observes)"""
    script = make_script(case, seed)
    return script, run_script(Mirror(case, engine), script)


def hooks_mirror_run(case, engine="numpy", seed=0):
    """(the second script, what the mirror observes)"""
    script = make_hooks_script(case, seed)
    return script, run_script(Mirror(case, engine), script)


def rel_field_error(got, want):
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def floor_of(obs_a, obs_b):
    """the largest relative difference of the four fields at every checkpoint of two mirror runs"""
    out = []
    for a, b in zip(obs_a, obs_b):
        assert (a["i"], a["op"]) == (b["i"], b["op"])
        if a["op"] in STEPPING:
            out.append(max(rel_field_error(a[k], b[k]) for k in ("u", "s", "uh", "sh")))
    return out
