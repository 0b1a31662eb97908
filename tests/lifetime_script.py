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

Nothing here needs a GPU.  Point location and the basis at a receiver are the library's device-free entry points
(sg_locate_points, sg_tabulate_cell), through tests/test_receivers_gpu.py _locate_on as in its host_samples."""
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
    def __init__(self, case, rng, omit):
        self.case, self.rng, self.omit = case, rng, omit
        self.ops = []
        self.stretch = 0
        self.nc = int(np.prod(case.n)) * ncls_of(case)
        self.nd = nnodes(case.dim, case.degree, case.cell)
        d = case.dim
        self.ushape, self.sshape = (self.nc, self.nd, d), (self.nc, self.nd, d, d)
        self.symmetric = case.sym        # the data handed over so far is symmetric

    def add(self, op, tag, **args):
        args["tag"] = tag
        self.ops.append((op, args))

    def wants(self, tag):
        assert tag in TAGS, tag
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


# ---- applying it ------------------------------------------------------------------------------------------------------------

def _snapshot(target):
    c = target.counters()
    return dict(u=target.get_field(FIELD_U), s=target.get_field(FIELD_S), uh=target.get_field(FIELD_UH),
                sh=target.get_field(FIELD_SH), steps=c["steps"], launches=list(c["launches"]), sym=target.is_sym(),
                stretch=getattr(target, "stretch", None))


def run_script(target, script):
    """Apply the script to `target` - a HipBlock, or anything with its method names - and return what can be observed, one
    dict per observing operation: {"i": index in the script, "op", "tag"} and, after a stepping call (a checkpoint), the four
    fields, the counters and is_sym(); after apply_F / apply_G the field written; for get_receivers the samples; for
    kernels the six stage kernel names."""
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
                       lebesgue=getattr(target, "rec_lebesgue", None), what=getattr(target, "rec_what", None))
        elif op == "kernels":
            obs = dict(names=[target.stage_kernel_name(st) for st in range(6)])
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
        self.rec_scales, self.rec_what = [], int(what)
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

    def _stepped(self, n):
        if {FIELD_U, FIELD_S} <= self._fresh:
            self.stretch = 0
        self._fresh = set()
        for _ in range(n):
            self._one_step()
        self.stretch += n

    def step(self, nsteps=1):
        self._stepped(int(nsteps))

    def run_stage(self, stage):
        """the six stages of a host-driven step: the mirror takes the whole step at sg_end_step"""
        assert 0 <= stage < 6

    def end_step(self):
        self._stepped(1)


def mirror_run(case, engine="numpy", seed=0):
    """(script, what the mirror observes)"""
    script = make_script(case, seed)
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
