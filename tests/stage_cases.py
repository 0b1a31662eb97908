"""The six fused LF4 stages stated once, on the oracle's operators, with inputs that give every term of a stage full weight.

A stage (include/seigen_hip.h enum sg_stage, hostapi.cpp lf4_stage) takes independent operand fields U, UH, S, SH; with
c3 = dt^3 / 24, F(T; u) = Minv f(T) - A u (A the sponge matrix) and G(u) = Minv g(u; lam, mu):

  UH1    UH <- F(S; U)
  STEMP  SH <- G(UH) + Ssrc
  U1     U  <- rho U + dt UH + c3 F(SH; U)          scalar / per-cell density, the explicit reference's convention
            or U + (dt UH + c3 F(SH; U)) / rho      physical
  SH1    SH <- G(U) + Ssrc
  UTEMP  UH <- dt U + c3 F(SH; U)
  S1     S  <- S + G(UH) + (dt + c3) Ssrc

stage_terms() returns the summands one by one - self, aux, lin (c_new times the linear part of F or G), sponge (c_new times
-A u), source - and stage_result() their sum.  Whole steps at a stable dt weigh the fused terms at 1e-4 and less of the
result, so a comparison of steps cannot see an error in them (tests/test_stage_cases_oracle.py measures that); a stage has no
stability limit, so build() fixes dt = 1.9 - dt and c3 = 0.286 of the same order, neither a trivial factor - and scales the
sponge, the source and, per stage, the operands by factors computed from the oracle's own terms until every term a stage has
is at least MIN_SHARE of the max-norm of its result.  The condition is asserted wherever inputs are drawn.

MUTATIONS restate the mistakes a fused epilogue can make; stage_terms(..., mutation=name) evaluates the stage with one of them.

Nothing here imports the library: the GPU rows (tests/test_stage_alone_gpu.py) upload what this module draws."""
import numpy as np

FIELDS = ("U", "UH", "S", "SH")
STAGES = ("UH1", "STEMP", "U1", "SH1", "UTEMP", "S1")
OUTPUT = {"UH1": "UH", "STEMP": "SH", "U1": "U", "SH1": "SH", "UTEMP": "UH", "S1": "S"}
OPERANDS = {"UH1": ("S", "U"), "STEMP": ("UH",), "U1": ("U", "UH", "SH"), "SH1": ("U",), "UTEMP": ("U", "SH"), "S1": ("S", "UH")}
DT = 1.9
MIN_SHARE = 0.05
DENSITIES = ("scalar", "cell", "physical")

# name: the stages it can be applied to, the density conventions under which it changes anything (None: all)
MUTATIONS = {
    "c_new 0.999": (STAGES, None),
    "source coefficient dt": (("S1",), None),
    "physical density on the dt term only": (("U1",), ("physical",)),
    "density of the neighbouring cell": (("U1",), ("cell", "physical")),
    "sponge operand from UH": (("U1",), None),
    "sponge dropped": (("UH1", "U1", "UTEMP"), None),
    "c_self rho under the physical convention": (("U1",), ("physical",)),
}


def max_norm(a):
    return float(np.abs(a).max())


def draw_density(convention, ncells, rng):
    """the family rows' densities: 1.1, per cell in the explicit convention, per cell physical"""
    assert convention in DENSITIES, convention
    if convention == "scalar":
        return 1.1
    return rng.uniform(0.9, 1.1, ncells) if convention == "cell" else rng.uniform(0.8, 1.5, ncells)


def draw_stress(shape, rng, sym):
    """symmetric in symmetric-storage rows; uniform on (-1, 1) in every entry otherwise, so s_ij != s_ji"""
    s = rng.uniform(-1, 1, shape)
    if not sym:
        return s
    return 0.5 * (s + np.swapaxes(s, -1, -2))


def scatter_source(ncells, nd, dim, nodes, vals):
    """the nodal source as the array the oracle adds: a node listed twice gets both values"""
    S = np.zeros((ncells * nd, dim, dim))
    np.add.at(S, np.asarray(nodes), vals)
    return S.reshape(ncells, nd, dim, dim)


class Operators(object):
    """F and G of one ElasticOperators in their parts, with the case's material; the sponge matrix is held here and never
    left on E, which several rows may share"""

    def __init__(self, E, lam, mu, absorb=None):
        self.E, self.lam, self.mu, self.absorb = E, lam, mu, absorb
        self.shape_u = (E.mesh.ncells, E.nd, E.dim)

    def F_lin(self, T):
        held, self.E.absorb = self.E.absorb, None
        try:
            return self.E.apply_F(T, None)
        finally:
            self.E.absorb = held

    def sponge(self, u):
        """-A u, or None where the case has no sponge cell"""
        if self.absorb is None:
            return None
        return -(self.absorb @ u.reshape(self.E.ops.N, self.E.dim)).reshape(self.shape_u)

    def G_lin(self, u):
        return self.E.apply_G(u, self.lam, self.mu)


def stage_terms(ops, stage, fields, dt, density, physical, Ssrc, mutation=None):
    """The summands of `stage` from the operand fields (a dict by field name; only OPERANDS[stage] are read), as a dict in
    the order self, aux, lin, sponge, source with the terms the stage has.  density: a float or one value per cell;
    Ssrc: the scattered source of the step, or None.  mutation: a key of MUTATIONS, applied if the stage is one of its."""
    if mutation is not None:
        assert mutation in MUTATIONS, mutation
        if stage not in MUTATIONS[mutation][0]:
            mutation = None
    c3 = dt ** 3 / 24.0
    rho = np.asarray(density, dtype=np.float64).reshape(-1, 1, 1) if np.ndim(density) else float(density)
    c_new_factor = 0.999 if mutation == "c_new 0.999" else 1.0
    T = {}

    def f_terms(c_new, stress, u_abs):
        T["lin"] = c_new * c_new_factor * ops.F_lin(stress)
        sp = None if mutation == "sponge dropped" else ops.sponge(u_abs)
        if sp is not None:
            T["sponge"] = c_new * c_new_factor * sp

    def g_terms(u, src_coef):
        T["lin"] = c_new_factor * ops.G_lin(u)
        if Ssrc is not None:
            T["source"] = src_coef * Ssrc

    if stage == "UH1":
        f_terms(1.0, fields["S"], fields["U"])
    elif stage in ("STEMP", "SH1"):
        g_terms(fields["UH" if stage == "STEMP" else "U"], 1.0)
    elif stage == "U1":
        rho_new = rho
        if mutation == "density of the neighbouring cell":
            assert np.ndim(rho), "a scalar density has no neighbour"
            rho_new = np.roll(rho, 1, axis=0)
        if physical:
            T["self"] = fields["U"] * (rho if mutation == "c_self rho under the physical convention" else 1.0)
            T["aux"] = dt * fields["UH"] / rho_new
            f_terms(c3, fields["SH"], fields["UH"] if mutation == "sponge operand from UH" else fields["U"])
            if mutation != "physical density on the dt term only":
                for k in ("lin", "sponge"):
                    if k in T:
                        T[k] = T[k] / rho_new
        else:
            T["self"] = rho_new * fields["U"]
            T["aux"] = dt * fields["UH"]
            f_terms(c3, fields["SH"], fields["UH"] if mutation == "sponge operand from UH" else fields["U"])
    elif stage == "UTEMP":
        T["aux"] = dt * fields["U"]
        f_terms(c3, fields["SH"], fields["U"])
    elif stage == "S1":
        T["self"] = fields["S"]
        g_terms(fields["UH"], dt if mutation == "source coefficient dt" else dt + c3)
    else:
        raise ValueError(stage)
    return {k: T[k] for k in ("self", "aux", "lin", "sponge", "source") if k in T}


def stage_result(terms):
    out = 0.0
    for t in terms.values():
        out = out + t
    return out


def shares(terms):
    """each term's max-norm over the max-norm of the stage's result"""
    total = max_norm(stage_result(terms))
    return {k: max_norm(t) / total for k, t in terms.items()}


def chain_step(ops, fields, dt, density, physical, Ssrc, mutation=None, mutate_stage=None, scale=None):
    """One whole LF4 step as the six stages in their order on the four fields (a dict, updated in place).  mutation: a key
    of MUTATIONS applied to the stages it names (to mutate_stage only, if given); scale = (stage, term or terms, factor): those
    terms of that stage times factor - the table of tests/test_stage_cases_oracle.py."""
    for stage in STAGES:
        terms = stage_terms(ops, stage, fields, dt, density, physical, Ssrc,
                            mutation if mutate_stage in (None, stage) else None)
        if scale is not None and scale[0] == stage:
            for name in (scale[1] if isinstance(scale[1], tuple) else (scale[1],)):
                if name in terms:
                    terms[name] = terms[name] * scale[2]
        fields[OUTPUT[stage]] = stage_result(terms)
    return fields


class StageCase(object):
    """Balanced inputs of one configuration: dt, the scaled sponge and source, and per stage the operand fields.

    build() draws them; `sigma` and `src_vals` are what a block is given (sg_set_absorption, sg_set_source), `Ssrc` the
    scattered entry 0 of the source, `inputs[stage]` the operand fields by name, `expected[stage]` the stage's result and
    `share[stage]` the weight of each of its terms."""

    def __init__(self, ops, dt, density, physical, sym, sigma, nodes, src_vals, Ssrc):
        self.ops, self.dt, self.density, self.physical, self.sym = ops, dt, density, physical, sym
        self.sigma, self.nodes, self.src_vals, self.Ssrc = sigma, nodes, src_vals, Ssrc
        self.inputs, self.expected, self.share = {}, {}, {}
        nc, nd, d = ops.shape_u
        self.shape = {"U": (nc, nd, d), "UH": (nc, nd, d), "S": (nc, nd, d, d), "SH": (nc, nd, d, d)}

    def terms(self, stage, fields=None, mutation=None):
        return stage_terms(self.ops, stage, self.inputs[stage] if fields is None else fields, self.dt, self.density,
                           self.physical, self.Ssrc, mutation)

    def draw(self, stage, rng, keep=None):
        """fresh operands of `stage`, each scaled by the max-norm of the oracle's term it enters (the sponge and the source
        keep the scale build() gave them); keep: operand fields to take as they are.  Asserts the balance."""
        dt, c3 = self.dt, self.dt ** 3 / 24.0
        ops = self.ops
        raw = {f: (rng.uniform(-1, 1, self.shape[f]) if f in ("U", "UH") else draw_stress(self.shape[f], rng, self.sym))
               for f in OPERANDS[stage]}
        f = {}
        if stage == "UH1":
            f["U"] = c3 * raw["U"]
            f["S"] = raw["S"] / max_norm(ops.F_lin(raw["S"]))
        elif stage == "STEMP":
            f["UH"] = raw["UH"] / max_norm(ops.G_lin(raw["UH"]))
        elif stage == "U1":
            f["U"] = raw["U"]
            f["UH"] = raw["UH"] / dt
            f["SH"] = raw["SH"] / (c3 * max_norm(ops.F_lin(raw["SH"])))
        elif stage == "SH1":
            f["U"] = raw["U"] / max_norm(ops.G_lin(raw["U"]))
        elif stage == "UTEMP":
            f["U"] = raw["U"]
            f["SH"] = raw["SH"] / (c3 * max_norm(ops.F_lin(raw["SH"])))
        else:
            f["S"] = raw["S"]
            f["UH"] = raw["UH"] / max_norm(ops.G_lin(raw["UH"]))
        for name, a in (keep or {}).items():
            f[name] = a
        terms = self.terms(stage, f)
        share = shares(terms)
        assert min(share.values()) >= MIN_SHARE, (stage, share)
        return f, stage_result(terms), share


def build(E, lam, mu, density, physical, sym, sigma0, absorb0, nodes, vals0, rng, dt=DT):
    """A StageCase on the operators E.  sigma0 [ncells, nodes of its degree]: the row's sponge before scaling, absorb0 its
    matrix (ScalarOperators.absorption_matrix, linear in sigma) - both None for a case without a sponge, and a sigma that is
    zero everywhere (a block of one cell of the kind `none`) counts as none; nodes, vals0 [nsteps, nnz, d, d]: the row's
    source before scaling, entry 0 the one the stages add.

    The sponge is scaled until c3 |A u| = 1 for a velocity of amplitude 1, the source until its scattered entry 0 is 1 in
    the max-norm; draw() does the rest per stage."""
    c3 = dt ** 3 / 24.0
    nc, nd, d = E.mesh.ncells, E.nd, E.dim
    if absorb0 is not None and absorb0.nnz and np.abs(absorb0.data).max() > 0:
        probe = rng.uniform(-1, 1, (nc, nd, d))
        k = 1.0 / (c3 * max_norm(absorb0 @ probe.reshape(nc * nd, d)))
        sigma, absorb = k * np.asarray(sigma0), (k * absorb0).tocsr()
    else:
        sigma, absorb = (None if sigma0 is None else np.asarray(sigma0)), None
    vals0 = np.asarray(vals0, dtype=np.float64)
    src_vals = vals0 / max_norm(scatter_source(nc, nd, d, nodes, vals0[0]))
    Ssrc = scatter_source(nc, nd, d, nodes, src_vals[0])
    case = StageCase(Operators(E, lam, mu, absorb), dt, density, physical, sym, sigma, np.asarray(nodes), src_vals, Ssrc)
    for stage in STAGES:
        case.inputs[stage], case.expected[stage], case.share[stage] = case.draw(stage, rng)
    return case
