"""The material-gradient loop on the oracle (a helper of tests/test_gradient_oracle.py and tests/test_gradient_gpu.py, no
test itself): the forward run, the adjoint run beside the stored forward states, the per-cell correlations of any pairing of
the two, the misfit and its central differences.

Forward: zero fields, a point force as velocity entries q_k psi (psi of sg_injector_weights: the library adds exactly amp * psi,
so q is held fixed when the material moves), q_0 before step 1 and q_k behind step k; d_k = R u after step k and before q_k
goes in (sg_locate_points + sg_tabulate_cell); J = 1/2 sum_k |d_k - obs_k|^2.  A step is the velocity half V: u += P s / rho
and then the stress half S: s += Q u, with per-cell lambda, mu and the physical per-cell rho (OracleLF4, density_physical).

Adjoint: in the energy inner product W = |det J| (rho/2 u^T Mhat u' + 1/(4 mu) s:Mhat:s' + wt tr Mhat tr') the adjoint of a
step is the step with -dt (tests/test_injectors_host.py), and W^-1 R^T r = (2 / rho_cell) r psi.  So the adjoint state gets
(2 / rho_cell) r_k psi, k = K .. 1, before adjoint step j + 1 = K - k + 1 and then holds a_k = W^-1 dJ/dx_k; after its velocity
half it holds W^-1 dJ/dy_k, y_k = V x_{k-1} the forward MID-step state (u_k, s_{k-1}).  The derivative of J with respect to a
cell's rho enters through V alone: dV/drho x_{k-1} = -(u_k - u_{k-1}) / rho, the pure increment of the step.  Hence

    dJ/drho_c = -1/2 sum_k |det J| a_mid^T Mhat (u_k - u_{k-1})       exactly,

with a_mid the adjoint velocity AFTER its velocity half; the same pairing with the not-yet-stepped adjoint stress gives
dJ/dlambda, dJ/dmu = -1/2 sensitivity(...) up to O(dt^2) (the compliance form s : C^-1 : s' differentiates dt C D u, the
leading term of Q u).  PAIRINGS names that pairing and the near misses the tests must tell from it."""
import numpy as np

from oracle.forms import ElasticOperators
from seigen_amd.backend import injector_weights
from seigen_amd.elastic import sensitivity
from tests.test_injectors_host import basis_at, make_cfg, mass_matrix
from tests.util import oracle_mesh

# adjoint state x forward state of every call; "midstep" is the gradient
PAIRINGS = (
    "midstep",              # adjoint after its velocity half x (step's own result - state before the step)
    "stress_after",         # adjoint after its whole step    x the same increment: the stress is half a step late
    "velocity_before",      # adjoint before its step         x the same increment: the velocity is half a step early
    "zero_lag",             # adjoint after its whole step x the re-wound forward state, weight dt: an imaging condition
    "entry_left_in",        # midstep, but the + state still holds the force entry q_k that followed the step
)


class Geometry(object):
    """mesh, operators and point tables of one row: (dim, degree, cubes, diagonal) on the unit box"""

    def __init__(self, dim, degree, n, diagonal="left"):
        self.dim, self.degree, self.n, self.diagonal = dim, degree, tuple(n), diagonal
        self.quad = diagonal == "quadrilateral"
        self.h = [1.0 / k for k in n]
        self.mesh = oracle_mesh(dim, n, (1.0,) * dim, diagonal)
        self.E = ElasticOperators(self.mesh, degree)
        self.nd, self.ncells = self.E.nd, self.mesh.ncells
        self.cfg = make_cfg(dim, degree, n, self.h, self.quad)
        self.M = mass_matrix(dim, degree, self.quad)
        self.detj = float(np.prod(self.h))

    def points(self, pts):
        """(cell, phi, psi) of physical points: the receivers' row and the injectors' column"""
        pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, self.dim)
        cell, phi = basis_at(self.cfg, pts, self.quad)
        cell_i, psi = injector_weights(self.cfg, pts, self.nd)
        assert np.array_equal(cell, cell_i) and (cell >= 0).all()
        return cell, phi, psi

    def zeros(self):
        return np.zeros((self.ncells, self.nd, self.dim)), np.zeros((self.ncells, self.nd, self.dim, self.dim))

    def forms(self, a, b):
        """|det J| (u^T Mhat u', s : Mhat : s', tr Mhat tr') per cell: [ncells, 3]"""
        (ua, sa), (ub, sb) = a, b
        uu = np.einsum("cai,ab,cbi->c", ua, self.M, ub)
        ss = np.einsum("caij,ab,cbij->c", sa, self.M, sb)
        tt = np.einsum("ca,ab,cb->c", np.trace(sa, axis1=-2, axis2=-1), self.M, np.trace(sb, axis1=-2, axis2=-1))
        return self.detj * np.stack([uu, ss, tt], axis=-1)


def velocity_half(E, u, s, mat, dt):
    """stages UH1, STEMP, U1 of OracleLF4.step with density_physical: the same expressions in the same order"""
    lam, mu, rho = mat
    uh1 = E.apply_F(s, u)
    uh2 = E.apply_F(E.apply_G(uh1, lam, mu), u)
    return u + (dt * uh1 + (dt ** 3 / 24.0) * uh2) / np.asarray(rho, dtype=np.float64).reshape(-1, 1, 1)


def stress_half(E, u, s, mat, dt):
    """stages SH1, UTEMP, S1"""
    lam, mu, rho = mat
    sh1 = E.apply_G(u, lam, mu)
    sh2 = E.apply_G(E.apply_F(sh1, u), lam, mu)
    return s + dt * sh1 + (dt ** 3 / 24.0) * sh2


def add_entries(u, cell, psi, amp):
    """u + sum_r amp[r] psi_r in the cells that hold the points (a copy)"""
    u = u.copy()
    for r in range(len(cell)):
        u[cell[r]] += psi[r][:, None] * amp[r][None, :]
    return u


def forward(geo, mat, dt, xs, q, xr, keep=False):
    """d [K, R, dim]; with keep also own[k - 1] = the result of step k before its entry and start[k - 1] = the state step k
    started from (entry q_{k-1} included), k = 1 .. K"""
    cs, _, psis = geo.points(xs)
    cr, phir, _ = geo.points(xr)
    q = np.asarray(q, dtype=np.float64).reshape(len(q), len(cs), geo.dim)
    u, s = geo.zeros()
    u = add_entries(u, cs, psis, q[0])
    d, own, start = [], [], []
    for k in range(1, len(q) + 1):
        if keep:
            start.append((u, s))
        u = velocity_half(geo.E, u, s, mat, dt)
        s = stress_half(geo.E, u, s, mat, dt)
        d.append(np.array([phir[r] @ u[cr[r]] for r in range(len(cr))]))
        if keep:
            own.append((u, s))
        if k < len(q):
            u = add_entries(u, cs, psis, q[k])
    return (np.array(d), own, start) if keep else np.array(d)


def misfit(d, obs):
    return 0.5 * float(np.sum((d - obs) ** 2))


def residual_entries(geo, mat, xr, res):
    """the adjoint's series: entry j = (2 / rho_cell) r_{K-j} at the receivers, the last residual first"""
    cr, _, _ = geo.points(xr)
    return res[::-1] * (2.0 / np.asarray(mat[2], dtype=np.float64)[cr])[None, :, None]


def gradient_loop(geo, mat, dt, xs, q, xr, obs, pairings=("midstep",)):
    """{"J", "d", "acc": {pairing: [ncells, 3]}, "scale": {pairing: [3]}, "terms": {pairing: [calls, ncells, 3]}}: the
    accumulated (uu, ss, tt) of every requested pairing, every single call's term, and scale_k = the sum over the calls of
    the largest absolute per-cell term - what an error of the accumulators is measured against, since the sums cancel."""
    d, own, start = forward(geo, mat, dt, xs, q, xr, keep=True)
    K = len(d)
    res = d - obs
    series = residual_entries(geo, mat, xr, res)
    cr, _, psir = geo.points(xr)
    cs, _, psis = geo.points(xs)
    q = np.asarray(q, dtype=np.float64).reshape(K, len(cs), geo.dim)
    au, as_ = geo.zeros()
    terms = {p: [] for p in pairings}
    for j in range(K):
        k = K - j
        au = add_entries(au, cr, psir, series[j])
        before = (au, as_)
        au = velocity_half(geo.E, au, as_, mat, -dt)
        mid = (au, as_)
        as_ = stress_half(geo.E, au, as_, mat, -dt)
        after = (au, as_)
        plus, minus = own[k - 1], start[k - 1]
        for p in pairings:
            if p == "zero_lag":
                calls = [(dt, after, minus)]
            elif p == "entry_left_in":
                left = (add_entries(plus[0], cs, psis, q[k]), plus[1]) if k < K else plus
                calls = [(1.0, mid, left), (-1.0, mid, minus)]
            else:
                a = {"midstep": mid, "stress_after": after, "velocity_before": before}[p]
                calls = [(1.0, a, plus), (-1.0, a, minus)]
            terms[p] += [w * geo.forms(a, x) for w, a, x in calls]
    terms = {p: np.array(t) for p, t in terms.items()}
    return {"J": misfit(d, obs), "d": d,
            "acc": {p: t.sum(axis=0) for p, t in terms.items()},
            "scale": {p: np.abs(t).max(axis=1).sum(axis=0) for p, t in terms.items()},
            "terms": terms}


def gradient_of(dim, mat, acc):
    """dJ/d(rho, lambda, mu) per cell from the accumulators of the midstep pairing: -1/2 sensitivity"""
    lam, mu, rho = mat
    K = sensitivity(dim, rho, lam, mu, {"uu": acc[:, 0], "ss": acc[:, 1], "tt": acc[:, 2]})
    return {k: -0.5 * v for k, v in K.items()}


def central_differences(J_of, mat, cells, eps=1e-5, params=("rho", "lambda", "mu")):
    """{param: [len(cells)]}: (J(m_c (1 + eps)) - J(m_c (1 - eps))) / (2 eps m_c) for the listed cells; J_of(mat) -> J"""
    index = {"lambda": 0, "mu": 1, "rho": 2}
    out = {}
    for p in params:
        g = []
        for c in cells:
            J = []
            for sign in (1.0, -1.0):
                m = [np.array(a, dtype=np.float64) for a in mat]
                m[index[p]][c] *= 1.0 + sign * eps
                J.append(J_of(tuple(m)))
            g.append((J[0] - J[1]) / (2.0 * eps * mat[index[p]][c]))
        out[p] = np.array(g)
    return out


def material(ncells, seed):
    """per-cell (lambda, mu, rho)"""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.4, 0.8, ncells), rng.uniform(0.2, 0.4, ncells), rng.uniform(0.8, 1.6, ncells)


def ricker(t, a, t0):
    return (1.0 - 2.0 * a * (t - t0) ** 2) * np.exp(-a * (t - t0) ** 2)


# ---- the rows of tests/test_gradient_gpu.py: one per layout, from the table of tests/test_correlate_gpu.py ------------------
# (name, dim, degree, cubes, diagonal, dtype, SEIGEN_HIP_PATH)
ROWS = [
    ("mfma-P4-sym", 3, 4, (3, 2, 2), "left", "f64", None),
    ("mfma-P3-sym", 3, 3, (4, 3, 2), "left", "f64", None),
    ("tile-tri-P3", 2, 3, (5, 3), "left", "f64", None),
    ("tile-quad-P2", 2, 2, (5, 3), "quadrilateral", "f64", None),
    ("hexm-DQ3", 3, 3, (3, 2, 2), "quadrilateral", "f64", None),
    ("lane-2d-P2", 2, 2, (5, 3), "left", "f64", "lane"),
    ("generic-2d-P2", 2, 2, (4, 3), "left", "f64", "generic"),
    ("mfma-P3-f32", 3, 3, (4, 3, 2), "left", "f32", None),
    ("tile-tri-P3-f32", 2, 3, (5, 3), "left", "f32", None),
]
DT_FACTOR = 0.3          # dt = DT_FACTOR * min(h) / degree^2
_ROW_CASES, _ROW_REFERENCES = {}, {}


def row_case(row):
    """the inputs of a row: per-cell lambda, mu, rho; a force series at one interior point and one on a grid line; three
    receivers, one of them in the interior source's cell; K = 6 steps in 3-D, 12 in 2-D"""
    name, dim, degree, n, diagonal = row[:5]
    key = (dim, degree, tuple(n), diagonal)      # no dtype, no path: the oracle is double, an f32 row shares its f64 row's case
    if key not in _ROW_CASES:
        geo = Geometry(dim, degree, n, diagonal)
        mat = material(geo.ncells, 10 * dim + degree)
        K = 6 if dim == 3 else 12
        dt = DT_FACTOR * min(geo.h) / degree ** 2
        xs = np.array([[0.41, 0.57, 0.33][:dim], [geo.h[0], 0.23, 0.61][:dim]])
        xr = np.array([[0.43, 0.55, 0.36][:dim], [0.8, 0.7, 0.2][:dim], [0.15, 0.3, 0.7][:dim]])
        k = np.arange(K)
        q = np.stack([np.cos(0.9 * k + 0.4 * i)[:, None] * np.array([1.0, 0.6, -0.8][:dim])[None] * (1.0 - 0.5 * i)
                      for i in range(len(xs))], axis=1) * dt
        d0 = forward(geo, mat, dt, xs, q, xr)
        j = np.arange(1, K + 1)
        obs = np.abs(d0).max() * np.stack([np.sin(0.7 * j + r)[:, None] * np.array([0.5, -0.3, 0.2][:dim])[None]
                                           for r in range(len(xr))], axis=1)
        _ROW_CASES[key] = dict(geo=geo, mat=mat, K=K, dt=dt, xs=xs, q=q, xr=xr, obs=obs)
    return _ROW_CASES[key]


def row_reference(row):
    """the oracle's loop of a row, once"""
    name, dim, degree, n, diagonal = row[:5]
    key = (dim, degree, tuple(n), diagonal)
    if key not in _ROW_REFERENCES:
        c = row_case(row)
        _ROW_REFERENCES[key] = gradient_loop(c["geo"], c["mat"], c["dt"], c["xs"], c["q"], c["xr"], c["obs"])
    return _ROW_REFERENCES[key]


DENSITY_ROWS = ("tile-tri-P3", "mfma-P4-sym")


def density_cells(row):
    """the four cells whose dJ/drho the device test takes by central differences: the interior source's (it holds a receiver
    too), the other receivers' cell with the largest entry, and the two largest that hold neither a source nor a receiver;
    every entry above 1e-3 of the largest (by the oracle's loop)"""
    case, ref = row_case(row), row_reference(row)
    geo = case["geo"]
    cs, cr = geo.points(case["xs"])[0], geo.points(case["xr"])[0]
    g = np.abs(gradient_of(row[1], case["mat"], ref["acc"]["midstep"])["rho"])
    held = {int(c) for c in cs} | {int(c) for c in cr}
    free = [int(c) for c in np.argsort(-g) if int(c) not in held][:2]
    receiver = max((int(c) for c in cr if int(c) != int(cs[0])), key=lambda c: g[c])
    cells = [int(cs[0]), receiver] + free
    assert int(cs[0]) in {int(c) for c in cr} and len(set(cells)) == 4
    assert g[cells].min() > 1e-3 * g.max(), g[cells] / g.max()
    return cells
