"""The adjoint-state material gradient on the oracle (CPU only): which sequence of the documented pieces - point-force
entries, receivers, residuals injected into a handle stepped with -dt, re-wound forward states, per-cell correlations,
`sensitivity` - is the derivative of the misfit J = 1/2 sum_k |R u_k - obs_k|^2, pinned against central differences of J
(tests/gradient_loop.py holds the loop and its derivation).

The pairing: the adjoint state after its VELOCITY HALF (stepped u, not yet stepped s), weights (+1, +1, +1) against the
forward step's own result, (-1, -1, -1) against the state that step started from; then dJ/dm = -1/2 sensitivity(...).
  rho          exact: a discrete identity.  Measured against central differences (relative step 1e-5) 3e-11 .. 4e-10 of the
               largest difference: that is the differences' floor.  Asserted to 1e-7.
  lambda, mu   second order in dt.  Measured on the 4 x 4 P2 case at dt = 1/80, 1/160, 1/320 over the same signals:
               lambda 1.31e-2, 3.23e-3, 8.04e-4 and mu 1.58e-2, 3.92e-3, 9.79e-4 of the largest difference (orders 2.0).
Near misses are first order: the adjoint stress after its step 35 % / 18 % / 9.1 % (lambda) and 69 % / 35 % / 18 % (mu), the
adjoint velocity before its step 17 % / 7.6 % / 3.5 % (rho); the zero-lag product (adjoint after its step x re-wound forward
state, weight dt), even with its best scale, 31 .. 51 % at every dt: an imaging condition, no gradient.  Leaving the force's
entry q_k in the + state puts sum_k q_k . a(x_s) into the source cell's uu: 130 % there."""
import numpy as np
import pytest

from oracle.lf4 import OracleLF4
from tests import gradient_loop as gl

# name, dim, degree, cubes, diagonal, steps, T
RHO_CASES = [
    ("tri-P2", 2, 2, (4, 4), "left", 64, 0.8),
    ("tri-P3", 2, 3, (3, 3), "left", 72, 0.8),
    ("quad-DQ2", 2, 2, (4, 4), "quadrilateral", 64, 0.8),
    ("tet-P2", 3, 2, (2, 2, 2), "left", 24, 0.8),
]


def signals(dim, T, K):
    """(q [K, 1, dim], obs [K, 3, dim]): one Ricker force and smooth data, functions of time sampled at the steps - the
    same signals at every dt"""
    dt = T / K
    q = (dt * gl.ricker(dt * np.arange(K), 60.0, 0.25))[:, None, None] * np.array([1.0, 0.6, -0.8][:dim])[None, None, :]
    tk = dt * np.arange(1, K + 1)
    obs = 2.0 * np.stack([np.sin(7.0 * tk + r)[:, None] * np.array([1.0, -0.5, 0.3][:dim])[None] for r in range(3)], axis=1)
    return q, obs


def make(dim, degree, n, diagonal, T, K, seed=3):
    """the force at xs in a cell that also holds receiver 0; receiver 1 on the grid line x_0 = m h_0 nearest to 1/2 (1/2 on
    the 4- and 2-cube meshes, 2/3 on the 3-cube mesh), and no other receiver coordinate on a grid line"""
    geo = gl.Geometry(dim, degree, n, diagonal)
    mat = gl.material(geo.ncells, seed)
    xs = np.array([[0.41, 0.57, 0.33][:dim]])
    line = geo.h[0] * round(0.5 / geo.h[0])
    xr = np.array([[0.43, 0.55, 0.36][:dim], [line, 0.23, 0.61][:dim], [0.8, 0.7, 0.2][:dim]])
    on_line = np.array([[any(x == m * geo.h[a] for m in range(n[a] + 1)) for a, x in enumerate(p)] for p in xr])
    assert on_line.sum() == 1 and on_line[1, 0] and 0.0 < line < 1.0, "exactly one receiver coordinate on a grid line"
    q, obs = signals(dim, T, K)
    return dict(geo=geo, mat=mat, dt=T / K, xs=xs, q=q, xr=xr, obs=obs)


def loop(c, pairings):
    return gl.gradient_loop(c["geo"], c["mat"], c["dt"], c["xs"], c["q"], c["xr"], c["obs"], pairings)


def differences(c, cells, params):
    def J_of(m):
        return gl.misfit(gl.forward(c["geo"], m, c["dt"], c["xs"], c["q"], c["xr"]), c["obs"])
    return gl.central_differences(J_of, c["mat"], cells, params=params)


def checked_cells(c, extra):
    """the source's cell, the receivers' cells and `extra` ones that hold neither"""
    geo = c["geo"]
    cs, cr = geo.points(c["xs"])[0], geo.points(c["xr"])[0]
    held = sorted({int(x) for x in cs} | {int(x) for x in cr})
    assert int(cs[0]) == int(cr[0]), "the force sits in a cell that also holds a receiver"
    assert not set(extra) & set(held) and len(extra) >= 1
    return held + list(extra), held


def miss(est, fd):
    return float(np.abs(est - fd).max() / np.abs(fd).max())


def best_scaled(est, fd):
    return est * float(est @ fd) / float(est @ est)


def test_the_halves_are_the_oracle_s_step():
    """velocity_half then stress_half of tests/gradient_loop.py are OracleLF4.step with density_physical, bit for bit"""
    c = make(2, 2, (4, 4), "left", 0.5, 40)
    geo, (lam, mu, rho) = c["geo"], c["mat"]
    rng = np.random.default_rng(9)
    u0, s0 = rng.uniform(-1.0, 1.0, geo.zeros()[0].shape), rng.uniform(-1.0, 1.0, geo.zeros()[1].shape)
    orc = OracleLF4(geo.mesh, geo.degree)
    orc.l, orc.mu, orc.density, orc.density_physical, orc.dt = lam, mu, rho, True, -c["dt"]
    orc.u0, orc.s0 = u0.copy(), s0.copy()
    orc.step(0.0)
    u = gl.velocity_half(geo.E, u0, s0, c["mat"], -c["dt"])
    s = gl.stress_half(geo.E, u, s0, c["mat"], -c["dt"])
    assert np.array_equal(u, orc.u1) and np.array_equal(s, orc.s1)


EXTRA = {"tri-P2": [5, 12, 17, 30], "tri-P3": [2, 9, 14], "quad-DQ2": [2, 6, 14], "tet-P2": [3, 20, 44]}


@pytest.mark.parametrize("name,dim,degree,n,diagonal,K,T", RHO_CASES, ids=[c[0] for c in RHO_CASES])
def test_density_gradient_is_exact(name, dim, degree, n, diagonal, K, T):
    """-1/2 K_rho of the mid-step pairing against central differences of J, per-cell lambda, mu, rho: 1e-7 of the largest
    difference (measured: tri-P2 4.8e-11, tri-P3 3.4e-11, quad-DQ2 3.8e-10, tet-P2 5.9e-11 - the differences' own floor).  Every
    checked entry exceeds 1e-3 of the largest, and cells that hold neither the source nor a receiver are among them.  The two
    slips this must catch, on the same inputs: the adjoint velocity before its step, and the force's entry left in."""
    c = make(dim, degree, n, diagonal, T, K)
    cells, held = checked_cells(c, EXTRA[name])
    out = loop(c, ("midstep", "velocity_before", "entry_left_in"))
    fd = differences(c, cells, ("rho",))["rho"]
    assert np.isfinite(fd).all() and np.abs(fd).min() > 1e-3 * np.abs(fd).max(), fd / np.abs(fd).max()
    err = {p: miss(gl.gradient_of(dim, c["mat"], out["acc"][p])["rho"][cells], fd) for p in out["acc"]}
    print("rho %s: J %.3e, midstep %.2e, velocity before its step %.2e, entry left in %.2e of the largest difference"
          % (name, out["J"], err["midstep"], err["velocity_before"], err["entry_left_in"]))
    assert err["midstep"] <= 1e-7, err
    assert err["velocity_before"] >= 10 * max(err["midstep"], 1e-7) and err["entry_left_in"] >= 10 * max(err["midstep"], 1e-7), err


@pytest.fixture(scope="module")
def levels():
    """the 4 x 4 P2 case at dt = 1/80, 1/160, 1/320: every pairing's miss per parameter, once for the tests below"""
    out = []
    for K in (64, 128, 256):
        c = make(2, 2, (4, 4), "left", 0.8, K)
        cells, held = checked_cells(c, EXTRA["tri-P2"])
        fd = differences(c, cells, ("rho", "lambda", "mu"))
        res = loop(c, gl.PAIRINGS)
        err = {}
        for p in gl.PAIRINGS:
            g = gl.gradient_of(2, c["mat"], res["acc"][p])
            err[p] = {k: miss(best_scaled(g[k][cells], fd[k]) if p == "zero_lag" else g[k][cells], fd[k]) for k in fd}
        out.append(dict(K=K, fd=fd, err=err, cells=cells, held=held))
        print("dt = 0.8 / %d:" % K, {p: {k: "%.3e" % v for k, v in e.items()} for p, e in err.items()})
    return out


# the finest level's miss of the mid-step pairing as measured on these inputs (see the module's docstring); asserted at twice
# that, which covers moving the seed and the cells
FINEST = {"lambda": 8.04e-4, "mu": 9.79e-4}


def test_lame_gradients_are_second_order(levels):
    """lambda and mu of the mid-step pairing over the same signals at dt, dt/2, dt/4: the observed order between successive
    levels is at least 1.8 (measured 2.02, 2.01 for lambda and 2.01, 2.00 for mu), the finest miss at most twice the measured
    8.04e-4 (lambda) and 9.79e-4 (mu) of the largest difference."""
    for k in ("lambda", "mu"):
        e = [lv["err"]["midstep"][k] for lv in levels]
        orders = [float(np.log2(e[i] / e[i + 1])) for i in range(2)]
        print("%s: miss %s, orders %s" % (k, ["%.3e" % x for x in e], ["%.2f" % o for o in orders]))
        assert min(orders) >= 1.8, (k, e, orders)
        assert e[2] <= 2.0 * FINEST[k], (k, e[2])
    for lv in levels:
        assert lv["err"]["midstep"]["rho"] <= 1e-7


def test_checked_entries_are_not_vacuous(levels):
    for lv in levels:
        assert len(lv["cells"]) > len(lv["held"]), "a checked cell that holds neither the source nor a receiver"
        for k, fd in lv["fd"].items():
            assert np.abs(fd).min() > 1e-3 * np.abs(fd).max(), (k, fd / np.abs(fd).max())


def test_near_misses_miss(levels):
    """At every dt each slip misses by at least 10 x the right pairing's error: the zero-lag product with its best scale (all
    three parameters), the adjoint stress after its step (lambda, mu), the adjoint velocity before its step (rho; the right
    pairing's error there is the differences' floor, taken as 1e-7)."""
    for lv in levels:
        right = {k: max(v, 1e-7) for k, v in lv["err"]["midstep"].items()}
        err = lv["err"]
        for k in ("rho", "lambda", "mu"):
            assert err["zero_lag"][k] >= 10 * right[k], (lv["K"], "zero_lag", k, err["zero_lag"][k], right[k])
        for k in ("lambda", "mu"):
            assert err["stress_after"][k] >= 10 * right[k], (lv["K"], "stress_after", k, err["stress_after"][k], right[k])
        assert err["velocity_before"]["rho"] >= 10 * right["rho"], (lv["K"], err["velocity_before"]["rho"])
        assert err["entry_left_in"]["rho"] >= 10 * right["rho"], (lv["K"], err["entry_left_in"]["rho"])


@pytest.mark.parametrize("row", gl.ROWS, ids=[r[0] for r in gl.ROWS])
def test_the_gpu_rows_accumulators_stand_clear_of_their_bound(row):
    """tests/test_gradient_gpu.py compares the device's accumulators with this loop's to 10 tol_of() x scale (5e-5 x scale
    for f32 blocks), scale_k the sum over the calls of the largest per-cell term.  The sums cancel - the increments are
    O(dt) of the states - so on every row's inputs the final max |acc_k| must be at least 100 x that bound, or the
    comparison would pass on noise."""
    from tests.test_parity_gpu import tol_of
    name, dim, degree, n, diagonal, dtype, path = row
    ref = gl.row_reference(row)
    bound = 5e-5 if dtype == "f32" else 10 * tol_of(degree, diagonal)
    acc, scale = np.abs(ref["acc"]["midstep"]).max(axis=0), ref["scale"]["midstep"]
    print(name, "max |acc_k| / scale_k:", acc / scale, "bound", bound)
    assert np.all(scale > 0) and np.all(acc >= 100 * bound * scale), (name, acc / scale)
    case = gl.row_case(row)
    assert case["K"] == (6 if dim == 3 else 12)
    cs = case["geo"].points(case["xs"])[0]
    assert len(set(cs)) == 2 and case["xs"][1, 0] == case["geo"].h[0], "one interior source point and one on a grid line"
    if name in gl.DENSITY_ROWS:
        assert len(gl.density_cells(row)) == 4
