"""The polynomial systems of the polynomial-dynamics tests (host shim, NumPy truth, GPU kernels), with the
conditions on the INPUTS asserted here so that a change of a case cannot hide a failure.  Shared, not a
test module.  The NumPy truth of every case is ``np_polynomial.NumpyPolynomial(system(key))``.

* vdp / vdp-plain: ``VanDerPol(1, dt=0.1)`` with ``normalization=[3, 3]`` and without;
* map1: d = 1, the discrete map ``x+ = 0.5 x + 0.4 x^3`` (``inner_euler_steps=0``);
* duffing-u: d = 2, m = 1, a forced Duffing oscillator with ``x0 u`` and ``u^2`` terms, normalised;
* chain3: d = 3, m = 2, nine terms with products of two states and ``u0 u1``, normalised;
* full: d = 4, m = 1, exactly ``POLY_MAX_TERMS`` seeded random terms, each of total degree
  ``POLY_MAX_DEGREE``, coefficients in +-0.2, row 2 without a term.
"""

import functools

import numpy as np

import np_polynomial
import np_rollout
from safe_learning_amd import _hip
from safe_learning_amd import functions as F

KEYS = ("vdp", "vdp-plain", "map1", "duffing-u", "chain3", "full")
POINT_COUNTS = (1, 63, 65, 1681)

VDP_NUM_POINTS, VDP_HORIZON, VDP_TOL = 41, 300, 0.01
MAP1_POINTS, MAP1_HORIZON, MAP1_TOL = 65, 200, 1e-3


def _full_terms():
    rng = np.random.default_rng(64)
    d, p = 4, 5
    rows = [0, 1, 3]
    terms = [[] for _ in range(d)]
    for k in range(_hip.POLY_MAX_TERMS):
        exponents = np.bincount(rng.integers(0, p, size=_hip.POLY_MAX_DEGREE), minlength=p)
        terms[rows[k % 3]].append((float(rng.uniform(-0.2, 0.2)), tuple(int(e) for e in exponents)))
    return terms


@functools.lru_cache(maxsize=None)
def system(key):
    """The engine-side spec of a case."""
    if key == "vdp":
        return F.VanDerPol(1, dt=0.1, normalization=[3, 3])
    if key == "vdp-plain":
        return F.VanDerPol(1, dt=0.1)
    if key == "map1":
        return F.PolynomialSystem([[(0.5, (1, 0)), (0.4, (3, 0))]], 1, 1, inner_euler_steps=0)
    if key == "duffing-u":
        return duffing(-0.5)
    if key == "chain3":
        terms = [[(1.0, (0, 1, 0, 0, 0)), (-0.5, (1, 0, 0, 0, 0)), (0.3, (0, 1, 1, 0, 0))],
                 [(-1.0, (1, 0, 0, 0, 0)), (-0.4, (0, 1, 0, 0, 0)), (1.0, (0, 0, 0, 1, 0)), (0.2, (1, 0, 1, 0, 0))],
                 [(-0.6, (0, 0, 1, 0, 0)), (0.5, (0, 0, 0, 0, 1)), (0.25, (0, 0, 0, 1, 1)), (-0.1, (1, 1, 0, 0, 0))]]
        return F.PolynomialSystem(terms, 3, 2, dt=0.05, normalization=[[1.5, 2.0, 1.0], [2.0, 0.5]])
    if key == "full":
        return F.PolynomialSystem(_full_terms(), 4, 1, dt=0.05, normalization=[[1.2, 0.8, 1.5, 1.0], [2.0]])
    raise KeyError(key)


def duffing(cubic):
    """x0' = x1, x1' = -x0 + cubic x0^3 - 0.3 x1 + u + 0.25 x0 u - 0.1 u^2 (duffing-u: cubic = -0.5)."""
    terms = [[(1.0, (0, 1, 0))],
             [(-1.0, (1, 0, 0)), (cubic, (3, 0, 0)), (-0.3, (0, 1, 0)), (1.0, (0, 0, 1)), (0.25, (1, 0, 1)),
              (-0.1, (0, 0, 2))]]
    return F.PolynomialSystem(terms, 2, 1, dt=0.05, normalization=[[2, 2], [1.5]])


@functools.lru_cache(maxsize=None)
def truth(key):
    return np_polynomial.NumpyPolynomial(system(key))


def check_systems():
    """Input-side conditions on the systems themselves."""
    s = system("chain3")
    flat = [e for row in s.terms for _, e in row]
    assert (s.state_dim, s.action_dim) == (3, 2) and len(flat) >= 7
    assert any(sum(e[:3]) == 2 and max(e[:3]) == 1 and sum(e[3:]) == 0 for e in flat)      # x_i x_j
    assert any(e[3] == 1 and e[4] == 1 for e in flat)                                       # u0 u1
    s = system("full")
    flat = [(c, e) for row in s.terms for c, e in row]
    assert len(flat) == _hip.POLY_MAX_TERMS and all(sum(e) == _hip.POLY_MAX_DEGREE for _, e in flat)
    assert all(abs(c) <= 0.2 for c, _ in flat) and s.terms[2] == [] and all(s.terms[i] for i in (0, 1, 3))
    assert any(e[4] > 0 for _, e in flat)                                                   # the action is read
    s = system("duffing-u")
    flat = [e for row in s.terms for _, e in row]
    assert (1, 0, 1) in flat and (0, 0, 2) in flat and (3, 0, 0) in flat
    assert system("map1").inner_euler_steps == 0 and system("vdp").inner_euler_steps == 10
    assert system("vdp").terms == [[(-1.0, (0, 1, 0))], [(1.0, (1, 0, 0)), (1.0, (2, 1, 0)), (-1.0, (0, 1, 0))]]


def points(key, n, seed=7):
    """``n`` seeded (states, actions) in [-1, 1] (normalised units), with non-finite and signed-zero rows
    from 8 points on: they are ordinary IEEE values and must come through."""
    s = system(key)
    rng = np.random.default_rng(seed + n)
    states = rng.uniform(-1.0, 1.0, size=(n, s.state_dim))
    actions = rng.uniform(-1.0, 1.0, size=(n, s.action_dim))
    if n >= 8:
        states[3, 0] = np.nan
        states[4, -1] = np.inf
        states[5, 0] = -np.inf
        states[6, :] = -0.0
        actions[7, 0] = np.nan
        states[2, :] = 1e200                        # overflows in the powers
    return states, actions


def same_bits(a, b):
    """Equal as bit patterns, every NaN counted as one value (NaN positions equal)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(nan_a, nan_b) and np.array_equal(a.view(np.uint64)[~nan_a], b.view(np.uint64)[~nan_b]))


def assert_same_bits(got, want, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not same_bits(got, want):
        with np.errstate(all="ignore"):
            bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
            bad |= np.signbit(got) != np.signbit(want)
        raise AssertionError("%s: %d of %d entries differ in their bits, first at %s: %r != %r"
                             % (what, bad.sum(), bad.size, np.argwhere(bad)[0], got[bad][0], want[bad][0]))


# ---- closed loops ----------------------------------------------------------------------------------------
POLICIES = {
    "vdp": (np.zeros((1, 2)), None),
    "vdp-plain": (np.zeros((1, 2)), None),
    "map1": (np.zeros((1, 1)), None),
    "duffing-u": (np.array([[-0.8, -0.6]]), (-1.0, 1.0)),
    "chain3": (np.array([[-0.5, -0.7, 0.1], [0.2, 0.1, -0.9]]), (-1.0, 1.0)),
    "full": (np.array([[-0.4, 0.3, -0.2, 0.5]]), (-1.0, 1.0)),
}


def engine_policy(key):
    K, limits = POLICIES[key]
    policy = F.LinearSystem((K,))
    return policy if limits is None else F.Saturation(policy, *limits)


def oracle_policy(key):
    import oracle
    K, limits = POLICIES[key]
    policy = oracle.LinearSystem((K,))
    return policy if limits is None else oracle.Saturation(policy, *limits)


@functools.lru_cache(maxsize=None)
def vdp_roa():
    """The NumPy truth of the vdp region of attraction -> (mask, trajectories [n, 2, horizon]); the
    conditions the comparison rests on are asserted."""
    import oracle
    grid = oracle.GridWorld([[-1, 1]] * 2, VDP_NUM_POINTS)
    step = np_rollout.closed_loop(truth("vdp"), oracle_policy("vdp"))
    with np.errstate(all="ignore"):
        roa, traj = np_rollout.compute_roa(grid, step, VDP_HORIZON, VDP_TOL, no_traj=False)
        end = traj[:, :, -1]
        dist = np_rollout.distances(end)
    finite = np.isfinite(end).all(axis=1)
    band = (dist > VDP_TOL / 10) & (dist < 10 * VDP_TOL)
    print("vdp ROA: %d of %d inside, %d non-finite, %d within a decade of tol, largest inside distance %.3g"
          % (roa.sum(), roa.size, (~finite).sum(), band.sum(), dist[roa].max()))
    assert roa.size == 1681 and roa.sum() == 607 and (~finite).sum() == 1074 and not band.any()
    assert np.array_equal(roa, finite) and dist[roa].max() < 4e-6
    roa.setflags(write=False)
    traj.setflags(write=False)
    return roa, traj


@functools.lru_cache(maxsize=None)
def map1_roa():
    """-> (start points [65, 1], mask): 47 inside, 18 non-finite."""
    pts = np.linspace(-1.5, 1.5, MAP1_POINTS)[:, None]
    step = np_rollout.closed_loop(truth("map1"), oracle_policy("map1"))
    with np.errstate(all="ignore"):
        roa, traj = np_rollout.compute_roa(pts, step, MAP1_HORIZON, MAP1_TOL, no_traj=False)
        end = traj[:, :, -1]
        dist = np_rollout.distances(end)
    band = (dist > MAP1_TOL / 10) & (dist < 10 * MAP1_TOL)
    print("map1 ROA: %d of %d inside, %d non-finite, %d within a decade of tol"
          % (roa.sum(), roa.size, (~np.isfinite(end[:, 0])).sum(), band.sum()))
    assert roa.sum() == 47 and (~np.isfinite(end[:, 0])).sum() == 18 and not band.any()
    assert np.abs(pts[roa]).max() == 1.078125 and 1.078125 < np.sqrt(1.25)
    assert np.array_equal(roa, np.abs(pts[:, 0]) <= 1.078125)
    roa.setflags(write=False)
    return pts, roa


def start_states(key, n=65, seed=11):
    s = system(key)
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=(n, s.state_dim))


@functools.lru_cache(maxsize=None)
def trajectory_truth(key, steps=8):
    """``steps`` closed-loop steps from the 65 start states -> (states [n, steps + 1, d], actions [n, steps, m])."""
    states, actions = np_rollout.compute_trajectory(truth(key), oracle_policy(key), start_states(key), steps + 1)
    assert np.isfinite(states).all() and np.abs(states).max() < 10.0
    assert np.ptp(actions) > 0.5                                    # a policy that does something
    states.setflags(write=False)
    actions.setflags(write=False)
    return states, actions


# ---- Lyapunov verification -------------------------------------------------------------------------------
LYAPUNOV = {
    # key -> (system, grid limits, points per axis, radius of the initial set)
    "vdp": ("vdp", [[-1, 1]] * 2, [51, 51], 0.1),
    "vdp-pow2": ("vdp", [[-1, 1]] * 2, [64, 32], 0.1),           # the power-of-two cell decode of the sweep
    "chain3": ("chain3", [[-6, 6]] * 3, [9, 10, 11], 1.0),       # m = 2: the kernel that reads its dimensions
}
LYAPUNOV_LF, LYAPUNOV_LV = 0.5, 0.8                              # scalars; with tau = 0 the threshold is 0


def lyapunov_matrix(key):
    """P of V = x^T P x: the discrete Lyapunov equation of the closed loop's linearisation."""
    import scipy.linalg
    name = LYAPUNOV[key][0]
    lin = system(name).linearize()
    if name.startswith("vdp"):
        closed = lin
    else:
        closed = lin[0] + lin[1].dot(POLICIES[name][0])
    assert np.abs(np.linalg.eigvals(closed)).max() < 1.0
    return scipy.linalg.solve_discrete_lyapunov(closed.T, np.eye(len(closed)))


@functools.lru_cache(maxsize=None)
def lyapunov_truth(key):
    """The oracle's ``Lyapunov`` over the NumPy polynomial after ``update_safe_set`` -> (oracle object,
    initial set); the conditions the mask comparison rests on are asserted."""
    import oracle
    name, limits, num_points, radius = LYAPUNOV[key]
    grid = oracle.GridWorld(limits, num_points)
    initial = np.linalg.norm(grid.all_points, axis=1) <= radius
    value = oracle.QuadraticFunction(lyapunov_matrix(key))
    lyap = oracle.Lyapunov(grid, value, truth(name), LYAPUNOV_LF, LYAPUNOV_LV, 0.0, oracle_policy(name),
                           initial_set=initial.copy())
    lyap.update_safe_set()
    x = grid.all_points
    nxt = truth(name)(x, oracle_policy(name)(x))
    change = np.asarray(value(nxt)).ravel() - np.asarray(value(x)).ravel()
    off = ~initial
    margin, relative = np.abs(change[off]).min(), (np.abs(change[off]) / np.asarray(value(x)).ravel()[off]).min()
    print("Lyapunov %s: %d initial cells, %d of %d safe, smallest |V(f(x)) - V(x)| off the initial set %.3g "
          "(relative %.3g), c_max %.6g" % (key, initial.sum(), lyap.safe_set.sum(), grid.nindex, margin, relative,
                                           lyap.c_max))
    assert np.isfinite(nxt).all() and relative > 1e-6                 # no cell near the decision
    assert initial.sum() < lyap.safe_set.sum() < grid.nindex
    if key == "vdp":
        assert (initial.sum(), lyap.safe_set.sum(), grid.nindex) == (21, 471, 2601)
        assert 1.3e-3 < margin < 1.5e-3 and 1.6e-4 < relative < 1.8e-4
    return lyap, initial
