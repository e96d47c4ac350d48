"""The rollout test shapes and their NumPy-reference results, shared by the host tests
(tests/test_rollout_host.py) and the GPU tests (tests/test_gpu_rollout.py).  A result is computed
once per pytest session (the cart-pole regions of attraction take the oracle most of a minute each).
"""

import functools

import numpy as np

import cases
import np_rollout
import oracle
from safe_learning_amd import functions as F
from safe_learning_amd.benchmarks import build_specs

# ---- linear dynamics + saturated linear policy: bit for bit ---------------------------------------
LINEAR_STEPS = 200
LINEAR_CASES = {
    "1d": ("1d", dict(num_points=41)),
    "pendulum": ("pendulum", dict(num_points=[9, 11], dynamics="linear")),
    "cartpole": ("cartpole", dict(num_points=[3, 4, 5, 3], dynamics="linear")),
    "chain3": ("chain3", dict(num_points=[3, 4, 5], dynamics="linear")),          # cases.make_case_3d
}

# ---- Euler dynamics, first steps of every cell ---------------------------------------------------
EULER_STEPS = 8
# One Euler step is allowed 1e-12 / 1e-15 against NumPy (tests/test_hostsim.py: libm's sin / cos
# differ from NumPy's by an ulp); eight steps of a map with Lipschitz constant 1 + O(dt) get eight
# times that, rounded up.
EULER_RTOL, EULER_ATOL = 1e-11, 1e-14
EULER_CASES = {
    "pendulum": ("pendulum", dict(num_points=40, dynamics="analytic")),
    "cartpole": ("cartpole", dict(num_points=9, dynamics="analytic")),
}

# ---- regions of attraction, full horizon: saturated LQR on the Euler models ------------------------
# (name, points per axis, factor on the limits, horizon, tol)
ROA_CASES = {
    "pendulum-x1": ("pendulum", 101, 1.0, 500, 0.01),
    "pendulum-x3": ("pendulum", 101, 3.0, 500, 0.01),
    "cartpole-x1": ("cartpole", 13, 1.0, 1000, 0.1),
    "cartpole-x3": ("cartpole", 13, 3.0, 1000, 0.1),
}
ROA_END_STATE_ATOL = 1e-10      # in-ROA end states: two orders above what a 1e-14 perturbation of the
                                # start states moves them in the oracle, eight below the smallest tol


def make(name, kw):
    return cases.make_case_3d(**kw) if name == "chain3" else cases.make_case(name, **kw)


def roa_case(key):
    name, num, factor, horizon, tol = ROA_CASES[key]
    case = cases.make_case(name, num_points=num, dynamics="analytic")
    case["limits"] = [[factor * lo, factor * hi] for lo, hi in case["limits"]]
    return case, horizon, tol


def engine_grid(case):
    return F.GridWorld(case["limits"], case["num_points"])


def engine_pair(case):
    """(dynamics, policy) specs of the engine."""
    policy, dynamics, _, _ = build_specs(case)
    return dynamics, policy


def oracle_pair(case):
    policy, dynamics, _, _ = cases.oracle_specs(case)
    return dynamics, policy


def oracle_points(case):
    return oracle.GridWorld(case["limits"], case["num_points"]).all_points


@functools.lru_cache(maxsize=None)
def oracle_linear(key):
    """-> (start points, states [n, steps + 1, d], actions [n, steps, m])."""
    case = make(*LINEAR_CASES[key])
    dynamics, policy = oracle_pair(case)
    pts = oracle_points(case)
    states, actions = np_rollout.compute_trajectory(dynamics, policy, pts, LINEAR_STEPS + 1)
    return pts, states, actions


@functools.lru_cache(maxsize=None)
def oracle_euler(key):
    case = make(*EULER_CASES[key])
    dynamics, policy = oracle_pair(case)
    pts = oracle_points(case)
    states, actions = np_rollout.compute_trajectory(dynamics, policy, pts, EULER_STEPS + 1)
    return pts, states, actions


@functools.lru_cache(maxsize=None)
def oracle_roa(key):
    """-> (start points, end states, dist, roa) of the oracle, after the conditions on the INPUT:
    no cell ends with a distance in (tol / 10, 10 tol) - the mask does not hang on the last bits of
    anybody's arithmetic - every distance is finite, and both mask values occur."""
    case, horizon, tol = roa_case(key)
    dynamics, policy = oracle_pair(case)
    step = np_rollout.closed_loop(dynamics, policy)
    end = oracle_points(case)
    start = end
    for _ in range(1, horizon):
        end = step(end)
    dist = np_rollout.distances(end)
    roa = dist <= tol
    band = (dist > tol / 10) & (dist < 10 * tol)
    print("oracle ROA %s: in-ROA fraction %.3f, %d cells in the band (tol/10, 10 tol), %d non-finite"
          % (key, roa.mean(), band.sum(), (~np.isfinite(dist)).sum()))
    assert not band.any(), "%s: %d cells end within a decade of tol" % (key, band.sum())
    assert np.isfinite(dist).all()
    assert roa.any() and not roa.all()
    return start, end, dist, roa


def check_roa(key, got_roa, got_end):
    """The conditions of a ROA case on a computed mask [n] and end states [n, d]."""
    _, end, dist, roa = oracle_roa(key)
    got_roa = np.asarray(got_roa)
    assert got_roa.dtype == np.bool_ and got_roa.shape == roa.shape
    flips = int((got_roa != roa).sum())
    shift = float(np.abs(np.asarray(got_end)[roa] - end[roa]).max())
    print("ROA %s: %d mask flips of %d cells, largest in-ROA end-state difference %.3g"
          % (key, flips, roa.size, shift))
    assert flips == 0                                   # exactly the oracle's mask, nothing excluded
    np.testing.assert_allclose(np.asarray(got_end)[roa], end[roa], rtol=0, atol=ROA_END_STATE_ATOL)


# ---- interpolated policy on a coarser grid than the start points -----------------------------------
TRI_STEPS = 40
TRI_START = ([[-0.9, 0.9], [-0.9, 0.9]], [22, 18])     # no start point on a grid line of the table


def tri_case():
    case = cases.make_case("pendulum", num_points=[21, 17], dynamics="linear")
    table_points = [9, 7]
    axes = [np.linspace(lo, hi, n) for (lo, hi), n in zip(case["limits"], table_points)]
    pts = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, case["d"])
    act = np.clip(pts @ case["K"].T, *case["saturate"])
    # (a smooth bump on top of the clipped LQR law: the simplices of a cell disagree)
    act = act * (1.0 + 0.1 * np.sin(3.0 * pts[:, [0]]) * np.cos(2.0 * pts[:, [1]]))
    case["policy_table"] = {"num_points": table_points, "values": act}
    return case


def tri_start_points():
    return oracle.GridWorld(*TRI_START).all_points


def near_grid_line(otri, pts, rel=1e-9):
    """Points within ``rel`` grid spacings of a grid line of the table in some dimension.  The
    reference wraps a point into the unit cell with ``(x - offset) % unit_maxes`` and finds its
    rectangle with ``np.digitize`` on x itself (``functions.py:1116-1124``): within rounding of a
    grid line the two disagree about the side, so its interpolant jumps there (0.6 in this table,
    1e-18 below the vertex at the origin) - what it returns depends on the last bit of x, and with
    it everything a trajectory does afterwards."""
    disc = otri.discretization
    cell = (np.asarray(pts) - disc.offset) / disc.unit_maxes
    return (np.abs(cell - np.rint(cell)) < rel).any(axis=1)


@functools.lru_cache(maxsize=None)
def oracle_tri():
    """-> (start, states [n, steps + 1, d], actions, ok [n, steps]): ok[i, s] = no policy look-up
    of trajectory i up to and including step s was at an ambiguous point of the table
    (tests/exclusions.py: the reference's own answer depends on SciPy's search history there, and
    everything after it follows whichever answer it gave) or within rounding of one of its grid
    lines (``near_grid_line``)."""
    import exclusions
    case = tri_case()
    dynamics, policy = oracle_pair(case)
    otri = policy.fun if isinstance(policy, oracle.Saturation) else policy
    pts = tri_start_points()
    states, actions = np_rollout.compute_trajectory(dynamics, policy, pts, TRI_STEPS + 1)
    amb = np.stack([exclusions.ambiguous_points(otri, states[:, s, :]) | near_grid_line(otri, states[:, s, :])
                    for s in range(TRI_STEPS)], axis=1)
    ok = np.cumsum(amb, axis=1) == 0
    return pts, states, actions, ok


# ---- a NeuralNetwork policy ------------------------------------------------------------------------------
NETWORK_LAYERS, NETWORK_ACTS = [2, 1], ["tanh", None]
NETWORK_ROA = ("pendulum", 101, 1.0, 500, 0.01)


def network_parameters(case, gain=0.1):
    """Dense kernels [in, out] (no biases) of u = tanh(gain K x) / gain + 0.05 tanh(0.3 sum(x)): the
    LQR law near the origin, bent away from it."""
    d = case["d"]
    w1 = np.zeros((d, 2))
    w1[:, 0] = gain * case["K"][0]
    w1[:, 1] = 0.3
    return [w1, np.array([[1.0 / gain], [0.05]])]


def network_case():
    name, num, factor, horizon, tol = NETWORK_ROA
    case = cases.make_case(name, num_points=num, dynamics="analytic")
    case["limits"] = [[factor * lo, factor * hi] for lo, hi in case["limits"]]
    return case, horizon, tol


def oracle_network_policy(case):
    net = oracle.NeuralNetwork(NETWORK_LAYERS, NETWORK_ACTS, 1.0, False, parameters=network_parameters(case))
    return oracle.Saturation(net, *case["saturate"])


@functools.lru_cache(maxsize=None)
def oracle_network():
    """-> (start, first states [n, EULER_STEPS + 1, d], first actions, end states, dist, roa) with the
    input conditions of ``oracle_roa``."""
    case, horizon, tol = network_case()
    dynamics, _ = oracle_pair(case)
    policy = oracle_network_policy(case)
    start = oracle_points(case)
    states, actions = np_rollout.compute_trajectory(dynamics, policy, start, EULER_STEPS + 1)
    step = np_rollout.closed_loop(dynamics, policy)
    end = start
    for _ in range(1, horizon):
        end = step(end)
    dist = np_rollout.distances(end)
    roa = dist <= tol
    band = (dist > tol / 10) & (dist < 10 * tol)
    print("oracle ROA, network policy: in-ROA fraction %.3f, %d cells in the band" % (roa.mean(), band.sum()))
    assert not band.any() and np.isfinite(dist).all() and roa.any() and not roa.all()
    assert (np.abs(actions) == 1.0).any() and (np.abs(actions) < 1.0).any()
    return start, states, actions, end, dist, roa
