"""The reward_rollout test shapes and their NumPy-reference results (tests/np_reward_rollout.py over
the oracle), shared by the host tests (tests/test_reward_rollout_host.py) and the GPU tests
(tests/test_gpu_reward_rollout.py).  Built on tests/rollout_cases.py; a result is computed once per
pytest session.  Every condition here is asserted on the ORACLE's numbers alone and printed.

Condition on every converging case: ``min_t |max_t / tol - 1| >= 1e-6`` - the stopping step then
does not hang on the last bits of anybody's arithmetic.
"""

import functools

import numpy as np

import cases
import np_reward_rollout as NR
import rollout_cases as RC

STOP_MARGIN = 1e-6

# ---- linear dynamics + saturated linear policy: bit for bit -----------------------------------------
# key of RC.LINEAR_CASES -> (Q, R, discount, horizon, tol, steps the oracle sums, converged)
LINEAR = {
    "1d": (0.5 * np.eye(1), 0.3, 0.98, 400, 1e-2, 18, True),
    "chain3": (0.5 * np.eye(3), 0.3, 0.98, 400, 1e-2, 77, True),
    "pendulum": (np.diag([1.0, 2.0]), 1.2, 0.9, 400, 1e-3, 180, True),
    "cartpole": (0.5 * np.eye(4), 0.3, 0.98, 50, 1e-2, 50, False),        # the full-horizon branch
}

# ---- Euler models, saturated LQR ----------------------------------------------------------------------
# name -> (make_case keywords, Q, R, discount, horizon, tol, steps the oracle sums)
EULER = {
    "pendulum": (dict(num_points=41, dynamics="analytic"), np.diag([1.0, 2.0]), 1.2, 0.98, 1000, 1e-2, 393),
    "cartpole": (dict(num_points=7, dynamics="analytic"), 0.1 * np.eye(4), 0.1, 0.98, 1000, 1e-2, 679),
}
PERTURBATION = 1e-14            # relative, on the oracle's start states
TOLERANCE_FACTOR = 100.0        # the device's sin / cos differ from NumPy's by an ulp per evaluation,
                                # over ten sub-steps per step: two orders above one rounding of the input

# ---- more than one pass of the grid-stride loop --------------------------------------------------------
LARGE_1D_POINTS = 1050001       # > 2 x 2048 x 256 trajectories: two per thread, more than one pass
LARGE_PENDULUM = ([751, 701], 12)          # > 2048 x 256 cells; horizon 12: no convergence

# ---- interpolated policy / network policy -----------------------------------------------------------------
TRI = (np.diag([1.0, 2.0]), 1.2, 0.9, 40, 0.0)
NETWORK = (np.diag([1.0, 2.0]), 1.2, 0.98, 200, 1e-2)


def stop_margin(maxima, tol):
    """min_t |max_t / tol - 1| of the oracle's per-step maxima."""
    return float(np.min(np.abs(np.asarray(maxima) / tol - 1.0)))


def _check_margin(label, maxima, tol, steps, converged):
    margin = stop_margin(maxima, tol) if tol > 0 else np.inf
    print("oracle reward_rollout %s: %d steps, converged %s, closest max/tol - 1 = %.3g"
          % (label, steps, converged, margin))
    assert margin >= STOP_MARGIN, "%s: a per-step maximum lies within %.1g of tol" % (label, STOP_MARGIN)


def linear_case(key):
    """-> (case, reward matrix on [x, u], discount, horizon, tol)."""
    q, r, discount, horizon, tol, _, _ = LINEAR[key]
    return RC.make(*RC.LINEAR_CASES[key]), NR.quadratic_reward(q, r), discount, horizon, tol


@functools.lru_cache(maxsize=None)
def oracle_linear(key):
    """-> (start points, rollout, steps, converged, per-step maxima)."""
    case, matrix, discount, horizon, tol = linear_case(key)
    dynamics, policy = RC.oracle_pair(case)
    pts = RC.oracle_points(case)
    rollout, steps, converged, maxima = NR.reward_rollout(pts, dynamics, policy, matrix, discount, horizon, tol)
    _check_margin("linear " + key, maxima, tol, steps, converged)
    assert (steps, converged) == LINEAR[key][5:]
    assert np.isfinite(rollout).all()
    return pts, rollout, steps, converged, maxima


def euler_case(key):
    kw, q, r, discount, horizon, tol, _ = EULER[key]
    return cases.make_case(key, **kw), NR.quadratic_reward(q, r), discount, horizon, tol


@functools.lru_cache(maxsize=None)
def oracle_euler(key):
    """-> (start points, rollout, steps, converged, maxima, rtol): rtol = TOLERANCE_FACTOR x the
    largest relative change ``|delta| / max(|sum|, 1)`` of the oracle's own sums under a relative
    perturbation of its start states by PERTURBATION (three seeds) - from the oracle alone."""
    case, matrix, discount, horizon, tol = euler_case(key)
    dynamics, policy = RC.oracle_pair(case)
    pts = RC.oracle_points(case)
    rollout, steps, converged, maxima = NR.reward_rollout(pts, dynamics, policy, matrix, discount, horizon, tol)
    _check_margin("Euler " + key, maxima, tol, steps, converged)
    assert converged and steps == EULER[key][6]
    sensitivity = sensitivity_of(pts, dynamics, policy, matrix, discount, horizon, tol, rollout, steps)
    rtol = TOLERANCE_FACTOR * sensitivity
    print("oracle reward_rollout Euler %s: minimum %.16g, sensitivity to a %.0e perturbation %.3g, tolerance %.3g"
          % (key, rollout.min(), PERTURBATION, sensitivity, rtol))
    return pts, rollout, steps, converged, maxima, rtol


def sensitivity_of(pts, dynamics, policy, matrix, discount, horizon, tol, rollout, steps):
    worst = 0.0
    for seed in range(3):
        rng = np.random.default_rng(seed)
        moved = pts * (1.0 + PERTURBATION * rng.uniform(-1.0, 1.0, size=pts.shape))
        other, other_steps, _, _ = NR.reward_rollout(moved, dynamics, policy, matrix, discount, horizon, tol)
        assert other_steps == steps
        worst = max(worst, float(np.max(np.abs(other - rollout) / np.maximum(np.abs(rollout), 1.0))))
    return worst


def assert_sums_close(got, want, rtol):
    """|got - want| <= rtol max(|want|, 1), the figure printed."""
    err = float(np.max(np.abs(np.asarray(got) - want) / np.maximum(np.abs(want), 1.0)))
    print("largest |difference| / max(|sum|, 1) = %.3g (allowed %.3g)" % (err, rtol))
    assert err <= rtol


# ---- more than one pass ---------------------------------------------------------------------------------
def large_1d_case():
    _, matrix, discount, horizon, tol = linear_case("1d")
    return RC.make("1d", dict(num_points=LARGE_1D_POINTS)), matrix, discount, horizon, tol


@functools.lru_cache(maxsize=None)
def oracle_large_1d():
    case, matrix, discount, horizon, tol = large_1d_case()
    dynamics, policy = RC.oracle_pair(case)
    pts = RC.oracle_points(case)
    rollout, steps, converged, maxima = NR.reward_rollout(pts, dynamics, policy, matrix, discount, horizon, tol)
    _check_margin("linear 1d, %d points" % len(pts), maxima, tol, steps, converged)
    assert converged and steps == LINEAR["1d"][5]
    return pts, rollout, steps, converged


def large_pendulum_case():
    num, horizon = LARGE_PENDULUM
    _, q, r, discount, _, tol, _ = EULER["pendulum"]
    return (cases.make_case("pendulum", num_points=num, dynamics="analytic"), NR.quadratic_reward(q, r), discount,
            horizon, tol)


@functools.lru_cache(maxsize=None)
def oracle_large_pendulum():
    case, matrix, discount, horizon, tol = large_pendulum_case()
    dynamics, policy = RC.oracle_pair(case)
    pts = RC.oracle_points(case)
    rollout, steps, converged, maxima = NR.reward_rollout(pts, dynamics, policy, matrix, discount, horizon, tol)
    _check_margin("Euler pendulum %d cells" % len(pts), maxima, tol, steps, converged)
    assert not converged and steps == horizon
    return pts, rollout, steps, converged


# ---- interpolated policy --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_tri():
    """-> (start, rollout, steps, converged, ok [n]): ok = every policy look-up of the trajectory's
    summed terms was unambiguous (RC.oracle_tri)."""
    q, r, discount, horizon, tol = TRI
    assert horizon == RC.TRI_STEPS
    case = RC.tri_case()
    dynamics, policy = RC.oracle_pair(case)
    pts, _, _, ok = RC.oracle_tri()
    rollout, steps, converged, _ = NR.reward_rollout(pts, dynamics, policy, NR.quadratic_reward(q, r), discount,
                                                     horizon, tol)
    assert steps == horizon and not converged                          # tol 0: max < 0 never holds
    ok = ok[:, horizon - 1]
    print("oracle reward_rollout, table policy: %d of %d trajectories excluded" % ((~ok).sum(), ok.size))
    assert (~ok).mean() < 0.05
    return pts, rollout, steps, converged, ok


# ---- network policy ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_network():
    q, r, discount, horizon, tol = NETWORK
    case, _, _ = RC.network_case()
    dynamics, _ = RC.oracle_pair(case)
    policy = RC.oracle_network_policy(case)
    matrix = NR.quadratic_reward(q, r)
    pts = RC.oracle_points(case)
    rollout, steps, converged, maxima = NR.reward_rollout(pts, dynamics, policy, matrix, discount, horizon, tol)
    _check_margin("network policy", maxima, tol, steps, converged)
    sensitivity = sensitivity_of(pts, dynamics, policy, matrix, discount, horizon, tol, rollout, steps)
    rtol = TOLERANCE_FACTOR * sensitivity
    print("oracle reward_rollout network policy: sensitivity %.3g, tolerance %.3g" % (sensitivity, rtol))
    return pts, rollout, steps, converged, rtol
