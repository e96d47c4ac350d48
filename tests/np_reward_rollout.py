"""NumPy restatement of the reference's ``reward_rollout`` (``examples/utilities.py:522-545``) over
the ORACLE's callables (test infrastructure, like ``tests/np_rollout.py``)::

    rollout = 0
    for t in range(horizon):
        temp = (discount ** t) * reward(x, policy(x));  rollout += temp
        if np.max(np.abs(temp)) < tol: converged, stop         (this step's temp IS included)
        x = dynamics(x, policy(x))

The reward is ``oracle.QuadraticFunction`` on ``[x, policy(x)]`` - the notebooks'
``QuadraticFunction(block_diag(-Q, -R))`` called as ``reward(states, policy(states))``.
"""

import numpy as np

import np_rollout
import oracle


def quadratic_reward(q, r):
    """The notebooks' reward ``-(x Q x^T + u R u^T)`` as a matrix on ``[x, u]``."""
    q, r = np.atleast_2d(np.asarray(q, dtype=np.float64)), np.atleast_2d(np.asarray(r, dtype=np.float64))
    p = q.shape[0] + r.shape[0]
    matrix = np.zeros((p, p))
    matrix[:q.shape[0], :q.shape[0]] = -q
    matrix[q.shape[0]:, q.shape[0]:] = -r
    return matrix


def reward_on_states(reward_matrix, policy):
    """``x -> reward([x, policy(x)])`` as ``[n]`` values."""
    reward = oracle.QuadraticFunction(reward_matrix)
    return lambda states: np.asarray(reward(states, policy(states))).ravel()


def reward_rollout_callables(points, closed_loop_dynamics, reward_function, discount, horizon, tol):
    """The loop on any callables -> ``(rollout [n], steps, converged, per-step maxima [steps])``."""
    states = np.asarray(points, dtype=np.float64)
    rollout = np.zeros(len(states))
    maxima = []
    converged = False
    for t in range(horizon):
        temp = (discount ** t) * np.asarray(reward_function(states)).ravel()
        rollout += temp
        maxima.append(np.max(np.abs(temp)))
        if maxima[-1] < tol:
            converged = True
            break
        states = closed_loop_dynamics(states)
    return rollout, len(maxima), converged, np.asarray(maxima)


def reward_rollout(points, dynamics, policy, reward_matrix, discount, horizon, tol):
    """The loop over the oracle's ``dynamics``, ``policy`` and a quadratic reward on ``[x, u]``."""
    return reward_rollout_callables(points, np_rollout.closed_loop(dynamics, policy),
                                    reward_on_states(reward_matrix, policy), discount, horizon, tol)
