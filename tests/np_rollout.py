"""NumPy restatement of the reference's closed-loop simulation over the ORACLE's callables (test
infrastructure, like ``oracle/``):

* ``compute_trajectory`` - ``safe_learning/utilities.py:519-583``: one state at a time through
  ``dynamics(x, policy(x))``; ``[n, d]`` start states are simulated row by row the same way
  (every function of the oracle works row-wise, so a batch is the rows side by side).
* ``compute_roa`` - ``examples/utilities.py:654-686``: ``horizon - 1`` steps from every point of a
  grid, then ``||x - equilibrium||_2 <= tol``.

``closed_loop(dynamics, policy)`` is the notebooks' ``lambda x: dynamics(x, policy(x))``.
"""

import numpy as np


def closed_loop(dynamics, policy):
    def step(states):
        nxt = dynamics(states, policy(states))
        return nxt[0] if isinstance(nxt, tuple) else nxt
    return step


def compute_trajectory(dynamics, policy, initial_state, num_steps):
    """-> ``states [num_steps, d]``, ``actions [num_steps - 1, m]``; for ``[n, d]`` start states with
    n > 1 ``[n, num_steps, d]`` / ``[n, num_steps - 1, m]``."""
    initial_state = np.atleast_2d(np.asarray(initial_state, dtype=np.float64))
    n, d = initial_state.shape
    states = np.empty((n, num_steps, d))
    actions = None
    states[:, 0, :] = initial_state
    for i in range(num_steps - 1):
        u = np.asarray(policy(states[:, i, :]))
        if actions is None:
            actions = np.empty((n, num_steps - 1, u.shape[1]))
        nxt = dynamics(states[:, i, :], u)
        states[:, i + 1, :] = nxt[0] if isinstance(nxt, tuple) else nxt
        actions[:, i, :] = u
    if actions is None:
        actions = np.empty((n, 0, int(policy.output_dim)))
    return (states[0], actions[0]) if n == 1 else (states, actions)


def distances(end_states, equilibrium=None):
    end_states = np.asarray(end_states)
    if equilibrium is None:
        equilibrium = np.zeros((1, end_states.shape[1]))
    return np.linalg.norm(end_states - equilibrium, ord=2, axis=1, keepdims=True).ravel()


def compute_roa(grid, closed_loop_dynamics, horizon=100, tol=1e-3, equilibrium=None, no_traj=True):
    if isinstance(grid, np.ndarray):
        all_points = grid
    else:
        all_points = grid.all_points
    nindex, ndim = all_points.shape
    if no_traj:
        end_states = all_points
        for _ in range(1, horizon):
            end_states = closed_loop_dynamics(end_states)
    else:
        trajectories = np.empty((nindex, ndim, horizon))
        trajectories[:, :, 0] = all_points
        for t in range(1, horizon):
            trajectories[:, :, t] = closed_loop_dynamics(trajectories[:, :, t - 1])
        end_states = trajectories[:, :, -1]
    roa = distances(end_states, equilibrium) <= tol
    return roa if no_traj else (roa, trajectories)
