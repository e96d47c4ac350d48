"""Helpers kept from the reference's utilities (``safe_learning/utilities.py``) and closed-loop
simulation on the GPU: ``compute_trajectory`` (``utilities.py:519-583``) and the ``compute_roa``
(``examples/utilities.py:654-686``) and ``reward_rollout`` (``examples/utilities.py:522-545``) of the
notebooks."""

import numpy as np
import scipy.linalg

__all__ = ['dlqr', 'batchify', 'compute_trajectory', 'compute_roa', 'reward_rollout']


def dlqr(a, b, q, r):
    """Discrete-time LQR gain and cost-to-go, ``u = -k x`` (``utilities.py:327-357``)."""
    a, b, q, r = (np.atleast_2d(v) for v in (a, b, q, r))
    p = scipy.linalg.solve_discrete_are(a, b, q, r)
    k = np.linalg.solve(b.T.dot(p).dot(b) + r, b.T.dot(p).dot(a))
    return k, p


def batchify(arrays, batch_size):
    """Yield ``(start, [views])`` over consecutive batches (``utilities.py:224-249``)."""
    if not isinstance(arrays, (list, tuple)):
        arrays = (arrays,)
    start = 0
    while arrays[0][start:start + batch_size].size:
        yield start, [a[start:start + batch_size] for a in arrays]
        start += batch_size


# ---- closed-loop rollouts (csrc/sl_rollout.hip) ---------------------------------------------------

def _engine(d):
    """(context, model builder) of the rollouts: the point-evaluation context, which keeps tables
    and network parameters between calls (``_evaluate._builder``)."""
    from . import _evaluate
    return _evaluate._builder(d)


def _check_single_process():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError('closed-loop rollouts run on one GPU; under torch.distributed call them '
                                  'on one rank (the C entry point sl_rollout takes a range [lo, hi) for '
                                  'callers that shard by hand)')


def _check_pair(dynamics, policy):
    """The (dynamics, policy) specs the fused kernel takes."""
    from .functions import (CartPole, ConstantFunction, GPMeanFunction, InvertedPendulum, LinearSystem,
                            NeuralNetwork, PolynomialSystem, Saturation, Triangulation, UncertainFunction)
    if isinstance(dynamics, UncertainFunction):
        raise ValueError('the fused rollout needs deterministic dynamics; %s returns (mean, error): pass '
                         'a callable instead of the pair, e.g. `lambda x: dynamics(x, policy(x))[0]`'
                         % type(dynamics).__name__)
    if not isinstance(dynamics, (LinearSystem, InvertedPendulum, CartPole, PolynomialSystem, GPMeanFunction)):
        raise TypeError('unsupported dynamics spec %r: use LinearSystem, InvertedPendulum, CartPole, '
                        'PolynomialSystem, VanDerPol, the to_mean_function() of a GP model, or pass a callable '
                        'on states' % (dynamics,))
    inner = policy.fun if isinstance(policy, Saturation) else policy
    if not isinstance(inner, (LinearSystem, ConstantFunction, Triangulation, NeuralNetwork)):
        raise TypeError('unsupported policy spec %r: use LinearSystem, ConstantFunction, a Saturation of '
                        'either, a Triangulation or a NeuralNetwork, or pass a callable on states'
                        % (policy,))


def _fused(ctx, dynamics, reward=False):
    """The context's rollout (``reward``: reward rollout) for the dynamics spec: the kernels of
    ``csrc/sl_gp_rollout.hip`` for a ``GPMeanFunction``, those of ``csrc/sl_rollout.hip`` otherwise."""
    from .functions import GPMeanFunction
    name = 'reward_rollout' if reward else 'rollout'
    return getattr(ctx, name + '_mean' if isinstance(dynamics, GPMeanFunction) else name)


def _start_points(ctx, grid):
    """-> (GridWorld or None, device start points or None, n, d): a GridWorld starts the kernel at
    its cells, anything else is an explicit ``[n, d]`` point list."""
    from . import _evaluate
    from .functions import GridWorld
    if isinstance(grid, GridWorld):
        return grid, None, int(grid.nindex), int(grid.ndim)
    import torch
    if not isinstance(grid, torch.Tensor):
        grid = np.asarray(grid, dtype=np.float64)
    if grid.ndim != 2:
        raise ValueError('start states must be an [n, d] array, got shape %s' % (tuple(grid.shape),))
    points = _evaluate._to_device(ctx, grid)
    return None, points, int(points.shape[0]), int(points.shape[1])


def _rollout(dynamics, policy, grid, steps, trajectory=False, actions=False, steps_per_launch=0):
    """``steps`` closed-loop steps from every cell of a GridWorld or every row of ``[n, d]`` start
    states -> device tensors ``(end states [n, d], states [steps + 1, n, d] or None, actions
    [steps, n, m] or None)``; the state buffer is step-major, row 0 the start states."""
    import copy
    import torch
    from . import _evaluate
    from .functions import GridWorld, QuadraticFunction
    _check_pair(dynamics, policy)
    _check_single_process()
    steps = int(steps)
    if steps < 0:
        raise ValueError('the number of steps must not be negative')
    d = int(grid.ndim) if isinstance(grid, GridWorld) else int(grid.shape[-1])
    ctx, builder = _engine(d)
    world, start, n, d = _start_points(ctx, grid)
    if world is not None:
        builder.grid = copy.copy(world)
    desc = builder.upload(policy, dynamics, QuadraticFunction(np.eye(d)))
    m = int(desc.policy.m)
    dev = ctx.torch_device
    end = torch.empty((n, d), dtype=torch.float64, device=dev)
    states = acts = None
    rollout = _fused(ctx, dynamics)
    if trajectory:
        states = torch.empty((steps + 1, n, d), dtype=torch.float64, device=dev)
        rollout(0, n, start, 0, states[0])                         # row 0: the start states
        start = states[0]
    if actions:
        acts = torch.empty((steps, n, m), dtype=torch.float64, device=dev)
    rollout(0, n, start, steps, end, states[1:] if trajectory and steps else None,
            acts if actions and steps else None, steps_per_launch)
    return end, states, acts


def _membership(ctx, end, equilibrium, tol):
    """``||end - equilibrium||_2 <= tol`` per row as a device bool tensor (``sl_rollout_mask``)."""
    import torch
    n, d = end.shape
    dev = ctx.torch_device
    bits = torch.zeros(((n + 63) // 64,), dtype=torch.int64, device=dev)
    count = torch.zeros((1,), dtype=torch.int64, device=dev)
    ctx.rollout_mask(n, d, end, equilibrium, tol, bits, count)
    as_bytes = torch.empty((8 * ((n + 7) // 8),), dtype=torch.uint8, device=dev)
    ctx.bits_to_bytes(n, bits, as_bytes)
    return as_bytes[:n].to(torch.bool)


def compute_trajectory(dynamics, policy, initial_state, num_steps, steps_per_launch=0):
    """Simulate ``x <- dynamics(x, policy(x))`` from ``initial_state`` (``utilities.py:519-583``).

    Returns ``states [num_steps, d]`` (row 0 the initial state) and ``actions [num_steps - 1, m]``;
    for ``[n, d]`` initial states with n > 1 ``[n, num_steps, d]`` and ``[n, num_steps - 1, m]``,
    every row simulated on its own.  ``dynamics`` and ``policy`` are specs (``LinearSystem``,
    ``InvertedPendulum``, ``CartPole``, the ``to_mean_function()`` of a GP model; ``LinearSystem``,
    ``ConstantFunction``, ``Saturation``, ``Triangulation``, ``NeuralNetwork``): the whole simulation is one kernel per chunk of steps
    (``steps_per_launch``, 0 = chosen by the library; the result does not depend on it) with the
    state in registers.  A device tensor as ``initial_state`` keeps the results on the device."""
    import torch
    num_steps = int(num_steps)
    if num_steps < 1:
        raise ValueError('num_steps counts the initial state: it must be at least 1')
    keep = isinstance(initial_state, torch.Tensor)
    if not keep:
        initial_state = np.atleast_2d(np.asarray(initial_state, dtype=np.float64))
    elif initial_state.dim() == 1:
        initial_state = initial_state.reshape(1, -1)
    _, states, acts = _rollout(dynamics, policy, initial_state, num_steps - 1, trajectory=True,
                               actions=True, steps_per_launch=steps_per_launch)
    states, acts = states.permute(1, 0, 2), acts.permute(1, 0, 2)
    if states.shape[0] == 1:
        states, acts = states[0], acts[0]
    return (states, acts) if keep else (states.cpu().numpy(), acts.cpu().numpy())


def compute_roa(grid, closed_loop_dynamics, horizon=100, tol=1e-3, equilibrium=None, no_traj=True,
                steps_per_launch=0):
    """The states of ``grid`` that end within ``tol`` of ``equilibrium`` after ``horizon - 1`` steps
    of the closed loop (``examples/utilities.py:654-686``).

    ``grid``: a ``GridWorld`` (all its points) or an ``[n, d]`` array of start states.
    ``closed_loop_dynamics``: a ``(dynamics, policy)`` pair of specs - the fused kernel, see
    ``compute_trajectory`` - or any callable on ``[n, d]`` states as in the reference (a GP's mean, a
    composition of specs on device tensors ...), which is stepped ``horizon - 1`` times on the
    device.  Returns the boolean mask ``roa [n]``; with ``no_traj=False`` also ``trajectories`` of
    shape ``(n, d, horizon)`` - a permuted view of the step-major buffer the kernel writes, not a
    copy.  Device-tensor start states keep the results on the device."""
    import torch
    from . import _evaluate
    from .functions import GridWorld
    horizon = int(horizon)
    if horizon < 1:
        raise ValueError('horizon counts the start states: it must be at least 1')
    keep = isinstance(grid, torch.Tensor)
    d = int(grid.ndim) if isinstance(grid, GridWorld) else int(np.shape(grid)[-1])
    if equilibrium is not None and np.size(equilibrium) != d:
        raise ValueError('equilibrium has %d entries, the states %d' % (np.size(equilibrium), d))
    if isinstance(closed_loop_dynamics, (tuple, list)):
        if len(closed_loop_dynamics) != 2:
            raise ValueError('closed_loop_dynamics must be a (dynamics, policy) pair or a callable')
        dynamics, policy = closed_loop_dynamics
        end, states, _ = _rollout(dynamics, policy, grid, horizon - 1, trajectory=not no_traj,
                                  steps_per_launch=steps_per_launch)
        ctx = _evaluate._ctx()
    elif callable(closed_loop_dynamics):
        _check_single_process()
        ctx = _evaluate._ctx()
        points = grid.all_points if isinstance(grid, GridWorld) else grid
        if np.ndim(points) != 2:
            raise ValueError('start states must be an [n, d] array')
        end = _evaluate._to_device(ctx, points)
        states = None
        if not no_traj:
            states = torch.empty((horizon,) + tuple(end.shape), dtype=torch.float64, device=ctx.torch_device)
            states[0] = end
        for t in range(1, horizon):
            nxt = closed_loop_dynamics(end)
            nxt = nxt[0] if isinstance(nxt, tuple) else nxt
            end = _evaluate._to_device(ctx, nxt)
            if states is not None:
                states[t] = end
    else:
        raise TypeError('closed_loop_dynamics must be a (dynamics, policy) pair of specs or a callable')
    roa = _membership(ctx, end, equilibrium, tol)
    if not keep:
        roa = roa.cpu().numpy()
    if no_traj:
        return roa
    trajectories = states.permute(1, 2, 0)                           # (n, d, horizon), a view
    return roa, (trajectories if keep else trajectories.cpu().numpy())


def reward_rollout(grid, closed_loop_dynamics, reward_function, discount, horizon=250, tol=1e-3,
                   full_output=False, steps_per_launch=0):
    """The discounted return of the closed loop from every state of ``grid``
    (``examples/utilities.py:522-545``)::

        rollout = 0
        for t in range(horizon):
            temp = (discount ** t) * reward(x, policy(x));  rollout += temp
            if max over all states of |temp| < tol: converged, stop
            x = dynamics(x, policy(x))

    The stopping rule is global: the step at which the loop ends depends on the whole point set
    passed in, as in the reference.  A NaN or an infinite term never satisfies the test.

    ``grid``: a ``GridWorld`` (all its points) or an ``[n, d]`` array of start states.
    ``closed_loop_dynamics``: a ``(dynamics, policy)`` pair of specs as for ``compute_roa`` - the fused
    kernel; ``reward_function`` is then a ``QuadraticFunction`` on ``[x, u]`` (the notebooks'
    ``QuadraticFunction(block_diag(-Q, -R))``) - or any callable on ``[n, d]`` states with a callable
    ``reward_function`` on states returning ``[n]`` or ``[n, 1]`` (a GP's mean ...), stepped on
    device tensors with one maximum read back per step.  The weights ``discount ** t`` are computed
    on the host with that Python expression, so they are the reference's bit for bit.

    Returns ``rollout [n]`` (float64); with ``full_output=True`` ``(rollout, steps, converged)``:
    the number of reward terms summed and whether the test stopped the loop.  ``steps_per_launch``
    (0: chosen by the library) never changes the result.  Device-tensor start states keep the
    result on the device.  Nothing is printed."""
    import copy
    import torch
    from . import _evaluate
    from .functions import GridWorld, QuadraticFunction
    horizon = int(horizon)
    if horizon < 1:
        raise ValueError('horizon counts the reward terms: it must be at least 1')
    if not np.isfinite(discount):
        raise ValueError('discount must be finite, got %r' % (discount,))
    keep = isinstance(grid, torch.Tensor)
    pair = isinstance(closed_loop_dynamics, (tuple, list))
    spec_reward = isinstance(reward_function, QuadraticFunction)
    if pair and len(closed_loop_dynamics) != 2:
        raise ValueError('closed_loop_dynamics must be a (dynamics, policy) pair or a callable')
    if pair and not spec_reward:
        raise TypeError('a (dynamics, policy) pair of specs takes the fused kernel, which needs '
                        'reward_function as a QuadraticFunction on [x, u], got %r; for any other reward pass '
                        'closed_loop_dynamics and reward_function both as callables on states'
                        % (reward_function,))
    if not pair and not callable(closed_loop_dynamics):
        raise TypeError('closed_loop_dynamics must be a (dynamics, policy) pair of specs or a callable')
    if not pair and spec_reward:
        raise TypeError('a QuadraticFunction reward spec is a function of [x, u] and goes with a (dynamics, '
                        'policy) pair of specs; with a callable closed_loop_dynamics pass a callable reward on '
                        'states, e.g. `lambda x: reward(x, policy(x))`')
    if not pair and not callable(reward_function):
        raise TypeError('reward_function must be a callable on states when closed_loop_dynamics is one')
    weights = np.array([discount ** t for t in range(horizon)], dtype=np.float64)
    if pair:
        dynamics, policy = closed_loop_dynamics
        _check_pair(dynamics, policy)
        _check_single_process()
        d = int(grid.ndim) if isinstance(grid, GridWorld) else int(np.shape(grid)[-1])
        ctx, builder = _engine(d)
        world, start, n, d = _start_points(ctx, grid)
        if n < 1:
            raise ValueError('reward_rollout needs at least one start state')
        if world is not None:
            builder.grid = copy.copy(world)
        p = d + _evaluate._policy_output_dim(policy)
        if int(reward_function.matrix.shape[0]) != p:
            raise ValueError('the reward is quadratic in %d inputs, [x, u] has %d'
                             % (reward_function.matrix.shape[0], p))
        builder.upload(policy, dynamics, QuadraticFunction(np.eye(d)), reward=reward_function)
        dev = ctx.torch_device
        rollout = torch.empty((n,), dtype=torch.float64, device=dev)
        state = torch.empty((n, d), dtype=torch.float64, device=dev)
        d_weights = torch.from_numpy(weights).to(dev)
        run = _fused(ctx, dynamics, reward=True)
        steps, converged = run(0, n, start, horizon, d_weights, tol, rollout, state, steps_per_launch)
    else:
        _check_single_process()
        ctx = _evaluate._ctx()
        points = grid.all_points if isinstance(grid, GridWorld) else grid
        if np.ndim(points) != 2:
            raise ValueError('start states must be an [n, d] array')
        states = _evaluate._to_device(ctx, points)
        if states.shape[0] < 1:
            raise ValueError('reward_rollout needs at least one start state')
        rollout = torch.zeros((states.shape[0],), dtype=torch.float64, device=ctx.torch_device)
        steps, converged = horizon, False
        for t in range(horizon):
            reward = reward_function(states)
            reward = _evaluate._to_device(ctx, reward[0] if isinstance(reward, tuple) else reward).reshape(-1)
            if reward.shape[0] != rollout.shape[0]:
                raise ValueError('reward_function must return [n] or [n, 1] values, got %d for %d states'
                                 % (reward.shape[0], rollout.shape[0]))
            temp = float(weights[t]) * reward
            rollout += temp
            if float(temp.abs().max()) < tol:                        # (a NaN maximum compares false)
                steps, converged = t + 1, True
                break
            nxt = closed_loop_dynamics(states)
            states = _evaluate._to_device(ctx, nxt[0] if isinstance(nxt, tuple) else nxt)
    if not keep:
        rollout = rollout.cpu().numpy()
    return (rollout, steps, converged) if full_output else rollout
