"""Training steps for a ``LyapunovNetwork`` (``examples/lyapunov_function_learning.ipynb``).

The notebook grows the verified level set of a network towards the true region of attraction with
two ``optimizer.minimize(..., var_list=lyapunov_function.parameters)`` calls of plain gradient
descent: a pre-training towards given values (cell 25) and the region-of-attraction classifier with
a decrease penalty (cell 30).  Here a step is two engine calls - ``sl_nn_loss`` evaluates the loss
terms of the batch and the coefficient of every point, ``sl_nn_param_grad`` sums coefficient times
``dV/dK`` over the points on the matrix cores - and the update ``theta <- theta - lr * grad`` of
``network.weights`` on the host, where the master copy of the weights lives: the sweeps and the point
evaluations notice the edit through that copy.
"""

import numpy as np

from . import _hip

__all__ = ['balanced_class_weights', 'pretraining_step', 'roa_classification_step', 'policy_improvement_step',
           'value_function_step', 'supervised_value_step']


def _check_single_process():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError('the training steps run on one GPU; under torch.distributed call them on '
                                  'one rank and broadcast network.weights')


def balanced_class_weights(y_true, scale_by_total=True):
    """Per-sample weights that give both classes of a binary labelling the same total weight, and the
    class counts ``[negatives, positives]`` (``examples/utilities.py:737-750``).  A sample weighs one
    over the size of its class, times the number of samples with ``scale_by_total``; a class that is
    absent weighs nothing."""
    labels = np.asarray(y_true).astype(bool)
    positives = int(labels.sum())
    negatives = labels.size - positives
    weights = np.ones(labels.shape, dtype=float)
    weights[labels] /= max(positives, 1)
    weights[~labels] /= max(negatives, 1)
    if scale_by_total:
        weights *= labels.size
    return weights, np.array([negatives, positives])


def _column(ctx, values, m, what):
    """``values`` as a float64 device vector of ``m`` entries."""
    from . import _evaluate
    import torch
    if not isinstance(values, torch.Tensor):
        values = np.asarray(values, dtype=np.float64).reshape(-1, 1)
    out = _evaluate._to_device(ctx, values).reshape(-1)
    if out.numel() != m:
        raise ValueError('%d %s for %d states' % (out.numel(), what, m))
    return out


def _states(network, ctx, states):
    from . import _evaluate
    d_states = _evaluate._to_device(ctx, states)
    if d_states.shape[1] != network.input_dim:
        raise ValueError('the network expects %d inputs, the states have %d columns'
                         % (network.input_dim, d_states.shape[1]))
    return d_states


def _descend(network, ctx, d_points, d_coeff, learning_rate):
    gradient = network._weights_gradient(network._kernel_gradient(ctx, d_points, d_coeff))
    network.weights = [w - learning_rate * g for w, g in zip(network.weights, gradient)]


def pretraining_step(network, states, targets, learning_rate):
    """One gradient-descent step on ``mean |V(states) - targets|`` (cell 25 of the notebook); returns
    the objective BEFORE the step.  ``learning_rate=None`` evaluates the objective only."""
    import torch
    _check_single_process()
    if network.negate:
        raise ValueError('train the network itself, not its negation')
    ctx = network._on_engine()
    d_states = _states(network, ctx, states)
    m, d = d_states.shape
    d_targets = _column(ctx, targets, m, 'targets')
    losses = torch.empty(3, dtype=torch.float64, device=ctx.torch_device)
    coeff = torch.empty(m, dtype=torch.float64, device=ctx.torch_device)
    ctx.nn_loss(_hip.NN_LOSS_ABS, m, d, d_states, None, d_targets, None, 0.0, 0.0, 0.0, losses, coeff)
    if learning_rate is not None:
        _descend(network, ctx, d_states, coeff, float(learning_rate))
    return float(losses[0])


def roa_classification_step(lyapunov, states, roa_labels, class_weights, safe_level, lagrange_multiplier,
                            learning_rate, eps=1e-8):
    """One gradient-descent step of the notebook's cell 30 on the network ``lyapunov.lyapunov_function``:

        classifier_i = w_i max(-(2 l_i - 1)(safe_level - V(x_i)), 0)
        decrease_i   = l_i max(V(x_i+) - V(x_i), 0) / stop_gradient(V(x_i) + eps)
        objective    = mean_i (classifier_i + lagrange_multiplier * decrease_i)

    with ``x+ = dynamics(x, policy(x))`` of ``lyapunov`` (the mean, for uncertain dynamics), evaluated on
    the device and held constant.  Returns ``dict(objective, classifier_loss, decrease_loss)`` - the three
    means BEFORE the step; ``learning_rate=None`` evaluates them only (the notebook's test set)."""
    import torch
    from . import _evaluate
    _check_single_process()
    network = lyapunov.lyapunov_function
    from .functions import PolynomialFunction
    if isinstance(network, PolynomialFunction):
        raise NotImplementedError('roa_classification_step trains a LyapunovNetwork; a PolynomialFunction (%s) has '
                                  'no trainable parameters in the engine' % network.name)
    if not hasattr(network, '_kernel_gradient') or network.negate:
        raise TypeError('lyapunov.lyapunov_function must be a LyapunovNetwork')
    ctx = _evaluate._ctx()
    d_states = _states(network, ctx, states)
    m, d = d_states.shape
    d_labels = _column(ctx, roa_labels, m, 'labels')
    d_weights = _column(ctx, class_weights, m, 'class weights')
    actions = _evaluate.policy(lyapunov.policy, d_states)
    successors = _evaluate.dynamics(lyapunov.dynamics, d_states, actions)
    if isinstance(successors, tuple):
        successors = successors[0]
    d_next = successors.contiguous()
    ctx = network._on_engine()
    losses = torch.empty(3, dtype=torch.float64, device=ctx.torch_device)
    coeff = torch.empty(2 * m, dtype=torch.float64, device=ctx.torch_device)
    points = torch.empty((2 * m, d), dtype=torch.float64, device=ctx.torch_device)
    ctx.nn_loss(_hip.NN_LOSS_ROA, m, d, d_states, d_next, d_labels, d_weights, float(safe_level),
                float(lagrange_multiplier), float(eps), losses, coeff, points)
    if learning_rate is not None:
        _descend(network, ctx, points, coeff, float(learning_rate))
    objective, classifier, decrease = losses.tolist()
    return dict(objective=objective, classifier_loss=classifier, decrease_loss=decrease)


def policy_improvement_step(rl, states, learning_rate, reduction='mean', lyapunov=None, lagrange_multiplier=1.):
    """One gradient step of the policy-improvement half of policy iteration on ``rl.policy`` (a bare
    ``NeuralNetwork`` or ``Triangulation``): ``theta <- theta + learning_rate * dJ/dtheta`` with
    ``J = reduce_i rl.future_values(states_i)`` - plain gradient descent on ``-J``, the
    ``optimizer.minimize(-reduce(rl.future_values(states)), var_list=rl.policy.parameters)`` of
    ``examples/inverted_pendulum.ipynb`` cells 9/12 (``reduction='mean'``) and of
    ``tests/test_rl.py:59`` (``'sum'``).  Returns the objective ``J`` BEFORE the step;
    ``learning_rate=None`` evaluates it only.  ``states=None``: the grid's vertices.

    With ``lyapunov=`` the step is the SAFE policy update of the notebook's cell 17, run 200 at a time by
    its cells 21/22: ``J = reduce_i rl.future_values(states_i, lyapunov=lyapunov,
    lagrange_multiplier=lagrange_multiplier)``, the Lyapunov decrease as a soft constraint.  Out of
    scope: a ``LyapunovNetwork`` as the Lyapunov function, the dependence of the threshold on the
    policy's parameters through ``policy.lipschitz()`` inside a ``lipschitz_dynamics`` callable (the
    notebook's TensorFlow graph differentiates it; here ``L_f`` is a number or ``c + ||M x||_1``),
    optimisers other than plain gradient descent, and more than one rank.

    The gradient comes from ``rl.policy_gradient`` (``sl_action_gradient``, ``sl_decrease_gradient`` and the
    policy's ``parameter_gradient`` on the GPU); the update is assigned to ``policy.parameters`` on the host,
    where the master copy lives: sweeps, ``value_iteration``, the successor cache and ``Lyapunov``
    objects that share the policy notice the edit through its version token."""
    _check_single_process()
    if lyapunov is None:
        objective, gradient = rl.policy_gradient(states, reduction)
    else:
        objective, gradient = rl.policy_gradient(states, reduction, lyapunov=lyapunov,
                                                 lagrange_multiplier=lagrange_multiplier)
    if learning_rate is not None:
        policy, rate = rl.policy, float(learning_rate)
        if isinstance(gradient, list):
            policy.parameters = [w + rate * g for w, g in zip(policy.parameters, gradient)]
        else:
            policy.parameters = policy.parameters + rate * gradient
    return objective


def value_function_step(ac, states, learning_rate, scaling=1., reduction='mean', policy=None):
    """One gradient-descent step of the critic of an ``ActorCritic`` on ``scaling * reduce_i |V(x_i) -
    target_i|``, ``target = stop_gradient(r(x, u) + gamma V(f(x, u)))`` at ``u = policy(x)`` - the
    ``optimizer.minimize(value_objective, var_list=value_function.parameters)`` of
    ``examples/reinforcement_learning_pendulum.ipynb`` cells 34/48 and ``reinforcement_learning_cartpole.ipynb``
    cell 15: ``theta <- theta - learning_rate * scaling * gradient``.  ``policy=`` evaluates another policy than
    ``ac.policy`` (the pendulum notebook's cell 16 fits the value function of a fixed saturated LQR policy).
    Returns the UNSCALED objective before the step; ``learning_rate=None`` evaluates it only."""
    _check_single_process()
    objective, gradient = ac.value_gradient(states, reduction, policy=policy)
    if learning_rate is not None:
        network, step = ac.value_function, float(learning_rate) * float(scaling)
        network.parameters = [w - step * g for w, g in zip(network.parameters, gradient)]
    return objective


def supervised_value_step(value_function, states, targets, learning_rate):
    """One gradient-descent step of a ``NeuralNetwork`` with one output on ``mean |V(states) - targets|``
    (the supervised pre-training of ``examples/reinforcement_learning_pendulum.ipynb`` cell 31): ``V`` from the
    point kernels, the coefficients ``sign(V - y) / n`` formed on the device (``sign(0) = 0``), the sum over the
    batch by ``parameter_gradient``.  Returns the objective before the step; ``learning_rate=None`` evaluates it
    only."""
    import torch
    from . import _evaluate
    from .functions import NeuralNetwork
    _check_single_process()
    if type(value_function) is not NeuralNetwork or value_function.negate:
        raise TypeError('value_function must be a bare NeuralNetwork')
    if value_function.output_dim != 1:
        raise ValueError('a value function has one output, this network %d' % value_function.output_dim)
    ctx = _evaluate._ctx()
    d_states = _states(value_function, ctx, states)
    n = d_states.shape[0]
    d_targets = _column(ctx, targets, n, 'targets')
    error = _evaluate.policy(value_function, d_states).reshape(-1) - d_targets
    objective = float(error.abs().sum()) / n
    if learning_rate is not None:
        coeff = (torch.sign(error) * (1.0 / n)).reshape(-1, 1)
        gradient = value_function.parameter_gradient(d_states, coeff)
        rate = float(learning_rate)
        value_function.parameters = [w - rate * g for w, g in zip(value_function.parameters, gradient)]
    return objective
