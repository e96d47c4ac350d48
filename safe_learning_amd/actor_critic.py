"""``ActorCritic``: approximate policy iteration with a ``NeuralNetwork`` value function, on the HIP engine.

``examples/reinforcement_learning_pendulum.ipynb`` (cells 16, 31, 34, 48) and
``examples/reinforcement_learning_cartpole.ipynb`` (cell 15) alternate two gradient-descent steps on sampled
states, policy and value function both ``NeuralNetwork``s, the dynamics the true Euler models::

    target           = stop_gradient(r(x, u) + gamma * V(f(x, u))),   u = policy(x)
    value_objective  =  scaling * mean |V(x) - target|               -> var_list = value_function.parameters
    policy_objective = -scaling * mean (r(x, u) + gamma * V(f(x, u))) -> var_list = policy.parameters

Here one ``sl_critic_batch`` call evaluates the batch - successor, ``V(x)``, ``q = r + gamma V(x+)``, ``dq/du``
with the dynamics' action tangent and the value network's input gradient, the TD coefficients ``sign(V(x) - q)``
and the two sums - and the parameter gradients are the policy's ``parameter_gradient`` and
``sl_dense_param_grad`` on the value network.  The steps themselves are ``training.value_function_step`` and
``training.policy_improvement_step``.  Grid-free, one process; the weights' master copies stay on the host.
"""

import numpy as np

from . import _hip
from . import distributed as dist_utils
from ._model import ModelBuilder
from .functions import (CartPole, ConstantFunction, GPMeanFunction, InvertedPendulum, LinearSystem, NeuralNetwork,
                        PolynomialSystem, QuadraticFunction, Triangulation)

__all__ = ['ActorCritic', 'CriticEvaluation']


class CriticEvaluation(object):
    """What ``ActorCritic.evaluate`` returns, one row per state: ``actions`` ``[n, m]``, ``next_states``
    ``[n, d]``, ``values`` ``V(x)`` ``[n, 1]``, ``future_values`` ``r + gamma V(x+)`` ``[n, 1]``, ``td_error``
    ``V(x) - future_values`` ``[n, 1]`` and ``action_gradient`` ``d future_values / du`` ``[n, m]``."""

    __slots__ = ('actions', 'next_states', 'values', 'future_values', 'td_error', 'action_gradient')

    def __init__(self, **fields):
        for name in self.__slots__:
            setattr(self, name, fields[name])


class ActorCritic(object):
    """``policy``: any policy spec of the package (``policy_gradient`` needs a bare ``NeuralNetwork`` or
    ``Triangulation``); ``dynamics``: ``InvertedPendulum``, ``CartPole`` or ``LinearSystem``;
    ``reward_function``: a ``QuadraticFunction`` on ``[x, u]``; ``value_function``: a bare ``NeuralNetwork``
    with one output (layers up to 64 wide)."""

    def __init__(self, policy, dynamics, reward_function, value_function, gamma=0.98):
        if dist_utils.rank_and_world()[1] > 1:
            raise NotImplementedError('ActorCritic runs on one GPU; under torch.distributed use it on one rank '
                                      'and broadcast the parameters')
        if type(value_function) is not NeuralNetwork or value_function.negate:
            raise TypeError('value_function must be a bare NeuralNetwork, not %s%s'
                            % ('a negated ' if getattr(value_function, 'negate', False) else '',
                               type(value_function).__name__))
        if value_function.output_dim != 1:
            raise ValueError('a value function has one output, this network %d' % value_function.output_dim)
        if isinstance(dynamics, InvertedPendulum):
            d, m = 2, 1
        elif isinstance(dynamics, CartPole):
            d, m = 4, 1
        elif isinstance(dynamics, LinearSystem):
            d, m = dynamics.output_dim, dynamics.input_dim - dynamics.output_dim
            if m < 1:
                raise ValueError('linear dynamics of %d x %d have no action columns' % dynamics.matrix.shape)
        elif isinstance(dynamics, PolynomialSystem):
            raise TypeError('dynamics must be InvertedPendulum, CartPole or LinearSystem: a PolynomialSystem (%s) has '
                            'no action tangent in the engine yet' % type(dynamics).__name__)
        elif isinstance(dynamics, GPMeanFunction):
            raise TypeError('dynamics must be InvertedPendulum, CartPole or LinearSystem: the TD batches of '
                            'sl_critic_batch have no GP path, so a GPMeanFunction (%s) cannot be the model of an '
                            'ActorCritic (GP models: PolicyIteration with a Triangulation value function)'
                            % dynamics.name)
        else:
            raise TypeError('dynamics must be InvertedPendulum, CartPole or LinearSystem, not %s (GP models: '
                            'PolicyIteration.action_gradient with a Triangulation value function)'
                            % type(dynamics).__name__)
        if not isinstance(reward_function, QuadraticFunction):
            raise TypeError('reward_function must be a QuadraticFunction on [x, u]')
        if reward_function.ndim != d + m:
            raise ValueError('reward on %d inputs, [x, u] has %d' % (reward_function.ndim, d + m))
        if value_function.input_dim is None:
            value_function._layers_for_upload(d)
        if value_function.input_dim != d:
            raise ValueError('the value network expects %d inputs, the states have %d'
                             % (value_function.input_dim, d))
        if max(value_function.layers) > 64:
            raise ValueError('value-network layers up to 64 wide, got %d' % max(value_function.layers))
        self.policy = policy
        self.dynamics = dynamics
        self.reward_function = reward_function
        self.value_function = value_function
        self.gamma = gamma
        self.state_dim, self.action_dim = d, m
        from . import _evaluate
        self._ctx = _hip.Context()
        self._builder = ModelBuilder(self._ctx, _evaluate._dummy_grid(d))
        self._placeholder_policy = ConstantFunction(np.zeros(m))
        self._placeholder_value = QuadraticFunction(np.eye(d))

    # ---- one sl_critic_batch call ------------------------------------------------------------------------
    def _batch(self, states, policy, actions, reduction='mean', gradients=True):
        """-> dict of device tensors: states, actions, next, value [n], q [n], sums [2] and, with
        ``gradients``, dq_du [n, m] and coeff [n]."""
        import torch
        from . import _evaluate
        if reduction not in ('mean', 'sum'):
            raise ValueError("reduction must be 'mean' or 'sum', got %r" % (reduction,))
        ctx, d, m = self._ctx, self.state_dim, self.action_dim
        d_states = _evaluate._to_device(ctx, states)
        if d_states.shape[1] != d:
            raise ValueError('states of %d columns, the dynamics have %d states' % (d_states.shape[1], d))
        n = d_states.shape[0]
        if n == 0:
            raise ValueError('no states')
        if actions is None:
            chosen = self.policy if policy is None else policy
            if isinstance(chosen, (np.ndarray, torch.Tensor)):
                raise TypeError('an action table is not a policy of the states: pass it as `actions`')
            actions = _evaluate.policy(chosen, d_states)
        d_actions = _evaluate._action_rows(ctx, actions, n)
        if d_actions.shape[1] != m:
            raise ValueError('actions of %d columns, the dynamics take %d' % (d_actions.shape[1], m))
        self._builder.upload(self._placeholder_policy, self.dynamics, self._placeholder_value,
                             reward=self.reward_function, gamma=self.gamma)
        vf = self.value_function
        dev = ctx.torch_device
        out = dict(states=d_states, actions=d_actions,
                   next=torch.empty((n, d), dtype=torch.float64, device=dev),
                   value=torch.empty(n, dtype=torch.float64, device=dev),
                   q=torch.empty(n, dtype=torch.float64, device=dev),
                   sums=torch.empty(2, dtype=torch.float64, device=dev), dq_du=None, coeff=None)
        if gradients:
            out['dq_du'] = torch.empty((n, m), dtype=torch.float64, device=dev)
            out['coeff'] = torch.empty(n, dtype=torch.float64, device=dev)
        dims, acts, has_bias = vf._description()
        ctx.critic_batch(dims, acts, has_bias, vf.output_scale, vf._device_parameters(ctx), n, d_states, d_actions,
                         reduction, out['value'], out['q'], out['sums'], d_next=out['next'], d_dq_du=out['dq_du'],
                         d_coeff=out['coeff'])
        return out

    def evaluate(self, states, policy=None, actions=None):
        """Everything ``sl_critic_batch`` computes per state, as a ``CriticEvaluation``, at
        ``u = policy(states)`` (default ``self.policy``) or at the given ``actions`` (one row, or one per
        state).  Device tensors in, device tensors out; NumPy otherwise."""
        import torch
        keep = isinstance(states, torch.Tensor)
        b = self._batch(states, policy, actions)
        fields = dict(actions=b['actions'], next_states=b['next'], values=b['value'].reshape(-1, 1),
                      future_values=b['q'].reshape(-1, 1), td_error=(b['value'] - b['q']).reshape(-1, 1),
                      action_gradient=b['dq_du'])
        if not keep:
            fields = {k: v.cpu().numpy() for k, v in fields.items()}
        return CriticEvaluation(**fields)

    def future_values(self, states, policy=None, actions=None):
        """``r(x, u) + gamma V(f(x, u))`` -> ``[n, 1]``."""
        import torch
        q = self._batch(states, policy, actions, gradients=False)['q'].reshape(-1, 1)
        return q if isinstance(states, torch.Tensor) else q.cpu().numpy()

    def value_gradient(self, states, reduction='mean', policy=None, actions=None):
        """``(objective, gradient)`` of ``reduce_i |V(x_i) - target_i|`` with respect to
        ``value_function.parameters`` (a list shaped like them), the target ``r + gamma V(x+)`` held constant as
        the notebooks' ``tf.stop_gradient`` holds it: the gradient is ``sum_i w sign(V(x_i) - target_i) dV(x_i)/d
        theta`` (``sign(0) = 0``), summed on the GPU by ``sl_dense_param_grad``."""
        import torch
        b = self._batch(states, policy, actions, reduction)
        ctx, vf = self._ctx, self.value_function
        n = b['states'].shape[0]
        dims, acts, has_bias = vf._description()
        params = vf._device_parameters(ctx)
        flat = torch.empty(params.numel(), dtype=torch.float64, device=ctx.torch_device)
        ctx.dense_param_grad(dims, acts, has_bias, vf.output_scale, params, n, self.state_dim, b['states'],
                             b['coeff'], flat)
        total = float(b['sums'][0])
        return (total / n if reduction == 'mean' else total), vf._unflatten(flat.cpu().numpy())

    def policy_gradient(self, states, reduction='mean'):
        """``(objective, gradient)`` of ``J = reduce_i future_values(x_i)`` under ``self.policy`` with respect
        to its parameters (a bare ``NeuralNetwork`` or ``Triangulation``): ``dq/du`` of the batch, scaled by
        ``1/n`` for ``'mean'``, through the policy's ``parameter_gradient``.  The signature
        ``training.policy_improvement_step`` calls."""
        if reduction not in ('mean', 'sum'):
            raise ValueError("reduction must be 'mean' or 'sum', got %r" % (reduction,))
        policy = self.policy
        if type(policy) not in (NeuralNetwork, Triangulation) or policy.negate:
            raise TypeError('policy_gradient differentiates a bare NeuralNetwork or Triangulation policy, '
                            'not %s' % (('a negated ' if getattr(policy, 'negate', False) else '')
                                        + type(policy).__name__))
        b = self._batch(states, None, None, reduction)
        n = b['states'].shape[0]
        grad, total = b['dq_du'], float(b['sums'][1])
        if reduction == 'mean':
            grad = grad * (1.0 / n)
            total = total / n
        return total, policy.parameter_gradient(b['states'], grad)
