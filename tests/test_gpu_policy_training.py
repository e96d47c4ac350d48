"""Policy gradients of future_values on the GPU (needs an MI355X): sl_action_gradient, sl_policy_param_grad,
sl_tri_param_grad and the step built on them, against the NumPy reference of tests/np_policy_training.py
(itself checked against torch autograd, long double and the reference's known answer by
tests/test_policy_training_host.py).  Gradients are compared as |g - g_ref| <= tolerance * A with A the
reference's error companion and tolerance 32 times the reference's own measured error; every test prints the
ratio it measured before it asserts."""

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import guarded
import np_policy_training as T
from training_tolerance import UNIT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sl():
    import safe_learning_amd
    return safe_learning_amd


def _above_bound():
    """More points than the grid-stride launches hold at once: 2 x CUs x 256 and an odd remainder."""
    import torch
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count * 256 + 77


_pairs = {}


def _pair(sl, name):
    if name not in _pairs:
        _pairs[name] = T.system_pair(name, sl)
    return _pairs[name]


# ---- sl_action_gradient ------------------------------
@pytest.mark.parametrize("explicit", [True, False], ids=["actions", "policy"])
@pytest.mark.parametrize("name", T.SYSTEMS)
def test_action_gradient_matches_reference(sl, name, explicit):
    import torch
    orl, rl = _pair(sl, name)
    for n in (1, 63, 64, 65, 1000, _above_bound()):
        states, actions = T.system_states(name, n)
        u_ref = actions if explicit else T.policy_actions(orl.policy, states)
        ok = T.comparable(orl, states, u_ref)
        assert 1 - ok.mean() <= T.MAX_EXCLUDED or n < 100
        ref = T.action_gradient(orl, states, u_ref)
        got = rl.action_gradient(states, actions=actions if explicit else None)
        assert got.shape == ref["grad"].shape
        ratio = T.ratio_to_companion(got, ref["grad"], ref["A"], ok)
        print("%s, %s, n = %d: %.3f x 2^-53 of A (tolerance %.1f), %.4f left out, %.3f of the successors clipped"
              % (name, "explicit actions" if explicit else "policy", n, ratio,
                 32 * T.REFERENCE_RATIO["action", name, explicit], 1 - ok.mean(),
                 ((ref["next"] < -1) | (ref["next"] > 1)).any(axis=1).mean()))
        assert ratio * UNIT <= T.tolerance("action", name, explicit)
        if n == 1000:
            # Q of the same call equals future_values at the same states; tensors in, a tensor out
            d_states = torch.from_numpy(states).cuda()
            d_actions = torch.from_numpy(actions).cuda() if explicit else None
            _, d_grad, d_q = rl._action_gradient_device(d_states, None, d_actions)
            fv = rl.future_values(states, actions=actions if explicit else None)[:, 0]
            assert_allclose(d_q.cpu().numpy(), fv, rtol=1e-12, atol=0)
            assert_allclose(fv[ok], ref["q"][ok], rtol=1e-9, atol=1e-12)
            on_device = rl.action_gradient(d_states, actions=d_actions)
            assert isinstance(on_device, torch.Tensor) and on_device.is_cuda
            assert_array_equal(on_device.cpu().numpy(), got)
            assert_array_equal(d_grad.cpu().numpy(), got)
            if orl.value_function.project:
                assert ((ref["next"] < -1) | (ref["next"] > 1)).any(axis=1)[ok].any()


def test_action_gradient_on_the_grid(sl):
    """states=None: the grid's vertices (the 19 states of the reference's test)."""
    orl, rl = _pair(sl, "lqr")
    states = orl.state_space
    u = T.policy_actions(orl.policy, states)
    ref = T.action_gradient(orl, states, u)
    got = rl.action_gradient()
    ratio = T.ratio_to_companion(got, ref["grad"], ref["A"])
    print("lqr on its grid: %.3f x 2^-53 of A" % ratio)
    assert ratio * UNIT <= T.tolerance("action", "lqr", False)
    assert_array_equal(got, rl.action_gradient(rl.state_space))
    one_row = rl.action_gradient(actions=np.array([[0.25]]))
    ref_row = T.action_gradient(orl, states, np.full((len(states), 1), 0.25))
    assert T.ratio_to_companion(one_row, ref_row["grad"], ref_row["A"]) * UNIT <= T.tolerance("action", "lqr", True)


# ---- NeuralNetwork.parameter_gradient ------------------------------
@pytest.mark.parametrize("key", sorted(T.NETWORKS))
def test_network_parameter_gradient_matches_reference(sl, key):
    import torch
    onet, net = T.make_network(key, sl)
    for n in (1, 15, 16, 17, 1000, _above_bound()):
        points, coeff = T.make_batch(key, n)
        ok = T.relu_margin(onet, points) > 1e-9
        assert 1 - ok.mean() <= T.MAX_EXCLUDED and (ok.all() or n > 50)
        points, coeff = points[ok], coeff[ok]
        assert (coeff == 0).all(axis=1).any() or n < 3
        ref, comp = T.network_parameter_gradient(onet, points, coeff)
        got = net.parameter_gradient(points, coeff)
        assert [g.shape for g in got] == [p.shape for p in net.parameters]
        ratio = T.ratio_to_companion(got, ref, comp)
        tol = T.tolerance("network", key, n) if ok.all() else 32 * UNIT * T.ratio_to_companion(
            ref, T.network_parameter_gradient(onet, points, coeff, T.LONG)[0], comp)
        print("%s, n = %d: %.3f x 2^-53 of A (tolerance %.2f)" % (key, n, ratio, tol / UNIT))
        assert ratio * UNIT <= tol
        if n in (17, 1000):
            on_device = net.parameter_gradient(torch.from_numpy(points).cuda(), torch.from_numpy(coeff).cuda())
            for a, b in zip(on_device, got):
                assert_array_equal(a, b)


# ---- Triangulation.parameter_gradient ------------------------------
@pytest.mark.parametrize("key", sorted(T.TABLES))
def test_table_parameter_gradient_matches_reference(sl, key):
    import torch
    (otri, tri), points, coeff = T.table_case(key, sl)
    ref, comp = T.table_parameter_gradient(otri, points, coeff)
    got = tri.parameter_gradient(points, coeff)
    assert got.shape == ref.shape == (tri.nindex, coeff.shape[1])
    ratio = T.ratio_to_companion(got, ref, comp)
    print("%s: %.3f x 2^-53 of A (tolerance %.2f)" % (key, ratio, 32 * T.REFERENCE_RATIO["table", key]))
    assert ratio * UNIT <= T.tolerance("table", key)
    on_device = tri.parameter_gradient(torch.from_numpy(points).cuda(), torch.from_numpy(coeff).cuda())
    assert_array_equal(on_device, got)
    assert_array_equal((-tri).parameter_gradient(points, coeff), -got)
    # a vertex no point touches gets an exact zero: one point in the first cell
    lone = tri.parameter_gradient(points[-1:], coeff[-1:])
    assert (lone != 0).any(axis=1).sum() <= tri.input_dim + 1


# ---- determinism and bounds ------------------------------
def _twice(call, sizes):
    """Run ``call(*outputs)`` twice into guarded buffers -> the outputs' bits; the second run's must be the same."""
    first, again = guarded.run(call, sizes), guarded.run(call, sizes)
    for a, b in zip(first, again):
        assert_array_equal(a, b)
    return first


def test_entry_points_are_deterministic_and_stay_in_bounds(sl):
    import torch
    from safe_learning_amd import _evaluate
    n = _above_bound()
    # sl_action_gradient: GP dynamics, network policy
    orl, rl = _pair(sl, "pendulum")
    states, _ = T.system_states("pendulum", n)
    d_states = torch.from_numpy(states).cuda()
    rl._upload(rl.policy)
    d, m = states.shape[1], 1
    _twice(lambda grad, q, nxt: rl._ctx.action_gradient(n, d_states, None, grad, q, nxt), [n * m, n, n * d])
    # sl_policy_param_grad
    onet, net = T.make_network("notebook", sl)
    points, coeff = T.make_batch("notebook", n)
    ctx = net._on_engine()
    d_points, d_coeff = torch.from_numpy(points).cuda(), torch.from_numpy(coeff).cuda()
    total = sum(p.size for p in net.parameters)
    _twice(lambda grad: ctx.policy_param_grad(n, 2, d_points, d_coeff, grad), [total])
    # sl_tri_param_grad
    (otri, tri), points, coeff = T.table_case("2d-two", sl, n=5000)
    ctx, builder = _evaluate._builder(2)
    builder._upload_tri(1, tri)
    d_points, d_coeff = torch.from_numpy(points).cuda(), torch.from_numpy(coeff).cuda()
    _twice(lambda grad: ctx.tri_param_grad(1, len(points), d_points, d_coeff, grad), [tri.nindex * 2])


# ---- the reference's test through the product ------------------------------
def test_policy_iteration_of_the_reference(sl):
    """safe_learning/tests/test_rl.py:29-77 from -k/2 x: 10 x (one value_iteration() + 5
    policy_improvement_step(rl, None, 0.01, reduction='sum')), the reference run beside it."""
    import oracle
    c = T.lqr_case()
    g = c["g"]
    orl, rl = T.lqr_pair(sl, value_sweeps=0)
    step, worst = 0, 0.0
    for _ in range(g["outer_iterations"]):
        rl.value_iteration()
        orl.value_iteration()
        for _ in range(g["gd_steps"]):
            _, gradient = rl.policy_gradient(None, reduction='sum')
            before = rl.policy.parameters.copy()
            objective = sl.policy_improvement_step(rl, None, g["learning_rate"], reduction='sum')
            ref_objective, ref, comp = T.policy_improvement_step(orl, None, g["learning_rate"], 'sum')
            ratio = T.ratio_to_companion(gradient, ref, comp)
            worst = max(worst, ratio / (32 * T.REFERENCE_RATIO["steps-lqr", step]))
            print("step %d: gradient %.3f x 2^-53 of A (tolerance %.2f), objective %.12g" % (
                step, ratio, 32 * T.REFERENCE_RATIO["steps-lqr", step], objective))
            assert ratio * UNIT <= T.tolerance("steps-lqr", step)
            assert objective == pytest.approx(ref_objective, rel=1e-11)
            assert_array_equal(rl.policy.parameters, before + g["learning_rate"] * gradient)
            step += 1
    print("largest ratio / tolerance over the %d steps: %.3f" % (step, worst))
    true_value = oracle.QuadraticFunction(-c["p"])
    assert_allclose(rl.value_function.parameters, true_value(orl.state_space), atol=g["atol"])
    assert_allclose(rl.policy.parameters, -c["k"] * orl.policy.discretization.all_points, atol=g["atol"])


# ---- the notebook's shape ------------------------------
def test_notebook_shape_steps(sl):
    """Five 'mean' steps, lr 0.1, on 1000 sampled states of the pendulum case (two notebook-kernel heads, a
    [32, 32, 1] relu / relu / tanh policy): objectives and parameters track the reference step by step."""
    orl, rl = T.system_pair("pendulum", sl)
    states = T.notebook_states(orl)
    lr = T.NOTEBOOK_LOOP["learning_rate"]
    allowed = [np.zeros_like(p) for p in orl.policy.parameters]
    for step in range(T.NOTEBOOK_LOOP["steps"]):
        ok = T.comparable(orl, states, T.policy_actions(orl.policy, states), through_policy=True)
        assert 1 - ok.mean() <= T.MAX_EXCLUDED
        q_scale = float(np.abs(T.action_gradient(orl, states, T.policy_actions(orl.policy, states))["q"]).mean())
        objective = sl.policy_improvement_step(rl, states, lr, reduction='mean')
        ref_objective, ref, comp = T.policy_improvement_step(orl, states, lr, 'mean')
        # the parameters may be apart by the accumulated tolerance of the gradients so far
        tol = T.tolerance("steps-notebook", step)
        allowed = [a + lr * tol * c for a, c in zip(allowed, comp)]
        worst = max(float((np.abs(p - r) / np.where(a > 0, a, 1.0)).max())
                    for p, r, a in zip(rl.policy.parameters, orl.policy.parameters, allowed))
        print("step %d: objective %.15g (reference %.15g), parameters within %.3f of the accumulated tolerance"
              % (step, objective, ref_objective, worst))
        assert abs(objective - ref_objective) <= 2e-12 * q_scale
        for p, r, a in zip(rl.policy.parameters, orl.policy.parameters, allowed):
            assert (np.abs(p - r) <= a).all()
    # future_values and a value_iteration() sweep see the new parameters
    fresh = sl.NeuralNetwork(rl.policy.layers, rl.policy.nonlinearities, output_scale=rl.policy.output_scale,
                             use_bias=rl.policy.use_bias, parameters=[p.copy() for p in rl.policy.parameters])
    vf = sl.Triangulation(rl.value_function.discretization, rl.value_function.parameters.copy(), project=True)
    other = sl.PolicyIteration(fresh, rl.dynamics, rl.reward_function, vf, gamma=rl.gamma)
    assert_array_equal(rl.future_values(states), other.future_values(states))
    assert_array_equal(rl.future_values(), other.future_values())
    assert rl.value_iteration() == other.value_iteration()
    assert_array_equal(rl.value_function.parameters, vf.parameters)
    assert not np.array_equal(rl.policy.parameters[0], T.network_parameters("notebook")[0])


# ---- errors ------------------------------
def test_documented_errors_leave_the_parameters_alone(sl, monkeypatch):
    import cases
    from safe_learning_amd.benchmarks import build_specs
    orl, rl = T.system_pair("pendulum", sl)
    states = T.system_states("pendulum", 50)[0]
    before = [p.copy() for p in rl.policy.parameters]

    def unchanged():
        for p, b in zip(rl.policy.parameters, before):
            assert_array_equal(p, b)

    # Euler dynamics
    case = cases.make_case("pendulum", num_points=17, dynamics="analytic")
    _, euler, _, _ = build_specs(case)
    rl_euler = sl.PolicyIteration(rl.policy, euler, rl.reward_function, rl.value_function, gamma=rl.gamma)
    with pytest.raises(TypeError, match="LinearSystem and GP dynamics"):
        rl_euler.action_gradient(states)
    with pytest.raises(TypeError, match="LinearSystem and GP dynamics"):
        sl.policy_improvement_step(rl_euler, states, 0.1)
    unchanged()
    # the Lyapunov penalty
    with pytest.raises(NotImplementedError, match="Lyapunov penalty"):
        rl.action_gradient(states, lyapunov=object())
    with pytest.raises(NotImplementedError, match="Lyapunov penalty"):
        rl.policy_gradient(states, lyapunov=object())
    # a wrapped policy
    rl_sat = sl.PolicyIteration(sl.Saturation(rl.policy, -1., 1.), rl.dynamics, rl.reward_function,
                                rl.value_function, gamma=rl.gamma)
    with pytest.raises(TypeError, match="bare NeuralNetwork or Triangulation"):
        sl.policy_improvement_step(rl_sat, states, 0.1)
    assert rl_sat.action_gradient(states).shape == (50, 1)          # the action gradient itself takes it
    unchanged()
    # wrong coefficient shapes
    with pytest.raises(ValueError, match="coefficients of shape"):
        rl.policy.parameter_gradient(states, np.zeros((len(states), 2)))
    with pytest.raises(ValueError, match="coefficients of shape"):
        rl.policy.parameter_gradient(states, np.zeros((len(states) - 1, 1)))
    (_, tri), points, coeff = T.table_case("2d-two", sl)
    with pytest.raises(ValueError, match="coefficients of shape"):
        tri.parameter_gradient(points, coeff[:, :1])
    with pytest.raises(ValueError, match="reduction"):
        rl.policy_gradient(states, reduction='max')
    # more than one process
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(NotImplementedError, match="one GPU"):
        sl.policy_improvement_step(rl, states, 0.1)
    monkeypatch.undo()
    monkeypatch.setattr(rl, "_world", 2)
    with pytest.raises(NotImplementedError, match="one GPU"):
        rl.policy_gradient(states)
    unchanged()
