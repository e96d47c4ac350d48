"""Actor-critic on the GPU (needs an MI355X): sl_critic_batch, sl_dense_param_grad and the steps built on them
(``ActorCritic``, ``training.value_function_step``, ``training.supervised_value_step``) against the NumPy
reference of tests/np_actor_critic.py (itself checked against torch autograd, long double and the host build of
the kernel's header by tests/test_actor_critic_host.py).  Gradients are compared as |g - g_ref| <= tolerance * A
with A the reference's error companion and tolerance 32 times the reference's own measured error; every test prints
the ratio it measured before it asserts."""

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import guarded
import np_actor_critic as T
import np_policy_training as P
from training_tolerance import LONG, UNIT, ratio_to_companion

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sl():
    import safe_learning_amd
    return safe_learning_amd


def _above_bound():
    """More samples than the grid-stride launch holds at once: 2 x CUs x 256 and an odd remainder."""
    import torch
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count * 256 + 77


SIZES = (1, 63, 64, 65, 1000, "above")


def _critic_batch(ac, states, actions, reduction, skip=()):
    """One guarded sl_critic_batch call -> dict of the outputs' bits (uint64); ``skip``: outputs passed as NULL."""
    import torch
    ctx, vf = ac._ctx, ac.value_function
    ac._builder.upload(ac._placeholder_policy, ac.dynamics, ac._placeholder_value, reward=ac.reward_function,
                       gamma=ac.gamma)
    d_states, d_actions = torch.from_numpy(states).cuda(), torch.from_numpy(actions).cuda()
    n, d = states.shape
    m = actions.shape[1]
    names = [k for k in ("value", "q", "sums", "next", "dq_du", "coeff") if k not in skip]
    sizes = dict(value=n, q=n, sums=2, next=n * d, dq_du=n * m, coeff=n)
    dims, acts, has_bias = vf._description()

    def call(*outs):
        o = dict(zip(names, outs))
        ctx.critic_batch(dims, acts, has_bias, vf.output_scale, vf._device_parameters(ctx), n, d_states, d_actions,
                         reduction, o["value"], o["q"], o["sums"], d_next=o.get("next"), d_dq_du=o.get("dq_du"),
                         d_coeff=o.get("coeff"))
    return dict(zip(names, guarded.run(call, [sizes[k] for k in names])))


# ---- sl_critic_batch ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name,vkey", T.PAIRS)
def test_critic_batch_matches_reference(sl, name, vkey, size):
    from safe_learning_amd import _evaluate
    n = _above_bound() if size == "above" else size
    system, ovnet, _, ac = T.make_actor_critic(name, vkey, sl)
    d, m = system["d"], system["m"]
    states, actions = T.make_states(name, n)
    reduction = "sum" if n == 63 else "mean"
    bits = _critic_batch(ac, states, actions, reduction)
    got = {k: v.view(np.float64) for k, v in bits.items()}
    # x+: the successor of the point kernels, bit for bit
    assert_array_equal(got["next"].reshape(n, d), _evaluate.dynamics(ac.dynamics, states, actions))
    # V(x), and q against r + gamma V(x+), from the point kernels
    v_next = ac.value_function(got["next"].reshape(n, d))[:, 0]
    assert_allclose(got["value"], ac.value_function(states)[:, 0], rtol=1e-12, atol=0)
    r = ac.reward_function(np.hstack((states, actions)))[:, 0]
    assert_allclose(got["q"], r + system["gamma"] * v_next, rtol=1e-12, atol=0)
    # dq/du, the coefficients and the sums against the reference
    ref = T.critic_batch(system, ovnet, states, actions, reduction, exact=n <= T.EXACT_LIMIT)
    ok = T.comparable(system, ovnet, states, actions)
    assert 1 - ok.mean() <= T.MAX_EXCLUDED or n < 100
    ratio = ratio_to_companion(got["dq_du"].reshape(n, m), ref["dq_du"], ref["A"], ok)
    sums_ratio = ratio_to_companion(got["sums"], ref["sums"], ref["sumsA"])
    sums_tol = T.sums_tolerance(name, vkey, n)
    print("%s / %s, n = %d: dq/du %.3f x 2^-53 of A (tolerance %.1f), sums %.3f (tolerance %.2f), %.4f left out"
          % (name, vkey, n, ratio, T.tolerance("batch", name, vkey) / UNIT, sums_ratio, sums_tol / UNIT, 1 - ok.mean()))
    assert ratio * UNIT <= T.tolerance("batch", name, vkey)
    assert_array_equal(got["coeff"][ok], ref["coeff"][ok])
    assert set(np.unique(np.abs(got["coeff"]))) <= {0.0, 1.0 / n if reduction == "mean" else 1.0}
    assert sums_ratio * UNIT <= sums_tol
    if vkey in T.EXACT_NETS and n <= T.EXACT_LIMIT:
        # relu / linear networks: the kernel runs the header's operations, the reference restates them
        for key in ("value", "q", "coeff"):
            assert_array_equal(got[key], ref[key], err_msg=key)
        assert_array_equal(got["dq_du"].reshape(n, m), ref["dq_du"])
    # two calls return the same bits; outputs passed as NULL are skipped and change nothing else
    again = _critic_batch(ac, states, actions, reduction)
    for key in bits:
        assert_array_equal(again[key], bits[key], err_msg=key)
    lean = _critic_batch(ac, states, actions, reduction, skip=("next", "dq_du", "coeff"))
    for key in lean:
        assert_array_equal(lean[key], bits[key], err_msg=key)


def test_actor_critic_methods(sl):
    """evaluate / future_values / the two gradients through the public class, tensors in and tensors out."""
    import torch
    system, ovnet, opolicy, ac = T.make_actor_critic("cartpole", "nobias", sl)
    states, actions = T.make_states("cartpole", 300)
    ev = ac.evaluate(states)
    assert_allclose(ev.actions, ac.policy(states), rtol=0, atol=0)
    ref = T.critic_batch(system, ovnet, states, ev.actions)
    assert_array_equal(ev.td_error, ev.values - ev.future_values)
    assert_array_equal(ev.future_values[:, 0], ref["q"])
    assert_array_equal(ev.action_gradient, ref["dq_du"])
    on_device = ac.evaluate(torch.from_numpy(states).cuda())
    assert on_device.values.is_cuda and on_device.action_gradient.is_cuda
    assert_array_equal(on_device.future_values.cpu().numpy(), ev.future_values)
    assert_array_equal(ac.future_values(states), ev.future_values)
    assert_array_equal(ac.future_values(states, actions=actions)[:, 0],
                       T.critic_batch(system, ovnet, states, actions)["q"])
    saturated = sl.Saturation(ac.policy, -0.01, 0.01)
    assert np.abs(ac.evaluate(states, policy=saturated).actions).max() <= 0.01


# ---- sl_dense_param_grad -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(P.NETWORKS))
def test_dense_param_grad_equals_policy_param_grad(sl, key):
    """The same network as the context's policy network and through the arguments: identical bits."""
    import torch
    _, net = P.make_network(key, sl)
    for n in (1, 65, 1000):
        points, coeff = P.make_batch(key, n)
        ctx = net._on_engine()
        d_points, d_coeff = torch.from_numpy(points).cuda(), torch.from_numpy(coeff).cuda()
        total = sum(p.size for p in net.parameters)
        dims, acts, has_bias = net._description()
        (policy_bits,) = guarded.run(lambda out: ctx.policy_param_grad(n, points.shape[1], d_points, d_coeff, out),
                                     [total])
        (dense_bits,) = guarded.run(
            lambda out: ctx.dense_param_grad(dims, acts, has_bias, net.output_scale, net._device_parameters(ctx), n,
                                             points.shape[1], d_points, d_coeff, out), [total])
        assert_array_equal(dense_bits, policy_bits)


@pytest.mark.parametrize("n", (64, 1000))
@pytest.mark.parametrize("name,vkey", T.PAIRS)
def test_value_gradient_matches_reference(sl, name, vkey, n):
    system, ovnet, _, ac = T.make_actor_critic(name, vkey, sl)
    states, actions = T.make_states(name, n)
    ok = T.comparable(system, ovnet, states, actions)
    assert 1 - ok.mean() <= T.MAX_EXCLUDED or n < 100
    states, actions = states[ok], actions[ok]
    objective, got = ac.value_gradient(states, "sum", actions=actions)
    ref_objective, ref, comp, batch = T.value_gradient(system, ovnet, states, actions, "sum")
    assert [g.shape for g in got] == [p.shape for p in ac.value_function.parameters]
    ratio = ratio_to_companion(got, ref, comp)
    tol = T.tolerance("value", name, vkey, n) if ok.all() else 32 * UNIT * ratio_to_companion(
        ref, P.network_parameter_gradient(ovnet, states, batch["coeff"][:, None], LONG)[0], comp)
    print("%s / %s, n = %d: %.3f x 2^-53 of A (tolerance %.2f)" % (name, vkey, n, ratio, tol / UNIT))
    assert ratio * UNIT <= tol
    assert abs(objective - ref_objective) <= T.sums_tolerance(name, vkey, n) * batch["sumsA"][0]


# ---- the steps -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("steps-value", "steps-both"))
@pytest.mark.parametrize("name", ("pendulum", "cartpole"))
def test_steps_follow_the_reference(sl, name, kind):
    """Five critic steps, and five critic / actor steps in turn, at batch 100: the parameters track the reference's
    trajectory within the accumulated tolerance of the gradients so far.  The objectives are compared at 1e-9 of
    their companions' mean: the parameters are apart by some 1e-13 of theirs at most (learning rate x tolerance), a
    step that went wrong moves an objective by learning rate x gradient, 1e-3 and more."""
    loop = T.STEP_LOOP
    system, ovnet, opolicy, ac = T.make_actor_critic(name, loop["value_net"][name], sl)
    states = T.step_states(name, ovnet, opolicy)
    v_allowed = [np.zeros_like(p) for p in ovnet.parameters]
    p_allowed = [np.zeros_like(p) for p in opolicy.parameters]
    for step in range(loop["steps"]):
        tol = T.tolerance(kind, name, step)
        scale = T.critic_batch(system, ovnet, states, T.policy_actions(opolicy, states), exact=False)["sumsA"] / len(states)
        objective = sl.value_function_step(ac, states, loop["value_rate"], scaling=loop["scaling"])
        ref_objective, _, comp = T.value_function_step(system, ovnet, opolicy, states, loop["value_rate"], loop["scaling"])
        v_allowed = [a + loop["value_rate"] * loop["scaling"] * tol * c for a, c in zip(v_allowed, comp)]
        print("%s %s step %d: value objective %.15g (reference %.15g)" % (name, kind, step, objective, ref_objective))
        assert abs(objective - ref_objective) <= 1e-9 * scale[0]
        if kind == "steps-both":
            objective = sl.policy_improvement_step(ac, states, loop["policy_rate"])
            ref_objective, _, comp = T.policy_improvement_step(system, ovnet, opolicy, states, loop["policy_rate"])
            p_allowed = [a + loop["policy_rate"] * tol * c for a, c in zip(p_allowed, comp)]
            print("    policy objective %.15g (reference %.15g)" % (objective, ref_objective))
            assert abs(objective - ref_objective) <= 1e-9 * scale[1]
        for got, want, allowed in ((ac.value_function.parameters, ovnet.parameters, v_allowed),
                                   (ac.policy.parameters, opolicy.parameters, p_allowed)):
            worst = max(float((np.abs(p - r) / np.where(a > 0, a, 1.0)).max()) for p, r, a in zip(got, want, allowed))
            print("    parameters within %.3f of the accumulated tolerance" % worst)
            for p, r, a in zip(got, want, allowed):
                assert (np.abs(p - r) <= a).all()
    # the point kernels see the new weights
    fresh = sl.NeuralNetwork(ovnet.layers, ovnet.nonlinearities, output_scale=ovnet.output_scale,
                             use_bias=ovnet.use_bias, parameters=[p.copy() for p in ac.value_function.parameters])
    assert_array_equal(ac.value_function(states), fresh(states))
    assert not np.array_equal(ac.value_function.parameters[0], T.value_parameters(loop["value_net"][name], system["d"])[0])


def test_policy_improvement_raises_the_objective(sl):
    system, ovnet, opolicy, ac = T.make_actor_critic("pendulum", "notebook", sl)
    states, _ = T.make_states("pendulum", 100)
    before = sl.policy_improvement_step(ac, states, 1e-3)
    after = sl.policy_improvement_step(ac, states, None)
    print("J: %.15g -> %.15g" % (before, after))
    assert after > before


def test_supervised_value_step(sl):
    ovnet, vnet = T.make_value_network("notebook", 2, sl)
    states, _ = T.make_states("pendulum", 100)
    targets = -np.sum(states * states, axis=1)
    objective = sl.supervised_value_step(vnet, states, targets, 0.05)
    ref_objective, grad, comp = T.supervised_value_step(ovnet, states, targets, 0.05)
    assert objective == pytest.approx(ref_objective, rel=1e-12)
    _, g80, _ = T.supervised_value_step(T.make_value_network("notebook", 2)[0], states, targets, None, LONG)
    tol = 32 * UNIT * ratio_to_companion(grad, g80, comp)
    for p, r, a in zip(vnet.parameters, ovnet.parameters, comp):
        assert (np.abs(p - r) <= 0.05 * tol * a).all()
    assert sl.supervised_value_step(vnet, states, targets, None) < objective


# ---- errors ----------------------------------------------------------------------------------------------------------
def test_refusals_name_the_entry_point(sl):
    import torch
    system, _, _, ac = T.make_actor_critic("pendulum", "notebook", sl)
    ctx, vf = ac._ctx, ac.value_function
    states, actions = T.make_states("pendulum", 8)
    d_states, d_actions = torch.from_numpy(states).cuda(), torch.from_numpy(actions).cuda()
    out = [torch.zeros(k, dtype=torch.float64, device="cuda") for k in (8, 8, 2)]
    params = vf._device_parameters(ctx)
    dims, acts, has_bias = vf._description()

    def batch(dims=dims, acts=acts, has_bias=has_bias, n=8, context=ctx, reduction="mean"):
        context.critic_batch(dims, acts, has_bias, 1.0, params, n, d_states, d_actions, reduction, *out)

    with pytest.raises(sl.HipEngineError, match="sl_critic_batch.*sl_model_set"):
        batch()                                                             # the model not set
    ac.evaluate(states)
    batch()
    with pytest.raises(sl.HipEngineError, match="sl_critic_batch.*n = 0"):
        batch(n=0)
    with pytest.raises(sl.HipEngineError, match="sl_critic_batch.*width 65"):
        batch(dims=[2, 65, 64, 1])
    with pytest.raises(sl.HipEngineError, match="sl_critic_batch.*one output"):
        batch(dims=[2, 64, 64, 2])
    with pytest.raises(sl.HipEngineError, match="sl_critic_batch.*3 inputs"):
        batch(dims=[3, 64, 64, 1])
    with pytest.raises(sl.HipEngineError, match="sl_critic_batch.*5 layers"):
        batch(dims=[2, 4, 4, 4, 4, 1], acts=[2] * 5, has_bias=[0] * 5)
    # GP dynamics: unsupported, and the message names the call that serves them
    orl, rl = P.system_pair("pendulum", sl)
    rl.action_gradient(P.system_states("pendulum", 4)[0])
    with pytest.raises(sl.HipEngineError, match=r"sl_critic_batch failed \(-3\).*sl_action_gradient"):
        batch(context=rl._ctx)
    # sl_dense_param_grad
    coeff = torch.zeros(8, dtype=torch.float64, device="cuda")
    grad = torch.zeros(params.numel(), dtype=torch.float64, device="cuda")
    ctx.dense_param_grad(dims, acts, has_bias, 1.0, params, 8, 2, d_states, coeff, grad)
    with pytest.raises(sl.HipEngineError, match="sl_dense_param_grad.*n = 0"):
        ctx.dense_param_grad(dims, acts, has_bias, 1.0, params, 0, 2, d_states, coeff, grad)
    with pytest.raises(sl.HipEngineError, match="sl_dense_param_grad.*width 65"):
        ctx.dense_param_grad([2, 65, 1], [2, 0], [1, 0], 1.0, params, 8, 2, d_states, coeff, grad)
    with pytest.raises(sl.HipEngineError, match="sl_dense_param_grad.*3 columns"):
        ctx.dense_param_grad(dims, acts, has_bias, 1.0, params, 8, 3, d_states, coeff, grad)
    # the Python layer's own refusals
    with pytest.raises(TypeError, match="bare NeuralNetwork"):
        sl.ActorCritic(ac.policy, ac.dynamics, ac.reward_function, rl.value_function)
    with pytest.raises(TypeError, match="InvertedPendulum, CartPole or LinearSystem"):
        sl.ActorCritic(ac.policy, rl.dynamics, ac.reward_function, vf)
    with pytest.raises(ValueError, match="reduction"):
        ac.value_gradient(states, reduction="max")
