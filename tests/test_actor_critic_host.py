"""Host tests of the actor-critic path: the NumPy reference (tests/np_actor_critic.py) against torch autograd and
against itself in long double, the g++ build of safe_learning_amd/csrc/sl_critic.h against the reference bit for
bit, and the Python layer (``ActorCritic``, ``training.value_function_step``, ``training.supervised_value_step``)
on a stand-in engine."""

import ctypes as C
import subprocess
from fractions import Fraction

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import hostsim_build
import np_actor_critic as T
from np_policy_training import MAX_EXCLUDED, make_network
from oracle import np_functions as onp
from training_tolerance import ratio_to_companion

pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")


# ---- the emulated fused multiply-add ------------------------------------------------------------------------------
def test_fma64_is_the_exactly_rounded_fused_operation():
    rng = np.random.default_rng(0)
    a, b = rng.normal(size=4000), rng.normal(size=4000)
    c = -a * b * (1 + rng.normal(size=4000) * np.repeat([1e-17, 1e-9, 1.0, 1e9], 1000))     # heavy cancellation too
    a[:3], b[:3], c[:3] = [1 + 2.0 ** -30, 3.0, 0.0], [1 + 2.0 ** -30, 1 / 3, 0.0], [-1.0, -1.0, 0.0]
    got = T.fma64(a, b, c)
    for x, y, z, g in zip(a, b, c, got):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        assert g == float(exact), (x, y, z)                     # float(Fraction) rounds to nearest even, once


# ---- the header, compiled for the host ------------------------------------------------------------------------------
_DBL = C.POINTER(C.c_double)
_I32 = C.POINTER(C.c_int32)


def _p(a):
    return a.ctypes.data_as(_DBL)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("critic")
    exe = hostsim_build.program("critic.cpp", out, hostsim_build.SHIM_FLAGS)
    assert subprocess.run([exe], stdout=subprocess.PIPE, text=True).stdout.strip() == "critic: ok"
    return hostsim_build.shared("critic.cpp", out, hostsim_build.SHIM_FLAGS)


def test_shim_under_sanitizers(tmp_path_factory):
    exe = hostsim_build.sanitized_program_or_plain("critic.cpp", tmp_path_factory.mktemp("critic_san"),
                                                   hostsim_build.SHIM_FLAGS + ["-g"])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "critic: ok", run.stdout


def _descs(system):
    import safe_learning_amd as sl
    from safe_learning_amd import _hip
    dyn, reward = _hip.DynamicsDesc(), _hip.ValueDesc()
    dynamics, reward_function = T.make_dynamics(system, sl)
    if system["kind"] == "linear":
        dyn.kind = _hip.DYN_LINEAR
        for i, row in enumerate(system["matrix"]):
            for j, v in enumerate(row):
                dyn.matrix[i][j] = float(v)
    else:
        dynamics._write_dynamics(dyn)
    reward_function._write_value(reward)
    return dyn, reward


def _shim_dynamics(shim, system, states, actions):
    dyn, _ = _descs(system)
    n, d = states.shape
    m = actions.shape[1]
    nxt, jac = np.zeros((n, d)), np.zeros((n, d, m))
    assert shim.cr_dynamics(C.byref(dyn), d, m, C.c_int64(n), _p(states), _p(actions), _p(nxt), _p(jac)) == 0
    return nxt, jac


def _shim_batch(shim, system, vnet, states, actions, w):
    dyn, reward = _descs(system)
    n, d = states.shape
    m = actions.shape[1]
    dims = np.array([d] + list(vnet.layers), dtype=np.int32)
    codes = {None: 0, 'tanh': 1, 'relu': 2, 'sigmoid': 3}
    acts = np.array([codes[a] for a in vnet.nonlinearities], dtype=np.int32)
    nl = len(vnet.layers)
    has = np.array([int(vnet.use_bias and l < nl - 1) for l in range(nl)], dtype=np.int32)
    params = np.concatenate([p.ravel() for p in vnet.parameters])
    out = dict(next=np.zeros((n, d)), value=np.zeros(n), q=np.zeros(n), delta=np.zeros(n), coeff=np.zeros(n),
               dq_du=np.zeros((n, m)), g=np.zeros((n, d)))
    rc = shim.cr_batch(C.byref(dyn), C.byref(reward), C.c_double(system["gamma"]), nl, dims.ctypes.data_as(_I32),
                       acts.ctypes.data_as(_I32), has.ctypes.data_as(_I32), C.c_double(vnet.output_scale), _p(params),
                       d, m, C.c_int64(n), _p(states), _p(actions), C.c_double(w),
                       *[_p(out[k]) for k in ("next", "value", "q", "delta", "coeff", "dq_du", "g")])
    assert rc == 0
    return out


EULER = ("pendulum", "pendulum-plain", "cartpole", "cartpole-plain")


@pytest.mark.parametrize("name", EULER)
def test_euler_successor_and_tangent_bit_exact(shim, name):
    """With and without normalisation, friction 0 and > 0: x+ and dx+/du of the header are the reference's bits,
    and x+ is what the oracle's Euler model returns up to the difference between sl_sincos and libm."""
    system = T.SYSTEMS[name]
    states, actions = T.make_states(name, 300)
    states[0], actions[0] = 0.0, 0.0
    states[1] *= 3.0                                             # an angle beyond pi / 2: another quadrant
    nxt, jac = _shim_dynamics(shim, system, states, actions)
    ref_next, ref_jac, _ = T.dynamics_du(system, states, actions)
    assert_array_equal(nxt, ref_next)
    assert_array_equal(jac, ref_jac)
    if system["kind"] == "pendulum":
        model = onp.InvertedPendulum(system["mass"], system["length"], system["friction"], system["dt"],
                                     system["normalization"])
    else:
        model = onp.CartPole(system["pendulum_mass"], system["cart_mass"], system["length"], system["rot_friction"],
                             system["dt"], system["normalization"])
    np.testing.assert_allclose(nxt, model(states, actions), rtol=1e-12, atol=1e-14)


def test_linear_successor_and_columns_bit_exact(shim):
    for name in ("linear22", "linear41"):
        system = T.SYSTEMS[name]
        states, actions = T.make_states(name, 50)
        nxt, jac = _shim_dynamics(shim, system, states, actions)
        ref_next, ref_jac, _ = T.dynamics_du(system, states, actions)
        assert_array_equal(nxt, ref_next)
        assert_array_equal(jac, ref_jac)


@pytest.mark.parametrize("name", sorted(T.SYSTEMS))
@pytest.mark.parametrize("vkey", T.EXACT_NETS)
def test_per_sample_outputs_bit_exact(shim, name, vkey):
    """relu / linear value networks: every per-sample output of the header equals the reference bit for bit."""
    system = T.SYSTEMS[name]
    vnet, _ = T.make_value_network(vkey, system["d"])
    n = 64
    states, actions = T.make_states(name, n)
    states[0], actions[0] = 0.0, 0.0
    for reduction, w in (("mean", 1.0 / n), ("sum", 1.0)):
        got = _shim_batch(shim, system, vnet, states, actions, w)
        ref = T.critic_batch(system, vnet, states, actions, reduction)
        for key in ("next", "value", "q", "delta", "coeff", "dq_du", "g"):
            assert_array_equal(got[key], ref[key], err_msg=key)


@pytest.mark.parametrize("vkey", ("tanh", "mixed"))
def test_per_sample_outputs_of_smooth_networks(shim, vkey):
    """tanh and sigmoid are libm's on the host in both: the same bits unless NumPy's vector routines differ from
    libm's scalar ones, so these are compared within the tolerance rule."""
    system = T.SYSTEMS["cartpole"]
    vnet, _ = T.make_value_network(vkey, 4)
    states, actions = T.make_states("cartpole", 64)
    got = _shim_batch(shim, system, vnet, states, actions, 1.0)
    ref = T.critic_batch(system, vnet, states, actions, "sum")
    assert ratio_to_companion(got["dq_du"], ref["dq_du"], ref["A"]) <= 32 * 4
    np.testing.assert_allclose(got["value"], ref["value"], rtol=1e-13)
    np.testing.assert_allclose(got["q"], ref["q"], rtol=1e-13)


def test_zero_state_of_bias_free_relu_networks(shim):
    """Every pre-activation is exactly 0: relu passes no gradient, V(x) = q = 0 and sign(0) = 0."""
    for name in ("cartpole", "pendulum", "linear41"):
        system = T.SYSTEMS[name]
        vnet, _ = T.make_value_network("nobias", system["d"])
        states, actions = np.zeros((2, system["d"])), np.zeros((2, system["m"]))
        for out in (_shim_batch(shim, system, vnet, states, actions, 0.5), T.critic_batch(system, vnet, states, actions)):
            assert_array_equal(out["g"], 0.0)
            assert_array_equal(out["coeff"], 0.0)
            assert_array_equal(out["value"], 0.0)
            assert_array_equal(out["q"], 0.0)
            assert_array_equal(out["dq_du"], 0.0)


# ---- the reference against torch autograd ---------------------------------------------------------------------------
def _torch_dynamics(system, x, u):
    import torch
    if system["kind"] == "linear":
        return torch.cat((x, u), dim=1) @ torch.tensor(system["matrix"]).T
    coef, tx, tu, tx_inv = T.dynamics_coefficients(system)
    cols = [x[:, k] for k in range(x.shape[1])]
    act = u[:, 0]
    if tx is not None:
        cols, act = [c * t for c, t in zip(cols, tx)], act * tu[0]
    dt = coef[0]
    for _ in range(10):
        if system["kind"] == "pendulum":
            th, om = cols
            acc = coef[1] * torch.sin(th) + act / coef[2] - (coef[3] * om if coef[4] else 0.0)
            cols = [th + dt * om, om + dt * acc]
        else:
            px, th, v, om = cols
            m, M, L, b = coef[1:5]
            s, c = torch.sin(th), torch.cos(th)
            det = L * (M + m * s * s)
            vd = (act - coef[5] * om * om * s - b * om * c + coef[6] * torch.sin(2 * th)) * L / det
            wd = (act * c - coef[7] * om * om * torch.sin(2 * th) - coef[8] * om / coef[5] + coef[9] * s) / det
            cols = [px + dt * v, th + dt * om, v + dt * vd, om + dt * wd]
    if tx is not None:
        cols = [c * t for c, t in zip(cols, tx_inv)]
    return torch.stack(cols, dim=1)


def _torch_net(net, params, x):
    import torch
    acts = {None: lambda v: v, 'tanh': torch.tanh, 'relu': torch.relu, 'sigmoid': torch.sigmoid}
    it = iter(params)
    nl = len(net.layers)
    for l, name in enumerate(net.nonlinearities):
        x = x @ next(it)
        if net.use_bias and l < nl - 1:
            x = x + next(it)
        x = acts[name](x)
    return x * net.output_scale


def _torch_objectives(system, vnet, policy, states, detach):
    import torch
    vp = [torch.tensor(p, requires_grad=True) for p in vnet.parameters]
    pp = [torch.tensor(p, requires_grad=True) for p in policy.parameters]
    x = torch.tensor(states)
    u = _torch_net(policy, pp, x)
    z = torch.cat((x, u), dim=1)
    r = torch.einsum("ni,ij,nj->n", z, torch.tensor(system["reward"]), z)
    q = r + system["gamma"] * _torch_net(vnet, vp, _torch_dynamics(system, x, u))[:, 0]
    target = q.detach() if detach else q
    value_objective = (_torch_net(vnet, vp, x)[:, 0] - target).abs().mean()
    return vp, pp, value_objective, q.mean()


@pytest.mark.parametrize("name,vkey", [("pendulum", "notebook"), ("pendulum-plain", "mixed"), ("cartpole", "nobias"),
                                       ("cartpole-plain", "tanh"), ("linear22", "scaled"), ("linear41", "mixed")])
def test_reference_matches_torch_autograd(name, vkey):
    """Critic: the target detached; actor: the chain through the dynamics and the value network attached."""
    import torch
    system = T.SYSTEMS[name]
    vnet, _ = T.make_value_network(vkey, system["d"])
    policy, _ = make_network(system["policy"])
    states, _ = T.make_states(name, 120)
    vp, pp, value_objective, policy_objective = _torch_objectives(system, vnet, policy, states, detach=True)
    u = T.policy_actions(policy, states)
    objective, grad, comp, _ = T.value_gradient(system, vnet, states, u)
    assert objective == pytest.approx(float(value_objective.detach()), rel=1e-12)
    for g, t, a in zip(grad, torch.autograd.grad(value_objective, vp), comp):
        assert np.all(np.abs(g - t.numpy()) <= 1e-11 * a + 1e-300)
    objective, grad, comp = T.policy_gradient(system, vnet, policy, states)
    assert objective == pytest.approx(float(policy_objective.detach()), rel=1e-12)
    for g, t, a in zip(grad, torch.autograd.grad(policy_objective, pp), comp):
        assert np.all(np.abs(g - t.numpy()) <= 1e-10 * a + 1e-300)


def test_stop_gradient_is_real():
    """Without the detach the critic's gradient is another one: gamma V(x+) would be pulled towards V(x) as well."""
    import torch
    system = T.SYSTEMS["pendulum"]
    vnet, _ = T.make_value_network("notebook", 2)
    policy, _ = make_network(system["policy"])
    states, _ = T.make_states("pendulum", 120)
    vp, _, attached_objective, _ = _torch_objectives(system, vnet, policy, states, detach=False)
    attached = torch.autograd.grad(attached_objective, vp)
    _, grad, comp, _ = T.value_gradient(system, vnet, states, T.policy_actions(policy, states))
    worst = max(float(np.max(np.abs(g - t.numpy()) / np.maximum(a, 1e-300))) for g, t, a in zip(grad, attached, comp))
    assert worst > 1e-3


# ---- the reference against itself in long double --------------------------------------------------------------------
def _recorded_keys():
    return sorted(T.REFERENCE_RATIO, key=repr)


def test_reference_ratio_table_is_filled():
    kinds = {key[0] for key in T.REFERENCE_RATIO}
    assert kinds == {"batch", "delta", "sums", "value", "steps-value", "steps-both"}
    for pair in T.PAIRS:
        assert ("batch",) + pair in T.REFERENCE_RATIO and ("delta",) + pair in T.REFERENCE_RATIO


@pytest.mark.parametrize("key", _recorded_keys(), ids=repr)
def test_reference_error_stays_below_the_recorded_figure(key):
    measured = T.measure_reference_ratio(key)
    assert 0 < measured <= T.REFERENCE_RATIO[key], (key, measured)


@pytest.mark.parametrize("name", sorted(T.SYSTEMS))
def test_excluded_share(name):
    """The reference alone: at most MAX_EXCLUDED of a batch of n >= 100 lies at a kink."""
    system = T.SYSTEMS[name]
    for vkey in sorted(T.VALUE_NETS):
        vnet, _ = T.make_value_network(vkey, system["d"])
        for n in (100, 1000):
            states, actions = T.make_states(name, n)
            assert 1.0 - T.comparable(system, vnet, states, actions).mean() <= MAX_EXCLUDED, (vkey, n)
    if name in T.STEP_LOOP["value_net"]:
        vnet, _ = T.make_value_network(T.STEP_LOOP["value_net"][name], system["d"])
        policy, _ = make_network(system["policy"])
        assert len(T.step_states(name, vnet, policy)) >= 98


# ---- the Python layer without a GPU ---------------------------------------------------------------------------------
class _FakeEngine(object):
    """Stands in for a context: every call answered by the NumPy reference."""

    def __init__(self):
        import torch
        self.torch_device, self.calls = torch.device("cpu"), []
        self.system = self.policy_net = None

    @staticmethod
    def _network(dims, acts, has_bias, scale, flat):
        names = {0: None, 1: 'tanh', 2: 'relu', 3: 'sigmoid'}
        params, off = [], 0
        for l in range(len(acts)):
            count = dims[l] * dims[l + 1]
            params.append(np.array(flat[off:off + count]).reshape(dims[l], dims[l + 1]))
            off += count
            if has_bias[l]:
                params.append(np.array(flat[off:off + dims[l + 1]]))
                off += dims[l + 1]
        assert all(has_bias[:-1]) == any(has_bias[:-1]) and not has_bias[-1]
        return onp.NeuralNetwork(list(dims[1:]), [names[int(a)] for a in acts], output_scale=scale,
                                 use_bias=bool(any(has_bias)), parameters=params)

    def model_set(self, desc):
        self.calls.append("model_set")

    def policy_network_set(self, dims, acts, kernels, biases, scale):
        self.calls.append("policy_network_set")
        flat = []
        for k, b in zip(kernels, biases):
            flat += list(np.ravel(k)) + ([] if b is None else list(np.ravel(b)))
        self.policy_net = self._network(list(dims), list(acts), [b is not None for b in biases], scale, flat)

    def eval_points(self, what, n, d_points, d_out):
        import torch
        self.calls.append("eval_points")
        d_out.copy_(torch.from_numpy(T.policy_actions(self.policy_net, d_points.numpy())))

    def policy_param_grad(self, n, d, d_points, d_coeff, d_out):
        import torch
        self.calls.append("policy_param_grad")
        grad, _ = T.network_parameter_gradient(self.policy_net, d_points.numpy(), d_coeff.numpy())
        d_out.copy_(torch.from_numpy(np.concatenate([g.ravel() for g in grad])))

    def critic_batch(self, dims, acts, has_bias, scale, d_params, n, d_states, d_actions, reduction, d_value, d_q,
                     d_sums, d_next=None, d_dq_du=None, d_coeff=None):
        import torch
        self.calls.append(("critic_batch", n, reduction, d_dq_du is not None))
        vnet = self._network(dims, acts, has_bias, scale, d_params.numpy())
        b = T.critic_batch(self.system, vnet, d_states.numpy(), d_actions.numpy(), reduction)
        for tensor, key in ((d_value, "value"), (d_q, "q"), (d_sums, "sums"), (d_next, "next"), (d_dq_du, "dq_du"),
                            (d_coeff, "coeff")):
            if tensor is not None:
                tensor.copy_(torch.from_numpy(np.ascontiguousarray(b[key])))

    def dense_param_grad(self, dims, acts, has_bias, scale, d_params, n, d, d_points, d_coeff, d_out):
        import torch
        self.calls.append(("dense_param_grad", n, d))
        vnet = self._network(dims, acts, has_bias, scale, d_params.numpy())
        grad, _ = T.network_parameter_gradient(vnet, d_points.numpy(), d_coeff.numpy().reshape(n, -1))
        d_out.copy_(torch.from_numpy(np.concatenate([g.ravel() for g in grad])))


@pytest.fixture
def fake_engine(monkeypatch):
    import copy
    from safe_learning_amd import _evaluate, _hip
    from safe_learning_amd import functions as F
    from safe_learning_amd._model import ModelBuilder
    engine = _FakeEngine()
    builder = ModelBuilder(engine, None)

    def _builder(d):
        builder.grid = copy.copy(F.GridWorld([[0., 1.]] * d, 2))
        return engine, builder
    monkeypatch.setattr(_evaluate, "_builder", _builder)
    monkeypatch.setattr(_evaluate, "_ctx", lambda: engine)
    monkeypatch.setattr(_hip, "Context", lambda: engine)
    return engine


@pytest.mark.parametrize("name,vkey", [("pendulum", "notebook"), ("cartpole", "nobias"), ("linear22", "scaled")])
def test_python_layer(fake_engine, name, vkey):
    import safe_learning_amd as sl
    system, ovnet, opolicy, ac = T.make_actor_critic(name, vkey, sl)
    fake_engine.system = system
    d, m = system["d"], system["m"]
    states, actions = T.make_states(name, 40)
    ev = ac.evaluate(states)
    ref = T.critic_batch(system, ovnet, states, T.policy_actions(opolicy, states))
    assert ev.actions.shape == (40, m) and ev.next_states.shape == (40, d) and ev.action_gradient.shape == (40, m)
    assert ev.values.shape == ev.future_values.shape == ev.td_error.shape == (40, 1)
    assert_array_equal(ev.values[:, 0], ref["value"])
    assert_array_equal(ev.td_error[:, 0], ref["delta"])
    assert_array_equal(ev.action_gradient, ref["dq_du"])
    assert_array_equal(ac.future_values(states, actions=actions)[:, 0],
                       T.critic_batch(system, ovnet, states, actions)["q"])
    assert ac.future_values(states, actions=actions[:1]).shape == (40, 1)          # one action row for every state
    import torch
    assert isinstance(ac.evaluate(torch.from_numpy(states)).values, torch.Tensor)  # tensors in, tensors out
    # the two gradients, both reductions
    for reduction in ("mean", "sum"):
        objective, grad = ac.value_gradient(states, reduction)
        ref_objective, ref_grad, _, _ = T.value_gradient(system, ovnet, states, T.policy_actions(opolicy, states),
                                                         reduction)
        assert objective == float(ref_objective)
        assert [g.shape for g in grad] == [p.shape for p in ac.value_function.parameters]
        for g, r in zip(grad, ref_grad):
            assert_array_equal(g, r)
        objective, grad = ac.policy_gradient(states, reduction)
        ref_objective, ref_grad, _ = T.policy_gradient(system, ovnet, opolicy, states, reduction)
        assert objective == pytest.approx(float(ref_objective), rel=1e-15)
        for g, r in zip(grad, ref_grad):
            assert_array_equal(g, r)
    # steps: the unscaled objective before the step, learning_rate=None only evaluates, the version moves
    before = [p.copy() for p in ac.value_function.parameters]
    version = ac.value_function._version
    objective = sl.value_function_step(ac, states, None, scaling=3.0)
    assert ac.value_function._version == version
    assert sl.value_function_step(ac, states, 0.05, scaling=3.0) == objective
    assert ac.value_function._version != version
    ref_objective, ref_grad, _ = T.value_function_step(system, ovnet, opolicy, states, 0.05, scaling=3.0)
    assert objective == ref_objective
    for p, b, r, g in zip(ac.value_function.parameters, before, ovnet.parameters, ref_grad):
        assert_array_equal(p, r)
        assert_array_equal(p, b - (0.05 * 3.0) * g)
    # ... the next batch sees the new weights (the device copy follows the version)
    assert_array_equal(ac.evaluate(states).values[:, 0],
                       T.critic_batch(system, ovnet, states, T.policy_actions(opolicy, states))["value"])
    # policy=: another policy than ac.policy
    other = sl.Saturation(sl.NeuralNetwork(opolicy.layers, opolicy.nonlinearities, output_scale=opolicy.output_scale,
                                           use_bias=opolicy.use_bias,
                                           parameters=[0.5 * p for p in opolicy.parameters]), -10.0, 10.0)
    half, _ = make_network(system["policy"])
    half.parameters = [0.5 * p for p in half.parameters]
    assert sl.value_function_step(ac, states, None, policy=other) == \
        T.value_function_step(system, ovnet, half, states, None)[0]
    # the actor's step through training.policy_improvement_step, unchanged
    version = ac.policy._version
    objective = sl.policy_improvement_step(ac, states, 0.02)
    ref_objective, _, _ = T.policy_improvement_step(system, ovnet, opolicy, states, 0.02)
    assert objective == pytest.approx(ref_objective, rel=1e-15) and ac.policy._version != version
    for p, r in zip(ac.policy.parameters, opolicy.parameters):
        assert_array_equal(p, r)


def test_supervised_value_step(fake_engine):
    import safe_learning_amd as sl
    ovnet, vnet = T.make_value_network("notebook", 2, sl)
    states, _ = T.make_states("pendulum", 50)
    targets = -np.sum(states * states, axis=1)
    assert sl.supervised_value_step(vnet, states, targets, None) == \
        pytest.approx(T.supervised_value_step(ovnet, states, targets, None)[0], rel=1e-15)
    version = vnet._version
    objective = sl.supervised_value_step(vnet, states, targets, 0.1)
    assert objective == pytest.approx(T.supervised_value_step(ovnet, states, targets, 0.1)[0], rel=1e-15)
    assert vnet._version != version
    for p, r in zip(vnet.parameters, ovnet.parameters):
        assert_array_equal(p, r)
    with pytest.raises(ValueError):
        sl.supervised_value_step(vnet, states, targets[:-1], 0.1)
    with pytest.raises(TypeError):
        sl.supervised_value_step(-vnet, states, targets, 0.1)
    with pytest.raises(ValueError):
        sl.supervised_value_step(make_network("wide", sl)[1], states, targets, 0.1)


def test_refusals(fake_engine, monkeypatch):
    import safe_learning_amd as sl
    system = T.SYSTEMS["pendulum"]
    _, vnet = T.make_value_network("notebook", 2, sl)
    _, policy = make_network("notebook", sl)
    dyn, reward = T.make_dynamics(system, sl)
    grid = sl.GridWorld([[-1., 1.]] * 2, 5)
    with pytest.raises(TypeError):
        sl.ActorCritic(policy, dyn, reward, sl.Triangulation(grid, np.zeros((25, 1))))
    with pytest.raises(TypeError):
        sl.ActorCritic(policy, dyn, reward, -vnet)
    with pytest.raises(ValueError):
        sl.ActorCritic(policy, dyn, reward, make_network("wide", sl)[1])                 # two outputs
    with pytest.raises(ValueError):
        sl.ActorCritic(policy, dyn, reward, T.make_value_network("notebook", 4, sl)[1])  # four inputs
    with pytest.raises(TypeError):
        sl.ActorCritic(policy, sl.QuadraticFunction(np.eye(3)), reward, vnet)
    with pytest.raises(TypeError):
        sl.ActorCritic(policy, dyn, sl.LinearSystem((np.eye(3),)), vnet)
    with pytest.raises(ValueError):
        sl.ActorCritic(policy, dyn, sl.QuadraticFunction(np.eye(2)), vnet)
    with pytest.raises(ValueError):
        sl.ActorCritic(policy, dyn, reward, sl.NeuralNetwork([65, 1], ['relu', None], input_dim=2))
    ac = sl.ActorCritic(policy, dyn, reward, vnet)
    fake_engine.system = system
    states, _ = T.make_states("pendulum", 10)
    with pytest.raises(ValueError):
        ac.value_gradient(states, reduction="max")
    with pytest.raises(ValueError):
        ac.policy_gradient(states, reduction="max")
    with pytest.raises(ValueError):
        ac.evaluate(np.zeros((3, 3)))
    with pytest.raises(ValueError):
        ac.evaluate(states, actions=np.zeros((3, 1)))
    with pytest.raises(ValueError):
        ac.evaluate(states, actions=np.zeros((10, 2)))
    with pytest.raises(TypeError):
        ac.evaluate(states, policy=np.zeros((10, 1)))
    with pytest.raises(TypeError):
        sl.ActorCritic(sl.Saturation(policy, -1., 1.), dyn, reward, vnet).policy_gradient(states)
    from safe_learning_amd import distributed
    monkeypatch.setattr(distributed, "rank_and_world", lambda: (0, 2))
    with pytest.raises(NotImplementedError):
        sl.ActorCritic(policy, dyn, reward, vnet)


def test_package_exports():
    import safe_learning_amd as sl
    from safe_learning_amd import actor_critic, training
    assert sl.ActorCritic is actor_critic.ActorCritic
    assert sl.value_function_step is training.value_function_step
    assert sl.supervised_value_step is training.supervised_value_step
