"""The safe policy update on the GPU (needs an MI355X): sl_decrease_gradient, Lyapunov.decrease_gradient,
PolicyIteration.action_gradient / policy_gradient(..., lyapunov=) and training.policy_improvement_step(...,
lyapunov=), against the NumPy reference of tests/np_safe_policy_training.py (itself checked against central
differences of the oracle, torch autograd and long double by tests/test_safe_policy_training_host.py).
Results are compared as |got - ref| <= tolerance * A with A the reference's error companion and tolerance 32
times the reference's own measured error; every test prints the ratio it measured before it asserts."""

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import guarded
import np_policy_training as T
import np_safe_policy_training as S

pytestmark = pytest.mark.gpu

UNIT = S.UNIT
POLICY_OF = {"pendulum": "notebook", "cartpole": "ragged", "two": "wide", "rbf": "notebook", "ragged": "notebook"}
SIZES = (1, 15, 16, 17, 1000)


@pytest.fixture(scope="module")
def sl():
    import safe_learning_amd
    return safe_learning_amd


_objects = {}


def _setup(sl, key):
    """-> dict(case, odynamics, safe, dynamics, policy, lyap) of one configuration; the product's dynamics and
    policy are shared by the configurations of a system (their uploads too)."""
    system, n_gp, v_kind, lv_kind = key
    base = (system, n_gp)
    if base not in _objects:
        case = S._case(system, n_gp)
        _objects[base] = dict(case=case, odynamics=S._oracle_dynamics(case), dynamics=S.product_dynamics(sl, case),
                              policy=T.make_network(POLICY_OF[system], sl)[1])
    if key not in _objects:
        shared = _objects[base]
        safe = S.safe_spec(shared["case"], v_kind, lv_kind)
        _objects[key] = dict(shared, safe=safe, lyap=S.product_lyapunov(sl, shared["case"], safe, shared["dynamics"],
                                                                        shared["policy"]))
    return _objects[key]


def _ids(key):
    return "-".join(str(v) for v in key)


# ---- sl_decrease_gradient through Lyapunov.decrease_gradient ------------------------------
@pytest.mark.parametrize("key", S.GPU_KEYS, ids=_ids)
def test_decrease_gradient_matches_reference(sl, key):
    import torch
    from safe_learning_amd import _evaluate, _hip
    o = _setup(sl, key)
    lyap, tol_grad, tol_c = o["lyap"], *S.tolerance(key)
    for n in SIZES:
        states, actions = S.states_of(key[0], n)
        ok = S.comparable(o["odynamics"], o["safe"], states, actions)
        assert 1 - ok.mean() <= S.MAX_EXCLUDED or n < 100
        ref = S.constraint_terms(o["odynamics"], o["safe"], states, actions)
        grad, c = lyap.decrease_gradient(states, actions)
        assert grad.shape == ref["grad"].shape and c.shape == (n, 1)
        ratio = T.ratio_to_companion(grad, ref["grad"], ref["A"], ok)
        ratio_c = T.ratio_to_companion(c[:, 0], ref["c"], ref["A_c"], ok)
        print("%s, n = %d: dC/du %.3f (tolerance %.1f), C %.3f (tolerance %.1f) x 2^-53 of A, %.4f left out"
              % (key, n, ratio, tol_grad / UNIT, ratio_c, tol_c / UNIT, 1 - ok.mean()))
        assert ratio * UNIT <= tol_grad and ratio_c * UNIT <= tol_c
        if n != 1000:
            continue
        assert (ref["A"][ok] > 0).all() and (ref["A_c"][ok] > 0).all()
        # tensors in, tensors out, the same bits
        d_states, d_actions = torch.from_numpy(states).cuda(), torch.from_numpy(actions).cuda()
        d_grad, d_c = lyap.decrease_gradient(d_states, d_actions)
        assert d_grad.is_cuda and d_c.is_cuda
        assert_array_equal(d_grad.cpu().numpy(), grad)
        assert_array_equal(d_c.cpu().numpy(), c)
        # actions=None: the policy, evaluated once - the same bits as its actions given explicitly
        u = _evaluate.policy(lyap.policy, d_states)
        by_policy = lyap.decrease_gradient(d_states)
        explicit = lyap.decrease_gradient(d_states, u)
        assert_array_equal(by_policy[0].cpu().numpy(), explicit[0].cpu().numpy())
        assert_array_equal(by_policy[1].cpu().numpy(), explicit[1].cpu().numpy())
        # d_terms against sl_eval_points(SL_EVAL_DECREASE), which evaluates the policy itself
        d = states.shape[1]
        lyap._upload_model()
        terms = torch.empty((n, 2 + 2 * d), dtype=torch.float64, device="cuda")
        g2 = torch.empty_like(by_policy[0])
        lyap._ctx.decrease_gradient(n, d_states, None, g2, None, terms)
        record = torch.empty_like(terms)
        lyap._ctx.eval_points(_hip.EVAL_DECREASE, n, d_states, record)
        assert_array_equal(g2.cpu().numpy(), by_policy[0].cpu().numpy())
        terms, record = terms.cpu().numpy(), record.cpu().numpy()
        assert_array_equal(terms[:, 0] - terms[:, 1], by_policy[1].cpu().numpy()[:, 0])
        at_policy = S.constraint_terms(o["odynamics"], o["safe"], states, u.cpu().numpy())
        ok_p = S.comparable(o["odynamics"], o["safe"], states, u.cpu().numpy())
        assert 1 - ok_p.mean() <= S.MAX_EXCLUDED
        companions = np.hstack((at_policy["A_c"][:, None], at_policy["A_c"][:, None], at_policy["A_mean"],
                                at_policy["A_e"] + at_policy["error"]))
        worst = T.ratio_to_companion(terms, record, companions, ok_p)
        print("%s: d_terms vs SL_EVAL_DECREASE %.3f x 2^-53 of A (tolerance %.1f)" % (key, worst, tol_c / UNIT))
        assert worst * UNIT <= tol_c


# ---- determinism and bounds ------------------------------
@pytest.mark.parametrize("key", [("pendulum", None, "negtable", "abs_grad"), ("rbf", 300, "quadratic", "abs_linear"),
                                 ("two", None, "quadratic", "abs_linear")], ids=_ids)
def test_entry_point_is_deterministic_and_stays_in_bounds(sl, key):
    import torch
    o = _setup(sl, key)
    lyap = o["lyap"]
    n = 1000
    states, actions = S.states_of(key[0], n)
    d, m = states.shape[1], actions.shape[1]
    d_states, d_actions = torch.from_numpy(states).cuda(), torch.from_numpy(actions).cuda()
    lyap._upload_model()
    sizes = [n * m, n, n * (2 + 2 * d)]
    for acts in (d_actions, None):
        first = guarded.run(lambda g, c, t: lyap._ctx.decrease_gradient(n, d_states, acts, g, c, t), sizes)
        again = guarded.run(lambda g, c, t: lyap._ctx.decrease_gradient(n, d_states, acts, g, c, t), sizes)
        for a, b in zip(first, again):
            assert_array_equal(a, b)
        # 1000 points in one call = 992 + 8 points in two
        head = guarded.run(lambda g, c, t: lyap._ctx.decrease_gradient(
            992, d_states[:992], None if acts is None else acts[:992], g, c, t), [992 * m, 992, 992 * (2 + 2 * d)])
        tail = guarded.run(lambda g, c, t: lyap._ctx.decrease_gradient(
            8, d_states[992:].contiguous(), None if acts is None else acts[992:].contiguous(), g, c, t),
            [8 * m, 8, 8 * (2 + 2 * d)])
        for whole, a, b in zip(first, head, tail):
            assert_array_equal(whole, np.concatenate((a, b)))


# ---- policy_gradient and policy_improvement_step ------------------------------
def _pair_with(sl, policy_kind):
    """-> (oracle PolicyIteration, product PolicyIteration, case) of the notebook-kernel pendulum with a
    NeuralNetwork policy ('network') or a 7 x 7 Triangulation policy ('table')."""
    import oracle
    orl, rl = T.system_pair("pendulum", sl)
    case = S._case("pendulum")
    if policy_kind == "table":
        ogrid = oracle.GridWorld(case["limits"], 7)
        pts = ogrid.all_points
        values = (0.4 * np.sin(2.0 * pts[:, 0]) - 0.3 * pts[:, 1] + 0.1 * pts[:, 0] * pts[:, 1])[:, None]
        orl.policy = oracle.Triangulation(ogrid, values)
        rl.policy = sl.Triangulation(sl.GridWorld(case["limits"], 7), values.copy())
    return orl, rl, case


def _comparable_through_policy(orl, safe, states):
    import exclusions
    u = T.policy_actions(orl.policy, states)
    ok = T.comparable(orl, states, u, through_policy=True) & S.comparable(orl.dynamics, safe, states, u)
    if not hasattr(orl.policy, "layers"):
        ok &= ~exclusions.ambiguous_points(orl.policy, states)
    return ok


@pytest.mark.parametrize("v_lv", [("quadratic", "abs_linear"), ("negtable", "abs_grad")], ids="-".join)
@pytest.mark.parametrize("policy_kind", ["network", "table"])
def test_policy_gradient_matches_reference(sl, policy_kind, v_lv):
    orl, rl, case = _pair_with(sl, policy_kind)
    safe = S.safe_spec(case, *v_lv)
    lyap = S.product_lyapunov(sl, case, safe, rl.dynamics, rl.policy)
    states, _ = S.states_of("pendulum", 1000)
    ok = _comparable_through_policy(orl, safe, states)
    assert 1 - ok.mean() <= S.MAX_EXCLUDED
    states = states[ok]
    plain = {r: rl.policy_gradient(states, r) for r in ("mean", "sum")}
    for reduction in ("mean", "sum"):
        for lam in (0, 1, 10):
            objective, gradient = rl.policy_gradient(states, reduction, lyapunov=lyap, lagrange_multiplier=lam)
            if lam == 0:
                # the unpenalised result bit for bit
                assert objective == plain[reduction][0]
                for g, p in zip(T._as_list(gradient), T._as_list(plain[reduction][1])):
                    assert_array_equal(g, p)
                continue
            ref_objective, ref, comp = S.safe_policy_gradient(orl, safe, states, reduction, lam)
            _, ref80, _ = S.safe_policy_gradient(orl, safe, states, reduction, lam, S.LONG)
            own = T.ratio_to_companion(ref, ref80, comp)
            ratio = T.ratio_to_companion(gradient, ref, comp)
            print("%s policy, %s, %s, lambda = %g: %.3f x 2^-53 of A (reference vs long double %.3f: tolerance %.2f), "
                  "objective %.12g" % (policy_kind, "-".join(v_lv), reduction, lam, ratio, own, 32 * own, objective))
            assert ratio * UNIT <= 32 * own * UNIT
            assert objective == pytest.approx(float(ref_objective), rel=1e-10)
            assert any((g != p).any() for g, p in zip(T._as_list(gradient), T._as_list(plain[reduction][1])))


def test_safe_notebook_shape_steps(sl):
    """Five safe 'mean' steps, lr 0.1, lambda 1, on 1000 sampled states of the notebook-kernel pendulum with the
    notebook's Lyapunov function -V (a negated table) and L_v = |gradient|: the parameters track the reference step
    by step, and the safe set of the Lyapunov object follows the new parameters."""
    orl, rl, case = _pair_with(sl, "network")
    safe = S.safe_spec(case, "negtable", "abs_grad")
    lyap = S.product_lyapunov(sl, case, safe, rl.dynamics, rl.policy)
    states, _ = S.states_of("pendulum", 1000)
    ok = _comparable_through_policy(orl, safe, states)
    assert 1 - ok.mean() <= S.MAX_EXCLUDED
    states = states[ok]
    lr, lam = 0.1, 1.0
    allowed = [np.zeros_like(p) for p in orl.policy.parameters]
    for step in range(5):
        assert 1 - _comparable_through_policy(orl, safe, states).mean() <= S.MAX_EXCLUDED
        _, g64, comp = S.safe_policy_gradient(orl, safe, states, "mean", lam)
        _, g80, _ = S.safe_policy_gradient(orl, safe, states, "mean", lam, S.LONG)
        own = T.ratio_to_companion(g64, g80, comp)
        objective = sl.policy_improvement_step(rl, states, lr, reduction='mean', lyapunov=lyap, lagrange_multiplier=lam)
        ref_objective, ref, comp = S.safe_policy_improvement_step(orl, safe, states, lr, 'mean', lam)
        # the parameters may be apart by the accumulated tolerance of the gradients so far
        allowed = [a + lr * 32 * own * UNIT * c for a, c in zip(allowed, comp)]
        worst = max(float((np.abs(p - r) / np.where(a > 0, a, 1.0)).max())
                    for p, r, a in zip(rl.policy.parameters, orl.policy.parameters, allowed))
        print("step %d: objective %.15g (reference %.15g), reference vs long double %.3f, parameters within %.3f of the "
              "accumulated tolerance" % (step, objective, ref_objective, own, worst))
        assert objective == pytest.approx(ref_objective, rel=1e-10)
        for p, r, a in zip(rl.policy.parameters, orl.policy.parameters, allowed):
            assert (np.abs(p - r) <= a).all()
    assert not np.array_equal(rl.policy.parameters[0], T.network_parameters("notebook")[0])
    # the Lyapunov object shares the policy: its safe set is that of a fresh object with the final parameters
    fresh_policy = sl.NeuralNetwork(rl.policy.layers, rl.policy.nonlinearities, output_scale=rl.policy.output_scale,
                                    use_bias=rl.policy.use_bias, parameters=[p.copy() for p in rl.policy.parameters])
    fresh = S.product_lyapunov(sl, case, safe, rl.dynamics, fresh_policy)
    for obj in (lyap, fresh):
        obj.initial_safe_set = np.array([obj.discretization.nindex // 2])
        obj.update_safe_set()
    assert_array_equal(lyap.safe_set, fresh.safe_set)
    assert lyap.c_max == fresh.c_max
    assert_array_equal(lyap.decrease_gradient(states)[0], fresh.decrease_gradient(states)[0])


# ---- data updates ------------------------------
def test_gradient_follows_new_data(sl):
    case = S._case("rbf", 63)
    states, actions = S.states_of("rbf", 200)
    rng = np.random.default_rng(4)
    x_new, y_new = rng.uniform(-1, 1, (1, 3)), rng.uniform(-0.5, 0.5, (1, 2))

    def build(with_point):
        dynamics = S.product_dynamics(sl, case)
        safe = S.safe_spec(case)
        lyap = S.product_lyapunov(sl, case, safe, dynamics, T.make_network("notebook", sl)[1])
        return dynamics, lyap

    dynamics, lyap = build(False)
    before = lyap.decrease_gradient(states, actions)
    dynamics.add_data_point(x_new, y_new)                      # 64 points: the row block's last row
    after = lyap.decrease_gradient(states, actions)
    assert (after[0] != before[0]).any()
    other, fresh = build(False)
    other.add_data_point(x_new, y_new)
    want = fresh.decrease_gradient(states, actions)
    assert_array_equal(after[0], want[0])
    assert_array_equal(after[1], want[1])
    dynamics.add_data_point(x_new + 0.1, y_new)                # 65 points: a new row block
    other.add_data_point(x_new + 0.1, y_new)
    again, want = lyap.decrease_gradient(states, actions), S.product_lyapunov(
        sl, case, S.safe_spec(case), other, lyap.policy).decrease_gradient(states, actions)
    assert_array_equal(again[0], want[0])
    assert_array_equal(again[1], want[1])


# ---- errors ------------------------------
def test_documented_errors_leave_the_model_alone(sl):
    import cases
    import torch
    from safe_learning_amd import _hip
    from safe_learning_amd.benchmarks import build_specs, network_weights
    orl, rl, case = _pair_with(sl, "network")
    safe = S.safe_spec(case, "negtable", "abs_grad")
    lyap = S.product_lyapunov(sl, case, safe, rl.dynamics, rl.policy)
    states, actions = S.states_of("pendulum", 50)
    before = lyap.decrease_gradient(states, actions)
    params = [p.copy() for p in rl.policy.parameters]
    table = lyap.lyapunov_function.parameters.copy()

    def unchanged():
        for p, b in zip(rl.policy.parameters, params):
            assert_array_equal(p, b)
        assert_array_equal(lyap.lyapunov_function.parameters, table)
        after = lyap.decrease_gradient(states, actions)
        assert_array_equal(after[0], before[0])
        assert_array_equal(after[1], before[1])

    # a LyapunovNetwork as V_L
    network = sl.LyapunovNetwork(2, [4, 8], ['tanh', 'tanh'], 1e-8, network_weights(2, [4, 8]))
    lyap_net = sl.Lyapunov(lyap.discretization, network, rl.dynamics, safe["lf"],
                           sl.Norm1Function(sl.Gradient(network)), safe["tau"], rl.policy)
    with pytest.raises(TypeError, match="LyapunovNetwork"):
        lyap_net.decrease_gradient(states, actions)
    with pytest.raises(TypeError, match="LyapunovNetwork"):
        rl.policy_gradient(states, lyapunov=lyap_net)
    lyap_net._upload_model()
    d_states, d_actions = torch.from_numpy(states).cuda(), torch.from_numpy(actions).cuda()
    out = torch.empty((50, 1), dtype=torch.float64, device="cuda")
    with pytest.raises(_hip.HipEngineError, match="SL_V_NETWORK"):
        lyap_net._ctx.decrease_gradient(50, d_states, d_actions, out)
    unchanged()
    # Euler dynamics
    _, euler, _, _ = build_specs(cases.make_case("pendulum", num_points=17, dynamics="analytic"))
    lyap_euler = sl.Lyapunov(lyap.discretization, sl.QuadraticFunction(case["P"]), euler, safe["lf"], 0.5, safe["tau"],
                             rl.policy)
    with pytest.raises(TypeError, match="uncertain GP dynamics"):
        lyap_euler.decrease_gradient(states, actions)
    lyap_euler._upload_model()
    with pytest.raises(_hip.HipEngineError, match="Euler dynamics"):
        lyap_euler._ctx.decrease_gradient(50, d_states, d_actions, out)
    rl_euler = sl.PolicyIteration(rl.policy, euler, rl.reward_function, rl.value_function, gamma=rl.gamma)
    with pytest.raises(TypeError, match="uncertain dynamics"):
        rl_euler.policy_gradient(states, lyapunov=lyap_euler)
    linear = sl.LinearSystem((np.eye(2), np.ones((2, 1))))
    lyap_linear = sl.Lyapunov(lyap.discretization, sl.QuadraticFunction(case["P"]), linear, safe["lf"], 0.5, safe["tau"],
                              rl.policy)
    lyap_linear._upload_model()
    with pytest.raises(_hip.HipEngineError, match="linear dynamics"):
        lyap_linear._ctx.decrease_gradient(50, d_states, d_actions, out)
    unchanged()
    # a foreign dynamics object
    foreign = S.product_lyapunov(sl, case, safe, S.product_dynamics(sl, case), rl.policy)
    with pytest.raises(ValueError, match="lyapunov.dynamics must be the dynamics object"):
        rl.policy_gradient(states, lyapunov=foreign)
    with pytest.raises(ValueError, match="lyapunov.dynamics must be the dynamics object"):
        sl.policy_improvement_step(rl, states, 0.1, lyapunov=foreign)
    # a wrong action width, a wrong number of rows, a wrong state width
    with pytest.raises(ValueError, match="actions must be"):
        lyap.decrease_gradient(states, np.zeros((50, 2)))
    with pytest.raises(ValueError, match="actions must be"):
        lyap.decrease_gradient(states, np.zeros((49, 1)))
    with pytest.raises(ValueError, match="states of 3 columns"):
        lyap.decrease_gradient(np.zeros((5, 3)))
    # anything that is not a Lyapunov
    with pytest.raises(NotImplementedError, match="Lyapunov penalty"):
        rl.policy_gradient(states, lyapunov=object())
    unchanged()
