"""Closed-loop rollouts of a GP's posterior mean on the GPU (csrc/sl_gp_rollout.hip; needs an MI355X), through the
public functions: ``GPMeanFunction.__call__``, ``compute_roa``, ``compute_trajectory`` and ``reward_rollout`` with
a ``(to_mean_function(), policy)`` pair, against the NumPy reference (tests/np_gp_rollout.py) with the cases,
conditions and bounds of tests/test_gp_rollout_host.py: masks without a flip, states and returns within 32 x the
float64 reference's own distance to its long-double companion plus 4 ulps of the state scale."""

import signal

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import np_gp_rollout as R

pytestmark = pytest.mark.gpu

TEST_SECONDS = 120
ALL_CASES = sorted(R.ROA_CASES) + sorted(R.OTHER_CASES)


@pytest.fixture(autouse=True)
def _time_limit():
    """Every test runs under its own time limit: SIGALRM with its default action ends the process (also while
    it waits inside a HIP call), so nothing more is started on the GPU after a hang."""
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    signal.alarm(TEST_SECONDS)
    yield
    signal.alarm(0)


def _sl():
    import safe_learning_amd as sl
    return sl


def _pair(name):
    """-> (case, parent, mean function, policy, grid) of the engine."""
    sl = _sl()
    case = R.make(name)[0]
    parent = R.engine_dynamics(case)
    return case, parent, parent.to_mean_function(), R.engine_policy(case), sl.GridWorld(case["limits"], case["num_points"])


def _last_kernel():
    from safe_learning_amd import _evaluate
    return _evaluate._ctx().last_kernel()


# ---- the mean at points ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_CASES)
def test_mean_at_points(name):
    """``f(states, actions)`` equals ``sl_action_gradient``'s ``d_next`` - the existing device statement of the same
    sum - bit for bit, and the posterior mean of ``sl_eval_points`` within the posterior tolerance."""
    import torch
    from gp_cases import reference_gp_tolerance
    from safe_learning_amd import _evaluate
    sl = _sl()
    case, parent, f, policy, grid = _pair(name)
    ro = R.reference(name)[5]
    d, m = case["d"], case["m"]
    x = np.ascontiguousarray(np.vstack((ro.states[0], ro.states[len(ro.actions) - 1])))
    u = np.ascontiguousarray(np.vstack((ro.actions[0], ro.actions[-1])))
    mean = f(x, u)
    assert isinstance(mean, np.ndarray) and mean.shape == x.shape and "k_gp_mean_points" in _last_kernel()
    on_device = f(torch.from_numpy(x).cuda(), torch.from_numpy(u).cuda())
    assert isinstance(on_device, torch.Tensor) and on_device.is_cuda
    assert_array_equal(on_device.cpu().numpy(), mean)
    assert_array_equal(f(np.hstack((x, u))), mean)
    # sl_action_gradient's successor under the same heads
    ctx, builder = _evaluate._builder(d)
    value = sl.Triangulation(sl.GridWorld(case["limits"], [3] * d), np.zeros((3 ** d, 1)), project=True)
    builder.upload(sl.ConstantFunction(np.zeros(m)), parent, value, reward=sl.QuadraticFunction(-np.eye(d + m)), gamma=0.9)
    n = len(x)
    d_x, d_u = torch.from_numpy(x).cuda(), torch.from_numpy(u).cuda()
    grad = torch.empty((n, m), dtype=torch.float64, device="cuda")
    nxt = torch.empty((n, d), dtype=torch.float64, device="cuda")
    ctx.action_gradient(n, d_x, d_u, grad, None, nxt)
    assert_array_equal(nxt.cpu().numpy(), mean)
    # the posterior call of the parent
    heads = [h for h in R.case_heads(case) if len(h["X"])]
    cond = max(float(np.linalg.cond(R._oracle_kernel(h["kernel"]).K(h["X"]) + h["noise"] * np.eye(len(h["X"]))))
               for h in heads)
    posterior = _evaluate.dynamics(parent, x, u)[0]
    tol = reference_gp_tolerance(cond)
    print("mean at points %s: cond %.3g, largest |f - posterior mean| %.3g (rtol %.3g)"
          % (name, cond, np.abs(mean - posterior).max(), tol))
    assert_allclose(mean, posterior, rtol=tol, atol=tol * np.abs(posterior).max())
    # ... and the reference's step
    steps = np.vstack((ro.states[1], ro.states[len(ro.actions)]))
    assert np.abs(mean - steps).max() <= ro.bound()[-1]


# ---- masks, trajectories and returns ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_CASES)
def test_roa_and_trajectories_match_reference(name):
    sl = _sl()
    case, horizon, tol, _, _, ro, roa = R.reference(name)
    _, parent, f, policy, grid = _pair(name)
    mask, traj = sl.compute_roa(grid, (f, policy), horizon=horizon, tol=tol, no_traj=False)
    kernel = _last_kernel()
    assert "k_gp_rollout<general=%d, d=%d>" % (int(name == "table-policy"), case["d"]) in kernel, kernel
    states = traj.transpose(2, 0, 1)                                    # [horizon, n, d]
    flips = int((mask != roa).sum())
    ratio = ro.ratio(states)
    print("mean rollout %s (GPU): %d mask flips of %d, largest |states - reference| / bound %.3g (bound at the end "
          "%.3g); %s" % (name, flips, len(roa), ratio, ro.bound()[-1], kernel))
    assert mask.dtype == np.bool_ and flips == 0                        # nothing excluded
    assert_array_equal(states[0], ro.states[0])
    assert ratio <= 1.0
    assert np.abs(states[-1][roa] - ro.end[roa]).max() <= ro.bound()[-1]
    # no_traj=True: the same end states; compute_trajectory: the same rows and the reference's actions
    assert_array_equal(sl.compute_roa(grid, (f, policy), horizon=horizon, tol=tol), mask)
    pts = R.start_points(case)[:7]
    s, a = sl.compute_trajectory(f, policy, pts, horizon)
    assert_array_equal(s, traj.transpose(0, 2, 1)[:7])
    assert np.abs(a.transpose(1, 0, 2) - ro.actions[:, :7]).max() <= ro.bound()[-1] * max(1.0, np.abs(case["K"]).sum())


@pytest.mark.parametrize("name,discount,horizon,tol,stops", [("pendulum-stack", 0.8, 40, 0.1, True),
                                                             ("cartpole", 0.98, 25, 1e-6, False),
                                                             ("table-policy", 0.8, 40, 0.1, True)])
def test_reward_rollout_matches_reference(name, discount, horizon, tol, stops):
    """Returns, step count and the stopping flag against the reference, for the closed-form flavours and for the
    interpolated policy (two trajectories per thread, the wavefront maximum taken after the second); the steps per
    launch (the library's choice, 1, 7) and cells against explicit points give identical bits."""
    sl = _sl()
    case, _, _, model, opolicy, _, _ = R.reference(name)
    _, parent, f, policy, grid = _pair(name)
    pts = R.start_points(case)
    reward = R.reward_matrix(case)
    ref = R.RewardRollout(model, opolicy, pts, reward, discount, horizon, tol)
    assert ref.gap > R.GAP and ref.converged == stops and (ref.steps < horizon) == stops      # one case stops early
    results = []
    for per_launch, start in ((0, grid), (1, grid), (7, grid), (0, pts)):
        total, steps, converged = sl.reward_rollout(start, (f, policy), sl.QuadraticFunction(reward), discount,
                                                    horizon=horizon, tol=tol, full_output=True,
                                                    steps_per_launch=per_launch)
        assert "k_gp_reward_rollout<general=%d, d=%d>" % (int(name == "table-policy"), case["d"]) in _last_kernel()
        assert (steps, converged) == (ref.steps, ref.converged)
        results.append(total)
    ratio = ref.ratio(results[0])
    print("mean returns %s (GPU): %d of %d terms, largest |sum - reference| / bound %.3g (bound %.3g); %s"
          % (name, ref.steps, horizon, ratio, ref.bound(), _last_kernel()))
    assert ratio <= 1.0
    for other in results[1:]:
        assert_array_equal(other, results[0])


# ---- identities, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pendulum-stack", "cartpole", "notebook-kernels"])
def test_identities(name):
    import torch
    sl = _sl()
    case, parent, f, policy, grid = _pair(name)
    horizon = R.make(name)[1]
    pts = R.start_points(case)
    mask, traj = sl.compute_roa(grid, (f, policy), horizon=horizon, tol=0.2, no_traj=False)
    # steps per launch: 1, 7, the whole horizon, the library's choice
    for per_launch in (1, 7, horizon - 1):
        m2, t2 = sl.compute_roa(grid, (f, policy), horizon=horizon, tol=0.2, no_traj=False, steps_per_launch=per_launch)
        assert_array_equal(t2, traj)
        assert_array_equal(m2, mask)
    # the same call again gives identical bits
    m0, t0 = sl.compute_roa(grid, (f, policy), horizon=horizon, tol=0.2, no_traj=False)
    assert_array_equal(t0, traj)
    assert_array_equal(m0, mask)
    # cells = explicit start points; device tensors stay on the device
    m3, t3 = sl.compute_roa(pts, (f, policy), horizon=horizon, tol=0.2, no_traj=False)
    assert_array_equal(t3, traj)
    assert_array_equal(m3, mask)
    m4, t4 = sl.compute_roa(torch.from_numpy(pts).cuda(), (f, policy), horizon=horizon, tol=0.2, no_traj=False)
    assert m4.is_cuda and t4.is_cuda
    assert_array_equal(t4.cpu().numpy(), traj)
    # the end states of no_traj=True are the last trajectory row
    from safe_learning_amd import utilities as U
    end, _, _ = U._rollout(f, policy, grid, horizon - 1)
    assert_array_equal(end.cpu().numpy(), traj[:, :, -1])
    # T fused steps = T applications of f(x, policy(x)), over the whole horizon
    x = pts
    for t in range(1, horizon):
        x = f(x, policy(x))
        assert_array_equal(x, traj[:, :, t])


# ---- other policy kinds -----------------------------------------------------------------------------------------------
def test_network_policy():
    """A NeuralNetwork policy goes through single-step launches under the action table (the Triangulation policy
    is the table-policy case above)."""
    sl = _sl()
    case, horizon, tol, policy, ro, roa = R.network_reference()
    f = R.engine_dynamics(case).to_mean_function()
    grid = sl.GridWorld(case["limits"], case["num_points"])
    mask, traj = sl.compute_roa(grid, (f, policy), horizon=horizon, tol=tol, no_traj=False)
    assert "k_policy_network + k_gp_rollout" in _last_kernel()
    ratio = ro.ratio(traj.transpose(2, 0, 1))
    print("mean rollout, network policy (GPU): %d mask flips, largest |states - reference| / bound %.3g"
          % ((mask != roa).sum(), ratio))
    assert_array_equal(mask, roa)
    assert ratio <= 1.0
    total, steps, converged = sl.reward_rollout(grid, (f, policy), sl.QuadraticFunction(R.reward_matrix(case)), 0.8,
                                                horizon=12, tol=1e-9, full_output=True)
    assert "k_policy_network + k_gp_reward_rollout" in _last_kernel()
    assert (steps, converged) == (12, False) and np.isfinite(total).all()


# ---- the view is live ---------------------------------------------------------------------------------------------------
def test_view_follows_its_parent():
    sl = _sl()
    name = "pendulum"
    case, horizon, tol, model, opolicy, ro, roa = R.reference(name)
    _, parent, f, policy, grid = _pair(name)
    _, before = sl.compute_roa(grid, (f, policy), horizon=horizon, tol=tol, no_traj=False)
    assert ro.ratio(before.transpose(2, 0, 1)) <= 1.0
    # three more observations, far from the model's mean
    rng = np.random.default_rng(11)
    x_new = rng.uniform(-0.5, 0.5, (3, 3))
    y_new = parent(x_new[:, :2], x_new[:, 2:])[0] + rng.normal(0, 0.02, (3, 2))
    for x, y in zip(x_new, y_new):
        parent.add_data_point(x[None, :], y[None, :])
    grown = dict(case, dynamics=dict(case["dynamics"], X=np.vstack((case["dynamics"]["X"], x_new)),
                                     Y=np.vstack((case["dynamics"]["Y"], y_new))))
    ro2 = R.Rollout(R.MeanModel(R.case_heads(grown)), opolicy, R.start_points(case), horizon - 1)
    _, after = sl.compute_roa(grid, (f, policy), horizon=horizon, tol=tol, no_traj=False)
    ratio = ro2.ratio(after.transpose(2, 0, 1))
    print("after add_data_point: largest change %.3g, |states - reference| / bound %.3g" % (np.abs(after - before).max(), ratio))
    assert np.abs(after - before).max() > 1e3 * ro.bound()[-1] and ratio <= 1.0
    # new hyper-parameters
    gp = parent.gaussian_process
    gp.kern.lengthscales = np.asarray(gp.kern.lengthscales) * 0.8
    gp.update_cache()
    tuned = dict(grown, dynamics=dict(grown["dynamics"], lengthscales=np.asarray(case["dynamics"]["lengthscales"]) * 0.8))
    ro3 = R.Rollout(R.MeanModel(R.case_heads(tuned)), opolicy, R.start_points(case), horizon - 1)
    _, tuned_traj = sl.compute_roa(grid, (f, policy), horizon=horizon, tol=tol, no_traj=False)
    ratio = ro3.ratio(tuned_traj.transpose(2, 0, 1))
    print("after new lengthscales: largest change %.3g, |states - reference| / bound %.3g"
          % (np.abs(tuned_traj - after).max(), ratio))
    assert np.abs(tuned_traj - after).max() > 1e3 * ro2.bound()[-1] and ratio <= 1.0


# ---- errors -----------------------------------------------------------------------------------------------------------
def test_error_paths():
    import copy
    import torch
    from safe_learning_amd import _evaluate
    from safe_learning_amd._hip import HipEngineError
    sl = _sl()
    case, parent, f, policy, grid = _pair("pendulum")
    n, d = grid.nindex, grid.ndim
    want = sl.compute_roa(grid, (f, policy), horizon=3, tol=10.0)        # (leaves its model on the context)
    ctx, builder = _evaluate._builder(d)
    builder.grid = copy.copy(grid)
    builder.upload(policy, f, sl.QuadraticFunction(np.eye(d)))
    state = torch.zeros((n, d), dtype=torch.float64, device="cuda")
    with pytest.raises(HipEngineError, match="past the grid"):
        ctx.rollout_mean(0, n + 1, None, 2, state)
    with pytest.raises(HipEngineError, match="bad range"):
        ctx.rollout_mean(0, n, None, -1, state)
    with pytest.raises(HipEngineError, match="bad range"):
        ctx.rollout_mean(5, 2, None, 1, state)
    with pytest.raises(HipEngineError, match="bad range"):
        ctx.rollout_mean(0, n, None, 1, None)
    ctx.rollout_mean(3, 3, None, 5, state)                               # nothing to do is fine
    # the unchanged refusals of the deterministic entry points
    with pytest.raises(HipEngineError, match=r"\(-3\).*GP dynamics"):
        ctx.rollout(0, n, None, 2, state)
    # a per-vertex table is defined at the vertices only: one step, not two
    builder.upload(np.zeros((n, 1)), f, sl.QuadraticFunction(np.eye(d)))
    ctx.rollout_mean(0, n, None, 1, state)
    with pytest.raises(HipEngineError, match="vertices"):
        ctx.rollout_mean(0, n, None, 2, state)
    # a linear model belongs to sl_rollout
    linear = sl.LinearSystem((np.hstack((case["A_true"], case["B_true"])),))
    builder.upload(policy, linear, sl.QuadraticFunction(np.eye(d)), reward=sl.QuadraticFunction(-np.eye(d + 1)))
    with pytest.raises(HipEngineError, match=r"\(-3\).*sl_rollout"):
        ctx.rollout_mean(0, n, None, 2, state)
    weights = torch.ones((4,), dtype=torch.float64, device="cuda")
    total = torch.zeros((n,), dtype=torch.float64, device="cuda")
    with pytest.raises(HipEngineError, match=r"\(-3\).*sl_reward_rollout"):
        ctx.reward_rollout_mean(0, n, None, 4, weights, 0.0, total, state)
    inputs = torch.zeros((n, d + 1), dtype=torch.float64, device="cuda")
    with pytest.raises(HipEngineError, match=r"\(-3\).*SL_DYN_GP"):
        ctx.gp_mean_points(n, inputs, state)
    # the pair form with the UncertainFunction itself raises what it raised
    with pytest.raises(ValueError, match="callable"):
        sl.compute_roa(grid, (parent, policy))
    # the context still works
    assert_array_equal(sl.compute_roa(grid, (f, policy), horizon=3, tol=10.0), want)
