"""Closed-loop rollouts on the GPU (csrc/sl_rollout.hip; needs an MI355X): ``compute_trajectory`` and
``compute_roa`` through the real kernels against the NumPy reference (tests/np_rollout.py over the
oracle's callables), with the comparisons and tolerances of tests/test_rollout_host.py, and against a
run of the reference itself (tests/golden/reference_roa.npz)."""

import os
import signal

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import exclusions
import rollout_cases as RC
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

TEST_SECONDS = 420       # no test here needs more (the cart-pole oracles: most of a minute each)


@pytest.fixture(autouse=True)
def _time_limit():
    """Every test runs under its own time limit: SIGALRM with its default action ends the process
    (also while it waits inside a HIP call), so nothing more is started on the GPU after a hang."""
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    signal.alarm(TEST_SECONDS)
    yield
    signal.alarm(0)


def _U():
    from safe_learning_amd import utilities
    return utilities


# ---- linear dynamics, saturated linear policy: bit for bit ----------------------------------------
@pytest.mark.parametrize("key", sorted(RC.LINEAR_CASES))
def test_linear_rollout_bit_exact(key):
    U = _U()
    pts, states, actions = RC.oracle_linear(key)
    case = RC.make(*RC.LINEAR_CASES[key])
    dynamics, policy = RC.engine_pair(case)
    s, a = U.compute_trajectory(dynamics, policy, pts, RC.LINEAR_STEPS + 1)
    assert_array_equal(s, states)
    assert_array_equal(a, actions)
    s1, a1 = U.compute_trajectory(dynamics, policy, pts[1], RC.LINEAR_STEPS + 1)     # one state: [steps, d]
    assert_array_equal(s1, states[1])
    assert_array_equal(a1, actions[1])
    for chunk in (1, 7):
        sc, ac = U.compute_trajectory(dynamics, policy, pts, RC.LINEAR_STEPS + 1, steps_per_launch=chunk)
        assert_array_equal(sc, states)
        assert_array_equal(ac, actions)
    # from the cells of the grid: GridWorld.all_points
    end, grid_states, _ = U._rollout(dynamics, policy, RC.engine_grid(case), RC.LINEAR_STEPS, trajectory=True)
    assert_array_equal(grid_states.cpu().numpy(), states.transpose(1, 0, 2))
    assert_array_equal(end.cpu().numpy(), states[:, -1])


def test_table_policy_rollout():
    U = _U()
    pts, states, actions, ok = RC.oracle_tri()
    dynamics, policy = RC.engine_pair(RC.tri_case())
    s, a = U.compute_trajectory(dynamics, policy, pts, RC.TRI_STEPS + 1)
    from safe_learning_amd import _evaluate
    assert "k_rollout<general=1" in _evaluate._ctx().last_kernel()        # uploaded as SL_POLICY_TRI
    assert_allclose(a[ok], actions[ok], rtol=1e-10, atol=1e-12)
    assert_allclose(s[:, 1:][ok], states[:, 1:][ok], rtol=1e-10, atol=1e-12)
    exclusions.report("test_gpu_rollout::test_table_policy_rollout", ok, "successor")


# ---- Euler dynamics ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(RC.EULER_CASES))
def test_euler_rollout_first_steps(key):
    U = _U()
    pts, states, actions = RC.oracle_euler(key)
    dynamics, policy = RC.engine_pair(RC.make(*RC.EULER_CASES[key]))
    s, a = U.compute_trajectory(dynamics, policy, pts, RC.EULER_STEPS + 1)
    assert_array_equal(s[:, 0], pts)
    assert_allclose(s, states, rtol=RC.EULER_RTOL, atol=RC.EULER_ATOL)
    assert_allclose(a, actions, rtol=RC.EULER_RTOL, atol=RC.EULER_ATOL)


@pytest.mark.parametrize("key", sorted(RC.ROA_CASES))
def test_roa_mask_matches_oracle(key):
    U = _U()
    RC.oracle_roa(key)                                    # (the conditions on the input first)
    case, horizon, tol = RC.roa_case(key)
    pair = RC.engine_pair(case)
    grid = RC.engine_grid(case)
    roa = U.compute_roa(grid, pair, horizon=horizon, tol=tol)
    end, _, _ = U._rollout(pair[0], pair[1], grid, horizon - 1)
    RC.check_roa(key, roa, end.cpu().numpy())


def test_trajectories_and_end_states_agree():
    """``no_traj=False``: the last step equals the ``no_traj=True`` end states, step 0 the grid points;
    a device-tensor grid keeps everything on the device."""
    import torch
    U = _U()
    key = "pendulum-x1"
    start, _, _, want = RC.oracle_roa(key)
    case, horizon, tol = RC.roa_case(key)
    pair, grid = RC.engine_pair(case), RC.engine_grid(case)
    roa, traj = U.compute_roa(grid, pair, horizon=horizon, tol=tol, no_traj=False)
    assert traj.shape == (grid.nindex, 2, horizon) and roa.dtype == np.bool_
    assert_array_equal(roa, want)
    assert_array_equal(traj[:, :, 0], grid.all_points)
    assert_array_equal(traj[:, :, 0], start)
    end, _, _ = U._rollout(pair[0], pair[1], grid, horizon - 1)
    assert_array_equal(traj[:, :, -1], end.cpu().numpy())
    d_roa, d_traj = U.compute_roa(torch.from_numpy(start).cuda(), pair, horizon=horizon, tol=tol, no_traj=False)
    assert d_roa.is_cuda and d_roa.dtype == torch.bool and d_traj.is_cuda
    assert d_traj.stride() == (2, 1, 2 * grid.nindex)                  # a view of [horizon][n][d]
    assert_array_equal(d_roa.cpu().numpy(), want)
    assert_array_equal(d_traj.cpu().numpy(), traj)
    # horizon 1: no step at all
    assert_array_equal(U.compute_roa(grid, pair, horizon=1, tol=0.5), np.linalg.norm(start, axis=1) <= 0.5)


def test_chunking_and_start_states_do_not_change_results():
    """10^6 cells x 499 steps: one step per launch, the library's choice and the whole horizon in one
    launch give bit-identical end states and masks; so do the cells of the grid and the explicit
    ``grid.all_points``."""
    import safe_learning_amd as sl
    U = _U()
    case, horizon, tol = RC.roa_case("pendulum-x1")
    pair = RC.engine_pair(case)
    grid = sl.GridWorld(case["limits"], [1001, 1001])
    runs = {}
    for label, chunk in (("one", 1), ("default", 0), ("all", horizon - 1)):
        end, _, _ = U._rollout(pair[0], pair[1], grid, horizon - 1, steps_per_launch=chunk)
        runs[label] = (end.cpu().numpy(), U.compute_roa(grid, pair, horizon=horizon, tol=tol, steps_per_launch=chunk))
    for label in ("one", "all"):
        assert_array_equal(runs[label][0], runs["default"][0])
        assert_array_equal(runs[label][1], runs["default"][1])
    roa = runs["default"][1]
    assert 0.5 < roa.mean() < 0.75                       # (0.630 on the 101 x 101 grid of the same limits)
    end, _, _ = U._rollout(pair[0], pair[1], grid.all_points, horizon - 1)
    assert_array_equal(end.cpu().numpy(), runs["default"][0])
    assert_array_equal(U.compute_roa(grid.all_points, pair, horizon=horizon, tol=tol), roa)
    # an equilibrium other than the origin, against NumPy's norm on the same end states
    eq = np.array([[0.01, -0.02]])
    dist = np.linalg.norm(runs["default"][0] - eq, ord=2, axis=1)
    assert_array_equal(U.compute_roa(grid, pair, horizon=horizon, tol=0.03, equilibrium=eq), dist <= 0.03)


# ---- a run of the reference itself ----------------------------------------------------------------------------
def test_reference_run_is_reproduced():
    """tests/golden/reference_roa.npz alone (the reference's compute_roa / compute_trajectory on its own
    InvertedPendulum / CartPole / LinearSystem / Saturation): masks exactly - the fixture's generator
    asserts that no cell ends within a decade of tol - end states of the in-ROA cells at 1e-10, the
    first steps of every trajectory at the Euler tolerance."""
    import safe_learning_amd as sl
    from test_rollout_host import reference_case
    U = _U()
    data = np.load(os.path.join(GOLDEN_DIR, "reference_roa.npz"))
    for key in ("pendulum", "cartpole"):
        case, horizon, tol = reference_case(data, key)
        pair, grid = RC.engine_pair(case), RC.engine_grid(case)
        assert_array_equal(grid.all_points, data[key + "_points"])
        want = data[key + "_roa"]
        roa, traj = U.compute_roa(grid, pair, horizon=horizon, tol=tol, no_traj=False)
        assert_array_equal(roa, want)
        assert want.any() and not want.all()
        assert_allclose(traj[:, :, -1][want], data[key + "_end"][want], rtol=0, atol=RC.ROA_END_STATE_ATOL)
        steps = min(data[key + "_traj"].shape[2], RC.EULER_STEPS + 1)
        assert_allclose(traj[:, :, :steps], data[key + "_traj"][:, :, :steps], rtol=RC.EULER_RTOL,
                        atol=RC.EULER_ATOL)
    dynamics = sl.LinearSystem((data["linear_A"], data["linear_B"]))
    policy = sl.LinearSystem((data["linear_K"],))
    states, actions = U.compute_trajectory(dynamics, policy, data["linear_x0"], int(data["linear_num_steps"]))
    assert states.shape == data["linear_states"].shape and actions.shape == data["linear_actions"].shape
    assert_allclose(states, data["linear_states"], rtol=1e-13, atol=1e-15)
    assert_allclose(actions, data["linear_actions"], rtol=1e-13, atol=1e-15)
    assert_allclose(states[-1], 0.0, atol=0.01)                              # test_utilities.py:113


# ---- a NeuralNetwork policy: step by step inside the library -------------------------------------------------
def test_network_policy_rollout():
    """One step is allowed the 1e-12 / 1e-14 of tests/test_gpu_network_policy.py (the policy at points,
    the device tanh) on top of the Euler step's 1e-12 / 1e-15; eight steps eight times that, rounded up
    (the Euler tolerance of rollout_cases with the policy's absolute term)."""
    import safe_learning_amd as sl
    U = _U()
    start, states, actions, end_ref, _, want = RC.oracle_network()
    case, horizon, tol = RC.network_case()
    dynamics, _ = RC.engine_pair(case)
    net = sl.NeuralNetwork(RC.NETWORK_LAYERS, RC.NETWORK_ACTS, output_scale=1.0, use_bias=False,
                           input_dim=case["d"], seed=0)
    net.parameters = RC.network_parameters(case)
    policy = sl.Saturation(net, *case["saturate"])
    grid = RC.engine_grid(case)
    s, a = U.compute_trajectory(dynamics, policy, start, RC.EULER_STEPS + 1)
    from safe_learning_amd import _evaluate
    assert "k_policy_network" in _evaluate._ctx().last_kernel()
    assert_allclose(a[:, 0], actions[:, 0], rtol=1e-12, atol=1e-14)
    assert_allclose(s[:, :2], states[:, :2], rtol=2e-12, atol=2e-14)
    assert_allclose(s, states, rtol=2e-11, atol=2e-13)
    assert_allclose(a, actions, rtol=2e-11, atol=2e-13)
    roa = U.compute_roa(grid, (dynamics, policy), horizon=horizon, tol=tol)
    end, _, _ = U._rollout(dynamics, policy, grid, horizon - 1)
    flips = int((roa != want).sum())
    print("network policy: %d mask flips, largest in-ROA end-state difference %.3g"
          % (flips, np.abs(end.cpu().numpy()[want] - end_ref[want]).max()))
    assert flips == 0
    assert_allclose(end.cpu().numpy()[want], end_ref[want], rtol=0, atol=RC.ROA_END_STATE_ATOL)
    # from explicit points the same bits as from the cells
    assert_array_equal(U.compute_roa(grid.all_points, (dynamics, policy), horizon=horizon, tol=tol), roa)


# ---- any callable: a GP's mean ------------------------------------------------------------------------------------
def test_callable_closed_loop_gp_mean():
    import torch
    from gp_cases import INFORMED
    from safe_learning_amd import _evaluate
    U = _U()
    case = RC.make("pendulum", dict(num_points=[24, 20], n_gp=60, **INFORMED))
    dynamics, policy = RC.engine_pair(case)
    grid = RC.engine_grid(case)

    def mean_step(x):
        return _evaluate.dynamics(dynamics, x, _evaluate.policy(policy, x))[0]

    horizon, tol = 30, 0.2
    x = torch.from_numpy(grid.all_points).cuda()
    by_hand = [x]
    for _ in range(1, horizon):
        x = mean_step(x).contiguous()
        by_hand.append(x)
    dist = torch.linalg.vector_norm(x, dim=1).cpu().numpy()
    assert not ((dist > tol * 0.999) & (dist < tol * 1.001)).any()
    want = dist <= tol
    assert want.any() and not want.all()
    roa, traj = U.compute_roa(grid, mean_step, horizon=horizon, tol=tol, no_traj=False)
    assert_array_equal(roa, want)
    assert_array_equal(traj, torch.stack(by_hand, dim=2).cpu().numpy())
    assert_array_equal(U.compute_roa(grid.all_points, lambda s: mean_step(s), horizon=horizon, tol=tol), want)
    # the pair form names the callable form
    with pytest.raises(ValueError, match="callable"):
        U.compute_roa(grid, (dynamics, policy), horizon=horizon, tol=tol)


# ---- errors are errors ---------------------------------------------------------------------------------------------
def test_error_paths():
    import torch
    import safe_learning_amd as sl
    from safe_learning_amd import _evaluate
    from safe_learning_amd._hip import HipEngineError
    from gp_cases import INFORMED
    U = _U()
    case = RC.make(*RC.LINEAR_CASES["pendulum"])
    dynamics, policy = RC.engine_pair(case)
    grid = RC.engine_grid(case)
    n, d = grid.nindex, grid.ndim
    U.compute_roa(grid, (dynamics, policy), horizon=3)                   # (leaves its model on the context)
    ctx = _evaluate._ctx()
    state = torch.zeros((n, d), dtype=torch.float64, device="cuda")
    with pytest.raises(HipEngineError, match="past the grid"):
        ctx.rollout(0, n + 1, None, 2, state)
    with pytest.raises(HipEngineError, match="bad range"):
        ctx.rollout(0, n, None, -1, state)
    with pytest.raises(HipEngineError, match="bad range"):
        ctx.rollout(5, 2, None, 1, state)
    with pytest.raises(HipEngineError, match="bad range"):
        ctx.rollout(0, n, None, 1, None)
    bits = torch.zeros(((n + 63) // 64,), dtype=torch.int64, device="cuda")
    count = torch.zeros((1,), dtype=torch.int64, device="cuda")
    with pytest.raises(HipEngineError, match="bad argument"):
        ctx.rollout_mask(n, 0, state, None, 0.1, bits, count)
    with pytest.raises(HipEngineError, match="bad argument"):
        ctx.rollout_mask(n, d, state, None, 0.1, None, count)
    ctx.rollout_mask(0, d, None, None, 0.1, None, count)                 # nothing to do is fine
    ctx.rollout_mask(n, d, state, None, 0.1, bits, count)
    assert int(count.item()) == n                                        # all at the origin
    # a per-vertex table is defined at the vertices only: one step, not two
    import copy
    _, builder = _evaluate._builder(d)          # (the context's own builder: it tracks what the context holds)
    builder.grid = copy.copy(grid)
    builder.upload(np.zeros((n, 1)), dynamics, sl.QuadraticFunction(np.eye(d)))
    ctx.rollout(0, n, None, 1, state)
    with pytest.raises(HipEngineError, match="vertices"):
        ctx.rollout(0, n, None, 2, state)
    # GP dynamics are not simulated inside the kernel
    gp_case = RC.make("pendulum", dict(num_points=[9, 11], n_gp=20, **INFORMED))
    builder.upload(policy, RC.engine_pair(gp_case)[0], sl.QuadraticFunction(np.eye(d)))
    with pytest.raises(HipEngineError, match=r"\(-3\).*GP dynamics"):
        ctx.rollout(0, n, None, 2, state)
    # the context still works
    assert U.compute_roa(grid, (dynamics, policy), horizon=3, tol=10.0).all()
