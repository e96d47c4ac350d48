"""reward_rollout on the GPU (csrc/sl_rollout.hip: k_reward_rollout, k_reward_fold; needs an MI355X)
through ``safe_learning_amd.utilities.reward_rollout`` against the NumPy reference
(tests/np_reward_rollout.py over the oracle's callables), with the shapes, conditions and tolerances of
tests/reward_rollout_cases.py, and against a run of the reference itself
(tests/golden/reference_reward_rollout.npz)."""

import os
import signal

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import exclusions
import np_reward_rollout as NR
import reward_rollout_cases as RRC
import rollout_cases as RC
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

TEST_SECONDS = 120       # no test here needs more (the oracles: seconds each)


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


def _reward(matrix):
    import safe_learning_amd as sl
    return sl.QuadraticFunction(matrix)


def _last_kernel():
    from safe_learning_amd import _evaluate
    return _evaluate._ctx().last_kernel()


# ---- 1. linear dynamics, saturated linear policy: bit for bit, whatever the launches are --------------------
@pytest.mark.parametrize("key", sorted(RRC.LINEAR))
def test_linear_sums_bit_exact(key):
    U = _U()
    pts, want, steps, converged, _ = RRC.oracle_linear(key)
    case, matrix, discount, horizon, tol = RRC.linear_case(key)
    pair, reward = RC.engine_pair(case), _reward(matrix)
    for chunk in (0, 1, 6, 17, 18):
        got, got_steps, got_flag = U.reward_rollout(pts, pair, reward, discount, horizon=horizon, tol=tol,
                                                    full_output=True, steps_per_launch=chunk)
        assert_array_equal(got, want)
        assert (got_steps, got_flag) == (steps, converged), chunk
        assert "k_reward_rollout<general=0, d=%d" % case["d"] in _last_kernel()
        assert "%d steps in" % steps in _last_kernel()
    # from the cells of the grid: GridWorld.all_points
    got, got_steps, got_flag = U.reward_rollout(RC.engine_grid(case), pair, reward, discount, horizon=horizon,
                                                tol=tol, full_output=True)
    assert_array_equal(got, want)
    assert (got_steps, got_flag) == (steps, converged)


# ---- 2. Euler models ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(RRC.EULER))
def test_euler_sums(key):
    U = _U()
    pts, want, steps, converged, _, rtol = RRC.oracle_euler(key)
    case, matrix, discount, horizon, tol = RRC.euler_case(key)
    pair, reward = RC.engine_pair(case), _reward(matrix)
    got, got_steps, got_flag = U.reward_rollout(RC.engine_grid(case), pair, reward, discount, horizon=horizon,
                                                tol=tol, full_output=True)
    assert (got_steps, got_flag) == (steps, converged)
    RRC.assert_sums_close(got, want, rtol)
    # the launches do not change a bit
    for chunk in (1, 50):
        again = U.reward_rollout(pts, pair, reward, discount, horizon=horizon, tol=tol, full_output=True,
                                 steps_per_launch=chunk)
        assert_array_equal(again[0], got)
        assert again[1:] == (got_steps, got_flag)
    # a run of the reference itself
    data = np.load(os.path.join(GOLDEN_DIR, "reference_reward_rollout.npz"))
    assert_array_equal(pts, data[key + "_points"])
    assert_array_equal(matrix, data[key + "_reward_matrix"])
    assert (discount, horizon, tol) == (float(data["discount"]), int(data["horizon"]), float(data["tol"]))
    assert got_steps == int(data[key + "_steps"])
    RRC.assert_sums_close(got, data[key + "_rollout"], rtol)


# ---- 3. more than one pass of the grid-stride loop ----------------------------------------------------------------
def test_more_than_one_pass_linear_two_per_thread():
    """1 050 001 trajectories of the "1d" case: two per thread, more than 2 x 2048 x 256 - the maxima
    a workgroup keeps in LDS span its passes; the last trajectory shares its thread with a lane past
    the end."""
    U = _U()
    pts, want, steps, converged = RRC.oracle_large_1d()
    case, matrix, discount, horizon, tol = RRC.large_1d_case()
    assert len(pts) > 2 * 2048 * 256 and len(pts) % 2 == 1
    got, got_steps, got_flag = U.reward_rollout(RC.engine_grid(case), (RC.engine_pair(case)), _reward(matrix),
                                                discount, horizon=horizon, tol=tol, full_output=True)
    assert (got_steps, got_flag) == (steps, converged)
    assert got[-1] == want[-1]
    assert_array_equal(got, want)


def test_more_than_one_pass_euler_pendulum():
    U = _U()
    pts, want, steps, converged = RRC.oracle_large_pendulum()
    case, matrix, discount, horizon, tol = RRC.large_pendulum_case()
    assert len(pts) > 2048 * 256
    got, got_steps, got_flag = U.reward_rollout(RC.engine_grid(case), RC.engine_pair(case), _reward(matrix),
                                                discount, horizon=horizon, tol=tol, full_output=True)
    assert (got_steps, got_flag) == (steps, converged) == (horizon, False)
    rtol, atol = horizon * RC.EULER_RTOL, horizon * RC.EULER_ATOL
    assert_allclose(got[-1], want[-1], rtol=rtol, atol=atol)
    assert_allclose(got, want, rtol=rtol, atol=atol)


# ---- 4. interpolated policy ---------------------------------------------------------------------------------------
def test_table_policy_sums():
    U = _U()
    pts, want, steps, converged, ok = RRC.oracle_tri()
    q, r, discount, horizon, tol = RRC.TRI
    pair = RC.engine_pair(RC.tri_case())
    got, got_steps, got_flag = U.reward_rollout(pts, pair, _reward(NR.quadratic_reward(q, r)), discount,
                                                horizon=horizon, tol=tol, full_output=True)
    assert "k_reward_rollout<general=1" in _last_kernel()                # uploaded as SL_POLICY_TRI
    assert (got_steps, got_flag) == (steps, converged)
    assert_allclose(got[ok], want[ok], rtol=1e-10)
    exclusions.report("test_gpu_reward_rollout::test_table_policy_sums", ok, "successor")


# ---- 5. a NeuralNetwork policy: step by step inside the library ----------------------------------------------------
def test_network_policy_sums():
    import safe_learning_amd as sl
    U = _U()
    pts, want, steps, converged, rtol = RRC.oracle_network()
    q, r, discount, horizon, tol = RRC.NETWORK
    case, _, _ = RC.network_case()
    dynamics, _ = RC.engine_pair(case)
    net = sl.NeuralNetwork(RC.NETWORK_LAYERS, RC.NETWORK_ACTS, output_scale=1.0, use_bias=False,
                           input_dim=case["d"], seed=0)
    net.parameters = RC.network_parameters(case)
    policy = sl.Saturation(net, *case["saturate"])
    got, got_steps, got_flag = U.reward_rollout(RC.engine_grid(case), (dynamics, policy),
                                                _reward(NR.quadratic_reward(q, r)), discount, horizon=horizon,
                                                tol=tol, full_output=True)
    assert "k_policy_network + k_reward_rollout" in _last_kernel()
    assert (got_steps, got_flag) == (steps, converged)
    RRC.assert_sums_close(got, want, rtol)
    # from explicit points the same bits as from the cells
    assert_array_equal(U.reward_rollout(pts, (dynamics, policy), _reward(NR.quadratic_reward(q, r)), discount,
                                        horizon=horizon, tol=tol), got)


# ---- 6. the callable path on the device --------------------------------------------------------------------------
def test_callable_path_equals_fused_path():
    """The loop of the reference on device tensors, composed from the point evaluations (policy,
    dynamics, the quadratic reward at [x, u]: the same device functions), equals the fused kernel bit
    for bit on a linear case; device tensors in, device tensors out."""
    import torch
    from safe_learning_amd import _evaluate
    U = _U()
    pts, want, steps, converged, _ = RRC.oracle_linear("pendulum")
    case, matrix, discount, horizon, tol = RRC.linear_case("pendulum")
    dynamics, policy = RC.engine_pair(case)
    reward = _reward(matrix)

    def step(x):
        return _evaluate.dynamics(dynamics, x, _evaluate.policy(policy, x))

    def reward_on_states(x):
        return _evaluate.value(reward, torch.cat([x, _evaluate.policy(policy, x)], dim=1))

    x0 = torch.from_numpy(pts).cuda()
    fused = U.reward_rollout(x0, (dynamics, policy), reward, discount, horizon=horizon, tol=tol, full_output=True)
    stepwise = U.reward_rollout(x0, step, reward_on_states, discount, horizon=horizon, tol=tol, full_output=True)
    assert fused[0].is_cuda and stepwise[0].is_cuda and fused[0].dtype == torch.float64
    assert fused[1:] == stepwise[1:] == (steps, converged)
    assert_array_equal(stepwise[0].cpu().numpy(), fused[0].cpu().numpy())
    assert_array_equal(fused[0].cpu().numpy(), want)


# ---- 7. errors are errors ----------------------------------------------------------------------------------------------
def test_error_paths():
    import copy
    import torch
    import safe_learning_amd as sl
    from safe_learning_amd import _evaluate
    from safe_learning_amd._hip import HipEngineError
    from gp_cases import INFORMED
    U = _U()
    case, matrix, discount, horizon, tol = RRC.linear_case("pendulum")
    dynamics, policy = RC.engine_pair(case)
    grid = RC.engine_grid(case)
    n, d = grid.nindex, grid.ndim
    reward = _reward(matrix)
    U.reward_rollout(grid, (dynamics, policy), reward, discount, horizon=3)     # (leaves its model on the context)
    ctx = _evaluate._ctx()
    state = torch.zeros((n, d), dtype=torch.float64, device="cuda")
    sums = torch.zeros((n,), dtype=torch.float64, device="cuda")
    weights = torch.ones((4,), dtype=torch.float64, device="cuda")
    assert ctx.reward_rollout(0, n, None, 4, weights, 0.0, sums, state) == (4, False)
    with pytest.raises(HipEngineError, match="past the grid"):
        ctx.reward_rollout(0, n + 1, None, 4, weights, 0.0, sums, state)
    with pytest.raises(HipEngineError, match="bad range"):
        ctx.reward_rollout(0, n, None, 0, weights, 0.0, sums, state)
    with pytest.raises(HipEngineError, match="bad range"):
        ctx.reward_rollout(5, 2, None, 4, weights, 0.0, sums, state)
    with pytest.raises(HipEngineError, match="bad range"):
        ctx.reward_rollout(0, n, None, 4, weights, 0.0, None, state)
    with pytest.raises(HipEngineError, match="bad range"):
        ctx.reward_rollout(0, n, None, 4, None, 0.0, sums, state)
    _, builder = _evaluate._builder(d)          # (the context's own builder: it tracks what the context holds)
    builder.grid = copy.copy(grid)
    # a reward that is not quadratic: the model was uploaded without one
    builder.upload(policy, dynamics, sl.QuadraticFunction(np.eye(d)))
    with pytest.raises(HipEngineError, match=r"\(-1\).*reward is not a quadratic"):
        ctx.reward_rollout(0, n, None, 4, weights, 0.0, sums, state)
    # a per-vertex table is defined at the vertices only: one step, not two
    builder.upload(np.zeros((n, 1)), dynamics, sl.QuadraticFunction(np.eye(d)), reward=reward)
    assert ctx.reward_rollout(0, n, None, 1, weights, 0.0, sums, state) == (1, False)
    with pytest.raises(HipEngineError, match="vertices"):
        ctx.reward_rollout(0, n, None, 2, weights, 0.0, sums, state)
    # GP dynamics are not simulated inside the kernel
    gp_case = RC.make("pendulum", dict(num_points=[9, 11], n_gp=20, **INFORMED))
    builder.upload(policy, RC.engine_pair(gp_case)[0], sl.QuadraticFunction(np.eye(d)), reward=reward)
    with pytest.raises(HipEngineError, match=r"\(-3\).*GP dynamics"):
        ctx.reward_rollout(0, n, None, 4, weights, 0.0, sums, state)
    with pytest.raises(ValueError, match="callable"):
        U.reward_rollout(grid, (RC.engine_pair(gp_case)[0], policy), reward, discount)
    # an interpolated policy whose table (slot 1) was never uploaded: a fresh context
    from safe_learning_amd import _hip
    from safe_learning_amd._model import ModelBuilder
    recorder = _Recorder()
    ModelBuilder(recorder, copy.copy(grid)).upload(policy, dynamics, sl.QuadraticFunction(np.eye(d)), reward=reward)
    recorder.desc.policy.kind = _hip.POLICY_TRI
    fresh = _hip.Context()
    fresh.model_set(recorder.desc)
    with pytest.raises(HipEngineError, match="policy table .* not set"):
        fresh.reward_rollout(0, n, None, 4, weights, 0.0, sums, state)
    # the context still works
    got = U.reward_rollout(grid, (dynamics, policy), reward, discount, horizon=horizon, tol=tol)
    assert_array_equal(got, RRC.oracle_linear("pendulum")[1])


class _Recorder(object):
    """Takes a model description instead of uploading it."""

    def __init__(self):
        import torch
        self.torch_device = torch.device("cpu")

    def model_set(self, desc):
        self.desc = desc
