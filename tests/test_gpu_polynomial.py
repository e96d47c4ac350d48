"""Polynomial dynamics on the GPU (SL_DYN_POLYNOMIAL: csrc/sl_polynomial.h through the sweep, point-evaluation,
rollout and Bellman kernels; needs an MI355X) against the NumPy restatement (tests/np_polynomial.py).

The arithmetic is multiplications and additions in one stated order, compiled without contraction, and has no
transcendental: the kernels' next states equal the restatement's BIT FOR BIT, after one step and after three
hundred.  That is derived, not measured - every comparison of states below is an equality of bit patterns.
Cases, conditions and NumPy results: tests/polynomial_cases.py.
"""

import os
import signal

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import np_reward_rollout as NR
import oracle
import polynomial_cases as PC
import reward_rollout_cases as RRC
import rollout_cases as RC
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

TEST_SECONDS = 120


@pytest.fixture(autouse=True)
def _time_limit():
    """Every test runs under its own time limit: SIGALRM with its default action ends the process
    (also while it waits inside a HIP call), so nothing more is started on the GPU after a hang."""
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    signal.alarm(TEST_SECONDS)
    yield
    signal.alarm(0)


@pytest.fixture(scope="module")
def sl():
    import safe_learning_amd
    return safe_learning_amd


def _last_kernel():
    from safe_learning_amd import _evaluate
    return _evaluate._ctx().last_kernel()


# ---- 1. point evaluation ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", PC.KEYS)
def test_point_evaluation_bit_exact(sl, key):
    PC.check_systems()
    spec, truth = PC.system(key), PC.truth(key)
    for n in PC.POINT_COUNTS:
        states, actions = PC.points(key, n)
        got = spec(states, actions)
        PC.assert_same_bits(got, truth(states, actions), "%s, %d points" % (key, n))
        # compiled for (d, 1) where the action is one column, reading its dimensions otherwise
        want = spec.state_dim if spec.action_dim == 1 and spec.state_dim <= 4 else 0
        assert "k_det_sweep<general=0, d=%d, dynamics=5" % want in _last_kernel()


# ---- 2. rollouts -----------------------------------------------------------------------------------------------
def test_vdp_roa(sl):
    data = np.load(os.path.join(GOLDEN_DIR, "reference_vanderpol.npz"))
    roa, traj = PC.vdp_roa()
    grid = sl.GridWorld([[-1, 1]] * 2, PC.VDP_NUM_POINTS)
    pair = (PC.system("vdp"), PC.engine_policy("vdp"))
    ends = []
    for chunk in (0, 1, 7):
        got, got_traj = sl.compute_roa(grid, pair, horizon=PC.VDP_HORIZON, tol=PC.VDP_TOL, no_traj=False,
                                       steps_per_launch=chunk)
        assert "k_rollout<general=0, d=2, dynamics=5>" in _last_kernel()
        assert_array_equal(got, roa)
        assert_array_equal(got, data["roa"])
        ends.append(got_traj[:, :, -1])
        PC.assert_same_bits(got_traj[:, :, :12], traj[:, :, :12], "first 12 steps, steps_per_launch %d" % chunk)
        PC.assert_same_bits(ends[-1][roa], traj[:, :, -1][roa], "in-ROA end states, steps_per_launch %d" % chunk)
        # every state of every trajectory, the ones that left the finite numbers included
        PC.assert_same_bits(got_traj, traj, "all %d steps, steps_per_launch %d" % (PC.VDP_HORIZON, chunk))
    assert_allclose(ends[0][roa], data["roa_end"][roa], rtol=0, atol=RC.ROA_END_STATE_ATOL)
    only = sl.compute_roa(grid, pair, horizon=PC.VDP_HORIZON, tol=PC.VDP_TOL)
    assert_array_equal(only, roa)


def test_map1_roa(sl):
    pts, roa = PC.map1_roa()
    pair = (PC.system("map1"), PC.engine_policy("map1"))
    for chunk in (0, 1, 7):
        got = sl.compute_roa(pts, pair, horizon=PC.MAP1_HORIZON, tol=PC.MAP1_TOL, steps_per_launch=chunk)
        assert_array_equal(got, roa)
        assert got.sum() == 47
    assert "k_rollout<general=0, d=1, dynamics=5>" in _last_kernel()


@pytest.mark.parametrize("key", ["chain3", "full", "duffing-u"])
def test_trajectories_bit_exact(sl, key):
    states, actions = PC.trajectory_truth(key)
    for chunk in (0, 1, 7):
        got_states, got_actions = sl.compute_trajectory(PC.system(key), PC.engine_policy(key), PC.start_states(key),
                                                        states.shape[1], steps_per_launch=chunk)
        PC.assert_same_bits(got_states, states, "%s states, steps_per_launch %d" % (key, chunk))
        PC.assert_same_bits(got_actions, actions, "%s actions, steps_per_launch %d" % (key, chunk))
    assert "dynamics=5" in _last_kernel()


# ---- 3. reward_rollout -------------------------------------------------------------------------------------------
def test_vdp_reward_rollout(sl):
    """All 441 cells of [-1/3, 1/3]^2 converge.  The dynamics are the restatement's bit for bit and policy and
    reward are the linear / quadratic forms tests/test_gpu_reward_rollout.py compares with equality under a
    linear system: the same equality here, whatever the launches are."""
    limits, num = [[-1. / 3, 1. / 3]] * 2, 21
    matrix, discount, horizon, tol = NR.quadratic_reward(np.diag([1.0, 2.0]), 1.2), 0.9, 400, 1e-3
    pts = oracle.GridWorld(limits, num).all_points
    want, steps, converged, maxima = NR.reward_rollout(pts, PC.truth("vdp"), PC.oracle_policy("vdp"), matrix,
                                                       discount, horizon, tol)
    RRC._check_margin("vdp", maxima, tol, steps, converged)
    assert converged and np.isfinite(want).all() and 20 < steps < horizon
    pair, reward = (PC.system("vdp"), PC.engine_policy("vdp")), sl.QuadraticFunction(matrix)
    for chunk in (0, 1, 7):
        got, got_steps, got_flag = sl.reward_rollout(sl.GridWorld(limits, num), pair, reward, discount,
                                                     horizon=horizon, tol=tol, full_output=True,
                                                     steps_per_launch=chunk)
        assert (got_steps, got_flag) == (steps, converged)
        RRC.assert_sums_close(got, want, 0.0)
        assert_array_equal(got, want)
        assert "k_reward_rollout<general=0, d=2, dynamics=5>" in _last_kernel()


# ---- 4. Lyapunov ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(PC.LYAPUNOV))
def test_update_safe_set(sl, key):
    olyap, initial = PC.lyapunov_truth(key)
    name, limits, num_points, _ = PC.LYAPUNOV[key]
    grid = sl.GridWorld(limits, num_points)
    lyap = sl.Lyapunov(grid, sl.QuadraticFunction(PC.lyapunov_matrix(key)), PC.system(name), PC.LYAPUNOV_LF,
                       PC.LYAPUNOV_LV, 0.0, PC.engine_policy(name), initial_set=initial.copy())
    lyap.update_safe_set()
    assert_array_equal(lyap.safe_set, olyap.safe_set)
    assert lyap.c_max == olyap.c_max
    note = lyap._ctx.last_kernel()
    want = {"vdp": "k_det_sweep<general=0, d=2, dynamics=5, pow2=0>",
            "vdp-pow2": "k_det_sweep<general=0, d=2, dynamics=5, pow2=1>",
            "chain3": "k_det_sweep<general=0, d=0, dynamics=5, pow2=0>"}[key]
    assert want in note, note
    # the next states the sweep decided on, cell by cell
    x = olyap.discretization.all_points
    got = PC.system(name)(x, olyap.policy(x))
    PC.assert_same_bits(got, PC.truth(name)(x, olyap.policy(x)), key)


# ---- 5. PolicyIteration ----------------------------------------------------------------------------------------------
def _duffing_pair(sl, spec, v0):
    import scipy.linalg
    limits, num = [[-1, 1]] * 2, [15, 13]
    qmat = -scipy.linalg.block_diag(np.eye(2), 0.1 * np.eye(1))
    vgrid, ovgrid = sl.GridWorld(limits, num), oracle.GridWorld(limits, num)
    vf = sl.Triangulation(vgrid, v0.copy(), project=True)
    ovf = oracle.Triangulation(ovgrid, v0.copy(), project=True)
    rl = sl.PolicyIteration(sl.Triangulation(vgrid, np.zeros((vgrid.nindex, 1))), spec, sl.QuadraticFunction(qmat),
                            vf, gamma=0.95)
    orl = oracle.PolicyIteration(oracle.Triangulation(ovgrid, np.zeros((ovgrid.nindex, 1))),
                                 PC.np_polynomial.NumpyPolynomial(spec), oracle.QuadraticFunction(qmat), ovf,
                                 gamma=0.95)
    return rl, orl, vf, ovf


def test_policy_iteration(sl):
    import scipy.sparse
    import scipy.sparse.linalg
    v0 = -np.random.default_rng(4).random((15 * 13, 1))
    rl, orl, vf, ovf = _duffing_pair(sl, PC.system("duffing-u"), v0)
    actions = np.linspace(-1, 1, 9)[:, None]
    # discrete_policy_optimization: every action value, every vertex (no exclusions)
    q = rl.discrete_policy_optimization(actions, return_values=True).cpu().numpy()
    oq, obest = orl.discrete_policy_optimization(actions)
    assert_allclose(q, oq, rtol=1e-9, atol=1e-12)
    top2 = np.sort(oq, axis=1)[:, -2:]
    tie = np.abs(top2[:, 1] - top2[:, 0]) <= 1e-9 * np.abs(top2[:, 1])
    assert not np.any((rl.policy.parameters[:, 0] != actions[obest, 0]) & ~tie)
    assert len(np.unique(obest)) > 2                                       # a policy that depends on the state
    # three Bellman optimality sweeps (the successor cache serves the second and third)
    for sweep in range(3):
        old = ovf.parameters.copy()
        oq, _ = orl.discrete_policy_optimization(actions)
        res = rl.value_iteration(actions)
        ovf.parameters = oq.max(axis=1)[:, None]
        assert_allclose(vf.parameters[:, 0], ovf.parameters[:, 0], rtol=1e-9, atol=1e-12, err_msg=str(sweep))
        assert_allclose(res, np.max(np.abs(ovf.parameters - old)), rtol=1e-9)
        vf.parameters = ovf.parameters.copy()                              # the same table into the next sweep
    assert rl.successor_cache_info["hits"] >= 2
    # exact policy evaluation of the greedy table against a sparse solve on the oracle's operator
    x = orl.state_space
    u = orl.policy.parameters
    rl.policy = u.copy()
    rl.evaluate_policy(tol=1e-13)
    w, simp = ovf._get_weights(orl.dynamics(x, u))
    n = len(x)
    P = scipy.sparse.csr_matrix((w.ravel(), (np.repeat(np.arange(n), w.shape[1]), simp.ravel())), shape=(n, n))
    exact = scipy.sparse.linalg.spsolve((scipy.sparse.identity(n, format="csr") - orl.gamma * P).tocsc(),
                                        orl.reward_function(x, u).ravel())
    assert_allclose(vf._host_parameters()[:, 0], exact, rtol=1e-9, atol=1e-9 * np.abs(exact).max())


def test_new_table_drops_what_was_derived_from_the_old_one(sl):
    """One coefficient changes (a new PolynomialSystem on the same PolicyIteration): the term table is not in
    the model description's bytes, yet the next sweeps must be a fresh context's bit for bit - nothing of the
    successor cache, the policy-select arrays or the operator rows of the old dynamics may survive."""
    v0 = -np.random.default_rng(5).random((15 * 13, 1))
    actions = np.linspace(-1, 1, 9)[:, None]
    rl, _, vf, _ = _duffing_pair(sl, PC.system("duffing-u"), v0)
    for _ in range(2):
        rl.value_iteration(actions)                                        # fills the cache, then hits it
    rl.value_iteration()                                                   # the select arrays of the greedy policy
    rl.evaluate_policy(tol=1e-12)
    assert rl.successor_cache_info["hits"] >= 1
    table, greedy = vf._host_parameters().copy(), rl.policy.parameters.copy()
    changed = PC.duffing(-0.4)
    rl.dynamics = changed
    fresh, _, fresh_vf, _ = _duffing_pair(sl, changed, table)
    fresh.policy = sl.Triangulation(fresh_vf.discretization, greedy.copy())
    for step in ("policy sweep", "max sweep", "max sweep again", "evaluate"):
        if step == "policy sweep":
            a, b = rl.value_iteration(), fresh.value_iteration()
        elif step == "evaluate":
            rl.evaluate_policy(tol=1e-12)
            fresh.evaluate_policy(tol=1e-12)
            a = b = 0.0
        else:
            a, b = rl.value_iteration(actions), fresh.value_iteration(actions)
        assert a == b, step
        PC.assert_same_bits(vf._host_parameters(), fresh_vf._host_parameters(), step)
        assert_array_equal(rl.policy.parameters, fresh.policy.parameters)
    # and the change is one the sweeps see
    other, _, other_vf, _ = _duffing_pair(sl, PC.system("duffing-u"), table)
    other.value_iteration(actions)
    fresh2, _, fresh2_vf, _ = _duffing_pair(sl, changed, table)
    fresh2.value_iteration(actions)
    assert not np.array_equal(other_vf._host_parameters(), fresh2_vf._host_parameters())


# ---- 6. errors ---------------------------------------------------------------------------------------------------------
def test_errors_name_the_library_message(sl):
    from safe_learning_amd import _hip
    ctx = _hip.Context()
    rows = np.zeros(_hip.POLY_MAX_TERMS + 1, dtype=np.int32)
    coef = np.ones(_hip.POLY_MAX_TERMS + 1)
    expo = np.zeros((_hip.POLY_MAX_TERMS + 1, 3), dtype=np.uint8)
    ctx.last_kernel()
    with pytest.raises(sl.HipEngineError, match="SL_POLY_MAX_TERMS"):
        ctx.dynamics_polynomial_set(2, 1, rows, coef, expo, 10, 0.01)
    expo[0] = [_hip.POLY_MAX_DEGREE, 1, 0]
    with pytest.raises(sl.HipEngineError, match="SL_POLY_MAX_DEGREE"):
        ctx.dynamics_polynomial_set(2, 1, rows[:1], coef[:1], expo[:1], 10, 0.01)
    with pytest.raises(sl.HipEngineError, match="row 2 of 2 states"):
        ctx.dynamics_polynomial_set(2, 1, rows[:1] + 2, coef[:1], expo[:1] * 0, 10, 0.01)
    # kind 5 without a table, then with a table of other dimensions
    desc = _hip.ModelDesc()
    desc.grid = sl.GridWorld([[-1, 1]] * 2, 5)._desc()
    desc.policy.kind, desc.policy.m = _hip.POLICY_CONST, 1
    desc.dynamics.kind = _hip.DYN_POLYNOMIAL
    desc.value.kind = _hip.V_QUADRATIC
    with pytest.raises(sl.HipEngineError, match="without a term table"):
        ctx.model_set(desc)
    ctx.dynamics_polynomial_set(3, 1, rows[:1], coef[:1], np.zeros((1, 4), dtype=np.uint8), 10, 0.01)
    with pytest.raises(sl.HipEngineError, match="3 states and 1 actions, the model has 2 and 1"):
        ctx.model_set(desc)
    ctx.dynamics_polynomial_set(2, 1, rows[:1], coef[:1], np.zeros((1, 3), dtype=np.uint8), 10, 0.01)
    ctx.model_set(desc)
    assert ctx.last_kernel() == ""                                          # no kernel was launched
    # the Python layer: a grid of another dimension than the system, before anything is uploaded
    with pytest.raises(ValueError, match="has 2 states, the grid has 3 dimensions"):
        sl.compute_roa(sl.GridWorld([[-1, 1]] * 3, 3), (PC.system("vdp"), sl.LinearSystem((np.zeros((1, 3)),))))
    with pytest.raises(ValueError, match="total degree"):
        sl.PolynomialSystem([[(1.0, (_hip.POLY_MAX_DEGREE, 1))]], 1, 1)
    # no action tangents: the library's own refusal names the kind
    import torch
    lyap_desc = desc
    out = torch.zeros((4, 1), dtype=torch.float64, device=ctx.torch_device)
    pts = torch.zeros((4, 2), dtype=torch.float64, device=ctx.torch_device)
    with pytest.raises(sl.HipEngineError, match="SL_DYN_POLYNOMIAL"):
        ctx.decrease_gradient(4, pts, None, out)
    ctx.model_set(lyap_desc)
    ctx.close()
