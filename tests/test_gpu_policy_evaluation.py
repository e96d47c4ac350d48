"""PolicyIteration.evaluate_policy: exact policy values on the GPU (needs an MI355X).

The operator rows (sl_policy_operator) against the oracle's barycentric weights and the sweep,
the solver (sl_value_solve) against dense / sparse / LP solutions of the same system."""

import json
import os

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse
import scipy.sparse.linalg
from numpy.testing import assert_allclose, assert_array_equal

import cases
import exclusions
import oracle
from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sl():
    import safe_learning_amd
    return safe_learning_amd


def _pair(sl, name, nv, gamma=0.95, project=True, **kw):
    """Engine and oracle PolicyIteration on the same case (value table: random, non-positive)."""
    from safe_learning_amd.benchmarks import build_specs
    make = cases.make_case_3d if name == "chain3" else (lambda **k: cases.make_case(name, **k))
    case = make(num_points=nv, **kw)
    d, limits = case["d"], case["limits"]
    qmat = -scipy.linalg.block_diag(np.eye(d), 0.1 * np.eye(1))
    vgrid, ovgrid = sl.GridWorld(limits, nv), oracle.GridWorld(limits, nv)
    v0 = -np.random.default_rng(4).random((vgrid.nindex, 1))
    policy, dynamics, _, _ = build_specs(case)
    opolicy, odynamics, _, _ = cases.oracle_specs(case)
    vf = sl.Triangulation(vgrid, v0, project=project)
    ovf = oracle.Triangulation(ovgrid, v0, project=project)
    rl = sl.PolicyIteration(policy, dynamics, sl.QuadraticFunction(qmat), vf, gamma=gamma)
    orl = oracle.PolicyIteration(opolicy, odynamics, oracle.QuadraticFunction(qmat), ovf, gamma=gamma)
    return rl, orl, vf, ovf


def _rows(rl):
    cols, w, r, _ = rl._rows
    return cols.cpu().numpy(), w.cpu().numpy(), r.cpu().numpy()


def _oracle_operator(orl, ovf):
    """P (sparse, the oracle's weights at the successors of the oracle's policy) and r."""
    x = orl.state_space
    u = orl.policy(x)
    nxt = orl.dynamics(x, u)
    nxt = nxt[0] if isinstance(nxt, tuple) else nxt
    w, simp = ovf._get_weights(nxt)
    n = len(x)
    P = scipy.sparse.csr_matrix((w.ravel(), (np.repeat(np.arange(n), w.shape[1]), simp.ravel())),
                                shape=(n, n))
    return P, orl.reward_function(x, u).ravel()


def test_reference_known_answer(sl):
    """The 4-state operator of the reference's test_optimization, k = 4, through sl_value_solve."""
    import torch
    from safe_learning_amd import _hip
    with open(os.path.join(ROOT, "tests", "golden", "reference_policy_evaluation.json")) as f:
        case = json.load(f)
    P, r, gamma = np.array(case["transition"]), np.array(case["reward"]), case["gamma"]
    expected = np.linalg.solve(np.eye(4) - gamma * P, r)
    ctx = _hip.Context()
    dev = ctx.torch_device
    cols = torch.from_numpy(np.tile(np.arange(4, dtype=np.int32)[:, None], (1, 4))).to(dev)
    w = torch.from_numpy(np.ascontiguousarray(P.T)).to(dev)
    rr = torch.from_numpy(r).to(dev)
    for method in (_hip.SOLVE_GMRES, _hip.SOLVE_JACOBI):
        v = torch.zeros(4, dtype=torch.float64, device=dev)
        out = ctx.value_solve(4, 4, cols, w, rr, gamma, v, 1e-14, 100000, 4, method)
        assert out["converged"], out
        assert_allclose(v.cpu().numpy(), expected, rtol=1e-12)
        # (the second row sums to 1.1: kappa = gamma * 1.1 > 1, no bound, no safeguard)
        assert out["kappa"] == gamma * np.abs(P).sum(axis=1).max()
        assert out["bound"] == np.inf
    v = torch.zeros(4, dtype=torch.float64, device=dev)
    with pytest.raises(_hip.HipEngineError, match="gamma"):
        ctx.value_solve(4, 4, cols, w, rr, 1.0, v, 1e-10, 100, 4, _hip.SOLVE_GMRES)
    bad = cols.clone()
    bad[0, 0] = 4                                        # a column outside [0, n): refused
    with pytest.raises(_hip.HipEngineError, match="columns"):
        ctx.value_solve(4, 4, bad, w, rr, gamma, v, 1e-10, 100, 4, _hip.SOLVE_GMRES)


@pytest.mark.parametrize("name,nv,kw", [
    ("pendulum", [9, 9], dict(dynamics="linear")),
    ("1d", 25, dict()),
])
def test_lp_equivalence(sl, name, nv, kw):
    from scipy.optimize import linprog
    rl, orl, vf, ovf = _pair(sl, name, nv, gamma=0.9, **kw)
    P, r = _oracle_operator(orl, ovf)
    n = P.shape[0]
    A = scipy.sparse.identity(n, format="csr") - rl.gamma * P
    exact = scipy.sparse.linalg.spsolve(A.tocsc(), r)
    res = rl.evaluate_policy(tol=1e-13, method="gmres")
    got = vf._host_parameters()[:, 0]
    # (a successor clipped onto an upper face can get a weight of a few ulp below zero)
    assert rl.last_solve["negative_rows"] == 0 or _rows(rl)[1].min() > -1e-12
    assert res == rl.last_residual <= 1e-13 * np.abs(r).max()
    assert_allclose(got, exact, rtol=1e-10, atol=1e-10 * np.abs(exact).max())
    # the reference's LP: max sum V  s.t.  V - gamma P V <= r
    lp = linprog(-np.ones(n), A_ub=A, b_ub=r, bounds=[(None, None)] * n, method="highs")
    assert lp.status == 0
    assert_allclose(got, lp.x, rtol=1e-6, atol=1e-6 * np.abs(lp.x).max())


@pytest.mark.parametrize("name,nv,kw", [
    ("1d", 33, dict()),
    ("pendulum", [15, 17], dict(dynamics="linear")),
    ("pendulum", [15, 15], dict(dynamics="analytic")),
    ("cartpole", [5, 6, 5, 6], dict(dynamics="analytic")),
    ("pendulum", [13, 13], dict(n_gp=70)),
    ("cartpole", [4, 5, 4, 5], dict(n_gp=90)),
    ("chain3", [5, 6, 7], dict(dynamics="linear")),           # k_policy_operator_rows<3>, rows of 4 entries
])
def test_rows_versus_sweep_and_oracle(sl, name, nv, kw):
    from test_policy_rows_host import load_shim, _Rows
    rl, orl, vf, ovf = _pair(sl, name, nv, **kw)
    rl._upload(rl.policy)
    _build_rows(rl)
    cols, w, r = _rows(rl)
    table = vf._host_parameters()[:, 0].copy()
    expected = rl.future_values()[:, 0]
    kernel = rl._ctx.lib.sl_last_kernel(rl._ctx.handle).decode()
    shim = _Rows(load_shim(), vf)
    got = shim.combine(cols, w, r, rl.gamma, table)
    print("compared sweep: %s" % kernel)
    assert kernel
    # The rows take their weights from sl_tri_locate_fast<D>, as the sweeps with compile-time dimensions
    # do: bit for bit.  A 3-D grid is swept by the runtime-dimension k_bellman<A, 0, 0>, whose
    # sl_tri_eval sums the same barycentric weights in another order: agreement to rounding (the
    # bound of the GP cases), and the kernel name says that this is the sweep compared.
    runtime_dims = name == "chain3"
    assert ("d=3" in kernel) == runtime_dims, kernel
    if "n_gp" in kw or runtime_dims:
        assert_allclose(got, expected, rtol=1e-12, atol=1e-12 * np.abs(expected).max(), err_msg=kernel)
    else:
        assert_array_equal(got, expected, err_msg=kernel)
    # the same through the device's row combine (k_value_matvec): two Jacobi steps, out of matvecs,
    # return the first step's iterate r + gamma P V
    import torch
    from safe_learning_amd import _hip
    v = torch.from_numpy(table.copy()).to(rl._ctx.torch_device)
    out = rl._ctx.value_solve(len(table), cols.shape[0], rl._rows[0], rl._rows[1], rl._rows[2], rl.gamma,
                              v, 0.0, 2, 2, _hip.SOLVE_JACOBI)
    assert out["matvecs"] == 2 and not out["converged"]
    device = v.cpu().numpy()
    assert_array_equal(device, got)
    assert out["residual_inf"] == np.abs(shim.combine(cols, w, r, rl.gamma, got) - got).max()
    # the rows against the oracle's weights at the oracle's successors
    P, orr = _oracle_operator(orl, ovf)
    n = P.shape[0]
    mine = scipy.sparse.csr_matrix((w.T.ravel(), (np.repeat(np.arange(n), w.shape[0]), cols.T.ravel())),
                                   shape=(n, n))
    tol = 1e-9 if "n_gp" in kw else 1e-12
    assert abs(mine - P).max() <= tol
    assert_allclose(r, orr, rtol=1e-12, atol=1e-14)


def _build_rows(rl):
    """The rows of rl's current policy on rl's context (what evaluate_policy builds first)."""
    import torch
    n, k = rl.discretization.nindex, rl.discretization.ndim + 1
    dev = rl._ctx.torch_device
    rl._rows = (torch.empty((k, n), dtype=torch.int32, device=dev),
                torch.empty((k, n), dtype=torch.float64, device=dev),
                torch.empty(n, dtype=torch.float64, device=dev),
                torch.empty(2, dtype=torch.float64, device=dev))
    rl._rows_key = (n, k, str(dev))
    rl._ctx.policy_operator(0, n, *rl._rows)


@pytest.mark.parametrize("name,nv,kw,policy", [
    ("1d", 41, dict(), "own"),
    ("pendulum", [17, 17], dict(dynamics="analytic"), "own"),
    ("pendulum", [15, 15], dict(dynamics="analytic"), "constant"),
    ("pendulum", [15, 15], dict(dynamics="analytic"), "table_same_grid"),
    ("pendulum", [15, 15], dict(dynamics="analytic"), "table_other_grid"),
    ("pendulum", [15, 15], dict(dynamics="analytic"), "network"),
    ("pendulum", [15, 15], dict(dynamics="analytic"), "greedy"),
    ("pendulum", [13, 13], dict(n_gp=70), "own"),
    ("cartpole", [5, 5, 5, 5], dict(n_gp=90), "greedy"),
])
def test_fixed_point(sl, name, nv, kw, policy):
    """After evaluate_policy the value-iteration sweep hardly moves the table (its residual is the
    solve's, up to rounding) and the table is within `bound` of where many sweeps lead."""
    rl, orl, vf, ovf = _pair(sl, name, nv, **kw)
    grid = vf.discretization
    m = 1
    if policy == "constant":
        rl.policy = sl.ConstantFunction(np.array([0.3]))
    elif policy == "table_same_grid":
        rl.policy = sl.Triangulation(grid, np.sin(np.arange(grid.nindex))[:, None] * 0.5)
    elif policy == "table_other_grid":
        pgrid = sl.GridWorld(grid.limits, [5, 7])
        rl.policy = sl.Triangulation(pgrid, np.cos(np.arange(pgrid.nindex))[:, None] * 0.5)
    elif policy == "network":
        rl.policy = sl.NeuralNetwork([8, m], ["tanh", "tanh"], output_scale=0.5, use_bias=True,
                                     input_dim=grid.ndim, seed=3)
    elif policy == "greedy":
        actions = np.linspace(-1, 1, 5)[:, None]
        rl.value_iteration(actions)
        rl.value_iteration(actions)
    start = vf._host_parameters().copy()
    res = rl.evaluate_policy(tol=1e-11, method="gmres" if policy in ("own", "greedy") else "jacobi")
    s = rl.last_solve
    assert s["kappa"] <= rl.gamma * (1 + 1e-12) and s["negative_rows"] == 0
    assert res == s["residual"] <= 1e-11 * np.abs(rl._rows[2].cpu().numpy()).max()
    solved = vf._host_parameters().copy()
    vi = sl.PolicyIteration(rl.policy, rl.dynamics, rl.reward_function, vf, gamma=rl.gamma)
    r1 = vi.value_iteration()
    assert r1 <= s["residual"] * (1 + 1e-6) + 1e-12 * np.abs(solved).max()
    # many sweeps from the same start approach the same table
    vf.parameters = start
    for _ in range(int(np.log(1e-13) / np.log(rl.gamma)) + 50):
        last = vi.value_iteration()
    far = vf._host_parameters()[:, 0]
    assert last < 1e-10 * np.abs(far).max()
    assert np.abs(far - solved[:, 0]).max() <= s["bound"] + last / (1 - rl.gamma) + 1e-12 * np.abs(far).max()


def test_policy_iteration_loop(sl):
    """evaluate_policy + discrete_policy_optimization until the policy stops changing, against
    NumPy (spsolve on the oracle's operator, the oracle's greedy step).

    The evaluated policy is the per-vertex action table of the greedy step.  (Interpolating that
    table as a Triangulation at its own vertices - what reusing the greedy Triangulation as the
    policy would do - extrapolates at many vertices in the reference's point location, differently
    in the oracle and the engine, and the loop can then cycle.)"""
    rl, orl, vf, ovf = _pair(sl, "pendulum", [15, 15], gamma=0.9, dynamics="analytic")
    actions = np.linspace(-1, 1, 5)[:, None]
    grid, ogrid = vf.discretization, ovf.discretization
    table = np.zeros((grid.nindex, 1))
    orl.policy = oracle.Triangulation(ogrid, table.copy())
    x = orl.state_space
    for it in range(30):
        rl.policy = table.copy()
        rl.evaluate_policy(tol=1e-13)
        u = orl.policy.parameters
        nxt = orl.dynamics(x, u)
        w, simp = ovf._get_weights(nxt)
        n = len(x)
        P = scipy.sparse.csr_matrix((w.ravel(), (np.repeat(np.arange(n), w.shape[1]), simp.ravel())),
                                    shape=(n, n))
        r = orl.reward_function(x, u).ravel()
        ovf.parameters = scipy.sparse.linalg.spsolve(
            (scipy.sparse.identity(n, format="csr") - orl.gamma * P).tocsc(), r)[:, None]
        assert_allclose(vf._host_parameters()[:, 0], ovf.parameters[:, 0], rtol=1e-9,
                        atol=1e-9 * np.abs(ovf.parameters).max(), err_msg=str((it, rl.last_solve)))
        rl.discrete_policy_optimization(actions)
        orl.discrete_policy_optimization(actions)
        new = rl.policy._host_parameters().copy()
        assert_array_equal(new, orl.policy.parameters)
        if np.array_equal(new, table):
            break
        table = new
    assert it < 29                                       # the policy stopped changing


def test_determinism_methods_and_errors(sl):
    from safe_learning_amd.reinforcement_learning import OptimizationError
    rl, orl, vf, ovf = _pair(sl, "pendulum", [21, 23], dynamics="analytic")
    start = vf._host_parameters().copy()
    rl.evaluate_policy(tol=1e-12, method="gmres")
    first = vf._host_parameters().copy()
    vf.parameters = start
    rl.evaluate_policy(tol=1e-12, method="gmres")
    assert_array_equal(vf._host_parameters(), first)            # bit-identical tables
    g = rl.last_solve
    vf.parameters = start
    rl.evaluate_policy(tol=1e-12, method="jacobi")
    j = rl.last_solve
    assert j["jacobi_cycles"] == 0 and j["method"] == "jacobi"
    scale = np.abs(first).max()
    assert np.abs(vf._host_parameters() - first).max() <= g["bound"] + j["bound"] + 1e-12 * scale
    # out of matvecs: OptimizationError, the table as it was
    vf.parameters = start
    for method in ("gmres", "jacobi"):
        for budget in (2, 7, 40):
            with pytest.raises(OptimizationError, match="Optimization problem is"):
                rl.evaluate_policy(tol=1e-14, max_matvecs=budget, method=method, restart=4)
            assert rl.last_solve["matvecs"] <= budget
            assert_array_equal(vf._host_parameters(), start)
    with pytest.raises(ValueError):
        rl.evaluate_policy(method="cg")
    rl.gamma = 1.0
    with pytest.raises(ValueError):
        rl.evaluate_policy()
    rl.gamma = 0.95
    with pytest.raises(NotImplementedError, match="evaluate_policy"):
        rl.optimize_value_function()


def test_negative_rows_reported_without_projection(sl):
    """Successors that leave the grid without projection are extrapolated: negative weights."""
    rl, orl, vf, ovf = _pair(sl, "pendulum", [9, 9], project=False, dynamics="linear")
    rl.policy = sl.ConstantFunction(np.array([1.0]))
    from safe_learning_amd.reinforcement_learning import OptimizationError
    try:                                     # kappa > 1: convergence is not guaranteed
        rl.evaluate_policy(tol=1e-8, method="gmres")
    except OptimizationError:
        pass
    assert rl.last_solve["negative_rows"] > 0
    assert rl.last_solve["kappa"] > rl.gamma


def test_policy_tensor_edited_in_place(sl):
    import torch
    rl, orl, vf, ovf = _pair(sl, "pendulum", [15, 15], dynamics="analytic")
    grid = vf.discretization
    table = torch.full((grid.nindex, 1), 0.2, dtype=torch.float64, device=rl._ctx.torch_device)
    rl.policy = table
    rl.evaluate_policy(tol=1e-12)
    table.fill_(-0.4)                                      # in place: same pointer, new actions
    rl.evaluate_policy(tol=1e-12)
    got = vf._host_parameters().copy()
    fresh, _, fvf, _ = _pair(sl, "pendulum", [15, 15], dynamics="analytic")
    fresh.policy = sl.ConstantFunction(np.array([-0.4]))
    fvf.parameters = got
    fresh.evaluate_policy(tol=1e-12)
    assert np.abs(fvf._host_parameters() - got).max() <= 2 * fresh.last_solve["bound"] + 1e-12


def test_full_size_c5_policy(sl):
    """64^4 with the 1024-point GP and the greedy table policy of three max sweeps: converges, and
    sampled vertices satisfy V = r + gamma V(f(x, pi(x))) against the oracle."""
    from safe_learning_amd.benchmarks import headline_case, build_specs
    case = headline_case(num_points=64, n_gp=1024)
    policy, dynamics, _, _ = build_specs(case)
    grid = sl.GridWorld(case["limits"], case["num_points"])
    vf = sl.Triangulation(grid, np.zeros((grid.nindex, 1)), project=True)
    reward = sl.QuadraticFunction(-scipy.linalg.block_diag(0.1 * np.eye(4), 0.1 * np.eye(1)))
    rl = sl.PolicyIteration(policy, dynamics, reward, vf, gamma=0.98)
    actions = np.linspace(-1, 1, 9)[:, None]
    for _ in range(3):
        rl.value_iteration(actions)
    rl.discrete_policy_optimization(actions)
    rl.evaluate_policy(tol=1e-10)
    s = rl.last_solve
    assert s["residual"] <= 1e-10 * 10.0 and s["kappa"] <= 0.98 * (1 + 1e-12)
    v = vf._host_parameters()[:, 0]
    rng = np.random.default_rng(0)
    idx = rng.choice(grid.nindex, 2000, replace=False)
    x = grid.all_points[idx]
    u = rl.policy._host_parameters()[idx]
    opolicy, odynamics, _, _ = cases.oracle_specs(case)
    nxt = odynamics(x, u)
    nxt = nxt[0] if isinstance(nxt, tuple) else nxt
    ovf = oracle.Triangulation(oracle.GridWorld(case["limits"], case["num_points"]), v[:, None], project=True)
    target = oracle.QuadraticFunction(-scipy.linalg.block_diag(0.1 * np.eye(4), 0.1 * np.eye(1)))(x, u)[:, 0] \
        + 0.98 * ovf(nxt)[:, 0]
    # (successors on a face shared by simplices whose interpolations differ - extrapolated
    # upper faces - may be located in another simplex by the oracle: tests/exclusions.py)
    # and a handful of successors the two locate differently on extrapolated upper faces)
    ok = ~exclusions.ambiguous_points(ovf, nxt)
    close = np.abs(v[idx] - target) <= 1e-8 * np.abs(v).max()
    assert ok.mean() > 0.99 and np.sum(ok & ~close) <= 4, np.flatnonzero(ok & ~close)


def test_diverging_solve_is_not_converged(sl):
    """kappa > 1: one row diverges (v0 <- 1 + 0.9 * 3 v0), one converges (v1 <- 1 + 0.9 * 0.5 v1).
    The iterate overflows; the solve must report that, never a small residual."""
    import torch
    from safe_learning_amd import _hip
    ctx = _hip.Context()
    dev = ctx.torch_device
    cols = torch.tensor([[0, 1]], dtype=torch.int32, device=dev)
    w = torch.tensor([[3.0, 0.5]], dtype=torch.float64, device=dev)
    r = torch.tensor([1.0, 1.0], dtype=torch.float64, device=dev)
    for method in (_hip.SOLVE_JACOBI, _hip.SOLVE_GMRES):
        for restart in (1, 4, 16):
            v = torch.zeros(2, dtype=torch.float64, device=dev)
            out = ctx.value_solve(2, 1, cols, w, r, 0.9, v, 1e-10, 100000, restart, method)
            got = v.cpu().numpy()
            if method == _hip.SOLVE_GMRES and out["converged"]:
                # (I - gamma P) is invertible here: GMRES may solve it although Jacobi diverges -
                # then with the true solution and a true residual
                assert_allclose(got, [1 / (1 - 2.7), 1 / (1 - 0.45)], rtol=1e-9)
                assert out["residual_inf"] <= 1e-10
                continue
            assert not out["converged"], (method, restart, out)
            assert out["residual_inf"] > 1.0, (method, restart, out)
            assert out["matvecs"] <= 100000
            assert out["kappa"] == 0.9 * 3.0 and out["bound"] == np.inf


def test_safeguard_falls_back_to_jacobi_on_the_device(sl):
    """A random convex operator on which GMRES(4) cycles do worse than kappa^s: the device takes
    Jacobi cycles from the better iterate and converges, like the NumPy model of DESIGN.md."""
    import torch
    from safe_learning_amd import _hip
    from test_policy_rows_host import solve_model
    rng = np.random.default_rng(0)
    n, k, gamma, m = 300, 3, 0.98, 4
    cols = rng.integers(0, n, size=(n, k))
    w = rng.random((n, k))
    w /= w.sum(axis=1, keepdims=True)
    P = np.zeros((n, n))
    np.add.at(P, (np.repeat(np.arange(n), k), cols.ravel()), w.ravel())
    r = rng.normal(size=n)
    exact = np.linalg.solve(np.eye(n) - gamma * P, r)
    _, model = solve_model(P, r, gamma, np.zeros(n), 1e-10, m, 20000)
    ctx = _hip.Context()
    dev = ctx.torch_device
    v = torch.zeros(n, dtype=torch.float64, device=dev)
    out = ctx.value_solve(n, k, torch.from_numpy(np.ascontiguousarray(cols.T, dtype=np.int32)).to(dev),
                          torch.from_numpy(np.ascontiguousarray(w.T)).to(dev), torch.from_numpy(r).to(dev),
                          gamma, v, 1e-10, 20000, m, _hip.SOLVE_GMRES)
    print("device", out, "model", model)
    assert model["jacobi_cycles"] > 0
    assert out["converged"] and out["jacobi_cycles"] > 0, out
    # the device takes the model's decisions: same cycles, safeguard cycles and matvecs
    assert (out["matvecs"], out["cycles"], out["jacobi_cycles"]) == \
        (model["matvecs"], model["cycles"], model["jacobi_cycles"])
    assert np.abs(v.cpu().numpy() - exact).max() <= out["bound"] * (1 + 1e-6) + 1e-12
