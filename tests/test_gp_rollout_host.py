"""CPU checks of the closed-loop rollouts of a GP's posterior mean (``to_mean_function()``,
safe_learning_amd/csrc/sl_gp_rollout.h).

The per-trajectory header is compiled with g++ into a test-only shim (tests/hostsim/gp_rollout.cpp):

* one step equals the mean of ``sl_pg_head`` + ``sl_pg_linear_part`` (tests/hostsim/policy_grad.cpp) bit for bit;
* trajectories, region-of-attraction masks and returns are compared with the float64 NumPy reference
  (tests/np_gp_rollout.py): masks without a flip, states and returns within 32 x the reference's own distance
  to its long-double companion plus 4 ulps of the state scale (the derivation is in that module);
* the chunk rule, the Python layer on a stand-in engine, and the resources of the new kernels.

Measured here (printed by the tests; float64 on x86-64 with glibc), largest |header - reference| / bound:
trajectories 1d 0.057, cartpole 0.042, cartpole-stack 0.053, pendulum 0.057, pendulum-stack 0.056, no-observations
0.029, notebook-kernels 0.086, table-policy 0.043; returns pendulum-stack 0.059, cartpole 0.037 (profiles/gp_rollout.md
has the GPU's figures beside them).
"""

import ctypes as C
import os
import sys

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import hostsim_build
import np_gp_rollout as R
from conftest import ROOT
from safe_learning_amd import _hip
from safe_learning_amd import functions as F
from safe_learning_amd import utilities as U
from safe_learning_amd._model import ModelBuilder

ALL_CASES = sorted(R.ROA_CASES) + sorted(R.OTHER_CASES)


class _Head(C.Structure):
    """SlPgHead of safe_learning_amd/csrc/sl_policy_grad.h (= SlGpHeadView of sl_gp_rollout.h)."""
    _fields_ = [("n", C.c_int), ("n_pad", C.c_int), ("dout", C.c_int), ("col0", C.c_int), ("variance", C.c_double),
                ("inv_ls", C.c_void_p), ("xs", C.c_void_p), ("alpha", C.c_void_p), ("kernel", C.c_void_p)]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    lib = hostsim_build.shared("gp_rollout.cpp", tmp_path_factory.mktemp("gp_rollout"), hostsim_build.SHIM_FLAGS)
    return lib


@pytest.fixture(scope="module")
def pg_shim(tmp_path_factory):
    return hostsim_build.shared("policy_grad.cpp", tmp_path_factory.mktemp("gp_rollout_pg"), hostsim_build.SHIM_FLAGS)


@pytest.fixture(scope="module")
def ro_shim(tmp_path_factory):
    return hostsim_build.shared("rollout.cpp", tmp_path_factory.mktemp("gp_rollout_ro"), hostsim_build.SHIM_FLAGS)


class _RecordingEngine(object):
    """Stands in for the context: keeps the model description, the policy table and the GP heads as the
    builder uploads them (alpha' = Linv^T alpha, inputs divided by the lengthscales), runs the shim."""

    def __init__(self, shim):
        import torch
        self.shim, self.torch_device, self.calls = shim, torch.device("cpu"), []
        self.heads, self.nheads, self.keep = (_Head * 6)(), 0, {}

    def model_set(self, desc):
        self.desc = desc

    def tri_set(self, slot, grid_desc, simplices, hyperplanes, discrete_points, project, ncols, table):
        assert slot == 1
        self.tri = (grid_desc, np.ascontiguousarray(simplices, dtype=np.int32), np.ascontiguousarray(hyperplanes),
                    np.ascontiguousarray(np.concatenate(discrete_points)), np.ascontiguousarray(table.numpy()))
        g, simp, hyper, dp, tab = self.tri
        assert self.shim.gr_set_tri(C.byref(g), len(simp), _p(simp), _p(hyper), _p(dp), int(bool(project)),
                                    int(ncols), _p(tab)) == 0

    def _head(self, h, X, Linv, alpha, col0, variance, inv_ls, xs, kernel):
        alpha = np.ascontiguousarray(np.asarray(Linv).T.dot(alpha))
        hd = self.heads[h]
        hd.n = hd.n_pad = len(X)
        hd.dout, hd.col0, hd.variance = alpha.shape[1], col0, variance
        hd.inv_ls, hd.xs, hd.alpha = _p(inv_ls).value, _p(xs).value, _p(alpha).value
        hd.kernel = None if kernel is None else C.cast(C.pointer(kernel), C.c_void_p)
        self.keep[h] = (alpha, inv_ls, xs, kernel)

    def gp_set_head(self, head, X, Linv, alpha, col0, variance, lengthscales):
        ls = np.broadcast_to(np.asarray(lengthscales, dtype=np.float64), (X.shape[1],))
        self._head(head, X, Linv, alpha, col0, float(variance), np.ascontiguousarray(1.0 / ls),
                   np.ascontiguousarray((X / ls).T), None)

    def gp_set_head_kernel(self, head, X, Linv, alpha, col0, factors):
        p = X.shape[1]
        kernel = _hip.GpKernel()
        kernel.nfactors = len(factors)
        for f, (kind, product, variance, inv) in enumerate(factors):
            kernel.factor[f].kind, kernel.factor[f].product = int(kind), int(product)
            for q in range(p):
                kernel.factor[f].variance[q] = float(variance[q])
                kernel.factor[f].inv_lengthscales[q] = float(inv[q])
        self._head(head, X, Linv, alpha, col0, 0.0, np.ones(p), np.ascontiguousarray(np.asarray(X).T), kernel)

    def gp_append_point(self, head, x, row, alpha_new):
        return False                                    # (re-pack: the stand-in keeps whole heads)

    def gp_configure(self, nheads, beta):
        self.nheads = nheads

    # ---- what the Python layer calls ---------------------------------------------------------------------
    def rollout(self, *args, **kw):
        raise AssertionError("a GPMeanFunction must not reach sl_rollout")

    reward_rollout = rollout

    def gp_mean_points(self, n, d_inputs, d_mean):
        import torch
        self.calls.append(("gp_mean_points", n))
        d, m = self.desc.grid.d, self.desc.policy.m
        inputs, out = np.ascontiguousarray(d_inputs.numpy()), np.zeros((n, d))
        assert self.shim.gr_mean(C.byref(self.desc.dynamics), self.nheads, self.heads, d, m, C.c_int64(n), 1,
                                 _p(inputs), _p(out)) == 0
        d_mean.copy_(torch.from_numpy(out))

    def run(self, start, steps, n=None, per_thread=1):
        """-> end [n, d], traj [steps, n, d], actions [steps, n, m]; start None: the grid points."""
        if start is not None:
            start = np.ascontiguousarray(start, dtype=np.float64)
            n = len(start)
        d, m = self.desc.grid.d, self.desc.policy.m
        end, traj, act = np.zeros((n, d)), np.zeros((max(steps, 1), n, d)), np.zeros((max(steps, 1), n, m))
        rc = self.shim.gr_rollout(C.byref(self.desc), self.nheads, self.heads, C.c_int64(n), _p(start), steps,
                                  per_thread, _p(end), _p(traj), _p(act))
        assert rc == 0
        return end, traj[:steps], act[:steps]

    def run_reward(self, start, weights, tol, chunk, n=None, per_thread=1):
        if start is not None:
            start = np.ascontiguousarray(start, dtype=np.float64)
            n = len(start)
        d = self.desc.grid.d
        total, state = np.zeros(n), np.zeros((n, d))
        steps, converged, redone = C.c_int64(0), C.c_int(0), C.c_int(0)
        weights = np.ascontiguousarray(weights, dtype=np.float64)
        rc = self.shim.gr_reward_rollout(C.byref(self.desc), self.nheads, self.heads, C.c_int64(n), _p(start),
                                         len(weights), _p(weights), C.c_double(tol), chunk, per_thread, _p(total),
                                         _p(state), C.byref(steps), C.byref(converged), C.byref(redone))
        assert rc == 0
        return total, state, int(steps.value), bool(converged.value), bool(redone.value)

    def rollout_mean(self, lo, hi, d_start, steps, d_state, d_traj=None, d_actions=None, steps_per_launch=0):
        import torch
        self.calls.append(("rollout_mean", lo, hi, d_start is None, steps, d_traj is not None,
                           d_actions is not None, steps_per_launch))
        start = None if d_start is None else d_start.numpy()
        end, traj, act = self.run(start, steps, n=hi - lo)
        d_state.copy_(torch.from_numpy(end))
        if d_traj is not None:
            assert d_traj.is_contiguous() and tuple(d_traj.shape) == traj.shape
            d_traj.copy_(torch.from_numpy(traj))
        if d_actions is not None:
            assert d_actions.is_contiguous() and tuple(d_actions.shape) == act.shape
            d_actions.copy_(torch.from_numpy(act))

    def reward_rollout_mean(self, lo, hi, d_start, horizon, d_weights, tol, d_sum, d_state, steps_per_launch=0):
        import torch
        self.calls.append(("reward_rollout_mean", lo, hi, d_start is None, horizon, steps_per_launch))
        start = None if d_start is None else d_start.numpy()
        total, state, steps, converged, _ = self.run_reward(start, d_weights.numpy(), tol, 32, n=hi - lo)
        d_sum.copy_(torch.from_numpy(total))
        d_state.copy_(torch.from_numpy(state))
        return steps, converged

    def rollout_mask(self, n, d, d_state, equilibrium, tol, d_bits, d_count):
        eq = np.zeros(d) if equilibrium is None else np.ravel(np.asarray(equilibrium, dtype=np.float64))
        self.member = np.linalg.norm(d_state.numpy() - eq[None, :], ord=2, axis=1) <= tol

    def bits_to_bytes(self, n, d_bits, d_bytes):
        import torch
        d_bytes[:n] = torch.from_numpy(self.member.astype(np.uint8))


def _engine_for(shim, name, reward=False):
    """-> (engine with the model of the case uploaded, case, engine dynamics spec, policy spec)."""
    case = R.make(name)[0]
    parent, policy = R.engine_dynamics(case), R.engine_policy(case)
    engine = _RecordingEngine(shim)
    grid = F.GridWorld(case["limits"], case["num_points"])
    ModelBuilder(engine, grid).upload(policy, parent.to_mean_function(), F.QuadraticFunction(np.eye(case["d"])),
                                      reward=F.QuadraticFunction(R.reward_matrix(case)) if reward else None)
    return engine, case, parent, policy


# ---- one step, bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_CASES)
def test_one_step_equals_policy_gradient_header(shim, pg_shim, name):
    """The header's one-step mean equals sl_pg_head + sl_pg_linear_part on the same heads: every point of the
    reference trajectories' first and last rows, RBF heads and kernel descriptions, one and two rows side by side."""
    engine, case, _, _ = _engine_for(shim, name)
    ro = R.reference(name)[5]
    d, m = case["d"], case["m"]
    inputs = np.ascontiguousarray(np.vstack([np.hstack((ro.states[s], ro.actions[s])) for s in (0, len(ro.actions) - 1)]))
    n = len(inputs)
    got, got2 = np.zeros((n, d)), np.zeros((n, d))
    for per_thread, out in ((1, got), (2, got2)):
        assert shim.gr_mean(C.byref(engine.desc.dynamics), engine.nheads, engine.heads, d, m, C.c_int64(n), per_thread,
                            _p(inputs), _p(out)) == 0
    # the policy-gradient header on a value table of its own (the successor does not depend on it)
    vf = F.Triangulation(F.GridWorld(case["limits"], [3] * d), np.zeros((3 ** d, 1)), project=True)
    vgrid = vf.discretization
    keep = [vgrid._desc(), np.ascontiguousarray(vf.unit_simplex_codes, dtype=np.int32),
            np.ascontiguousarray(vf.hyperplanes), np.ascontiguousarray(np.concatenate(vgrid.discrete_points)),
            np.ascontiguousarray(vf.parameters)]
    reward, value = _hip.ValueDesc(), _hip.ValueDesc()
    F.QuadraticFunction(np.eye(d + m))._write_value(reward)
    value.kind = _hip.V_TRI
    states, actions = np.ascontiguousarray(inputs[:, :d]), np.ascontiguousarray(inputs[:, d:])
    grad, q, nxt = np.zeros((n, m)), np.zeros(n), np.zeros((n, d))
    rc = pg_shim.pg_action_gradient(C.byref(keep[0]), len(keep[1]), _p(keep[1]), _p(keep[2]), _p(keep[3]), 1, _p(keep[4]),
                                    C.byref(engine.desc.dynamics), C.byref(reward), C.byref(value), C.c_double(0.9),
                                    engine.nheads, engine.heads, d, m, C.c_int64(n), _p(states), _p(actions), _p(grad),
                                    _p(q), _p(nxt))
    assert rc == 0
    assert np.isfinite(nxt).all() and np.ptp(nxt) > 0
    assert_array_equal(got, nxt)
    assert_array_equal(got2, nxt)


# ---- rollouts against the reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_CASES)
def test_rollout_matches_reference(shim, ro_shim, name):
    case, horizon, tol, _, _, ro, roa = R.reference(name)
    engine = _engine_for(shim, name)[0]
    n, steps = len(ro.end), horizon - 1
    end, traj, act = engine.run(None, steps, n=n)
    ratio = ro.ratio(traj, rows=np.arange(1, steps + 1))
    member = np.zeros(n, dtype=np.uint8)
    eq = np.zeros(case["d"])
    assert ro_shim.ro_mask(C.c_int64(n), case["d"], _p(end), _p(eq), C.c_double(tol), _p(member), None) == 0
    flips = int((member.astype(bool) != roa).sum())
    print("mean rollout %s (host): %d mask flips of %d, largest |states - reference| / bound %.3g (bound at the end "
          "%.3g)" % (name, flips, n, ratio, ro.bound()[-1]))
    assert flips == 0                                                   # nothing excluded
    assert ratio <= 1.0
    assert_array_equal(end, traj[-1])
    assert np.abs(act - ro.actions).max() <= ro.bound()[-1] * max(1.0, np.abs(case["K"]).sum())
    # explicit start points = the cells; two trajectories side by side (odd count included); chunks carried
    pts = R.start_points(case)
    assert_array_equal(engine.run(pts, steps)[1], traj)
    odd = pts[:len(pts) - (len(pts) % 2 == 0)]
    assert_array_equal(engine.run(odd, steps, per_thread=2)[1], traj[:, :len(odd)])
    carried = pts
    for chunk in (1, 7, steps - 8):
        carried = engine.run(carried, chunk)[0]
    assert_array_equal(carried, end)


@pytest.mark.parametrize("name,discount,horizon,tol,stops", [("pendulum-stack", 0.8, 40, 0.1, True),
                                                             ("cartpole", 0.98, 25, 1e-6, False),
                                                             ("table-policy", 0.8, 40, 0.1, True)])
def test_reward_rollout_matches_reference(shim, name, discount, horizon, tol, stops):
    case, _, _, model, policy, _, _ = R.reference(name)
    pts = R.start_points(case)
    ref = R.RewardRollout(model, policy, pts, R.reward_matrix(case), discount, horizon, tol)
    print("mean returns %s: reference stops after %d of %d terms (converged %s), nearest relative gap of a step "
          "maximum to tol %.3g, own error %.3g" % (name, ref.steps, horizon, ref.converged, ref.gap, ref.own_error))
    assert ref.gap > R.GAP and np.isfinite(ref.rollout).all()
    assert ref.converged == stops and (ref.steps < horizon) == stops
    engine = _engine_for(shim, name, reward=True)[0]
    weights = [discount ** t for t in range(horizon)]
    results = {}
    for chunk, per_thread in ((1, 1), (7, 1), (32, 1), (32, 2)):
        total, state, steps, converged, redone = engine.run_reward(pts, weights, tol, chunk, per_thread=per_thread)
        results[chunk, per_thread] = (total, state)
        assert (steps, converged) == (ref.steps, ref.converged)
        assert redone == (stops and chunk > 1 and ref.steps % chunk != 0)
    ratio = ref.ratio(results[1, 1][0])
    print("mean returns %s (host): largest |sum - reference| / bound %.3g (bound %.3g)" % (name, ratio, ref.bound()))
    assert ratio <= 1.0
    for key in results:
        assert_array_equal(results[key][0], results[1, 1][0])
        assert_array_equal(results[key][1], results[1, 1][1])
    assert_array_equal(engine.run_reward(None, weights, tol, 32, n=len(pts))[0], results[1, 1][0])


# ---- the chunk rule ------------------------------------------------------------------------------------------------
def test_chunk_rule(shim):
    chunk = lambda n, steps, points: shim.gr_chunk(C.c_int64(n), steps, C.c_int64(points))
    reward = lambda n, steps, points: shim.gr_reward_chunk(C.c_int64(n), steps, C.c_int64(points))
    assert chunk(480, 29, 60) == 29                                     # small problems: the whole horizon
    assert chunk(1 << 40, 10, 4096) == 1 and chunk(5, 0, 10) == 1       # never below one step
    assert chunk(1, 1 << 30, 1) == 1 << 20                              # never above 2^20
    assert chunk(64 ** 4, 1000, 4096) == 3                              # 2.7e11 / (1.7e7 x 4096) = 3.9
    assert chunk(100, 50, 0) == 50 and chunk(0, 50, 10) == 50
    for n, steps, points in ((1000, 500, 100), (10 ** 6, 5000, 1024), (10 ** 7, 100, 64)):
        base = chunk(n, steps, points)
        assert 1 <= base <= min(steps, 1 << 20)
        assert chunk(2 * n, steps, points) <= base and chunk(n, steps, 2 * points) <= base
        assert chunk(n, 2 * steps, points) >= base
        assert base == steps or abs(base * n * points - 2.7e11) <= n * points
        r = reward(n, steps, points)
        assert 1 <= r <= min(base, 32, 128)
    assert reward(480, 500, 60) == 32 and reward(64 ** 4, 500, 4096) == 3


# ---- the Python layer on a stand-in engine ------------------------------------------------------------------------
@pytest.fixture
def fake_engine(shim, monkeypatch):
    import copy
    from safe_learning_amd import _evaluate
    engine = _RecordingEngine(shim)
    builder = ModelBuilder(engine, None)

    def _engine(d):
        builder.grid = copy.copy(F.GridWorld([[0., 1.]] * d, 2))
        return engine, builder
    monkeypatch.setattr(U, "_engine", _engine)
    monkeypatch.setattr(_evaluate, "_builder", _engine)
    monkeypatch.setattr(_evaluate, "_ctx", lambda: engine)
    return engine


def test_wrapper_reaches_the_mean_rollouts(fake_engine):
    import torch
    case, horizon, tol, model, opolicy, ro, roa = R.reference("pendulum-stack")
    parent, policy = R.engine_dynamics(case), R.engine_policy(case)
    f = parent.to_mean_function()
    assert isinstance(f, F.GPMeanFunction) and isinstance(f, F.DeterministicFunction) and f.parent is parent
    assert (f.input_dim, f.output_dim, f._role) == (3, 2, 'dynamics') and f.name == parent.name + '_mean'
    assert isinstance(parent.functions[0].to_mean_function(), F.GPMeanFunction)
    pts = R.start_points(case)
    grid = F.GridWorld(case["limits"], case["num_points"])
    # f(states, actions): NumPy in, NumPy out; tensors in, tensors out; concatenated inputs
    x, u = ro.states[3], ro.actions[3]
    mean = f(x, u)
    assert isinstance(mean, np.ndarray) and mean.shape == x.shape
    assert np.abs(mean - ro.states[4]).max() <= ro.bound()[4]
    assert_array_equal(f(np.hstack((x, u))), mean)
    out = f(torch.from_numpy(x), torch.from_numpy(u))
    assert isinstance(out, torch.Tensor)
    assert_array_equal(out.numpy(), mean)
    with pytest.raises(ValueError, match="inputs"):
        f(x)
    # compute_roa, compute_trajectory, reward_rollout
    fake_engine.calls.clear()
    mask = U.compute_roa(grid, (f, policy), horizon=horizon, tol=tol)
    assert fake_engine.calls == [("rollout_mean", 0, grid.nindex, True, horizon - 1, False, False, 0)]
    assert mask.dtype == np.bool_
    assert_array_equal(mask, roa)
    mask, traj = U.compute_roa(torch.from_numpy(pts), (f, policy), horizon=horizon, tol=tol, no_traj=False,
                               steps_per_launch=7)
    assert isinstance(mask, torch.Tensor) and traj.shape == (len(pts), 2, horizon)
    assert fake_engine.calls[-1][-1] == 7
    assert ro.ratio(traj.numpy().transpose(2, 0, 1)) <= 1.0
    s, a = U.compute_trajectory(f, policy, pts[:5], 12)
    assert s.shape == (5, 12, 2) and a.shape == (5, 11, 1)
    assert_array_equal(s, traj.numpy().transpose(0, 2, 1)[:5, :12])
    fake_engine.calls.clear()
    ref = R.RewardRollout(model, opolicy, pts, R.reward_matrix(case), 0.8, 40, 0.1)
    total, steps, converged = U.reward_rollout(grid, (f, policy), F.QuadraticFunction(R.reward_matrix(case)), 0.8,
                                               horizon=40, tol=0.1, full_output=True)
    assert fake_engine.calls == [("reward_rollout_mean", 0, grid.nindex, True, 40, 0)]
    assert (steps, converged) == (ref.steps, ref.converged) and ref.ratio(total) <= 1.0


def test_wrapper_refusals(fake_engine, monkeypatch):
    import safe_learning_amd as sl
    case = R.make("pendulum")[0]
    parent, policy = R.engine_dynamics(case), R.engine_policy(case)
    f = parent.to_mean_function()
    pts = R.start_points(case)
    # the UncertainFunction itself still raises what it raised
    with pytest.raises(ValueError, match="callable"):
        U.compute_roa(pts, (parent, policy))
    with pytest.raises(ValueError, match="callable"):
        U.compute_trajectory(parent, policy, pts[0], 5)
    with pytest.raises(ValueError, match="callable"):
        U.reward_rollout(pts, (parent, policy), F.QuadraticFunction(np.eye(3)), 0.9)
    with pytest.raises(TypeError, match="GaussianProcess"):
        F.GPMeanFunction(F.LinearSystem((np.eye(2), np.zeros((2, 1)))))
    assert not fake_engine.calls
    # Lyapunov and ActorCritic refuse and say why
    grid = F.GridWorld(case["limits"], case["num_points"])
    with pytest.raises(TypeError, match="error bound"):
        sl.Lyapunov(grid, F.QuadraticFunction(case["P"]), f, 1.0, 1.0, 0.1, policy)
    critic = sl.NeuralNetwork([8, 1], ["tanh", None], use_bias=False, input_dim=2, seed=0)
    with pytest.raises(TypeError, match="sl_critic_batch"):
        sl.ActorCritic(policy, f, F.QuadraticFunction(-np.eye(3)), critic)
    # PolicyIteration treats it as its parent
    monkeypatch.setattr(_hip, "Context", lambda *a, **kw: fake_engine)
    value = F.Triangulation(F.GridWorld(case["limits"], [5, 5]), np.zeros((25, 1)), project=True)
    rl = sl.PolicyIteration(policy, f, F.QuadraticFunction(-np.eye(3)), value)
    assert rl.dynamics is parent
    # one process only
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    with pytest.raises(NotImplementedError, match="one GPU"):
        U.compute_roa(pts, (f, policy))
    with pytest.raises(NotImplementedError, match="one GPU"):
        U.reward_rollout(pts, (f, policy), F.QuadraticFunction(-np.eye(3)), 0.9)


def test_package_exports():
    import safe_learning_amd as sl
    assert sl.GPMeanFunction is F.GPMeanFunction and "GPMeanFunction" in F.__all__
    assert callable(sl.GaussianProcess.to_mean_function) and callable(sl.FunctionStack.to_mean_function)
    for name in ("sl_gp_mean_points", "sl_rollout_mean", "sl_reward_rollout_mean"):
        assert name in _hip.SIGNATURES
    for method in ("gp_mean_points", "rollout_mean", "reward_rollout_mean"):
        assert callable(getattr(_hip.Context, method))


# ---- the new kernels' resources ---------------------------------------------------------------------------------------
def test_new_kernels_are_free_of_scratch():
    """After ``build()``, every kernel of sl_gp_rollout.hip is in the library - the mean at points for d = 1 .. 4
    and generic, both rollouts for the closed-form policies at d = 1 .. 4 and generic and for the interpolated
    policy at (2, 1), the fold - and none uses scratch (tools/kernel_resources.py: the code object's metadata)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from safe_learning_amd._build import build
    build()
    now = kernel_resources.resources(_hip.LIB_PATH)
    mine = {name: res for name, res in now.items()
            if any(k in name for k in ("k_gp_mean_points", "k_gp_rollout", "k_gp_reward_rollout", "k_gp_reward_fold"))}
    for name in sorted(mine):
        print(name, mine[name])
    count = lambda key: sum(key in name for name in mine)
    assert count("16k_gp_mean_pointsI") == 5 and count("12k_gp_rolloutI") == 6
    assert count("19k_gp_reward_rolloutI") == 6 and count("k_gp_reward_fold") == 1
    assert all(res["scratch"] == 0 for res in mine.values()), mine
