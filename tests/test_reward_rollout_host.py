"""CPU checks of reward_rollout (safe_learning_amd/csrc/sl_reward_rollout.h, DESIGN.md "Closed-loop
rollouts").

The per-trajectory header and the launch loop around it are compiled with g++ into a test-only shim
(tests/hostsim/reward_rollout.cpp) and compared with the NumPy reference (tests/np_reward_rollout.py
over the oracle's callables): sums, per-step maxima, step count and flag bit for bit for linear
systems under a saturated linear policy, whatever the horizon is cut into; the Euler models at a
tolerance derived from the oracle alone (tests/reward_rollout_cases.py).  The NumPy reference itself
is compared with a run of the reference (tests/golden/reference_reward_rollout.npz), and the Python
layer runs over a fake engine.  The GPU tests (tests/test_gpu_reward_rollout.py) repeat the
comparisons through the real kernels.
"""

import ctypes as C
import os

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import hostsim_build
import np_reward_rollout as NR
import np_rollout
import reward_rollout_cases as RRC
import rollout_cases as RC
from conftest import GOLDEN_DIR
from safe_learning_amd import functions as F
from safe_learning_amd import utilities as U
from safe_learning_amd._model import ModelBuilder
from test_rollout_host import _FakeEngine, _RecordingCtx, _p


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """tests/hostsim/reward_rollout.cpp with the flags of test_rollout_host's shim."""
    return hostsim_build.shared("reward_rollout.cpp", tmp_path_factory.mktemp("reward_rollout"),
                                hostsim_build.SHIM_FLAGS)


def _weights(discount, horizon):
    return np.array([discount ** t for t in range(horizon)], dtype=np.float64)


def shim_reward_rollout(shim, desc, d, start, n, discount, horizon, tol, chunk=0, per_thread=1):
    """-> (sums [n], steps, converged, maxima [steps], launches, redone) of the shim's launch loop."""
    if start is not None:
        start = np.ascontiguousarray(start, dtype=np.float64)
        n = len(start)
    weights = _weights(discount, horizon)
    sums, state, maxima = np.zeros(n), np.zeros((n, d)), np.full(horizon, -1.0)
    steps, converged, launches, redone = C.c_int64(0), C.c_int(0), C.c_int(0), C.c_int(0)
    rc = shim.rr_reward_rollout(C.byref(desc), C.c_int64(n), _p(start), horizon, _p(weights), C.c_double(tol), chunk,
                                per_thread, _p(sums), _p(state), _p(maxima), C.byref(steps), C.byref(converged),
                                C.byref(launches), C.byref(redone))
    assert rc == 0
    assert (maxima[steps.value:] == -1.0).all()
    return sums, steps.value, bool(converged.value), maxima[:steps.value], launches.value, redone.value


class _Model(object):
    """The shim with the model and the reward of a case (the arrays stay alive with this object)."""

    def __init__(self, shim, case, reward_matrix):
        self.shim = shim
        self.grid = RC.engine_grid(case)
        dynamics, policy = RC.engine_pair(case)
        self.ctx = _RecordingCtx()
        ModelBuilder(self.ctx, self.grid).upload(policy, dynamics, F.QuadraticFunction(np.eye(self.grid.ndim)),
                                                 reward=F.QuadraticFunction(reward_matrix))
        self.d = self.grid.ndim
        if self.ctx.tri is not None:
            g, simp, hyper, dp, project, ncols, table = self.ctx.tri
            assert shim.ro_set_tri(C.byref(g), len(simp), _p(simp), _p(hyper), _p(dp), project, ncols,
                                   _p(table)) == 0

    def run(self, start, discount, horizon, tol, n=None, **kw):
        return shim_reward_rollout(self.shim, self.ctx.desc, self.d, start, n, discount, horizon, tol, **kw)


# ---- linear dynamics, saturated linear policy, quadratic reward: bit for bit ---------------------------
@pytest.mark.parametrize("key", sorted(RRC.LINEAR))
def test_linear_sums_bit_exact(shim, key):
    pts, want, steps, converged, maxima = RRC.oracle_linear(key)
    case, matrix, discount, horizon, tol = RRC.linear_case(key)
    model = _Model(shim, case, matrix)

    def check(got):
        assert_array_equal(got[0], want)
        assert got[1:3] == (steps, converged)
        assert_array_equal(got[3], maxima)

    check(model.run(pts, discount, horizon, tol))
    check(model.run(None, discount, horizon, tol, n=len(pts)))           # the cells of the grid
    check(model.run(pts, discount, horizon, tol, per_thread=2))          # two trajectories side by side
    odd = len(pts) - (len(pts) % 2 == 0)
    if converged:
        # an odd count: the spare lane simulates the last trajectory and contributes nothing (the
        # stop step of the subset is its own: compare with the oracle on the same subset)
        dynamics, policy = RC.oracle_pair(case)
        sub = NR.reward_rollout(pts[:odd], dynamics, policy, matrix, discount, horizon, tol)
        got = model.run(pts[:odd], discount, horizon, tol, per_thread=2)
        assert_array_equal(got[0], sub[0])
        assert got[1:3] == sub[1:3]
        assert_array_equal(got[3], sub[3])
    for chunk in (1, 7, 64):                                             # the horizon cut into launches
        check(model.run(pts, discount, horizon, tol, chunk=chunk))
        check(model.run(None, discount, horizon, tol, n=len(pts), chunk=chunk, per_thread=2))


def test_cut_positions(shim):
    """The "1d" case stops at step index 17: on a launch's last step (chunks of 18), on the next
    launch's first step (17), inside a launch (6 does not: 3 x 6 = 18; 400, cut to the cap of 128,
    does), step by step - the same bits, and the launch that overshoots is the only one run again."""
    pts, want, steps, converged, maxima = RRC.oracle_linear("1d")
    assert steps == 18 and converged
    case, matrix, discount, horizon, tol = RRC.linear_case("1d")
    model = _Model(shim, case, matrix)
    expected = {18: (1, 0), 17: (3, 1), 6: (3, 0), 1: (18, 0), 400: (2, 1)}     # chunk -> (launches, redone)
    for chunk, counts in expected.items():
        got = model.run(pts, discount, horizon, tol, chunk=chunk)
        assert_array_equal(got[0], want)
        assert got[1:3] == (steps, converged)
        assert_array_equal(got[3], maxima)
        assert got[4:] == counts, chunk


def test_nan_never_converges(shim):
    """A NaN term makes the maximum NaN: the test is false at every step, the loop runs the full
    horizon, and the other trajectories' sums are the oracle's over that horizon."""
    case, matrix, discount, _, tol = RRC.linear_case("pendulum")
    horizon = 60
    pts = RC.oracle_points(case).copy()
    pts[5, 0] = np.nan
    dynamics, policy = RC.oracle_pair(case)
    want, steps, converged, maxima = NR.reward_rollout(pts, dynamics, policy, matrix, discount, horizon, 1e30)
    assert steps == horizon and not converged and np.isnan(maxima).all()
    model = _Model(shim, case, matrix)
    for chunk in (0, 1, 7):
        got = model.run(pts, discount, horizon, 1e30, chunk=chunk)
        assert got[1:3] == (horizon, False)
        assert np.isnan(got[3]).all() and np.isnan(got[0][5])
        assert_array_equal(np.delete(got[0], 5), np.delete(want, 5))
    pts[5, 0] = np.inf                                                   # inf likewise (inf - inf: NaN sums)
    got = model.run(pts, discount, horizon, 1e30)
    assert got[1:3] == (horizon, False)


# ---- Euler models -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(RRC.EULER))
def test_euler_sums(shim, key):
    pts, want, steps, converged, maxima, rtol = RRC.oracle_euler(key)
    case, matrix, discount, horizon, tol = RRC.euler_case(key)
    model = _Model(shim, case, matrix)
    got = model.run(pts, discount, horizon, tol)
    assert got[1:3] == (steps, converged)
    RRC.assert_sums_close(got[0], want, rtol)
    again = model.run(None, discount, horizon, tol, n=len(pts), chunk=50)
    assert_array_equal(again[0], got[0])
    assert again[1:3] == got[1:3]


def test_table_policy_sums(shim):
    pts, want, steps, converged, ok = RRC.oracle_tri()
    q, r, discount, horizon, tol = RRC.TRI
    model = _Model(shim, RC.tri_case(), NR.quadratic_reward(q, r))
    assert model.ctx.desc.policy.kind == 4                                # SL_POLICY_TRI
    got = model.run(pts, discount, horizon, tol)
    assert got[1:3] == (steps, converged)
    assert_allclose(got[0][ok], want[ok], rtol=1e-10)
    import exclusions
    exclusions.report("test_reward_rollout_host::test_table_policy_sums", ok, "successor")


def test_chunk_choice(shim):
    """The library's steps per launch: 32 at most (the work past the stopping step stays small),
    fewer where a launch would exceed a second, never less than one."""
    assert shim.rr_chunk(C.c_int64(1681), 1000) == 32
    assert shim.rr_chunk(C.c_int64(3000000), 1000) == 32
    assert shim.rr_chunk(C.c_int64(1681), 5) == 5
    assert shim.rr_chunk(C.c_int64(1 << 40), 10) == 1
    assert 1 <= shim.rr_chunk(C.c_int64(2 * 10 ** 9), 1000) <= 32


# ---- the NumPy reference against a run of the reference itself --------------------------------------------
def reference_case(data, key):
    import cases
    num = [int(v) for v in data[key + "_num_points"]]
    case = cases.make_case(key, num_points=num, dynamics="analytic")
    case["limits"] = [[float(lo), float(hi)] for lo, hi in data[key + "_limits"]]
    return case


def test_numpy_reference_matches_reference_run():
    """tests/golden/reference_reward_rollout.npz (make_reference_reward_rollout.py: the reference's own
    reward_rollout on its own classes) against tests/np_reward_rollout.py over the oracle."""
    data = np.load(os.path.join(GOLDEN_DIR, "reference_reward_rollout.npz"))
    for key in ("pendulum", "cartpole"):
        case = reference_case(data, key)
        dynamics, policy = RC.oracle_pair(case)
        pts = RC.oracle_points(case)
        assert_array_equal(pts, data[key + "_points"])
        rollout, steps, converged, _ = NR.reward_rollout(pts, dynamics, policy, data[key + "_reward_matrix"],
                                                         float(data["discount"]), int(data["horizon"]),
                                                         float(data["tol"]))
        assert converged and steps == int(data[key + "_steps"]) == RRC.EULER[key][6]
        assert_allclose(rollout, data[key + "_rollout"], rtol=1e-12, atol=0)
        assert_array_equal(data[key + "_reward_matrix"], RRC.euler_case(key)[1])


# ---- the Python layer without a GPU ------------------------------------------------------------------------
class _FakeRewardEngine(_FakeEngine):
    """test_rollout_host's stand-in for the context, with ``reward_rollout`` served by the shim."""

    def __init__(self, shim, reward_shim):
        _FakeEngine.__init__(self, shim)
        self.reward_shim = reward_shim

    def reward_rollout(self, lo, hi, d_start, horizon, d_weights, tol, d_sum, d_state, steps_per_launch=0):
        import torch
        self.calls.append(("reward_rollout", lo, hi, d_start is None, horizon, tol, steps_per_launch))
        n, d = hi - lo, self.desc.grid.d
        assert d_weights.dtype == torch.float64 and tuple(d_weights.shape) == (horizon,)
        assert d_sum.dtype == torch.float64 and tuple(d_sum.shape) == (n,)
        assert d_state.dtype == torch.float64 and tuple(d_state.shape) == (n, d)
        self.weights = d_weights.numpy().copy()
        start = None if d_start is None else np.ascontiguousarray(d_start.numpy())
        sums, state, maxima = np.zeros(n), np.zeros((n, d)), np.zeros(horizon)
        steps, converged, launches, redone = C.c_int64(0), C.c_int(0), C.c_int(0), C.c_int(0)
        assert self.reward_shim.rr_reward_rollout(
            C.byref(self.desc), C.c_int64(n), _p(start), horizon, _p(self.weights), C.c_double(tol),
            steps_per_launch, 1, _p(sums), _p(state), _p(maxima), C.byref(steps), C.byref(converged),
            C.byref(launches), C.byref(redone)) == 0
        d_sum.copy_(torch.from_numpy(sums))
        d_state.copy_(torch.from_numpy(state))
        return int(steps.value), bool(converged.value)


@pytest.fixture
def fake_engine(shim, monkeypatch):
    import copy
    from safe_learning_amd import _evaluate
    engine = _FakeRewardEngine(shim, shim)               # (the reward shim contains rollout.cpp)
    builder = ModelBuilder(engine, None)

    def _engine(d):
        builder.grid = copy.copy(F.GridWorld([[0., 1.]] * d, 2))
        return engine, builder
    monkeypatch.setattr(U, "_engine", _engine)
    monkeypatch.setattr(_evaluate, "_ctx", lambda: engine)
    return engine


def _linear():
    key = "pendulum"
    case, matrix, discount, horizon, tol = RRC.linear_case(key)
    dynamics, policy = RC.engine_pair(case)
    return case, (dynamics, policy), F.QuadraticFunction(matrix), discount, horizon, tol, RRC.oracle_linear(key)


def test_wrapper_shapes_and_values(fake_engine, capsys):
    import torch
    case, pair, reward, discount, horizon, tol, (pts, want, steps, converged, _) = _linear()
    capsys.readouterr()
    got = U.reward_rollout(pts, pair, reward, discount, horizon=horizon, tol=tol)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (len(pts),)
    assert_array_equal(got, want)
    assert fake_engine.calls[-1] == ("reward_rollout", 0, len(pts), False, horizon, tol, 0)
    # the weights are the host's discount ** t, bit for bit
    assert_array_equal(fake_engine.weights, np.array([discount ** t for t in range(horizon)]))
    # a GridWorld starts the kernel at its cells; full_output; steps_per_launch is passed on
    grid = RC.engine_grid(case)
    got, got_steps, got_flag = U.reward_rollout(grid, pair, reward, discount, horizon=horizon, tol=tol,
                                                full_output=True, steps_per_launch=7)
    assert_array_equal(got, want)
    assert (got_steps, got_flag) == (steps, converged) and isinstance(got_steps, int) and got_flag is True
    assert fake_engine.calls[-1] == ("reward_rollout", 0, grid.nindex, True, horizon, tol, 7)
    # a horizon that ends first
    got, got_steps, got_flag = U.reward_rollout(pts, pair, reward, discount, horizon=10, tol=tol, full_output=True)
    assert (got_steps, got_flag) == (10, False)
    # device-tensor inputs stay tensors
    got = U.reward_rollout(torch.from_numpy(pts), pair, reward, discount, horizon=horizon, tol=tol)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float64 and tuple(got.shape) == (len(pts),)
    assert_array_equal(got.numpy(), want)
    # the defaults of the reference
    import inspect
    defaults = {k: v.default for k, v in inspect.signature(U.reward_rollout).parameters.items()}
    assert defaults["horizon"] == 250 and defaults["tol"] == 1e-3
    assert capsys.readouterr().out == ""                                 # nothing is printed


def test_wrapper_callable_path(fake_engine):
    """Callables as in the reference, stepped on (here: CPU) tensors - against the oracle's loop."""
    import torch
    case, pair, reward, discount, horizon, tol, (pts, want, steps, converged, _) = _linear()
    odyn, opol = RC.oracle_pair(case)
    step = np_rollout.closed_loop(odyn, opol)
    oreward = NR.reward_on_states(reward.matrix, opol)
    got, got_steps, got_flag = U.reward_rollout(pts, lambda x: step(x.numpy()), lambda x: oreward(x.numpy()),
                                                discount, horizon=horizon, tol=tol, full_output=True)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64
    assert_array_equal(got, want)
    assert (got_steps, got_flag) == (steps, converged)
    # [n, 1] rewards, a GridWorld, a tensor in and out
    grid = RC.engine_grid(case)
    got = U.reward_rollout(grid, lambda x: step(x.numpy()), lambda x: oreward(x.numpy())[:, None], discount,
                           horizon=horizon, tol=tol)
    assert_array_equal(got, want)
    got = U.reward_rollout(torch.from_numpy(pts), lambda x: torch.from_numpy(step(x.numpy())),
                           lambda x: torch.from_numpy(oreward(x.numpy())), discount, horizon=horizon, tol=tol)
    assert isinstance(got, torch.Tensor)
    assert_array_equal(got.numpy(), want)
    # one NaN reward: the full horizon, not converged; the other sums are the oracle's over that horizon
    def nan_reward(x):
        r = oreward(x.numpy())
        r[3] = np.nan
        return r
    full, _, _, _ = NR.reward_rollout(pts, odyn, opol, reward.matrix, discount, 40, 0.0)
    got, got_steps, got_flag = U.reward_rollout(pts, lambda x: step(x.numpy()), nan_reward, discount, horizon=40,
                                                tol=1e30, full_output=True)
    assert (got_steps, got_flag) == (40, False)
    assert np.isnan(got[3])
    assert_array_equal(np.delete(got, 3), np.delete(full, 3))
    assert not [c for c in fake_engine.calls if c[0] == "reward_rollout"]      # no fused call on this path
    with pytest.raises(ValueError, match=r"\[n\] or \[n, 1\]"):
        U.reward_rollout(pts, lambda x: step(x.numpy()), lambda x: np.zeros((len(x), 2)), discount)


def test_wrapper_argument_errors(fake_engine, monkeypatch):
    case, (dynamics, policy), reward, discount, horizon, tol, (pts, _, _, _, _) = _linear()
    pair = (dynamics, policy)
    gp_case = RC.make("pendulum", dict(num_points=5, n_gp=8))
    uncertain = RC.engine_pair(gp_case)[0]
    with pytest.raises(ValueError, match="callable"):
        U.reward_rollout(pts, (uncertain, policy), reward, discount)
    with pytest.raises(TypeError, match="policy"):
        U.reward_rollout(pts, (dynamics, np.zeros((len(pts), 1))), reward, discount)
    with pytest.raises(TypeError, match="dynamics"):
        U.reward_rollout(pts, (F.QuadraticFunction(np.eye(2)), policy), reward, discount)
    with pytest.raises(TypeError, match="pair"):
        U.reward_rollout(pts, 3.0, reward, discount)
    with pytest.raises(ValueError, match="pair"):
        U.reward_rollout(pts, (dynamics, policy, policy), reward, discount)
    with pytest.raises(ValueError, match="horizon"):
        U.reward_rollout(pts, pair, reward, discount, horizon=0)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="discount"):
            U.reward_rollout(pts, pair, reward, bad)
        with pytest.raises(ValueError, match="discount"):
            U.reward_rollout(pts, lambda x: x, lambda x: x[:, 0], bad)
    with pytest.raises(ValueError, match=r"\[n, d\]"):
        U.reward_rollout(np.zeros((2, 2, 2)), pair, reward, discount)
    with pytest.raises(ValueError, match=r"\[n, d\]"):
        U.reward_rollout(np.zeros((2, 2, 2)), lambda x: x, lambda x: x[:, 0], discount)
    with pytest.raises(ValueError, match="inputs"):
        U.reward_rollout(np.zeros((4, 3)), pair, F.QuadraticFunction(np.eye(4)), discount)   # 2-D policy, 3-D states
    with pytest.raises(ValueError, match=r"quadratic in 2 inputs, \[x, u\] has 3"):
        U.reward_rollout(pts, pair, F.QuadraticFunction(np.eye(2)), discount)
    with pytest.raises(ValueError, match="at least one"):
        U.reward_rollout(np.zeros((0, 2)), pair, reward, discount)
    # the two forms do not mix, and the message says which combination is meant
    with pytest.raises(TypeError, match=r"pair of specs takes the fused kernel.*QuadraticFunction on \[x, u\]"):
        U.reward_rollout(pts, pair, lambda x: x[:, 0], discount)
    with pytest.raises(TypeError, match=r"goes with a \(dynamics, policy\) pair.*callable reward on states"):
        U.reward_rollout(pts, lambda x: x, reward, discount)
    with pytest.raises(TypeError, match="callable on states"):
        U.reward_rollout(pts, lambda x: x, 3.0, discount)
    assert not fake_engine.calls
    # one GPU only
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    with pytest.raises(NotImplementedError, match="one GPU"):
        U.reward_rollout(pts, pair, reward, discount)
    with pytest.raises(NotImplementedError, match="one GPU"):
        U.reward_rollout(pts, lambda x: x, lambda x: x[:, 0], discount)


def test_package_exports():
    import safe_learning_amd as sl
    assert sl.reward_rollout is U.reward_rollout
    assert "reward_rollout" in U.__all__
