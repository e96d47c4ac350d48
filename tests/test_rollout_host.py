"""CPU checks of the closed-loop rollouts (safe_learning_amd/csrc/sl_rollout.h, DESIGN.md "Closed-loop
rollouts").

The per-trajectory header is compiled with g++ into a test-only shim (tests/hostsim/rollout.cpp) and
compared with the NumPy reference (tests/np_rollout.py over the oracle's callables): bit for bit for
linear systems under a saturated linear policy, to rounding for the Euler models and the
interpolated policy, and mask for mask on full-horizon regions of attraction.  The GPU tests
(tests/test_gpu_rollout.py) repeat the comparisons through the real kernels.
"""

import ctypes as C
import os

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import exclusions
import hostsim_build
import np_rollout
import rollout_cases as RC
from conftest import GOLDEN_DIR
from safe_learning_amd import functions as F
from safe_learning_amd import utilities as U
from safe_learning_amd._model import ModelBuilder


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return hostsim_build.shared("rollout.cpp", tmp_path_factory.mktemp("rollout"), hostsim_build.SHIM_FLAGS)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class _RecordingCtx(object):
    """Captures the model description and the policy table instead of uploading them."""

    def __init__(self):
        import torch
        self.torch_device = torch.device("cpu")
        self.tri = None

    def model_set(self, desc):
        self.desc = desc

    def tri_set(self, slot, grid_desc, simplices, hyperplanes, discrete_points, project, ncols, table):
        assert slot == 1
        self.tri = (grid_desc, np.ascontiguousarray(simplices, dtype=np.int32),
                    np.ascontiguousarray(hyperplanes), np.ascontiguousarray(np.concatenate(discrete_points)),
                    int(bool(project)), int(ncols), np.ascontiguousarray(table.numpy()))


class _Model(object):
    """The shim with the model of a case (the arrays stay alive with this object)."""

    def __init__(self, shim, case):
        self.shim = shim
        self.grid = RC.engine_grid(case)
        dynamics, policy = RC.engine_pair(case)
        self.ctx = _RecordingCtx()
        ModelBuilder(self.ctx, self.grid).upload(policy, dynamics, F.QuadraticFunction(np.eye(self.grid.ndim)))
        self.d, self.m = self.grid.ndim, int(self.ctx.desc.policy.m)
        if self.ctx.tri is not None:
            g, simp, hyper, dp, project, ncols, table = self.ctx.tri
            assert shim.ro_set_tri(C.byref(g), len(simp), _p(simp), _p(hyper), _p(dp), project, ncols,
                                   _p(table)) == 0

    def rollout(self, start, steps, per_thread=1, n=None):
        """-> end [n, d], states [steps, n, d], actions [steps, n, m]; start None: the grid points."""
        if start is not None:
            start = np.ascontiguousarray(start, dtype=np.float64)
            n = len(start)
        end = np.zeros((n, self.d))
        traj = np.zeros((steps, n, self.d))
        act = np.zeros((steps, n, self.m))
        rc = self.shim.ro_rollout(C.byref(self.ctx.desc), C.c_int64(n), _p(start), steps, per_thread,
                                  _p(end), _p(traj), _p(act))
        assert rc == 0
        return end, traj, act

    def mask(self, states, tol, equilibrium=None):
        states = np.ascontiguousarray(states, dtype=np.float64)
        eq = np.zeros(self.d) if equilibrium is None else np.ascontiguousarray(equilibrium, dtype=np.float64)
        member = np.zeros(len(states), dtype=np.uint8)
        dist = np.zeros(len(states))
        assert self.shim.ro_mask(C.c_int64(len(states)), self.d, _p(states), _p(eq), C.c_double(tol),
                                 _p(member), _p(dist)) == 0
        return member.astype(bool), dist


# ---- linear dynamics, saturated linear policy: bit for bit ----------------------------------------
@pytest.mark.parametrize("key", sorted(RC.LINEAR_CASES))
def test_linear_rollout_bit_exact(shim, key):
    pts, states, actions = RC.oracle_linear(key)
    model = _Model(shim, RC.make(*RC.LINEAR_CASES[key]))
    end, traj, act = model.rollout(pts, RC.LINEAR_STEPS)
    assert_array_equal(traj, states[:, 1:, :].transpose(1, 0, 2))        # the state after every step
    assert_array_equal(act, actions.transpose(1, 0, 2))                  # and the action that led to it
    assert_array_equal(end, states[:, -1, :])
    # the saturation was active somewhere and inactive somewhere (both branches compared)
    if key != "1d":
        assert (np.abs(actions) == 1.0).any() and (np.abs(actions) < 1.0).any()
    # start states generated from the cell index = GridWorld.all_points
    end_grid, traj_grid, _ = model.rollout(None, RC.LINEAR_STEPS, n=len(pts))
    assert_array_equal(end_grid, end)
    assert_array_equal(traj_grid, traj)
    # two trajectories stepped side by side (the linear kernels), odd count included
    end2, traj2, act2 = model.rollout(pts[:len(pts) - (len(pts) % 2 == 0)], RC.LINEAR_STEPS, per_thread=2)
    assert_array_equal(traj2, traj[:, :len(end2)])
    assert_array_equal(act2, act[:, :len(end2)])
    # the horizon cut into launches with the state carried between them
    carried = pts
    for chunk in (1, 7, 64, RC.LINEAR_STEPS - 72):
        carried, _, _ = model.rollout(carried, chunk)
    assert_array_equal(carried, end)


# ---- interpolated policy ------------------------------------------------------------------------------
def test_table_policy_rollout(shim):
    pts, states, actions, ok = RC.oracle_tri()
    model = _Model(shim, RC.tri_case())
    assert model.ctx.desc.policy.kind == 4                                # SL_POLICY_TRI
    _, traj, act = model.rollout(pts, RC.TRI_STEPS)
    traj, act = traj.transpose(1, 0, 2), act.transpose(1, 0, 2)           # [n, steps, .]
    assert_allclose(act[ok], actions[ok], rtol=1e-10, atol=1e-12)
    assert_allclose(traj[ok], states[:, 1:, :][ok], rtol=1e-10, atol=1e-12)
    exclusions.report("test_table_policy_rollout", ok, "successor")
    assert np.ptp(actions) > 0.5                                          # a policy that does something


# ---- Euler dynamics: the first steps of every cell --------------------------------------------------------
@pytest.mark.parametrize("key", sorted(RC.EULER_CASES))
def test_euler_rollout_first_steps(shim, key):
    pts, states, actions = RC.oracle_euler(key)
    model = _Model(shim, RC.make(*RC.EULER_CASES[key]))
    end, traj, act = model.rollout(pts, RC.EULER_STEPS)
    assert_allclose(traj, states[:, 1:, :].transpose(1, 0, 2), rtol=RC.EULER_RTOL, atol=RC.EULER_ATOL)
    assert_allclose(act, actions.transpose(1, 0, 2), rtol=RC.EULER_RTOL, atol=RC.EULER_ATOL)
    assert_array_equal(end, traj[-1])


# ---- regions of attraction, full horizon --------------------------------------------------------------------
# The four shapes run through the kernels in tests/test_gpu_rollout.py; here the two pendulum shapes
# and ONE cart-pole shape (each cart-pole shape costs the oracle most of a minute), so the CPU suite
# stays usable.
@pytest.mark.parametrize("key", ["pendulum-x1", "pendulum-x3", "cartpole-x3"])
def test_roa_mask_matches_oracle(shim, key):
    """The mask equals the oracle's exactly and the in-ROA end states agree at 1e-10 (conditions and the
    input-side assertions: rollout_cases.oracle_roa / check_roa, which print the measured figures)."""
    start, _, dist, roa = RC.oracle_roa(key)
    case, horizon, tol = RC.roa_case(key)
    model = _Model(shim, case)
    end, _, _ = model.rollout(None, horizon - 1, n=len(start))
    got, got_dist = model.mask(end, tol)
    RC.check_roa(key, got, end)
    assert_array_equal(got, got_dist <= tol)


def test_membership_is_numpy_norm(shim):
    """``dist`` is np.linalg.norm(.., ord=2, axis=1) bit for bit (squares summed left to right, then
    the root), compared rooted, NaN outside, an equilibrium other than the origin."""
    rng = np.random.default_rng(4)
    for d in (1, 2, 3, 4, 6):
        model = _Model.__new__(_Model)
        model.shim, model.d = shim, d
        x = rng.normal(size=(5000, d)) * 10.0 ** rng.integers(-4, 3, size=(5000, d))
        eq = rng.normal(size=d)
        for e in (None, eq):
            ref = np_rollout.distances(x, None if e is None else e[None, :])
            tol = float(np.median(ref))
            got, dist = model.mask(x, tol, e)
            assert_array_equal(dist, ref)
            assert_array_equal(got, ref <= tol)
        x[1, d - 1] = np.nan
        x[2, 0] = np.inf
        got, dist = model.mask(x, 1e300)
        assert not got[1] and not got[2] and got[3:].all()


def test_chunk_choice(shim):
    """The library's steps per launch: the whole horizon for small problems, near a second of
    the measured Euler cart-pole rate at 128^4, never less than one step."""
    assert shim.ro_chunk(C.c_int64(10201), 499) == 499
    assert 80 <= shim.ro_chunk(C.c_int64(128 ** 4), 1999) <= 110
    assert shim.ro_chunk(C.c_int64(1 << 40), 10) == 1
    assert shim.ro_chunk(C.c_int64(1), 1 << 30) == 1 << 20
    assert shim.ro_chunk(C.c_int64(5), 0) == 1


# ---- the NumPy reference against a run of the reference itself --------------------------------------------
def test_numpy_reference_matches_reference_run():
    """tests/golden/reference_roa.npz (make_reference_roa.py: the reference's own compute_roa and
    compute_trajectory on its own classes) against tests/np_rollout.py over the oracle."""
    import oracle
    data = np.load(os.path.join(GOLDEN_DIR, "reference_roa.npz"))
    for key in ("pendulum", "cartpole"):
        case, horizon, tol = reference_case(data, key)
        dynamics, policy = RC.oracle_pair(case)
        grid = oracle.GridWorld(case["limits"], case["num_points"])
        assert_array_equal(grid.all_points, data[key + "_points"])
        roa, traj = np_rollout.compute_roa(grid, np_rollout.closed_loop(dynamics, policy), horizon, tol,
                                           no_traj=False)
        assert_array_equal(roa, data[key + "_roa"])
        assert data[key + "_roa"].any() and not data[key + "_roa"].all()
        assert_allclose(traj[:, :, -1], data[key + "_end"], rtol=1e-9, atol=1e-12)
        assert_allclose(traj[:, :, :data[key + "_traj"].shape[2]], data[key + "_traj"], rtol=1e-10, atol=1e-13)
    dynamics = oracle.LinearSystem((data["linear_A"], data["linear_B"]))
    policy = oracle.LinearSystem((data["linear_K"],))
    states, actions = np_rollout.compute_trajectory(dynamics, policy, data["linear_x0"],
                                                    int(data["linear_num_steps"]))
    assert_allclose(states, data["linear_states"], rtol=1e-13, atol=1e-15)
    assert_allclose(actions, data["linear_actions"], rtol=1e-13, atol=1e-15)


def reference_case(data, key):
    """The case of a fixture entry (tests/golden/make_reference_roa.py builds the same)."""
    import cases
    num = [int(v) for v in data[key + "_num_points"]]
    case = cases.make_case(key, num_points=num, dynamics="analytic")
    case["limits"] = [[float(lo), float(hi)] for lo, hi in data[key + "_limits"]]
    return case, int(data[key + "_horizon"]), float(data[key + "_tol"])


# ---- the Python layer without a GPU --------------------------------------------------------------------------
class _FakeEngine(object):
    """Stands in for the context: records the calls, fills the outputs with what the shim computes."""

    def __init__(self, shim):
        import torch
        self.shim, self.torch_device, self.calls = shim, torch.device("cpu"), []
        self.tri = None

    def model_set(self, desc):
        self.desc = desc

    def rollout(self, lo, hi, d_start, steps, d_state, d_traj=None, d_actions=None, steps_per_launch=0):
        self.calls.append(("rollout", lo, hi, d_start is None, steps, d_traj is not None,
                           d_actions is not None, steps_per_launch))
        n, d = hi - lo, self.desc.grid.d
        start = None if d_start is None else np.ascontiguousarray(d_start.numpy())
        end = np.zeros((n, d))
        traj = np.zeros((max(steps, 1), n, d))
        act = np.zeros((max(steps, 1), n, self.desc.policy.m))
        assert self.shim.ro_rollout(C.byref(self.desc), C.c_int64(n), _p(start), steps, 1, _p(end), _p(traj),
                                    _p(act)) == 0
        import torch
        d_state.copy_(torch.from_numpy(end))
        if d_traj is not None:
            assert d_traj.is_contiguous() and tuple(d_traj.shape) == (steps, n, d)
            d_traj.copy_(torch.from_numpy(traj[:steps]))
        if d_actions is not None:
            assert d_actions.is_contiguous() and tuple(d_actions.shape) == (steps, n, self.desc.policy.m)
            d_actions.copy_(torch.from_numpy(act[:steps]))

    def rollout_mask(self, n, d, d_state, equilibrium, tol, d_bits, d_count):
        self.calls.append(("mask", n, d, tol))
        import torch
        eq = np.zeros(d) if equilibrium is None else np.ravel(np.asarray(equilibrium, dtype=np.float64))
        member = np.zeros(n, dtype=np.uint8)
        states = np.ascontiguousarray(d_state.numpy())
        assert self.shim.ro_mask(C.c_int64(n), d, _p(states), _p(eq), C.c_double(tol), _p(member), None) == 0
        self.member = member

    def bits_to_bytes(self, n, d_bits, d_bytes):
        import torch
        d_bytes[:n] = torch.from_numpy(self.member)


@pytest.fixture
def fake_engine(shim, monkeypatch):
    import copy
    from safe_learning_amd import _evaluate
    engine = _FakeEngine(shim)
    builder = ModelBuilder(engine, None)

    def _engine(d):
        builder.grid = copy.copy(F.GridWorld([[0., 1.]] * d, 2))
        return engine, builder
    monkeypatch.setattr(U, "_engine", _engine)
    monkeypatch.setattr(_evaluate, "_ctx", lambda: engine)
    return engine


def _linear_pair():
    case = RC.make(*RC.LINEAR_CASES["pendulum"])
    return case, RC.engine_pair(case)


def test_wrapper_shapes_and_values(fake_engine):
    case, (dynamics, policy) = _linear_pair()
    pts, states, actions = RC.oracle_linear("pendulum")
    # one initial state: the reference's shapes
    s, a = U.compute_trajectory(dynamics, policy, pts[3], 20)
    assert s.shape == (20, 2) and a.shape == (19, 1)
    assert_array_equal(s, states[3, :20])
    assert_array_equal(a, actions[3, :19])
    # [n, d] initial states
    s, a = U.compute_trajectory(dynamics, policy, pts[:5], 20, steps_per_launch=3)
    assert s.shape == (5, 20, 2) and a.shape == (5, 19, 1)
    assert_array_equal(s, states[:5, :20])
    assert fake_engine.calls[-1][-1] == 3
    s, a = U.compute_trajectory(dynamics, policy, pts[:5], 1)
    assert s.shape == (5, 1, 2) and a.shape == (5, 0, 1)
    assert_array_equal(s[:, 0], pts[:5])
    # compute_roa: horizon - 1 steps, grid or point list, trajectories as a view of the step-major buffer
    grid = RC.engine_grid(case)
    tol = 0.05
    want = np_rollout.distances(states[:, 60]) <= tol
    assert want.any() and not want.all()
    fake_engine.calls.clear()
    roa = U.compute_roa(grid, (dynamics, policy), horizon=61, tol=tol)
    assert roa.dtype == np.bool_ and roa.shape == (grid.nindex,)
    assert_array_equal(roa, want)
    assert fake_engine.calls[0] == ("rollout", 0, grid.nindex, True, 60, False, False, 0)
    roa, traj = U.compute_roa(pts, (dynamics, policy), horizon=61, tol=tol, no_traj=False)
    assert traj.shape == (len(pts), 2, 61)
    assert_array_equal(roa, want)
    assert_array_equal(traj, states[:, :61].transpose(0, 2, 1))
    import torch
    roa, traj = U.compute_roa(torch.from_numpy(pts), (dynamics, policy), horizon=61, tol=tol, no_traj=False)
    assert isinstance(roa, torch.Tensor) and roa.dtype == torch.bool
    assert traj.shape == (len(pts), 2, 61) and traj.stride() == (2, 1, 2 * len(pts))     # a view, no copy
    shifted = U.compute_roa(pts, (dynamics, policy), horizon=61, tol=tol, equilibrium=[[0.5, 0.0]])
    assert_array_equal(shifted, np_rollout.distances(states[:, 60], np.array([[0.5, 0.0]])) <= tol)
    # a callable, as in the reference
    odyn, opol = RC.oracle_pair(case)
    step = np_rollout.closed_loop(odyn, opol)
    roa = U.compute_roa(pts, lambda x: step(x.numpy()), horizon=61, tol=tol)
    assert_array_equal(roa, want)
    roa, traj = U.compute_roa(grid, lambda x: step(x.numpy()), horizon=5, tol=tol, no_traj=False)
    assert_array_equal(traj, states[:, :5].transpose(0, 2, 1))


def test_wrapper_argument_errors(fake_engine, monkeypatch):
    case, (dynamics, policy) = _linear_pair()
    pts = RC.oracle_points(case)
    gp_case = RC.make("pendulum", dict(num_points=5, n_gp=8))
    uncertain = RC.engine_pair(gp_case)[0]
    assert isinstance(uncertain, F.UncertainFunction)
    with pytest.raises(ValueError, match="callable"):
        U.compute_roa(pts, (uncertain, policy))
    with pytest.raises(ValueError, match="callable"):
        U.compute_trajectory(uncertain, policy, pts[0], 5)
    with pytest.raises(TypeError, match="policy"):
        U.compute_roa(pts, (dynamics, np.zeros((len(pts), 1))))
    with pytest.raises(TypeError, match="dynamics"):
        U.compute_roa(pts, (F.QuadraticFunction(np.eye(2)), policy))
    with pytest.raises(TypeError, match="pair"):
        U.compute_roa(pts, 3.0)
    with pytest.raises(ValueError, match="pair"):
        U.compute_roa(pts, (dynamics, policy, policy))
    with pytest.raises(ValueError, match="horizon"):
        U.compute_roa(pts, (dynamics, policy), horizon=0)
    with pytest.raises(ValueError, match="num_steps"):
        U.compute_trajectory(dynamics, policy, pts[0], 0)
    with pytest.raises(ValueError, match="equilibrium"):
        U.compute_roa(pts, (dynamics, policy), equilibrium=np.zeros(3))
    with pytest.raises(ValueError, match=r"\[n, d\]"):
        U.compute_roa(np.zeros((2, 2, 2)), (dynamics, policy))
    with pytest.raises(ValueError, match="inputs"):
        U.compute_roa(np.zeros((4, 3)), (dynamics, policy))             # a 2-D policy on 3-D states
    assert not fake_engine.calls
    # one GPU only
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    with pytest.raises(NotImplementedError, match="one GPU"):
        U.compute_roa(pts, (dynamics, policy))
    with pytest.raises(NotImplementedError, match="one GPU"):
        U.compute_roa(pts, lambda x: x)
    with pytest.raises(NotImplementedError, match="one GPU"):
        U.compute_trajectory(dynamics, policy, pts[0], 5)


def test_package_exports():
    import safe_learning_amd as sl
    assert sl.compute_roa is U.compute_roa and sl.compute_trajectory is U.compute_trajectory
