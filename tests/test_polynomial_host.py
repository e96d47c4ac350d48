"""CPU checks of the polynomial dynamics (safe_learning_amd/csrc/sl_polynomial.h).

The header is compiled with g++ into a test-only shim (tests/hostsim/polynomial.cpp) and compared BIT FOR
BIT with the NumPy restatement (tests/np_polynomial.py): the arithmetic is multiplications and additions in
one stated order, without contraction, so there is nothing to round differently.  The restatement in turn is
held against a run of the reference's own VanDerPol (tests/golden/reference_vanderpol.npz).  The GPU tests
(tests/test_gpu_polynomial.py) repeat the bit comparisons through the kernels.
"""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import hostsim_build
import np_rollout
import polynomial_cases as PC
from conftest import GOLDEN_DIR
from safe_learning_amd import _hip
from safe_learning_amd import functions as F
from safe_learning_amd import utilities as U
from safe_learning_amd._model import ModelBuilder


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return hostsim_build.shared("polynomial.cpp", tmp_path_factory.mktemp("polynomial"), hostsim_build.SHIM_FLAGS)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class _RecordingCtx(object):
    """Captures the model description and the term table instead of uploading them."""

    def __init__(self):
        import torch
        self.torch_device = torch.device("cpu")
        self.tables = []

    def model_set(self, desc):
        self.desc = desc

    def dynamics_polynomial_set(self, d, m, rows, coef, exponents, substeps, h):
        expo = np.zeros((len(rows), _hip.MAX_INPUT_DIM), dtype=np.uint8)
        expo[:, :d + m] = exponents
        self.tables.append((d, m, np.ascontiguousarray(rows, dtype=np.int32),
                            np.ascontiguousarray(coef, dtype=np.float64), expo, int(substeps), float(h)))


def _uploaded(spec):
    """(dynamics description, table arguments) as the model builder hands them to the engine."""
    ctx = _RecordingCtx()
    builder = ModelBuilder(ctx, F.GridWorld([[0., 1.]] * spec.state_dim, 2))
    policy = F.LinearSystem((np.zeros((spec.action_dim, spec.state_dim)),))
    builder.upload(policy, spec, F.QuadraticFunction(np.eye(spec.state_dim)))
    assert ctx.desc.dynamics.kind == _hip.DYN_POLYNOMIAL == 5 and len(ctx.tables) == 1
    return ctx.desc.dynamics, ctx.tables[0]


def _shim_eval(shim, spec, states, actions):
    desc, (d, m, rows, coef, expo, substeps, h) = _uploaded(spec)
    states = np.ascontiguousarray(states, dtype=np.float64)
    actions = np.ascontiguousarray(actions, dtype=np.float64)
    out = np.full((len(states), d), 7.0)
    rc = shim.poly_eval(C.byref(desc), d, m, len(rows), _p(rows), _p(coef), _p(expo), substeps, C.c_double(h),
                        C.c_int64(len(states)), _p(states), _p(actions), _p(out))
    assert rc == 0
    return out


# ---- the host build against the NumPy truth: bit for bit ---------------------------------------------------
@pytest.mark.parametrize("key", PC.KEYS)
def test_shim_equals_numpy_bit_for_bit(shim, key):
    PC.check_systems()
    for n in PC.POINT_COUNTS:
        states, actions = PC.points(key, n)
        want = PC.truth(key)(states, actions)
        got = _shim_eval(shim, PC.system(key), states, actions)
        PC.assert_same_bits(got, want, "%s, %d points" % (key, n))
        if n >= 8:
            assert np.isnan(want[3]).any() and not np.isfinite(want[2]).all()      # non-finite rows came through
            assert np.isfinite(want[8:]).all()


def test_shim_follows_a_short_rollout_bit_for_bit(shim):
    """Eight closed-loop steps with the NumPy policy between the steps: the bits stay equal step after step."""
    for key in ("chain3", "full", "duffing-u"):
        states, actions = PC.trajectory_truth(key)
        for s in range(actions.shape[1]):
            got = _shim_eval(shim, PC.system(key), states[:, s], actions[:, s])
            PC.assert_same_bits(got, states[:, s + 1], "%s step %d" % (key, s))


def test_table_is_sorted_by_row_and_validated(shim):
    rows = np.array([1, 0, 1, 0, 1], dtype=np.int32)
    coef = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
    expo = np.zeros((5, _hip.MAX_INPUT_DIM), dtype=np.uint8)
    expo[:, 0] = [1, 2, 3, 4, 5]
    expo[:, 2] = [0, 1, 0, 1, 0]
    row_start = np.zeros(8, dtype=np.int32)
    out_coef, out_expo = np.zeros(64), np.zeros(64, dtype=np.uint64)
    msg = C.create_string_buffer(200)

    def build(d, m, n, substeps=10):
        return shim.poly_build(d, m, n, _p(rows), _p(coef), _p(expo), substeps, C.c_double(0.01), _p(row_start),
                               _p(out_coef), _p(out_expo), msg)
    assert build(2, 1, 5) == 0
    assert_array_equal(row_start, [0, 2, 5, 5, 5, 5, 5, 5])
    assert_array_equal(out_coef[:5], [2.0, 4.0, 1.0, 3.0, 5.0])                  # stable within a row
    assert_array_equal(out_expo[:5], [0x10002, 0x10004, 1, 3, 5])
    assert build(2, 1, 0) == 0 and not row_start.any()                          # no terms at all
    assert build(1, 1, 5) == _hip.ERR_INVALID and b"row 1 of 1" in msg.value    # a row out of range
    assert build(2, 1, 5, substeps=-1) == _hip.ERR_INVALID
    expo[4, 3] = 1                                                              # an exponent past d + m inputs
    assert build(2, 1, 5) == _hip.ERR_INVALID and b"input 3 of 3" in msg.value
    expo[4, 3] = 0
    expo[0, 1] = _hip.POLY_MAX_DEGREE                                           # 1 + 8: over the degree cap
    assert build(2, 1, 5) == _hip.ERR_INVALID and b"SL_POLY_MAX_DEGREE" in msg.value


def test_program_under_sanitizers(tmp_path):
    """The stand-alone program: caps, rows out of range, width mismatch, empty rows, no terms, the sort - under
    the address and undefined-behaviour sanitizers where the toolchain has them."""
    exe = hostsim_build.sanitized_program_or_plain("polynomial.cpp", tmp_path, hostsim_build.SHIM_FLAGS)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "all checks passed" in run.stdout, run.stdout


# ---- the NumPy truth against a run of the reference itself ---------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN_DIR, "reference_vanderpol.npz"))


def test_numpy_truth_matches_reference_step(fixture):
    """One step, both normalisations.  The reference multiplies ``damping * (x**2 - 1) * y`` where the table
    adds ``damping x^2 y`` and ``-damping y``: measured difference at most 1.1e-15 on normalised states of
    magnitude <= 1; the bound is one decade above that."""
    states = fixture["step_states"]
    assert np.abs(states).max() <= 1.0 and len(states) == 500
    assert float(fixture["damping"]) == 1 and float(fixture["dt"]) == 0.1
    assert_array_equal(fixture["normalization"], [3, 3])
    for key, case in (("norm", "vdp"), ("plain", "vdp-plain")):
        got = PC.truth(case)(states, np.zeros((len(states), 1)))
        worst = np.abs(got - fixture["step_" + key]).max()
        print("one step (%s): largest difference from the reference %.3g" % (key, worst))
        assert_allclose(got, fixture["step_" + key], rtol=0, atol=1e-14)
        assert np.abs(got - states).max() > 1e-2                          # a step that moves the states


def test_linearize_matches_reference(fixture):
    for key, case in (("norm", "vdp"), ("plain", "vdp-plain")):
        ad = PC.system(case).linearize()
        assert ad.shape == (2, 2)
        assert_allclose(ad, fixture["linearize_" + key], rtol=1e-13, atol=0)


def test_numpy_truth_reproduces_reference_roa(fixture):
    roa, traj = PC.vdp_roa()
    assert (int(fixture["roa_num_points"]), int(fixture["roa_horizon"]), float(fixture["roa_tol"])) == (
        PC.VDP_NUM_POINTS, PC.VDP_HORIZON, PC.VDP_TOL)
    assert_array_equal(traj[:, :, 0], fixture["roa_points"])
    assert_array_equal(roa, fixture["roa"])
    assert_allclose(traj[:, :, -1][roa], fixture["roa_end"][roa], rtol=0, atol=1e-10)
    steps = fixture["roa_traj"].shape[2]
    # the first steps: the same cells have left the finite numbers, and inside the region (contracting, states
    # below 1) twelve steps of at most 1.1e-15 each stay under 1e-13
    # (cell by cell: the reference's matmul with the diagonal scale turns both coordinates into NaN at once)
    assert_array_equal(np.isfinite(traj[:, :, :steps]).all(axis=1), np.isfinite(fixture["roa_traj"]).all(axis=1))
    assert not np.isfinite(fixture["roa_traj"]).all() and np.abs(fixture["roa_traj"][roa]).max() < 1.0
    assert_allclose(traj[:, :, :steps][roa], fixture["roa_traj"][roa], rtol=0, atol=1e-13)


def test_map1_roa_condition():
    pts, roa = PC.map1_roa()
    assert len(pts) == 65 and roa.sum() == 47


# ---- the Python classes ----------------------------------------------------------------------------------
def test_package_exports():
    import safe_learning_amd as sl
    assert sl.PolynomialSystem is F.PolynomialSystem and sl.VanDerPol is F.VanDerPol
    assert issubclass(sl.VanDerPol, sl.PolynomialSystem) and sl.VanDerPol._role == "dynamics"
    assert _hip.DYN_POLYNOMIAL == 5 and _hip.POLY_MAX_TERMS == 64 and _hip.POLY_MAX_DEGREE == 8


def test_ode_and_linearize():
    vdp = PC.system("vdp-plain")
    x = np.array([[0.3, -0.7], [1.5, 2.0]])
    want = np.stack((-x[:, 1], x[:, 0] + 1.0 * (x[:, 0] ** 2 - 1.0) * x[:, 1]), axis=1)
    assert_allclose(vdp.ode(x), want, rtol=1e-15, atol=1e-16)
    duff = PC.system("duffing-u")
    x0, x1, u = 0.4, -0.2, 0.6
    got = duff.ode([[x0, x1]], [[u]])
    assert_allclose(got, [[x1, -x0 - 0.5 * x0 ** 3 - 0.3 * x1 + u + 0.25 * x0 * u - 0.1 * u * u]], rtol=1e-15)
    ad, bd = duff.linearize()
    import scipy.signal
    tx, tu = np.diag([2., 2.]), np.diag([1.5])
    a = np.linalg.inv(tx).dot(np.array([[0., 1.], [-1., -0.3]])).dot(tx)
    b = np.linalg.inv(tx).dot(np.array([[0.], [1.]])).dot(tu)
    want_a, want_b, _, _, _ = scipy.signal.cont2discrete((a, b, 0, 0), 0.05, method="zoh")
    assert_allclose(ad, want_a, rtol=1e-13)
    assert_allclose(bd, want_b, rtol=1e-13)
    # the linearisation is the first-order part of one call of the dynamics
    eps = 1e-6
    step = PC.truth("duffing-u")
    for k, e in enumerate(np.eye(2)):
        assert_allclose(step(eps * e[None], np.zeros((1, 1)))[0] / eps, ad[:, k], atol=2e-3)
    a_map, b_map = PC.system("map1").linearize()
    assert_array_equal(a_map, [[0.5]])
    assert_array_equal(b_map, [[0.0]])


def test_constructor_errors():
    with pytest.raises(ValueError, match="state_dim \\+ action_dim"):
        F.PolynomialSystem([[(1.0, (1, 0))], []], 2, 1)
    with pytest.raises(ValueError, match="term lists"):
        F.PolynomialSystem([[]], 2, 1)
    with pytest.raises(ValueError, match="degree"):
        F.PolynomialSystem([[(1.0, (_hip.POLY_MAX_DEGREE, 1))]], 1, 1)
    with pytest.raises(ValueError, match="terms"):
        F.PolynomialSystem([[(1.0, (1, 0))] * (_hip.POLY_MAX_TERMS + 1)], 1, 1)
    with pytest.raises(ValueError, match="negative"):
        F.PolynomialSystem([[(1.0, (-1, 0))]], 1, 1)
    with pytest.raises(ValueError, match="inner_euler_steps"):
        F.PolynomialSystem([[]], 1, 1, inner_euler_steps=-1)
    with pytest.raises(ValueError, match="states"):
        F.PolynomialSystem([[]] * 7, 7, 1)
    with pytest.raises(ValueError, match="normalization"):
        F.PolynomialSystem([[]], 1, 1, normalization=[[1.0, 2.0], [1.0]])


def test_builder_uploads_a_table_once_and_refuses_mismatches():
    ctx = _RecordingCtx()
    builder = ModelBuilder(ctx, F.GridWorld([[-1., 1.]] * 2, 5))
    policy = F.LinearSystem((np.zeros((1, 2)),))
    value = F.QuadraticFunction(np.eye(2))
    vdp, other = PC.system("vdp"), F.VanDerPol(1, dt=0.1, normalization=[3, 3])
    builder.upload(policy, vdp, value)
    builder.upload(policy, vdp, value)
    assert len(ctx.tables) == 1                                           # an unchanged spec is not uploaded again
    d = ctx.desc.dynamics
    assert (d.kind, d.normalize, d.tx[0], d.tx[1], d.tu[0]) == (5, 1, 3.0, 3.0, 1.0)
    assert d.tx_inv[0] == np.float64(3.0) ** -1
    assert ctx.tables[0][5:] == (10, 0.1 / 10)
    builder.upload(policy, other, value)                                  # an equal spec is still a new one
    builder.upload(policy, vdp, value)
    assert len(ctx.tables) == 3
    with pytest.raises(ValueError, match="grid has 2 dimensions"):
        builder.upload(policy, PC.system("map1"), value)
    with pytest.raises(ValueError, match="policy gives 1"):
        ModelBuilder(ctx, F.GridWorld([[-1., 1.]] * 3, 5)).upload(
            F.LinearSystem((np.zeros((1, 3)),)), PC.system("chain3"), F.QuadraticFunction(np.eye(3)))
    with pytest.raises(TypeError, match="PolynomialSystem, VanDerPol"):
        builder.upload(policy, object(), value)
    assert len(ctx.tables) == 3


class _FakeEngine(_RecordingCtx):
    """Stands in for the rollout context: records the calls."""

    def __init__(self):
        super(_FakeEngine, self).__init__()
        self.calls = []

    def rollout(self, lo, hi, d_start, steps, d_state, d_traj=None, d_actions=None, steps_per_launch=0):
        self.calls.append(("rollout", lo, hi, steps, self.desc.dynamics.kind))
        d_state.zero_()


@pytest.fixture
def fake_engine(monkeypatch):
    import copy
    from safe_learning_amd import _evaluate
    engine = _FakeEngine()
    builder = ModelBuilder(engine, None)

    def _engine(d):
        builder.grid = copy.copy(F.GridWorld([[0., 1.]] * d, 2))
        return engine, builder
    monkeypatch.setattr(U, "_engine", _engine)
    monkeypatch.setattr(_evaluate, "_ctx", lambda: engine)
    return engine


def test_rollout_wrapper_takes_the_new_classes(fake_engine):
    vdp, policy = PC.system("vdp"), PC.engine_policy("vdp")
    states, actions = U.compute_trajectory(vdp, policy, np.zeros((3, 2)), 5)
    assert states.shape == (3, 5, 2) and actions.shape == (3, 4, 1)
    assert fake_engine.calls[-1] == ("rollout", 0, 3, 4, 5) and len(fake_engine.tables) == 1
    with pytest.raises(ValueError, match="states"):
        U.compute_trajectory(vdp, F.LinearSystem((np.zeros((1, 3)),)), np.zeros((3, 3)), 5)     # 3-D states
    with pytest.raises(ValueError, match="actions"):
        U.compute_trajectory(PC.system("chain3"), F.LinearSystem((np.zeros((1, 3)),)), np.zeros((3, 3)), 5)
    with pytest.raises(TypeError, match="PolynomialSystem, VanDerPol"):
        U.compute_roa(np.zeros((4, 2)), (F.QuadraticFunction(np.eye(2)), policy))
    assert len(fake_engine.calls) == 2                   # (the start states' copy and the steps of the first call)


def test_gradients_refuse_polynomial_dynamics(monkeypatch):
    """ActorCritic, policy_gradient, action_gradient and decrease_gradient name PolynomialSystem in a TypeError
    before anything reaches the engine (no context is ever created here: there is no GPU)."""
    import safe_learning_amd as sl
    from safe_learning_amd import lyapunov as L
    from safe_learning_amd import reinforcement_learning as RL

    def no_engine(*args, **kwargs):
        raise AssertionError("the engine was reached")
    monkeypatch.setattr(_hip.Context, "__init__", no_engine)
    vdp = PC.system("vdp")
    with pytest.raises(TypeError, match="PolynomialSystem"):
        sl.ActorCritic(F.NeuralNetwork([4, 1], ["tanh", None], input_dim=2), vdp, F.QuadraticFunction(np.eye(3)),
                       F.NeuralNetwork([4, 1], ["tanh", None], input_dim=2))
    rl = RL.PolicyIteration.__new__(RL.PolicyIteration)
    rl.dynamics = vdp
    for call in (lambda: rl.action_gradient(), lambda: rl.policy_gradient(),
                 lambda: rl.action_gradient(np.zeros((2, 2)), actions=np.zeros((1, 1)))):
        with pytest.raises(TypeError, match="PolynomialSystem"):
            call()
    lyap = L.Lyapunov.__new__(L.Lyapunov)
    lyap.dynamics, lyap.lyapunov_function = vdp, F.QuadraticFunction(np.eye(2))
    with pytest.raises(TypeError, match="PolynomialSystem"):
        lyap.decrease_gradient(np.zeros((2, 2)))
