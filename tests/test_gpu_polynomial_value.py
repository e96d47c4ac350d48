"""A polynomial Lyapunov function on the GPU (SL_V_POLYNOMIAL: csrc/sl_poly_value.h through k_poly_values,
k_poly_sweep, k_poly_check and k_eval_simple; needs an MI355X) against the NumPy restatement
(tests/np_polynomial_value.py) and the oracle's ``Lyapunov`` with that restatement as V and L_v.

The arithmetic is multiplications and additions in one stated order, compiled without contraction: V and its
gradient equal the restatement's BIT FOR BIT - derived, not measured - and under dynamics the project already
holds bit for bit (PolynomialSystem, LinearSystem) so do the decrease masks, the safe sets and ``c_max``.
Cases, conditions and oracle results: tests/polynomial_value_cases.py.
"""

import signal

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import cases
import guarded
import np_polynomial_value as NPV
import oracle
import polynomial_value_cases as PVC

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


def _engine_lyapunov(sl, key, mode="norm1", tau=0.0, initial=None, adaptive=False):
    _, limits, num_points, _ = PVC.LYAPUNOV[key]
    value = PVC.lyapunov_value(key)
    dynamics, policy = PVC.engine_pair(key)
    return sl.Lyapunov(sl.GridWorld(limits, num_points), value, dynamics, PVC.LF, PVC.engine_lv(sl, value, mode), tau,
                       policy, initial_set=None if initial is None else initial.copy(), adaptive=adaptive)


# ---- 6. point evaluation -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("negate", [False, True])
@pytest.mark.parametrize("key", PVC.KEYS)
def test_point_evaluation_bit_exact(sl, key, negate):
    import torch
    from safe_learning_amd import _evaluate, _hip
    PVC.check_specs()
    spec = -PVC.spec(key) if negate else PVC.spec(key)
    truth = PVC.truth(key, negate)
    d = spec.input_dim
    for n in PVC.POINT_COUNTS:
        x = PVC.points(key, n)
        want_v, want_g = truth(x), truth.gradient(x)
        PVC.assert_same_bits(spec(x), want_v, "%s V, %d points" % (key, n))
        PVC.assert_same_bits(spec.gradient(x), want_g, "%s gradient, %d points" % (key, n))
        # the same through the entry point, the outputs between guard zones
        ctx = _evaluate._ctx()
        d_pts = torch.from_numpy(x).to(ctx.torch_device)
        lv_spec = sl.AbsGradient(spec)

        def call(value, grad, lv):
            _evaluate.value(spec, d_pts, lv_spec)                              # uploads spec and L_v
            ctx.eval_points(_hip.EVAL_VALUE, n, d_pts, value)
            ctx.eval_points(_hip.EVAL_GRADIENT, n, d_pts, grad)
            ctx.eval_points(_hip.EVAL_LV, n, d_pts, lv)

        value, grad, lv = guarded.run(call, [n, n * d, n * d])
        PVC.assert_same_bits(value.view(np.float64).reshape(n, 1), want_v, "guarded V")
        PVC.assert_same_bits(grad.view(np.float64).reshape(n, d), want_g, "guarded gradient")
        PVC.assert_same_bits(lv.view(np.float64).reshape(n, d), np.abs(want_g), "guarded |gradient|")
    # device tensors in, device tensors out
    d_out = spec.gradient(d_pts)
    assert isinstance(d_out, torch.Tensor) and d_out.shape == (PVC.POINT_COUNTS[-1], d)


def test_lipschitz_lyapunov_at_states(sl):
    """``lyap.lipschitz_lyapunov(states)`` under both gradient specs, through k_eval_simple."""
    key = "vdp"
    value, truth = PVC.lyapunov_value(key), NPV.NumpyPolynomialValue(PVC.lyapunov_value(key))
    x = np.random.default_rng(2).uniform(-1, 1, size=(65, 2))
    for mode, want in (("norm1", truth.norm1_gradient(x)), ("abs", truth.abs_gradient(x))):
        lyap = _engine_lyapunov(sl, key, mode, 0.002)
        PVC.assert_same_bits(lyap.lipschitz_lyapunov(x), want, mode)


# ---- 7. update_values ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,variant", [("vdp", 2), ("vdp-pow2", 2), ("chain3", 0), ("linear4", 4)])
def test_update_values_bit_exact(sl, key, variant):
    lyap = _engine_lyapunov(sl, key)
    assert lyap._ctx.last_kernel() == "k_poly_values<d=%d>" % variant
    truth = NPV.NumpyPolynomialValue(PVC.lyapunov_value(key))
    grid = oracle.GridWorld(*PVC.LYAPUNOV[key][1:3])
    PVC.assert_same_bits(lyap.values, truth(grid.all_points)[:, 0], key)
    assert list(grid.num_points) == {"vdp": [51, 51], "vdp-pow2": [64, 32], "chain3": [9, 10, 11], "linear4": [9] * 4}[key]
    # -V
    neg = sl.Lyapunov(lyap.discretization, -PVC.lyapunov_value(key), lyap.dynamics, PVC.LF, 0.5, 0.0, lyap.policy)
    PVC.assert_same_bits(neg.values, (-truth)(grid.all_points)[:, 0], key + " negated")


# ---- 8. update_safe_set, exact ---------------------------------------------------------------------------------------
NOTES = {"vdp": "k_poly_sweep<d=2, m=1, dynamics=5>", "vdp-pow2": "k_poly_sweep<d=2, m=1, dynamics=5>",
         "chain3": "k_poly_sweep<d=0, m=0, dynamics=5>", "linear4": "k_poly_sweep<d=4, m=1, dynamics=1>"}


@pytest.mark.parametrize("mode,positive_tau", PVC.MODES)
@pytest.mark.parametrize("key", ["vdp", "vdp-pow2", "chain3", "linear4"])
def test_update_safe_set_equals_the_oracle(sl, key, mode, positive_tau):
    tau = PVC.TAU[key] if positive_tau else 0.0
    olyap, initial = PVC.lyapunov_truth(key, mode, tau)
    lyap = _engine_lyapunov(sl, key, mode, tau, initial)
    lyap.update_safe_set()
    assert_array_equal(lyap.safe_set, olyap.safe_set)
    assert lyap.c_max == olyap.c_max
    assert lyap.safe_count == olyap.safe_set.sum()
    assert lyap._ctx.last_kernel() == NOTES[key], lyap._ctx.last_kernel()
    # the quartic part decides cells: the quadratic form alone gives another safe set
    if tau == 0.0 and key in ("vdp", "chain3"):
        P = PVC.lyapunov_matrix(key)
        quad = sl.Lyapunov(lyap.discretization, sl.QuadraticFunction(P), lyap.dynamics, PVC.LF, 0.8, 0.0, lyap.policy,
                           initial_set=initial.copy())
        quad.update_safe_set()
        assert quad.safe_set.sum() == {"vdp": 471, "chain3": 281}[key] != lyap.safe_set.sum()


@pytest.mark.parametrize("key", ["vdp", "chain3"])
def test_can_shrink_false_after_an_enlarged_initial_set(sl, key):
    tau = PVC.TAU[key]
    olyap, initial = PVC.lyapunov_truth(key, "abs", tau)
    _, limits, num_points, radius = PVC.LYAPUNOV[key]
    ogrid = oracle.GridWorld(limits, num_points)
    value = NPV.NumpyPolynomialValue(PVC.lyapunov_value(key))
    dynamics, policy = PVC.oracle_pair(key)
    fresh = oracle.Lyapunov(ogrid, value, dynamics, PVC.LF, value.abs_gradient, tau, policy, initial_set=initial.copy())
    lyap = _engine_lyapunov(sl, key, "abs", tau, initial)
    larger = np.linalg.norm(ogrid.all_points, axis=1) <= 2.5 * radius
    assert initial.sum() < larger.sum() < ogrid.nindex
    for step, (init, shrink, new_tau) in enumerate(((initial, True, tau), (larger, False, tau), (larger, False, 2 * tau),
                                                    (initial, True, 0.0))):
        for obj in (lyap, fresh):
            obj.initial_safe_set = init.copy()
            obj.tau = new_tau
            obj.update_safe_set(can_shrink=shrink)
        assert_array_equal(lyap.safe_set, fresh.safe_set, err_msg="step %d" % step)
        assert lyap.c_max == fresh.c_max, step
    assert fresh.safe_set.sum() == PVC.lyapunov_truth(key, "abs", 0.0)[0].safe_set.sum()


def test_interpolated_policy(sl):
    """An interpolated (Triangulation) policy: the one policy kind whose table descriptors k_poly_sweep stages in
    LDS.  The next states must be, bit for bit, those the table flavour of k_det_sweep computes under the same
    policy and a quadratic V (``sl_eval_points``), and decrease / threshold those of the restatement AT those
    next states - an oracle of the policy itself is not needed (the reference's choice on table faces depends on
    its search history)."""
    import torch
    from safe_learning_amd import _evaluate
    key, tau = "vdp", PVC.TAU["vdp"]
    _, limits, num_points, radius = PVC.LYAPUNOV[key]
    value, dynamics = PVC.lyapunov_value(key), PVC.engine_pair(key)[0]
    pgrid = sl.GridWorld(limits, [7, 9])
    policy = sl.Triangulation(pgrid, np.random.default_rng(8).uniform(-1, 1, size=(pgrid.nindex, 1)))
    grid = sl.GridWorld(limits, num_points)
    initial = np.linalg.norm(grid.all_points, axis=1) <= radius
    lyap = sl.Lyapunov(grid, value, dynamics, PVC.LF, sl.AbsGradient(value), tau, policy, initial_set=initial.copy())
    n, d = grid.nindex, 2
    dbg = torch.zeros((n, 2 + 2 * d), dtype=torch.float64, device=lyap._ctx.torch_device)
    lyap._upload_model()
    lyap._refresh_init_bits()
    lyap._ctx.lyap_sweep(0, n, lyap._d_init, lyap._d_values, lyap._d_neg, lyap._d_result, dbg)
    assert lyap._ctx.last_kernel() == "k_poly_sweep<d=2, m=1, dynamics=5> (interpolated policy from LDS)"
    rec = dbg.cpu().numpy()
    x = oracle.GridWorld(limits, num_points).index_to_state(np.arange(n))
    actions = _evaluate.policy(policy, x)
    assert np.ptp(actions) > 0.5
    nxt = _evaluate.dynamics(dynamics, x, actions)
    PVC.assert_same_bits(rec[:, 2:4], nxt, "next states")
    PVC.assert_same_bits(nxt, PVC.PC.truth(PVC.LYAPUNOV[key][0])(x, actions), "next states against NumPy")
    truth = NPV.NumpyPolynomialValue(value)
    PVC.assert_same_bits(rec[:, 0], (truth(nxt) - truth(x))[:, 0], "decrease")
    lv = truth.abs_gradient(x)
    PVC.assert_same_bits(rec[:, 1], (-(lv[:, 0] + lv[:, 1])) * (1.0 + PVC.LF) * tau, "threshold")
    neg = np.unpackbits(lyap._d_neg.cpu().numpy().view(np.uint8), bitorder="little")[:n].astype(bool)
    assert_array_equal(neg, rec[:, 0] < rec[:, 1])
    assert 0 < neg.sum() < n


# ---- 9. the notebook's candidate on the notebook's system --------------------------------------------------------------
@pytest.mark.parametrize("num_points", [51, 101])
def test_notebook_candidate_on_the_pendulum(sl, num_points):
    """``lyapunov_function_learning.ipynb``: the SOS candidate under the saturated LQR policy, tau = 0.  The
    smallest relative change of V off the initial set (4.1e-5 / 9.8e-6) is far above the ulps by which the
    device's sin and cos differ from the host's."""
    olyap, initial = PVC.notebook_truth(num_points)
    value = PVC.spec("sos")
    dynamics, policy = PVC.notebook_system(sl)
    lyap = sl.Lyapunov(sl.GridWorld([[-1, 1]] * 2, num_points), value, dynamics, PVC.LF,
                       sl.Norm1Function(sl.Gradient(value)), 0.0, policy, initial_set=initial.copy())
    PVC.assert_same_bits(lyap.values, olyap.values, "values")
    lyap.update_safe_set()
    assert lyap._ctx.last_kernel() == "k_poly_sweep<d=2, m=1, dynamics=2>"
    assert_array_equal(lyap.safe_set, olyap.safe_set)
    assert lyap.c_max == olyap.c_max                              # a value at a grid point


# ---- 10. GP dynamics ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rbf", "notebook"])
def test_gp_dynamics_records_and_masks(sl, kind):
    from test_gpu_lyapunov import _check_masks, _engine_records, _oracle_all
    lyap, olyap, initial, parts = PVC.gp_lyapunovs(kind)
    ref_rec, ref_neg = _oracle_all(olyap)
    PVC.check_gp_oracle(olyap, initial, ref_rec, ref_neg, parts, "GP " + kind)
    values, neg, rec = _engine_records(lyap)
    note = lyap._ctx.last_kernel()
    assert note.startswith("k_gp_small<general=0, d=2, m=1") and note.endswith(" + k_poly_check"), note
    d = 2
    PVC.assert_same_bits(values, olyap.values, "values")
    assert_allclose(rec[:, 2:2 + d], ref_rec[:, 2:2 + d], rtol=1e-9, atol=1e-12)       # mean
    assert_allclose(rec[:, 2 + d:], ref_rec[:, 2 + d:], rtol=1e-7, atol=1e-12)         # beta * sigma
    assert_allclose(rec[:, 1], ref_rec[:, 1], rtol=1e-9, atol=1e-14)                   # threshold
    assert_allclose(rec[:, 0], ref_rec[:, 0], rtol=1e-7, atol=1e-12)                   # decrease
    flips, _ = _check_masks(neg, ref_neg, rec, ref_rec, allowed=0)
    assert flips == 0
    lyap.update_safe_set()
    assert_array_equal(lyap.safe_set, olyap.safe_set)
    assert lyap.c_max == olyap.c_max


# ---- 11. downstream --------------------------------------------------------------------------------------------------
def test_adaptive_branch(sl):
    key, tau = "vdp", PVC.TAU["vdp"]
    _, limits, num_points, radius = PVC.LYAPUNOV[key]
    ogrid = oracle.GridWorld(limits, num_points)
    initial = np.linalg.norm(ogrid.all_points, axis=1) <= radius
    value = NPV.NumpyPolynomialValue(PVC.lyapunov_value(key))
    dynamics, policy = PVC.oracle_pair(key)
    olyap = oracle.Lyapunov(ogrid, value, dynamics, PVC.LF, value.abs_gradient, tau, policy, initial_set=initial.copy(),
                            adaptive=True)
    lyap = _engine_lyapunov(sl, key, "abs", tau, initial, adaptive=True)
    refined = 0
    for shrink, factor in ((True, 1.0), (False, 1.5)):
        lyap.update_safe_set(can_shrink=shrink, max_refinement=4, safety_factor=factor)
        olyap.update_safe_set(can_shrink=shrink, max_refinement=4, safety_factor=factor)
        assert_array_equal(lyap.safe_set, olyap.safe_set)
        assert_array_equal(lyap._refinement, olyap._refinement)
        assert lyap.c_max == olyap.c_max
        refined += int((olyap._refinement > 1).sum())
    assert refined >= 6 and initial.sum() < olyap.safe_set.sum() < ogrid.nindex


def test_get_safe_sample_on_the_gp_case(sl):
    import warnings
    lyap, olyap, _, _ = PVC.gp_lyapunovs("rbf")
    lyap.update_safe_set()
    olyap.update_safe_set()
    assert_array_equal(lyap.safe_set, olyap.safe_set)
    perturbations, limits = np.array([[0.], [0.1], [-0.1]]), np.array([[-1., 1.]])
    for positive in (True, False):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            sa, bound = sl.get_safe_sample(lyap, perturbations, limits, positive=positive)
            osa, obound = oracle.get_safe_sample(olyap, perturbations, limits, positive=positive)
        assert_allclose(bound, obound, rtol=1e-7)
        assert_array_equal(sa, osa)


def test_smallest_boundary_value_and_region(sl):
    spec, truth = PVC.spec("sos"), PVC.truth("sos")
    limits, num = [[-1, 1]] * 2, [41, 37]
    got = sl.smallest_boundary_value(spec, sl.GridWorld(limits, num))
    assert got == oracle.smallest_boundary_value(truth, oracle.GridWorld(limits, num))
    region = sl.get_lyapunov_region(spec, sl.GridWorld(limits, num), (20, 18))
    ref = oracle.get_lyapunov_region(truth, oracle.GridWorld(limits, num), (20, 18))
    assert_array_equal(region, ref)
    assert 0 < ref.sum() < ref.size


def test_sweep_in_two_ranges_through_the_c_abi(sl):
    """[0, 64 k) and [64 k, N) against one call: the mask words of the two ranges concatenate to those of
    the whole, and the smaller of their fail keys is the whole sweep's."""
    import torch
    from safe_learning_amd import _hip
    key, tau = "chain3", PVC.TAU["chain3"]
    olyap, initial = PVC.lyapunov_truth(key, "abs", tau)
    lyap = _engine_lyapunov(sl, key, "abs", tau, initial)
    lyap._upload_model()
    lyap._refresh_init_bits()
    n = lyap.discretization.nindex
    words, dev = (n + 63) // 64, lyap._ctx.torch_device
    d = 3
    values = lyap._d_values

    def sweep(lo, hi):
        nw = (hi - lo + 63) // 64
        neg = torch.zeros(nw, dtype=torch.int64, device=dev)
        result = torch.zeros(_hip.RESULT_WORDS, dtype=torch.int64, device=dev)
        dbg = torch.zeros((hi - lo, 2 + 2 * d), dtype=torch.float64, device=dev)
        lyap._ctx.lyap_sweep(lo, hi, lyap._d_init[lo // 64:lo // 64 + nw], values[lo:hi], neg, result, dbg)
        res = result.cpu().numpy()
        return neg.cpu().numpy(), (int(res[_hip.R_FAIL_V]) % (1 << 64), int(res[_hip.R_FAIL_I])), dbg.cpu().numpy()

    split = 64 * 7
    assert 0 < split < n and n % 64 != 0
    whole_neg, whole_key, whole_dbg = sweep(0, n)
    a_neg, a_key, a_dbg = sweep(0, split)
    b_neg, b_key, b_dbg = sweep(split, n)
    assert_array_equal(np.concatenate((a_neg, b_neg)), whole_neg)
    assert min(a_key, b_key) == whole_key and whole_key[0] != (1 << 64) - 1             # (a cell does fail)
    PVC.assert_same_bits(np.vstack((a_dbg, b_dbg)), whole_dbg, "records")
    bits = np.unpackbits(whole_neg.view(np.uint8), bitorder="little")[:n].astype(bool)
    assert_array_equal(bits, olyap.negative(olyap.discretization.index_to_state(np.arange(n))))
    assert len(whole_neg) == words and whole_key[1] < n


# ---- 12. state and errors ---------------------------------------------------------------------------------------------
def test_a_second_function_replaces_the_first(sl):
    key = "vdp"
    lyap = _engine_lyapunov(sl, key)
    first = lyap.values.copy()
    other = sl.PolynomialFunction([(1.0, (2, 0)), (3.0, (0, 2)), (0.5, (1, 3))], 2, [2.0, 0.5])
    lyap.lyapunov_function = other
    PVC.assert_same_bits(lyap.values, first, "values keep the old function's numbers until update_values()")
    # L_v still takes the gradient of the first function: said, not silently read as the second one's
    with pytest.raises(ValueError, match="must be built on the Lyapunov function itself"):
        lyap.update_values()
    lyap._lipschitz_lyapunov = sl.Norm1Function(sl.Gradient(other))
    lyap.update_values()
    grid = oracle.GridWorld(*PVC.LYAPUNOV[key][1:3])
    PVC.assert_same_bits(lyap.values, NPV.NumpyPolynomialValue(other)(grid.all_points)[:, 0], "second function")
    assert not np.array_equal(lyap.values, first)
    lyap.lyapunov_function = PVC.lyapunov_value(key)
    lyap._lipschitz_lyapunov = sl.Norm1Function(sl.Gradient(lyap.lyapunov_function))
    lyap.update_values()
    PVC.assert_same_bits(lyap.values, first, "back to the first")


def test_errors_name_the_call_and_the_spec(sl):
    import torch
    from safe_learning_amd import _hip
    ctx = _hip.Context()
    desc = _hip.ModelDesc()
    desc.grid = sl.GridWorld([[-1, 1]] * 2, 5)._desc()
    desc.policy.kind, desc.policy.m = _hip.POLICY_CONST, 1
    desc.dynamics.kind = _hip.DYN_LINEAR
    desc.value.kind = _hip.V_POLYNOMIAL
    with pytest.raises(sl.HipEngineError, match="call sl_value_polynomial_set first"):
        ctx.model_set(desc)
    ctx.value_polynomial_set(3, [1.0], [[1, 1, 0]])
    with pytest.raises(sl.HipEngineError, match="sl_value_polynomial_set is for 3 states, the model has 2"):
        ctx.model_set(desc)
    ctx.value_polynomial_set(2, [1.0], [[1, 1]])
    ctx.model_set(desc)
    desc.lipschitz.lv_kind = _hip.LIP_NORM_GRAD                               # accepted with the new kind
    ctx.model_set(desc)
    with pytest.raises(sl.HipEngineError, match="SL_POLY_MAX_DEGREE"):
        ctx.value_polynomial_set(2, [1.0], [[5, 4]])
    with pytest.raises(sl.HipEngineError, match="SL_POLYV_MAX_ENTRIES"):
        ctx.value_polynomial_set(2, np.ones(200), np.ones((200, 2), dtype=np.uint8))
    with pytest.raises(sl.HipEngineError, match="exponent on input 2 of 2"):
        ctx.value_polynomial_set(2, [1.0], [[1, 1, 1]])
    # a table of another dimension under the set model of the kind: the model is unset, not silently mismatched
    vals = torch.zeros(25, dtype=torch.float64, device=ctx.torch_device)
    ctx.values(0, 25, vals)
    ctx.value_polynomial_set(3, [1.0], [[1, 1, 0]])
    with pytest.raises(sl.HipEngineError, match="call sl_model_set first"):
        ctx.values(0, 25, vals)
    ctx.value_polynomial_set(2, [1.0], [[1, 1]])
    ctx.model_set(desc)
    ctx.values(0, 25, vals)
    # the signed gradient is the polynomial's only
    desc.value.kind, desc.lipschitz.lv_kind = _hip.V_QUADRATIC, _hip.LIP_CONST
    ctx.model_set(desc)
    pts = torch.zeros((4, 2), dtype=torch.float64, device=ctx.torch_device)
    out = torch.zeros((4, 2), dtype=torch.float64, device=ctx.torch_device)
    with pytest.raises(sl.HipEngineError, match="SL_EVAL_GRADIENT"):
        ctx.eval_points(_hip.EVAL_GRADIENT, 4, pts, out)
    ctx.close()


def test_refusals_name_the_spec(sl):
    lyap, _, _, _ = PVC.gp_lyapunovs("rbf")
    x = np.zeros((3, 2))
    with pytest.raises(NotImplementedError, match="decrease_gradient.*polynomial_function.*second derivatives"):
        lyap.decrease_gradient(x)
    # the library's own refusal, below the Python layer
    import torch
    lyap._upload_model()
    dev = lyap._ctx.torch_device
    pts = torch.zeros((4, 2), dtype=torch.float64, device=dev)
    grad, con = torch.zeros((4, 1), dtype=torch.float64, device=dev), torch.zeros((4, 1), dtype=torch.float64, device=dev)
    with pytest.raises(sl.HipEngineError, match="SL_V_POLYNOMIAL"):
        lyap._ctx.decrease_gradient(4, pts, None, grad, con)
    value = lyap.lyapunov_function
    case, dynamics, _ = PVC.gp_case("rbf")
    grid = sl.GridWorld(case["limits"], 9)
    table = sl.Triangulation(grid, np.zeros((grid.nindex, 1)), project=True)
    policy = sl.Triangulation(grid, np.zeros((grid.nindex, 1)))
    reward = sl.QuadraticFunction(-np.eye(3))
    rl = sl.PolicyIteration(policy, lyap.dynamics, reward, table, gamma=0.9)
    with pytest.raises(NotImplementedError, match="polynomial_function.*second derivatives"):
        rl.policy_gradient(x, lyapunov=lyap)
    with pytest.raises(NotImplementedError, match="polynomial_function.*value_function"):
        sl.PolicyIteration(policy, lyap.dynamics, reward, value)
    with pytest.raises(NotImplementedError, match="polynomial_function.*reward_function"):
        sl.PolicyIteration(policy, lyap.dynamics, value, table)
    with pytest.raises(NotImplementedError, match="roa_classification_step.*polynomial_function"):
        sl.roa_classification_step(lyap, x, np.ones(3), np.ones(3), 1.0, 1.0, 0.01)
