"""CPU checks of the LyapunovNetwork training path (safe_learning_amd/training.py, sl_nn_param_grad,
sl_nn_loss): the NumPy reference the GPU tests compare with (tests/np_lyapunov_training.py) is itself
checked here, and so is everything of the feature that runs without a GPU.

Measured here (printed by the tests; float64 on x86-64 with glibc):

* the reference's backward pass against central finite differences of oracle.LyapunovNetwork.__call__
  at step 1e-6: |fd - g| stays below 1.7 * 2^-53 * F / h on the four networks, F = sum_m |c_m| V(p_m)
  (the rounding error of the two function values, the truncation term h^2 f''' / 6 is 1e-12); asserted
  at 8 * 2^-53 * F / h, relative to |g| that is 4e-6 at worst;
* the reference in float64 against the same pass in np.longdouble, max |g64 - g80| / A in units of 2^-53,
  per batch size M = 1 / 15 / 16 / 17 / 1000 / 70 001:
    [64, 64, 64]      79.4 / 3.14 / 2.64 / 2.32 / 0.571 / 0.049
    [4]               1.83 / 0.408 / 0.623 / 0.811 / 0.362 / 0.028
    [5, 5, 17]        2013 / 12.5 / 59.3 / 12.9 / 5.863 / 0.693
    [16, 16, 16, 64]  445 / 23.2 / 8.97 / 8.24 / 1.355 / 0.216
    [8, 12], d = 5    13.4 / 2.51 / 6.21 / 3.14 / 1.068 / 0.148
    [18, 40, 64], 6   72.6 / 7.29 / 6.76 / 6.33 / 1.638 / 0.250
  (A does not carry the forward pass's rounding where a pre-activation cancels, so a few points are far from
  long double in units of A; over M points A grows like M, the error like sqrt(M)); another summation order of
  float64 at M = 1000: 0.308, 0.278, 1.625, 1.280.  On the step tests' [16, 16, 16] network: 6.276
  (pre-training coefficients), 10.23 (ROA coefficients).
  np_lyapunov_training.REFERENCE_RATIO holds these figures rounded up; the GPU tolerance of a batch is 32 times
  its figure;
* the largest |tanh| output on those batches: 0.902 (bound 0.96).
"""

import ctypes as C
import subprocess

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import hostsim_build
import np_lyapunov_training as T


# ---- 1. the reference against finite differences ---------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(T.NETWORKS))
def test_oracle_gradient_matches_finite_differences(key):
    net = T.make_network(key)
    points, coeff = T.make_batch(key, 24)
    grads, comps = T.parameter_gradient(net, points, coeff)
    assert [g.shape for g in grads] == [w.shape for w in net.weights] == [a.shape for a in comps]
    h = 1e-6
    scale = float(np.sum(np.abs(coeff) * np.ravel(net(points))))

    def f():
        return float(np.sum(coeff * np.ravel(net(points))))

    worst = 0.0
    for w, g in zip(net.weights, grads):
        fd = np.zeros_like(w)
        for idx in np.ndindex(*w.shape):
            old = w[idx]
            w[idx] = old + h
            up = f()
            w[idx] = old - h
            down = f()
            w[idx] = old
            fd[idx] = (up - down) / (2 * h)
        worst = max(worst, float(np.abs(fd - g).max()))
    unit = 2.0 ** -53 * scale / h
    print("%s: max |fd - g| = %.3g = %.2f x 2^-53 F / h" % (key, worst, worst / unit))
    assert worst <= 8 * unit


# ---- 2. the reference's own error: the GPU tolerance ------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(T.NETWORKS))
def test_reference_error_and_tanh_range(key):
    net = T.make_network(key)
    extended = np.finfo(np.longdouble).eps < 1e-18         # (no extended precision: nothing to measure)
    # the recorded ratio of every batch of the GPU test (the 70 001-point batches of the three large networks
    # take 12 s to half a minute in long double: measured once with the same function, 0.049, 0.216 and 0.250)
    for m in (1, 15, 16, 17, 1000, 70001):
        if m == 70001 and key in ("notebook", "four-layers", "six-inputs"):
            continue
        ratio = T.measure_reference_ratio(key, m)
        print("%s, M = %d: float64 vs long double %.3f x 2^-53 of A" % (key, m, ratio))
        if extended:
            assert 0.25 * T.REFERENCE_RATIO[key, m] <= ratio <= T.REFERENCE_RATIO[key, m]
    points, coeff = T.make_batch(key, 1000)
    g64, comp = T.parameter_gradient(net, points, coeff)
    perm, _ = T.parameter_gradient(net, points, coeff, order=np.random.default_rng(5).permutation(1000))
    print("%s: permuted order %.3f (x 2^-53 of A)" % (key, T.ratio_to_companion(perm, g64, comp)))
    assert T.ratio_to_companion(perm, g64, comp) <= 32 * T.REFERENCE_RATIO[key, 1000]
    # every batch the GPU test uses keeps the amplification of a tanh error below 24
    worst = max(T.max_abs_tanh(net, T.make_batch(key, m)[0]) for m in (1, 15, 16, 17, 1000, 70001))
    print("%s: largest |tanh| output %.3f" % (key, worst))
    assert worst <= T.MAX_TANH
    # a plain relative tolerance would not do: some entries cancel
    assert all((a >= np.abs(g)).all() for g, a in zip(g64, comp))


def test_step_batches_reference_error():
    """One figure per step of the reference's descent: the weights, and with them the coefficients of the
    batch, are others at every step (measure_step_ratios also asserts the tanh bound at every step)."""
    for key in ("steps-roa", "steps-pre"):
        ratios = T.measure_step_ratios(key)
        assert len(ratios) == T.NUM_STEPS
        for step, ratio in enumerate(ratios):
            print("%s, step %d: float64 vs long double %.3f x 2^-53 of A" % (key, step, ratio))
            if np.finfo(np.longdouble).eps < 1e-18:
                assert 0.25 * T.REFERENCE_RATIO[key, step] <= ratio <= T.REFERENCE_RATIO[key, step]


# ---- 3. the per-sample arithmetic, compiled for the host ----------------------------------------------------------
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("nn_train")
    exe = hostsim_build.program("nn_train.cpp", out, hostsim_build.SHIM_FLAGS)
    assert subprocess.run([exe], stdout=subprocess.PIPE, text=True).stdout.strip() == "nn_train: ok"
    return hostsim_build.shared("nn_train.cpp", out, hostsim_build.SHIM_FLAGS)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _shim_roa(shim, v, vn, labels, weights, c, lam, eps):
    out = np.zeros((5, len(v)))
    args = [np.ascontiguousarray(a, dtype=np.float64) for a in (v, vn, labels, weights)]
    assert shim.nt_roa(C.c_int64(len(v)), *[_p(a) for a in args], C.c_double(c), C.c_double(lam), C.c_double(eps),
                       _p(out)) == 0
    return out


ROA_CASES = {
    "both-classes": dict(labels="mixed"),
    "all-inside": dict(labels="ones"),
    "all-outside": dict(labels="zeros"),
}


@pytest.mark.parametrize("key", sorted(ROA_CASES))
def test_roa_loss_arithmetic_bit_exact(shim, key):
    rng = np.random.default_rng(11)
    m = 997
    v = rng.uniform(0.0, 2.0, m)
    vn = v * rng.uniform(0.5, 1.5, m)
    labels = {"mixed": (rng.uniform(size=m) < 0.4).astype(float), "ones": np.ones(m), "zeros": np.zeros(m)}[
        ROA_CASES[key]["labels"]]
    weights = rng.uniform(0.5, 3.0, m)
    c = 1.0
    v[:8] = c                                   # a zero hinge, in both classes
    vn[8:16] = v[8:16]                          # a zero decrease
    vn[16:24] = 0.25 * v[16:24]                 # V(x+) < V(x)
    v[24] = 0.0                                 # the origin: denominator eps alone
    vn[24] = 0.0
    for lam, eps in ((1000.0, 1e-8), (0.0, 0.0), (2.5, 1e-3)):
        terms = T.roa_terms(v, vn, labels, weights, c, lam, eps if v.min() + eps > 0 else 1e-8)
        out = _shim_roa(shim, v, vn, labels, weights, c, lam, eps if v.min() + eps > 0 else 1e-8)
        for row, name in enumerate(("classifier", "decrease", "objective", "coeff_x", "coeff_next")):
            assert_array_equal(out[row].view(np.uint64), terms[name].view(np.uint64), err_msg=name)
        assert not terms["hinge_on"][:8].any() and not out[3][:8][labels[:8] == 0].any()
        assert not terms["dec_on"][8:24].any() and not out[4][8:24].any()
        if key == "both-classes":
            assert terms["hinge_on"][labels > 0].any() and terms["hinge_on"][labels == 0].any()
            assert (terms["dec_on"] & (labels > 0)).any()
            if lam > 0:
                assert (out[4] > 0).any() and (out[3] < 0).any() and (out[3] > 0).any()
        if key == "all-outside":
            assert not out[1].any() and not out[4].any()
    # the coefficients ARE the derivative of the batch mean (finite differences on decided samples)
    terms = T.roa_terms(v, vn, labels, weights, c, 2.5, 1e-3)
    h = 1e-7
    for i in (30, 31, 32, 500):
        for which, name in ((0, "coeff_x"), (1, "coeff_next")):
            def mean(delta):
                a, b = v.copy(), vn.copy()
                (a if which == 0 else b)[i] += delta
                t = T.roa_terms(a, b, labels, weights, c, 2.5, 1e-3)
                denom = v + 1e-3                                       # (the denominator is held constant)
                return float(np.mean(t["classifier"] + 2.5 * labels * np.maximum(b - a, 0) / denom))
            assert_allclose((mean(h) - mean(-h)) / (2 * h), terms[name][i], rtol=1e-6, atol=1e-9)


def test_abs_loss_arithmetic_bit_exact(shim):
    rng = np.random.default_rng(12)
    m = 501
    v = rng.uniform(0.0, 1.0, m)
    targets = rng.uniform(0.0, 1.0, m)
    targets[:5] = v[:5]                         # sign(0) = 0
    out = np.zeros((5, m))
    assert shim.nt_abs(C.c_int64(m), _p(v), _p(targets), _p(out)) == 0
    terms = T.abs_terms(v, targets)
    for row, name in enumerate(("classifier", "decrease", "objective", "coeff_x", "coeff_next")):
        assert_array_equal(out[row].view(np.uint64), terms[name].view(np.uint64), err_msg=name)
    assert not out[3][:5].any() and set(np.unique(np.sign(out[3]))) == {-1.0, 0.0, 1.0}


def test_balanced_class_weights():
    from safe_learning_amd import balanced_class_weights
    labels = np.array([1, 0, 0, 1, 0, 0, 0, 0], dtype=bool)
    weights, counts = balanced_class_weights(labels)
    assert_array_equal(counts, [6, 2])
    assert_array_equal(weights, np.where(labels, (1.0 / 2) * 8, (1.0 / 6) * 8))       # 4 and 4 / 3
    assert weights[labels].sum() == pytest.approx(weights[~labels].sum())
    weights, counts = balanced_class_weights(labels, scale_by_total=False)
    assert_array_equal(weights, np.where(labels, 0.5, 1.0 / 6))
    weights, counts = balanced_class_weights(np.array([[0.0], [1.0], [1.0]]))          # the notebook's column
    assert weights.shape == (3, 1)
    assert_array_equal(weights.ravel(), [3.0, 1.5, 1.5])
    weights, counts = balanced_class_weights(np.ones(5, dtype=bool))                   # one class absent
    assert_array_equal(counts, [0, 5])
    assert_array_equal(weights, np.ones(5))
    weights, counts = balanced_class_weights(np.zeros(4), scale_by_total=False)
    assert_array_equal(counts, [4, 0])
    assert_array_equal(weights, np.full(4, 0.25))


def test_gpu_test_batches_are_decided():
    """The batches of tests/test_gpu_lyapunov_training.py: both classes, active and inactive hinges in both,
    active decrease terms at labelled states, and at most 1 % of the samples within 1e-12 of a kink - at the
    initial weights and along the five reference steps of each kind."""
    for kind in ("pendulum", "linear"):
        case = T.training_case(kind)
        batch = T.training_batch(case)
        labels = batch["labels"] > 0
        assert 0.2 < labels.mean() < 0.8
        net = T.oracle_network(case)
        for step in range(5):
            means, terms, _ = T.roa_classification_step(net, batch["states"], batch["successors"], batch["labels"],
                                                        batch["weights"], T.SAFE_LEVEL, T.LAGRANGE, 0.01)
            skipped = T.undecided(terms, "roa").mean()
            print("%s, ROA step %d: %s, %.2f %% undecided" % (kind, step, means, 100 * skipped))
            assert skipped <= 0.01
            assert terms["hinge_on"][labels].any() and terms["hinge_on"][~labels].any()
            assert not terms["hinge_on"][labels].all() and not terms["hinge_on"][~labels].all()
            assert (terms["dec_on"] & labels).any() and (~terms["dec_on"] & labels).any()
            assert means["classifier_loss"] > 0 and means["decrease_loss"] > 0
        net = T.oracle_network(case)
        for step in range(5):
            objective, terms, _ = T.pretraining_step(net, batch["states"], batch["targets"], 0.05)
            assert T.undecided(terms, "abs").mean() <= 0.01
            assert (terms["diff"] > 0).any() and (terms["diff"] < 0).any()


@pytest.mark.parametrize("key", ["five-inputs", "six-inputs"])
def test_wide_input_batch_is_decided(key):
    """The loss batches of tests/test_gpu_network_matrix.py::test_loss_kernel_with_five_and_six_inputs: the same
    properties, more than one workgroup of k_nn_loss (128 samples each) and a last one that is not full."""
    net = T.make_network(key)
    batch = T.wide_input_batch(net)
    m = len(batch["states"])
    assert m > 128 and m % 128 and batch["states"].shape[1] == net.input_dim > 4
    labels = batch["labels"] > 0
    assert 0.2 < labels.mean() < 0.8
    means, terms, _ = T.roa_classification_step(net, batch["states"], batch["successors"], batch["labels"],
                                                batch["weights"], T.SAFE_LEVEL, T.LAGRANGE, None, T.EPS)
    print("%s: %s, %.2f %% undecided" % (key, means, 100 * T.undecided(terms, "roa").mean()))
    assert T.undecided(terms, "roa").mean() <= 0.01
    assert terms["hinge_on"][labels].any() and terms["hinge_on"][~labels].any()
    assert not terms["hinge_on"][labels].all() and not terms["hinge_on"][~labels].all()
    assert (terms["dec_on"] & labels).any() and (~terms["dec_on"] & labels).any()
    assert means["classifier_loss"] > 0 and means["decrease_loss"] > 0
    _, terms, _ = T.pretraining_step(net, batch["states"], batch["targets"], None)
    assert T.undecided(terms, "abs").mean() <= 0.01
    assert (terms["diff"] > 0).any() and (terms["diff"] < 0).any()
    points = np.vstack((batch["states"], batch["successors"]))
    assert T.max_abs_tanh(net, points) <= T.MAX_TANH


# ---- 4. the reference optimisation does something ------------------------------------------------------------------
def test_oracle_sgd_makes_progress():
    import oracle
    from oracle.np_functions import LyapunovNetwork
    grid = oracle.GridWorld([[-1., 1.]] * 2, 41).all_points
    grid = grid[np.linalg.norm(grid, axis=1) <= 0.5]
    dims, acts = [16, 16, 16], ['tanh'] * 3
    shapes = LyapunovNetwork(2, dims, acts, weights=[]).weight_shapes()
    init = np.random.default_rng(0)
    net = LyapunovNetwork(2, dims, acts, weights=[init.uniform(-1, 1, s) * np.sqrt(6. / (s[0] + s[1])) for s in shapes])

    def target(x):
        return 0.1 * np.sum(x * x, axis=1)

    rng = np.random.default_rng(0)
    history = []
    for step in range(21):
        history.append(T.pretraining_step(net, grid, target(grid), None)[0])
        batch = grid[rng.choice(len(grid), 200, replace=False)]
        T.pretraining_step(net, batch, target(batch), 0.1)
    print("test-set objective: %.4g -> %.4g after 20 steps" % (history[0], history[20]))
    assert history[20] < 0.5 * history[0]


# ---- the Python layer without a GPU -----------------------------------------------------------------------------------
class _FakeEngine(object):
    """Stands in for the context: the two calls answered by the NumPy reference."""

    def __init__(self):
        import torch
        self.torch_device, self.calls, self.net = torch.device("cpu"), [], None

    def network_set(self, dims, activations, kernels):
        self.calls.append("network_set")
        self.kernels = [np.array(k) for k in kernels]

    def nn_param_grad(self, m, d, d_points, d_coeff, d_out):
        import torch
        self.calls.append(("nn_param_grad", m, d))
        G = T.kernel_gradient(self.net, d_points.numpy(), d_coeff.numpy())[0]
        d_out.copy_(torch.from_numpy(np.concatenate([g.ravel() for g in G])))

    def nn_loss(self, kind, m, d, d_states, d_next, d_labels, d_weights, c, lam, eps, d_losses, d_coeff, d_points=None):
        import torch
        self.calls.append(("nn_loss", kind, m, d))
        terms = T.abs_terms(T.values(self.net, d_states.numpy()), d_labels.numpy())
        d_losses.copy_(torch.tensor([terms["objective"].mean(), terms["classifier"].mean(), 0.0]))
        d_coeff.copy_(torch.from_numpy(terms["coeff_x"]))


@pytest.fixture
def fake_engine(monkeypatch):
    import copy
    from safe_learning_amd import _evaluate
    from safe_learning_amd import functions as F
    from safe_learning_amd._model import ModelBuilder
    engine = _FakeEngine()
    builder = ModelBuilder(engine, None)

    def _builder(d):
        builder.grid = copy.copy(F.GridWorld([[0., 1.]] * d, 2))
        return engine, builder
    monkeypatch.setattr(_evaluate, "_builder", _builder)
    monkeypatch.setattr(_evaluate, "_ctx", lambda: engine)
    return engine


def test_python_layer_maps_kernel_gradients_to_the_variables(fake_engine):
    import safe_learning_amd as sl
    for key in sorted(T.NETWORKS):
        onet = T.make_network(key)
        fake_engine.net = onet
        net = sl.LyapunovNetwork(onet.input_dim, onet.output_dims, onet.activations, eps=onet.eps,
                                 weights=[w.copy() for w in onet.weights])
        points, coeff = T.make_batch(key, 50)
        ref, _ = T.parameter_gradient(onet, points, coeff)
        got = net.parameter_gradient(points, coeff)
        for g, r in zip(got, ref):
            assert_array_equal(g, r)
        for g, r in zip((-net).parameter_gradient(points, coeff), ref):
            assert_array_equal(g, -r)
    # a step: the objective before it, the weights after it, and the engine told about them at the next call
    onet = T.make_network("ragged")
    fake_engine.net = onet
    net = sl.LyapunovNetwork(2, onet.output_dims, onet.activations, eps=onet.eps, weights=[w.copy() for w in onet.weights])
    points, _ = T.make_batch("ragged", 40)
    targets = 0.1 * np.sum(points * points, axis=1)
    before = [w.copy() for w in net.weights]
    objective = sl.pretraining_step(net, points, targets, None)
    for w, b in zip(net.weights, before):
        assert_array_equal(w, b)
    fake_engine.calls.clear()
    assert sl.pretraining_step(net, points, targets, 0.1) == objective
    assert fake_engine.calls == [("nn_loss", 1, 40, 2), ("nn_param_grad", 40, 2)]      # (same weights: no upload)
    ref_objective, _, _ = T.pretraining_step(onet, points, targets, 0.1)
    assert objective == ref_objective
    for w, r in zip(net.weights, onet.weights):
        assert_array_equal(w, r)
    fake_engine.calls.clear()
    sl.pretraining_step(net, points, targets, None)
    assert fake_engine.calls[0] == "network_set"                                      # the edit was noticed
    for k, r in zip(fake_engine.kernels, onet.kernels()):
        assert_array_equal(k, r)


def test_package_exports():
    import safe_learning_amd as sl
    from safe_learning_amd import training
    assert sl.pretraining_step is training.pretraining_step
    assert sl.roa_classification_step is training.roa_classification_step
    assert sl.balanced_class_weights is training.balanced_class_weights
    assert hasattr(sl.LyapunovNetwork, "parameter_gradient")
