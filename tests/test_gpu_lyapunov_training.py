"""GPU tests of the LyapunovNetwork training path: sl_nn_param_grad, sl_nn_loss,
LyapunovNetwork.parameter_gradient and the two steps of safe_learning_amd/training.py against the
NumPy reference tests/np_lyapunov_training.py (whose own checks are
tests/test_lyapunov_training_host.py).

Gradients are compared as |g - g_ref| <= tol * A with the reference's error companion A and tol =
np_lyapunov_training.tolerance(network, M): 32 times the reference's own float64 error on the same
batch (float64 against long double; it is 445 x 2^-53 A at M = 1 on the four-layer network and 0.22 at
M = 70 001, see np_lyapunov_training.REFERENCE_RATIO).  Every test prints the figure it measured before
it asserts.
"""

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import cases
import guarded
import np_lyapunov_training as T

pytestmark = pytest.mark.gpu

VALUE_RTOL = 1e-12             # the project's network-value tolerance (tests/test_gpu_configs.py)


@pytest.fixture(scope="module")
def sl():
    import safe_learning_amd
    return safe_learning_amd


def _engine_network(sl, onet):
    return sl.LyapunovNetwork(onet.input_dim, onet.output_dims, onet.activations, eps=onet.eps,
                              weights=[w.copy() for w in onet.weights])


def _batch_sizes():
    """Less than a tile, the tile edge, the notebook's batch, and one size at which the grid-stride loop of
    both kernels runs (more than 2 * CUs * 128 points: 70 001 on 256 CUs)."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return [1, 15, 16, 17, 1000, 2 * cus * 128 + 4465]


def _within(got, ref, comp, tol, label):
    ratio = T.ratio_to_companion(got, ref, comp)
    print("%s: max |g - g_ref| / A = %.3f x 2^-53 (allowed %.1f)" % (label, ratio, tol * 2.0 ** 53))
    for g, r, a in zip(got, ref, comp):
        assert g.shape == r.shape
        assert np.all(np.abs(g - r) <= tol * a), label


# ---- 1. parameter_gradient ----------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(T.NETWORKS))
def test_parameter_gradient_matches_oracle(sl, key):
    import torch
    onet = T.make_network(key)
    net = _engine_network(sl, onet)
    for m in _batch_sizes():
        points, coeff = T.make_batch(key, m)
        assert (coeff == 0).any() or m == 1
        ref, comp = T.parameter_gradient(onet, points, coeff)
        got = net.parameter_gradient(points, coeff)
        assert [g.shape for g in got] == [w.shape for w in net.weights]
        _within(got, ref, comp, T.tolerance(key, m), "%s, M = %d" % (key, m))
        if m == 1000:                          # device tensors in: the same numbers
            dev = net.parameter_gradient(torch.from_numpy(points).cuda(), torch.from_numpy(coeff).cuda())
            for a, b in zip(dev, got):
                assert_array_equal(a, b)


# ---- 2. determinism, and nothing written outside the buffers ----------------------------------------------------
def test_gradient_is_deterministic_and_stays_in_bounds(sl):
    import torch
    onet = T.make_network("notebook")
    net = _engine_network(sl, onet)
    ctx = net._on_engine()
    m = _batch_sizes()[-1]
    points, coeff = T.make_batch("notebook", m)
    d_points, d_coeff = torch.from_numpy(points).cuda(), torch.from_numpy(coeff).cuda()
    total = sum(k.size for k in onet.kernels())
    runs = [guarded.run(lambda grad: ctx.nn_param_grad(m, 2, d_points, d_coeff, grad), [total])[0] for _ in range(2)]
    assert_array_equal(runs[0], runs[1])
    nbytes, intact = ctx.nn_train_scratch()
    # (the area is one slice of `total` doubles per workgroup, the guard zones lie directly around it)
    assert nbytes >= 2 * 8 * total and nbytes % (8 * total) == 0
    assert intact, "a kernel wrote outside the scratch area"
    G = T.kernel_gradient(onet, points, coeff)[0]
    assert_allclose(runs[0].view(np.float64), np.concatenate([g.ravel() for g in G]), rtol=1e-9, atol=1e-9)
    a = net.parameter_gradient(points, coeff)
    b = net.parameter_gradient(points, coeff)
    for x, y in zip(a, b):
        assert_array_equal(x.view(np.uint64), y.view(np.uint64))


# ---- 3. sl_nn_loss ---------------------------------------------------------------------------------------------
def _loss_on_engine(sl, net, kind, batch):
    """-> losses [3], coefficients, points of one sl_nn_loss call on the reference's successors."""
    import torch
    from safe_learning_amd import _hip
    ctx = net._on_engine()
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in batch.items()}
    m, d = batch["states"].shape
    losses = torch.empty(3, dtype=torch.float64, device="cuda")
    if kind == "abs":
        coeff = torch.empty(m, dtype=torch.float64, device="cuda")
        points = torch.empty((m, d), dtype=torch.float64, device="cuda")
        ctx.nn_loss(_hip.NN_LOSS_ABS, m, d, dev["states"], None, dev["targets"], None, 0., 0., 0., losses, coeff,
                    points)
    else:
        coeff = torch.empty(2 * m, dtype=torch.float64, device="cuda")
        points = torch.empty((2 * m, d), dtype=torch.float64, device="cuda")
        ctx.nn_loss(_hip.NN_LOSS_ROA, m, d, dev["states"], dev["successors"], dev["labels"], dev["weights"],
                    T.SAFE_LEVEL, T.LAGRANGE, T.EPS, losses, coeff, points)
    return losses.cpu().numpy(), coeff.cpu().numpy(), points.cpu().numpy()


def _mean_atol(onet, batch, terms):
    """What a relative error VALUE_RTOL of V(x) and V(x+) can move the three means by: the hinge by
    w * rtol * V, the decrease term by l * rtol * (V + V+) / (V + eps)."""
    v, vn = T.values(onet, batch["states"]), T.values(onet, batch["successors"])
    cls = VALUE_RTOL * float(np.mean(batch["weights"] * v))
    dec = VALUE_RTOL * float(np.mean(batch["labels"] * (v + vn) / (v + T.EPS)))
    return np.array([cls + T.LAGRANGE * dec, cls, dec])


def _check_roa_loss(onet, batch, losses, coeff, label):
    m = len(batch["states"])
    means, terms, _ = T.roa_classification_step(onet, batch["states"], batch["successors"], batch["labels"],
                                                batch["weights"], T.SAFE_LEVEL, T.LAGRANGE, None, T.EPS)
    ref = np.array([means["objective"], means["classifier_loss"], means["decrease_loss"]])
    print("%s: losses %s, reference %s" % (label, losses, ref))
    assert np.all(np.abs(losses - ref) <= VALUE_RTOL * np.abs(ref) + _mean_atol(onet, batch, terms))
    skip = T.undecided(terms, "roa")
    assert skip.mean() <= 0.01
    ok = ~skip
    cx, cn = coeff[:m], coeff[m:]
    labelled = batch["labels"] > 0
    assert_array_equal((cn != 0)[ok & labelled], terms["dec_on"][ok & labelled])
    assert not np.any(cn[~labelled])
    assert_array_equal(((cx + cn) != 0)[ok], terms["hinge_on"][ok])
    assert_allclose(cx[ok], terms["coeff_x"][ok], rtol=VALUE_RTOL, atol=0)
    assert_allclose(cn[ok], terms["coeff_next"][ok], rtol=VALUE_RTOL, atol=0)
    print("%s: %d of %d samples left out, %d active hinges, %d active decrease terms"
          % (label, skip.sum(), m, terms["hinge_on"].sum(), (terms["dec_on"] & labelled).sum()))


def _check_abs_loss(onet, batch, losses, coeff, label):
    objective, terms, _ = T.pretraining_step(onet, batch["states"], batch["targets"], None)
    print("%s: objective %.17g, reference %.17g" % (label, losses[0], objective))
    atol = VALUE_RTOL * float(np.mean(T.values(onet, batch["states"])))
    assert abs(losses[0] - objective) <= VALUE_RTOL * objective + atol
    assert losses[1] == losses[0] and losses[2] == 0.0
    ok = ~T.undecided(terms, "abs")
    assert ok.mean() >= 0.99
    assert_array_equal(coeff[ok], terms["coeff_x"][ok])               # +-1 / m or 0: exact


@pytest.mark.parametrize("kind", ["pendulum", "linear"])
def test_loss_kernel_matches_oracle(sl, kind):
    case = T.training_case(kind)
    batch = T.training_batch(case)
    onet = T.oracle_network(case)
    net = _engine_network(sl, onet)
    m = len(batch["states"])
    # SL_NN_LOSS_ROA
    losses, coeff, points = _loss_on_engine(sl, net, "roa", batch)
    assert_array_equal(points, np.vstack((batch["states"], batch["successors"])))
    _check_roa_loss(onet, batch, losses, coeff, "%s, ROA" % kind)
    # SL_NN_LOSS_ABS
    losses, coeff, points = _loss_on_engine(sl, net, "abs", batch)
    assert_array_equal(points, batch["states"])
    _check_abs_loss(onet, batch, losses, coeff, "%s, ABS" % kind)
    # the successors the engine computes itself, through the public step without an update
    from safe_learning_amd.benchmarks import build_lyapunov
    lyap = build_lyapunov(case)
    got = sl.roa_classification_step(lyap, batch["states"], batch["labels"], batch["weights"], T.SAFE_LEVEL,
                                     T.LAGRANGE, None, eps=T.EPS)
    means, terms, _ = T.roa_classification_step(onet, batch["states"], batch["successors"], batch["labels"],
                                                batch["weights"], T.SAFE_LEVEL, T.LAGRANGE, None, T.EPS)
    atol = _mean_atol(onet, batch, terms)
    for k, name in enumerate(("objective", "classifier_loss", "decrease_loss")):
        print("%s, step without update: %s %.17g, reference %.17g" % (kind, name, got[name], means[name]))
        # (successors that differ in the last place move V(x+) like a value error does: twice the room)
        assert abs(got[name] - means[name]) <= VALUE_RTOL * abs(means[name]) + 2 * atol[k]
    for w, w0 in zip(lyap.lyapunov_function.weights, case["V"]["weights"]):
        assert_array_equal(w, w0)                                     # learning_rate=None: no update


# ---- 4. five steps of each kind, each from the oracle's weights ----------------------------------------------------
def _check_step(got_weights, onet, comps, lr, key, step):
    """new weights within lr * tol * A of the oracle's, tol from the reference's own error at this step."""
    tol = T.tolerance(key, step)
    label = "%s, step %d" % (key, step)
    worst = 0.0
    for w, ow, a in zip(got_weights, onet.weights, comps):
        bound = lr * tol * a
        diff = np.abs(w - ow)
        # (the subtraction w - lr g rounds once more, in both: half an ulp of w on either side)
        slack = np.spacing(np.abs(ow))
        assert np.all(diff <= bound + slack), label
        if (a > 0).any():
            worst = max(worst, float((diff[a > 0] / (lr * a[a > 0])).max()) * 2.0 ** 53)
    print("%s: max |w - w_ref| / (lr A) = %.3f x 2^-53 (allowed %.1f)" % (label, worst, tol * 2.0 ** 53))


def test_five_steps_of_each_kind(sl):
    from safe_learning_amd.benchmarks import build_lyapunov
    import oracle
    case = T.training_case("pendulum")
    batch = T.training_batch(case)
    lyap = build_lyapunov(case)
    net = lyap.lyapunov_function
    # pre-training
    onet, lr = T.oracle_network(case), T.STEP_LR["steps-pre"]
    for step in range(T.NUM_STEPS):
        net.weights = [w.copy() for w in onet.weights]
        got = sl.pretraining_step(net, batch["states"], batch["targets"], lr)
        objective, terms, comps = T.pretraining_step(onet, batch["states"], batch["targets"], lr)
        atol = VALUE_RTOL * float(np.mean(terms["classifier"] + batch["targets"]))
        assert abs(got - objective) <= VALUE_RTOL * objective + atol
        _check_step(net.weights, onet, comps, lr, "steps-pre", step)
    # region-of-attraction classification
    onet, lr = T.oracle_network(case), T.STEP_LR["steps-roa"]
    for step in range(T.NUM_STEPS):
        net.weights = [w.copy() for w in onet.weights]
        got = sl.roa_classification_step(lyap, batch["states"], batch["labels"], batch["weights"], T.SAFE_LEVEL,
                                         T.LAGRANGE, lr, eps=T.EPS)
        before = T.oracle_network(case)
        before.weights = [w.copy() for w in onet.weights]
        means, terms, comps = T.roa_classification_step(onet, batch["states"], batch["successors"], batch["labels"],
                                                        batch["weights"], T.SAFE_LEVEL, T.LAGRANGE, lr, T.EPS)
        atol = _mean_atol(before, batch, terms)
        for k, name in enumerate(("objective", "classifier_loss", "decrease_loss")):
            assert abs(got[name] - means[name]) <= VALUE_RTOL * abs(means[name]) + 2 * atol[k], (step, name)
        _check_step(net.weights, onet, comps, lr, "steps-roa", step)
    # the sweeps see the new weights
    final = [w.copy() for w in net.weights]
    lyap.update_values()
    case2 = dict(case)
    case2["V"] = dict(case["V"], weights=final)
    olyap = cases.oracle_lyapunov(case2)
    assert_allclose(lyap.values, olyap.values, rtol=VALUE_RTOL, atol=1e-18)
    assert not np.array_equal(final[0], case["V"]["weights"][0])
    lyap.update_safe_set()
    olyap.update_safe_set()
    print("safe set after the steps: %d cells (initial set %d), oracle %d"
          % (lyap.safe_set.sum(), np.count_nonzero(cases.initial_safe_mask(case)), olyap.safe_set.sum()))
    assert_array_equal(lyap.safe_set, olyap.safe_set)
    assert olyap.safe_set.sum() > np.count_nonzero(cases.initial_safe_mask(case))
    pts = batch["states"][::7]
    assert_allclose(np.ravel(net(pts)), T.values(olyap.lyapunov_function, pts), rtol=VALUE_RTOL, atol=1e-18)


# ---- 5. errors ---------------------------------------------------------------------------------------------------
def test_errors(sl, monkeypatch):
    import torch
    from safe_learning_amd import _hip
    onet = T.make_network("one-layer")
    net = _engine_network(sl, onet)
    points, coeff = T.make_batch("one-layer", 16)
    d_points, d_coeff = torch.from_numpy(points).cuda(), torch.from_numpy(coeff).cuda()
    out = torch.zeros(16, dtype=torch.float64, device="cuda")
    losses = torch.zeros(3, dtype=torch.float64, device="cuda")
    fresh = _hip.Context()                                           # no network uploaded
    with pytest.raises(sl.HipEngineError, match="network not set"):
        fresh.nn_param_grad(16, 4, d_points, d_coeff, out)
    with pytest.raises(sl.HipEngineError, match="network not set"):
        fresh.nn_loss(_hip.NN_LOSS_ABS, 16, 4, d_points, None, d_coeff, None, 0., 0., 0., losses, out)
    # a network of more inputs than a state has dimensions uploads, but the kernels hold 6 per point
    wide = sl.LyapunovNetwork(8, [16], ["tanh"])
    wide._upload(fresh)
    d_wide = torch.zeros((16, 8), dtype=torch.float64, device="cuda")
    with pytest.raises(sl.HipEngineError, match=r"sl_nn_param_grad: state dimension 8 outside \[1,6\]"):
        fresh.nn_param_grad(16, 8, d_wide, d_coeff, torch.zeros(16 * 8, dtype=torch.float64, device="cuda"))
    with pytest.raises(sl.HipEngineError, match=r"sl_nn_loss: state dimension 8 outside \[1,6\]"):
        fresh.nn_loss(_hip.NN_LOSS_ABS, 16, 8, d_wide, None, d_coeff, None, 0., 0., 0., losses, out)
    fresh.close()
    with pytest.raises(sl.HipEngineError, match="state dimension 8 outside"):
        wide.parameter_gradient(np.zeros((16, 8)), coeff)
    with pytest.raises(sl.HipEngineError, match="state dimension 8 outside"):
        sl.pretraining_step(wide, np.zeros((16, 8)), coeff, None)
    ctx = net._on_engine()
    with pytest.raises(sl.HipEngineError, match=r"points of 3 columns, the network takes 4"):
        ctx.nn_param_grad(16, 3, d_points, d_coeff, out)
    with pytest.raises(sl.HipEngineError, match=r"points of 2 columns, the network takes 4"):
        ctx.nn_loss(_hip.NN_LOSS_ABS, 16, 2, d_points, None, d_coeff, None, 0., 0., 0., losses, out)
    with pytest.raises(sl.HipEngineError, match="m = 0"):
        ctx.nn_param_grad(0, 4, d_points, d_coeff, out)
    with pytest.raises(sl.HipEngineError, match="m = -1"):
        ctx.nn_loss(_hip.NN_LOSS_ABS, -1, 4, d_points, None, d_coeff, None, 0., 0., 0., losses, out)
    with pytest.raises(sl.HipEngineError, match="unknown loss kind"):
        ctx.nn_loss(7, 16, 4, d_points, None, d_coeff, None, 0., 0., 0., losses, out)
    with pytest.raises(sl.HipEngineError, match="SL_NN_LOSS_ROA needs"):
        ctx.nn_loss(_hip.NN_LOSS_ROA, 16, 4, d_points, None, d_coeff, None, 0., 0., 0., losses, out)
    # the Python layer names the mismatch before the engine sees it
    with pytest.raises(ValueError, match="expects 4 inputs"):
        net.parameter_gradient(points[:, :3], coeff)
    with pytest.raises(ValueError, match="15 coefficients for 16 points"):
        net.parameter_gradient(points, coeff[:15])
    with pytest.raises(ValueError, match="15 targets for 16 states"):
        sl.pretraining_step(net, points, coeff[:15], None)
    case = T.training_case("linear")
    batch = T.training_batch(case)
    from safe_learning_amd.benchmarks import build_lyapunov
    lyap = build_lyapunov(case)
    with pytest.raises(ValueError, match="labels for 1681 states"):
        sl.roa_classification_step(lyap, batch["states"], batch["labels"][:-1], batch["weights"], 1.0, 1.0, None)
    quadratic = build_lyapunov(cases.make_case("pendulum", num_points=9, dynamics="linear"))
    with pytest.raises(TypeError, match="LyapunovNetwork"):
        sl.roa_classification_step(quadratic, batch["states"], batch["labels"], batch["weights"], 1.0, 1.0, None)
    # one process only (a second rank cannot be started here: the check is reached through the module it asks)
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    with pytest.raises(NotImplementedError, match="one GPU"):
        sl.pretraining_step(net, points, coeff, None)
    with pytest.raises(NotImplementedError, match="one GPU"):
        sl.roa_classification_step(lyap, batch["states"], batch["labels"], batch["weights"], 1.0, 1.0, None)
