"""The LyapunovNetwork kernels of sl_nn.hip against the long-double truth of tests/np_network_truth.py
(needs an MI355X): one small sweep per ``k_nn_check_mfma<layers, d>`` instantiation - the generic d = 0
flavour through each of its doors, 5 and 6 inputs (the second input slab) among them -, a sweep over a
sub-range, the device tanh in ulp, and ``sl_nn_loss`` on a 5-input and a 6-input batch.

Every sweep must NAME its instantiation.  V, the two records of every cell and the mask are held against the
truth at tolerances measured from the float64 reference's own error (np_network_truth); on top of that every
case keeps the comparison with the float64 oracle that tests/test_gpu_lyapunov.py makes.  Every measured
figure is printed before its assertion."""

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import cases
import np_lyapunov_training as T
import np_network_truth as N
from test_gpu_lyapunov import _check_masks, _compare_safe_sets, _engine_records, _oracle_all

pytestmark = pytest.mark.gpu

LONG = np.longdouble


@pytest.fixture(scope="module")
def sl():
    import safe_learning_amd
    return safe_learning_amd


def _against_oracle(lyap, olyap, values, neg, rec):
    """What test_network_lyapunov_function asserts."""
    assert_allclose(lyap.values, olyap.values, rtol=1e-12, atol=1e-15)
    ref_rec, ref_neg = _oracle_all(olyap)
    assert_allclose(rec, ref_rec, rtol=1e-8, atol=1e-13)
    flips, _ = _check_masks(neg, ref_neg, rec, ref_rec, allowed=4)
    if flips == 0 and np.array_equal(lyap.values, olyap.values):
        _compare_safe_sets(lyap, olyap, 0)


# ---- (a) one sweep per instantiation -------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", sorted(N.CASES))
def test_sweep_instantiation(sl, case_id):
    from safe_learning_amd.benchmarks import build_lyapunov
    case = N.make(case_id)
    if case["d"] > 4:
        # no other test sweeps a 5-D grid, or a 6-D one under deterministic dynamics: the quadratic V first, so
        # that a failure below belongs to the network
        quadratic = N.quadratic_case(case_id, N.QUADRATIC_TAU)
        qlyap, qolyap = build_lyapunov(quadratic), cases.oracle_lyapunov(quadratic)
        assert_array_equal(qlyap.values, qolyap.values)
        _, qneg, qrec = _engine_records(qlyap)
        ref_rec, ref_neg = _oracle_all(qolyap)
        assert_allclose(qrec, ref_rec, rtol=1e-12, atol=1e-15)
        _check_masks(qneg, ref_neg, qrec, ref_rec, allowed=0)
        assert ref_neg.any() and not ref_neg.all()
    lyap, olyap = build_lyapunov(case), cases.oracle_lyapunov(case)
    values, neg, rec = _engine_records(lyap)
    note = lyap._ctx.last_kernel()
    print("%s: %s" % (case_id, note))
    assert N.kernel_note(case_id) in note
    assert_array_equal(values, lyap.values)
    kernels = lyap.lyapunov_function.kernels()
    for k, ok in zip(kernels, N.oracle_network(case).kernels()):
        assert_array_equal(k, ok)
    figures = N.check_against_truth(case_id, case, kernels, values, neg, rec)
    # the properties the host test established with the oracle's successors hold with the engine's too
    assert figures["undecided"] <= 0.01 * figures["cells"]
    assert 0 < figures["negative"] < figures["cells"]
    assert figures["max_abs_tanh"] <= T.MAX_TANH
    _against_oracle(lyap, olyap, values, neg, rec)


# ---- (b) a sweep over a sub-range ------------------------------------------------------------------------------
def test_sweep_over_a_sub_range(sl):
    """A shard sweeps [lo, hi) with lo != 0: values[idx - lo], the mask word (wbase - lo) >> 6 and init_bits of
    that word.  Records, mask words and the reduced key of [64, hi) and [128, hi) equal the slice of the full
    sweep bit for bit."""
    import torch
    from safe_learning_amd import _hip
    from safe_learning_amd.benchmarks import build_lyapunov
    from safe_learning_amd.lyapunov import vbits_to_float
    case = N.make(N.SUBRANGE_CASE)
    total = int(np.prod(case["num_points"]))
    hi = total - 7
    assert total >= 200 and hi % 16 != 0 and hi > 128 + 64
    # an initial set with bits all over the range (the case's own disc lies below cell 128)
    case["initial_set"] = np.random.default_rng(7).uniform(size=total) < 0.3
    lyap = build_lyapunov(case)
    d = case["d"]
    values, neg, rec = _engine_records(lyap)
    assert N.kernel_note(N.SUBRANGE_CASE) in lyap._ctx.last_kernel()
    init = case["initial_set"]
    words = lyap._d_neg.cpu().numpy().view(np.uint64)
    init_words = lyap._d_init.cpu().numpy().view(np.uint64)
    assert_array_equal(np.unpackbits(init_words.view(np.uint8), bitorder="little")[:total].astype(bool), init)

    def key_of(result):
        result = result.cpu().numpy().view(np.uint64)
        return int(result[_hip.R_FAIL_V]), int(result[_hip.R_FAIL_I].view(np.int64))

    def expected_key(lo, hi):
        open_cells = np.flatnonzero(~(neg[lo:hi] | init[lo:hi])) + lo
        assert len(open_cells) > 0
        best = open_cells[np.lexsort((open_cells, values[open_cells]))[0]]
        return float(values[best]), int(best)

    vbits, index = key_of(lyap._d_result)
    assert (vbits_to_float(vbits), index) == expected_key(0, total)
    dev = lyap._ctx.torch_device
    for lo in (64, 128):
        n, nwords = hi - lo, -(-(hi - lo) // 64)
        assert init[lo:hi].any() and not init[lo:hi].all()
        d_init = lyap._d_init[lo >> 6:(lo >> 6) + nwords].clone()
        d_values = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
        lyap._ctx.values(lo, hi, d_values)
        d_neg = torch.zeros(nwords, dtype=torch.int64, device=dev)
        d_result = torch.zeros(_hip.RESULT_WORDS, dtype=torch.int64, device=dev)
        dbg = torch.full((n, 2 + 2 * d), float("nan"), dtype=torch.float64, device=dev)
        lyap._ctx.lyap_sweep(lo, hi, d_init, d_values, d_neg, d_result, dbg)
        assert N.kernel_note(N.SUBRANGE_CASE) in lyap._ctx.last_kernel()
        assert_array_equal(d_values.cpu().numpy().view(np.uint64), values[lo:hi].view(np.uint64))
        assert_array_equal(dbg.cpu().numpy().view(np.uint64), rec[lo:hi].view(np.uint64))
        # the words of the full sweep from word lo / 64 on, the last one cut at hi
        expect = words[lo >> 6:(lo >> 6) + nwords].copy()
        if n % 64:
            expect[-1] &= np.uint64((1 << (n % 64)) - 1)
        assert_array_equal(d_neg.cpu().numpy().view(np.uint64), expect)
        vbits, index = key_of(d_result)
        print("[%d, %d): reduced key (%r, %d)" % (lo, hi, vbits_to_float(vbits), index))
        assert (vbits_to_float(vbits), index) == expected_key(lo, hi)
        assert lo <= index < hi


# ---- (c) the device tanh in ulp --------------------------------------------------------------------------------
TANH_SEGMENTS = [(1e-300, 1e-290), (1e-12, 1e-7), (1e-7, 1e-3), (1e-3, 0.17), (0.17, 0.18), (0.18, 0.52), (0.52, 0.53),
                 (0.53, 2.0), (2.0, 10.0), (10.0, 19.1), (19.1, 40.1), (40.0, 1e300)]
TANH_ULPS = 4.0                 # sl_model.h: "within 4 ulp of the library routine", read against the truth


def _neighbours(x, count=4):
    below, above = [x], [np.nextafter(x, np.inf)]
    for _ in range(count - 1):
        below.append(np.nextafter(below[-1], -np.inf))
        above.append(np.nextafter(above[-1], np.inf))
    return below + above


def test_device_tanh_in_ulp(sl):
    """sl_tanh (sl_model.h) through a policy network of one unit with the weight 1 and no bias: k_policy_network
    computes fma(x, 1, 0), sl_tanh of it and the product with the output scale 1 - the routine's value bit for
    bit.  (-0 does not reach the routine this way, nor any other: every accumulator starts at +0 and
    -0 * 1 + 0 = +0.  Its output is asserted to be +0.)"""
    from safe_learning_amd import _evaluate
    net = sl.NeuralNetwork([1], ["tanh"], output_scale=1.0, use_bias=False, input_dim=1,
                           parameters=[np.array([[1.0]])])
    rng = np.random.default_rng(11)
    per_segment = 12000
    pieces, labels = [], []
    for lo, hi in TANH_SEGMENTS:
        pieces.append(np.exp(rng.uniform(np.log(lo), np.log(hi), per_segment)))
        labels.append("[%g, %g]" % (lo, hi))
    switches = [(j + 0.5) * np.log(2.0) / 2 for j in range(6)] + [40.0]
    pieces.append(np.array([v for s in switches for v in _neighbours(s)]))
    labels.append("around the switches of k and 40")
    denormal = np.array([5e-324, 1e-310, 2.0 ** -1022])
    pieces.append(denormal)
    labels.append("denormal points")
    x = np.concatenate(pieces)
    owner = np.concatenate([np.full(len(p), k) for k, p in enumerate(pieces)])
    assert 2e5 <= 2 * len(x) <= 5e5
    pos = _evaluate.policy(net, x[:, None])[:, 0]
    neg = _evaluate.policy(net, -x[:, None])[:, 0]
    truth = np.tanh(x.astype(LONG))
    errors = N.ulp_error(pos, truth)
    for k, label in enumerate(labels):
        print("tanh %-32s largest error %.3f ulp (%d points)" % (label, errors[owner == k].max(), (owner == k).sum()))
    worst = int(np.argmax(errors))
    print("tanh: largest error %.3f ulp at x = %r" % (errors[worst], x[worst]))
    assert errors.max() <= TANH_ULPS
    assert_array_equal(neg.view(np.uint64), (-pos).view(np.uint64))          # odd, bit for bit
    assert np.all(np.abs(pos) <= 1.0)
    assert np.all(pos[x >= 19.1] == 1.0) and np.all(neg[x >= 19.1] == -1.0)
    assert_array_equal(pos[owner == len(pieces) - 1], denormal)               # exactly x
    # zeros and non-finite points (the entry point takes them as they are)
    special = _evaluate.policy(net, np.array([[0.0], [-0.0], [np.inf], [-np.inf], [np.nan]]))[:, 0]
    assert_array_equal(special[:4], [0.0, 0.0, 1.0, -1.0])
    assert not np.signbit(special[0]) and not np.signbit(special[1])
    assert np.isnan(special[4])


# ---- the loss kernel on 5- and 6-input batches -------------------------------------------------------------------
@pytest.mark.parametrize("key,layers,inputs", [("five-inputs", 2, 5), ("six-inputs", 3, 6)])
def test_loss_kernel_with_five_and_six_inputs(sl, key, layers, inputs):
    """k_nn_loss<2> and k_nn_loss<3> with both input slabs in use, both kinds, checked as
    test_loss_kernel_matches_oracle checks them (the training kernels set no kernel note: the instantiation follows
    from the network's layer count, sl_with_dim<1, 2, 3, 4>(nlayers))."""
    from test_gpu_lyapunov_training import _check_abs_loss, _check_roa_loss, _engine_network, _loss_on_engine
    onet = T.make_network(key)
    assert onet.input_dim == inputs and onet.num_layers == layers
    net = _engine_network(sl, onet)
    batch = T.wide_input_batch(onet)
    losses, coeff, points = _loss_on_engine(sl, net, "roa", batch)
    assert_array_equal(points, np.vstack((batch["states"], batch["successors"])))
    _check_roa_loss(onet, batch, losses, coeff, "%s, ROA" % key)
    losses, coeff, points = _loss_on_engine(sl, net, "abs", batch)
    assert_array_equal(points, batch["states"])
    _check_abs_loss(onet, batch, losses, coeff, "%s, ABS" % key)
