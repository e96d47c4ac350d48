"""CPU checks of tests/np_network_truth.py, the long-double reference of the LyapunovNetwork kernels, and of
the cases of tests/test_gpu_network_matrix.py - with the float64 oracle standing in for the device.

Per case: the recorded reference ratios bound a re-measurement, at most 1 % of the cells are undecided, both
mask classes occur, no tanh output exceeds np_lyapunov_training.MAX_TANH, and the float64 records pass the
comparison the GPU test makes.  Once: the ledger names every instantiation sl_nn_check_launch compiles, the
oracle's network equals the float64 chain bit for bit, ulp_error measures what it says, and the components case
would see two exchanged gradient components.
"""

import os
import re

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import cases
import np_lyapunov_training as T
import np_network_truth as N

LONG = np.longdouble
EXTENDED = np.finfo(LONG).eps < 1e-18          # (no extended precision: nothing to measure)
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "safe_learning_amd", "csrc")


def _oracle_sweep(case):
    olyap = cases.oracle_lyapunov(case)
    idx = np.arange(olyap.discretization.nindex)
    rec = cases.oracle_cell_records(olyap, idx)
    neg = olyap.negative(olyap.discretization.index_to_state(idx))
    return olyap, np.ravel(olyap.values), neg, rec


@pytest.mark.parametrize("case_id", sorted(N.CASES))
def test_case_is_well_posed_and_its_ratios_hold(case_id):
    case = N.make(case_id)
    spec = N.CASES[case_id]
    assert case["d"] == len(spec["grid"]) and int(np.prod(spec["grid"])) <= 450
    assert (case["tau"] > 0) == (spec["tau"] > 0)
    ratio_v, ratio_g = N.measure_reference_ratio(case_id, case)
    print("%s: float64 vs long double, V %.3f and grad V %.3f x 2^-53" % (case_id, ratio_v, ratio_g))
    if EXTENDED:
        for got, recorded in zip((ratio_v, ratio_g), N.REFERENCE_RATIO[case_id]):
            assert 0.25 * recorded <= got <= recorded
    tol_v, tol_g = N.tolerances(case_id)
    assert tol_v <= N.VALUE_RTOL
    olyap, values, neg, rec = _oracle_sweep(case)
    onet = N.oracle_network(case)
    figures = N.check_against_truth(case_id, case, onet.kernels(), values, neg, rec)
    assert figures["undecided"] <= 0.01 * figures["cells"]
    assert 0 < figures["negative"] < figures["cells"]
    assert figures["max_abs_tanh"] <= T.MAX_TANH
    if case["tau"] > 0:                              # thresholds are not denormal
        thr = np.abs(figures["truth"]["threshold"])
        assert np.all(thr[~figures["truth"]["exact"]] > 1e-12)
    if N.is_uncertain(case):                         # the gradient of V(next) counts
        assert np.all(rec[:, 2 + case["d"]:] > 0)


@pytest.mark.parametrize("case_id", ["linear5", "linear6"])
def test_quadratic_pre_sweep_has_both_classes(case_id):
    """The 5-D and 6-D grids are swept with the quadratic V first: a stable closed loop, cells of both classes."""
    case = N.quadratic_case(case_id, N.QUADRATIC_TAU)
    closed = case["A_true"] + case["B_true"] @ case["K"]
    assert np.abs(np.linalg.eigvals(closed)).max() < 0.95
    olyap = cases.oracle_lyapunov(case)
    idx = np.arange(olyap.discretization.nindex)
    neg = olyap.negative(olyap.discretization.index_to_state(idx))
    print("%s: %d of %d cells negative with the quadratic V" % (case_id, neg.sum(), len(neg)))
    assert 10 <= neg.sum() <= len(neg) - 10


def test_ledger_names_every_compiled_instantiation():
    source = open(os.path.join(CSRC, "sl_nn.hip")).read()
    launch = source[source.index("int sl_nn_check_launch"):source.index("// ---- training")]
    lists = re.findall(r"sl_with_dim<([0-9, ]+)>", launch)
    assert lists == ["2, 4, 0", "1, 2, 3, 4"]
    compiled = {(nl, d) for nl in (1, 2, 3, 4) for d in (2, 4, 0)}
    assert {(c["layers"], c["inst_d"]) for c in N.CASES.values()} == compiled
    assert 'k_nn_check_mfma<layers=%d, d=%d>' in launch
    variant = open(os.path.join(CSRC, "sl_common.h")).read()
    assert "if (M.m.policy.m == 1 && M.m.grid.d >= 1 && M.m.grid.d <= 4) return M.m.grid.d;\n    return 0;" in variant
    for case_id, spec in N.CASES.items():
        case = N.quadratic_case(case_id)
        d, m = case["d"], case["m"]
        note_d = d if (m == 1 and 1 <= d <= 4) else 0
        assert spec["note_d"] == note_d and spec["inst_d"] == (note_d if note_d in (2, 4) else 0), case_id
        assert spec["layers"] == len(spec["dims"]) == len(spec["acts"])
    # every door of the generic flavour, the second input slab partly filled and full
    doors = {(N.quadratic_case(c)["d"], N.quadratic_case(c)["m"]) for c, s in N.CASES.items() if s["inst_d"] == 0}
    assert doors == {(1, 1), (3, 1), (2, 2), (5, 1), (6, 1)}
    # the training kernels: every layer count, and inputs in the second slab
    assert {len(dims) for _, dims, _ in T.NETWORKS.values()} == {1, 2, 3, 4}
    assert {5, 6} <= {d for d, _, _ in T.NETWORKS.values()}
    assert N.CASES[N.COMPONENTS_CASE]["lv"] == "abs_grad" and N.CASES[N.COMPONENTS_CASE]["kw"]["dynamics"] == "gp"
    assert int(np.prod(N.CASES[N.SUBRANGE_CASE]["grid"])) >= 200 and N.CASES[N.SUBRANGE_CASE]["layers"] == 3


@pytest.mark.parametrize("case_id", ["linear6", "two-actions", "chain3-linear"])
def test_oracle_network_equals_the_float64_chain(case_id):
    case = N.make(case_id)
    onet = N.oracle_network(case)
    points = np.vstack(N.oracle_inputs(case)[:2])
    c64 = N.chain(onet.kernels(), onet.activations, points, np.float64)
    assert_array_equal(np.ravel(onet(points)), c64["V"])
    assert_array_equal(onet.gradient(points), c64["grad"])
    assert_array_equal(T.values(onet, points), c64["V"])
    assert np.all(c64["A_g"] >= np.abs(c64["grad"]))
    assert c64["max_abs_tanh"] == T.max_abs_tanh(onet, points)


def test_ulp_error():
    one = LONG(1)
    assert_array_equal(N.ulp_of(np.array([1.0, 1.5, 0.75, 0.0, 5e-324, 2.0 ** -1022, 2.0 ** -1030], dtype=LONG)),
                       np.array([2.0 ** -52, 2.0 ** -52, 2.0 ** -53, 5e-324, 5e-324, 5e-324, 5e-324], dtype=LONG))
    # just below a power of two the spacing is that of the doubles below it
    assert N.ulp_of(one - LONG(2) ** -60) == LONG(2) ** -53
    assert N.ulp_error(np.nextafter(1.0, 2.0), one)[()] == 1.0
    assert N.ulp_error(np.nextafter(1.0, 0.0), one)[()] == 0.5
    assert N.ulp_error(3 * 5e-324, LONG(5e-324))[()] == 2.0
    if EXTENDED:
        assert N.ulp_error(1.0, one + LONG(2) ** -54)[()] == 0.25


def test_components_case_sees_exchanged_gradient_components():
    """chain3-gp: abs_grad under GP dynamics weighs |g_k(next)| with err_k; with components 0 and 1 of the truth's
    gradient exchanged, the decrease of some decided cell leaves its allowance (so a kernel that permuted them
    would fail the GPU test)."""
    case_id = N.COMPONENTS_CASE
    case = N.make(case_id)
    onet = N.oracle_network(case)
    _, _, _, rec = _oracle_sweep(case)
    d = case["d"]
    tol_v, tol_g = N.tolerances(case_id)
    tr = N.truth_records(onet.kernels(), onet.activations, N.grid_points(case), rec[:, 2:2 + d], rec[:, 2 + d:],
                         "abs_grad", True, case["lf"], case["tau"], tol_v, tol_g)
    swapped = tr["next"]["grad"][:, [1, 0, 2]]
    moved = np.abs(N.decrease(tr["x"]["V"], tr["next"]["V"], swapped, rec[:, 2 + d:], "abs_grad", True)
                   - tr["decrease"])
    seen = ~tr["undecided"] & (moved > tr["allow_decrease"])
    print("exchanged components move %d of %d decided cells beyond the allowance (largest: %.3g allowances)"
          % (seen.sum(), (~tr["undecided"]).sum(), float(np.max(moved / tr["allow_decrease"]))))
    assert seen.sum() >= 0.5 * len(seen)
