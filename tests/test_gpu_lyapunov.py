"""Parity of the HIP engine with the oracle - the tests proper (need an MI355X).

Everything goes through the C ABI (libslhip.so) via safe_learning_amd.  Bars:
 * deterministic linear / quadratic pipeline: values, per-cell records and masks bit-exact;
 * Euler dynamics (device sin/cos) and GP dynamics: records within RTOL_GP = 1e-9 relative
   (requirement: 1e-5), masks equal except cells within rounding of the threshold;
 * safe_set and c_max equal to the oracle's sequential prefix rule.
"""


import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import cases
import exclusions
import oracle

pytestmark = pytest.mark.gpu

RTOL_GP = 1e-9      # north_star asks for 1e-5 relative on V and GP mean / var


@pytest.fixture(scope="module")
def sl():
    import safe_learning_amd
    return safe_learning_amd


def _engine_records(lyap):
    """Run the sweep with the debug record buffer: values, negative mask, [dec, thr, mean, err]."""
    import torch
    d = lyap.discretization.ndim
    n = lyap._hi - lyap._lo
    dbg = torch.zeros((n, 2 + 2 * d), dtype=torch.float64, device=lyap._ctx.torch_device)
    lyap._upload_model()
    lyap._refresh_init_bits()
    lyap._ctx.lyap_sweep(lyap._lo, lyap._hi, lyap._d_init, lyap._d_values, lyap._d_neg,
                         lyap._d_result, dbg)
    bits = lyap._d_neg.cpu().numpy().view(np.uint8)
    neg = np.unpackbits(bits, bitorder="little")[:n].astype(bool)
    return lyap._d_values[:n].cpu().numpy(), neg, dbg.cpu().numpy()


def _oracle_all(olyap, chunk=20000):
    n = olyap.discretization.nindex
    recs, negs = [], []
    for s in range(0, n, chunk):
        idx = np.arange(s, min(n, s + chunk))
        recs.append(cases.oracle_cell_records(olyap, idx))
        negs.append(olyap.negative(olyap.discretization.index_to_state(idx)))
    return np.vstack(recs), np.concatenate(negs)


def _check_masks(neg, ref_neg, rec, ref_rec, allowed=2):
    differs = neg != ref_neg
    margin = np.abs(ref_rec[:, 0] - ref_rec[:, 1])
    scale = np.maximum(np.abs(ref_rec[:, 0]), np.abs(ref_rec[:, 1]))
    assert not np.any(differs & (margin > 1e-9 * np.maximum(scale, 1e-300))), \
        "negative mask differs away from the threshold"
    assert differs.sum() <= allowed
    log_mask_flips(int(differs.sum()), len(neg), float(np.min(margin / np.maximum(scale, 1e-300))))
    return int(differs.sum()), float(np.min(margin / np.maximum(scale, 1e-300)))


def log_mask_flips(flips, cells, min_margin=None, test=None):
    """GP decrease masks are compared with a margin rule (bit-exactness is required for deterministic
    dynamics only): every comparison logs how many cells flipped - they lie within 1e-9 relative of
    the threshold - so that the parity report (gpurun_out/parity_exclusions.json) shows the count
    instead of hiding it behind `<= allowed`."""
    import os
    test = test or os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0]
    entry = {"test": test, "kind": "GP mask flips within 1e-9 relative of the threshold", "points": int(cells),
             "flips": int(flips), "excluded": 0.0}
    if min_margin is not None:
        entry["smallest_relative_margin"] = float(min_margin)
    exclusions.LOG.append(entry)
    print("parity [GP mask] %s: %d of %d cells flipped" % (test, flips, cells))


def _compare_safe_sets(lyap, olyap, flips, neg=None):
    """safe_set and c_max against the oracle's sequential prefix rule.  When cells within rounding
    of the threshold flipped (``flips`` > 0) the oracle's rule is applied to the ENGINE's decrease
    mask instead of its own - the comparison is made modulo the flipped cells, never skipped."""
    lyap.update_safe_set()
    if flips and neg is not None:
        grid = olyap.discretization
        olyap.negative = lambda states: neg[grid.state_to_index(states)]
    olyap.update_safe_set()
    assert_array_equal(lyap.safe_set, olyap.safe_set)
    assert lyap.c_max == olyap.c_max or (np.isnan(lyap.c_max) and np.isnan(olyap.c_max))


# ---------------------------------------------------------------------------------------------
# the reference's own known answers through the engine
# ---------------------------------------------------------------------------------------------
def test_reference_known_answers(sl, golden):
    g = golden["lyapunov_update_safe_set"]
    for case in g["cases"]:
        grid = sl.GridWorld(g["limits"], g["num_points"])
        lyap = sl.Lyapunov(grid, sl.QuadraticFunction([[1.0]]),
                           sl.LinearSystem((np.array(g["dynamics_matrix"]),)), g["lf"], g["lv"],
                           case["tau"], sl.LinearSystem((np.array([[g["policy_gain"]]]),)),
                           initial_set=g["initial_set"])
        lyap.update_safe_set()
        assert_array_equal(lyap.safe_set, np.array(case["expected_safe_set"]))
    g = golden["lyapunov_safe_set_init"]
    grid = sl.GridWorld(g["limits"], g["num_points"])
    lyap = sl.Lyapunov(grid, sl.QuadraticFunction(np.eye(2)),
                       sl.LinearSystem((np.array(g["dynamics_matrix"]), np.zeros((2, 1)))),
                       g["lf"], g["lv"], g["tau"], sl.LinearSystem((np.zeros((1, 2)),)),
                       initial_set=g["initial_set"])
    assert_array_equal(lyap.safe_set, np.array(g["expected_safe_set"]))
    lyap0 = sl.Lyapunov(grid, sl.QuadraticFunction(np.eye(2)),
                        sl.LinearSystem((np.array(g["dynamics_matrix"]), np.zeros((2, 1)))),
                        g["lf"], g["lv"], g["tau"], sl.LinearSystem((np.zeros((1, 2)),)))
    assert not lyap0.safe_set.any()


def test_mfma_fragment_layout(sl):
    """A(16x4) B(4x16) through v_mfma_f64_16x16x4_f64 with asymmetric operands."""
    from safe_learning_amd import _hip
    ctx = _hip.Context()
    rng = np.random.default_rng(0)
    a, b = rng.normal(size=(16, 4)), rng.normal(size=(4, 16))
    assert_allclose(ctx.debug_mfma(a, b), a.dot(b), rtol=1e-14, atol=1e-14)
    eye = np.zeros((16, 4)); eye[:4, :4] = np.eye(4)
    assert_allclose(ctx.debug_mfma(eye, b)[:4], b, rtol=0, atol=0)


def test_mfma_4x4x4_block_layout(sl):
    """v_mfma_f64_4x4x4_4b_f64: four independent 4x4x4 products; block b owns lanes 4b..4b+3 of
    every row of 16 lanes (A: row i = lane % 4, k = lane // 16; B: column j = lane % 4, k = lane // 16;
    D: column j = lane % 4, row i = lane // 16).  The cbsz / abid bits do not give an A-block
    broadcast for FP64 (the result then matches none of the four block broadcasts)."""
    from safe_learning_amd import _hip
    ctx = _hip.Context()
    rng = np.random.default_rng(1)
    a, b, c = rng.normal(size=(3, 64))
    lanes = np.arange(64)
    blk, low, high = (lanes // 4) % 4, lanes % 4, lanes // 16
    ref = np.zeros(64)
    for lane in lanes:
        i, j, bk = high[lane], low[lane], blk[lane]
        acc = c[lane]
        for k in range(4):
            acc += a[i + 4 * bk + 16 * k] * b[j + 4 * bk + 16 * k]
        ref[lane] = acc
    assert_allclose(ctx.debug_mfma4(a, b, c, 0)[0], ref, rtol=1e-14, atol=1e-14)
    for abid in range(4):
        bcast = [c[l] + sum(a[high[l] + 4 * abid + 16 * k] * b[low[l] + 4 * blk[l] + 16 * k]
                            for k in range(4)) for l in lanes]
        assert not np.allclose(ctx.debug_mfma4(a, b, c, 1 + abid)[0], bcast)


# ---------------------------------------------------------------------------------------------
# deterministic dynamics
# ---------------------------------------------------------------------------------------------
DET_EXACT = [
    ("1d", dict()),
    ("1d", dict(tau_scale=0.0)),
    ("1d", dict(num_points=64)),
    ("1d", dict(num_points=65)),
    ("pendulum", dict(num_points=33, dynamics="linear", tau_scale=0.0)),
    ("pendulum", dict(num_points=[17, 40], dynamics="linear", tau_scale=0.02)),
    ("pendulum", dict(num_points=128, dynamics="linear", tau_scale=0.0)),     # power-of-two path
    ("cartpole", dict(num_points=8, dynamics="linear", tau_scale=0.0)),
    ("cartpole", dict(num_points=[5, 6, 7, 9], dynamics="linear", tau_scale=0.01)),
]


@pytest.mark.parametrize("name,kw", DET_EXACT)
def test_deterministic_bit_exact(sl, name, kw):
    from safe_learning_amd.benchmarks import build_lyapunov
    case = cases.make_case(name, **kw)
    lyap, olyap = build_lyapunov(case), cases.oracle_lyapunov(case)
    assert_array_equal(lyap.values, olyap.values)
    values, neg, rec = _engine_records(lyap)
    ref_rec, ref_neg = _oracle_all(olyap)
    assert_array_equal(values, olyap.values)
    assert_array_equal(rec, ref_rec)
    assert_array_equal(neg, ref_neg)                      # bit-exact mask (north_star)
    _compare_safe_sets(lyap, olyap, 0)


@pytest.mark.parametrize("name,kw", [
    ("pendulum", dict(num_points=100, dynamics="analytic", tau_scale=0.0)),
    ("pendulum", dict(num_points=100, dynamics="analytic", tau_scale=0.02)),
    ("cartpole", dict(num_points=12, dynamics="analytic", tau_scale=0.0)),
])
def test_euler_dynamics(sl, name, kw):
    from safe_learning_amd.benchmarks import build_lyapunov
    case = cases.make_case(name, **kw)
    lyap, olyap = build_lyapunov(case), cases.oracle_lyapunov(case)
    values, neg, rec = _engine_records(lyap)
    ref_rec, ref_neg = _oracle_all(olyap)
    assert_array_equal(values, olyap.values)
    assert_allclose(rec, ref_rec, rtol=1e-11, atol=1e-14)
    flips, _ = _check_masks(neg, ref_neg, rec, ref_rec)
    _compare_safe_sets(lyap, olyap, flips, neg)


# ---------------------------------------------------------------------------------------------
# GP dynamics (FP64 MFMA kernel), every kernel configuration
# ---------------------------------------------------------------------------------------------
from gp_cases import GP_CASES          # non-degenerate by construction, see tests/gp_cases.py


def _assert_non_degenerate(case, ref_neg, olyap, min_growth):
    """The workload must exercise both outcomes of the decrease check and grow the level set -
    otherwise mask parity is vacuous (an all-False mask compares equal to anything that writes
    zeros)."""
    init = np.zeros(len(ref_neg), dtype=bool)
    init[cases.initial_safe_mask(case)] = True
    assert ref_neg.any() and (~ref_neg).any(), "degenerate workload: one class only"
    grown = int((olyap.safe_set & ~init).sum())
    assert grown >= min_growth, "safe set grew by %d cells only" % grown
    return grown


@pytest.mark.parametrize("name,kw,cfg,min_growth", GP_CASES)
def test_gp_dynamics(sl, name, kw, cfg, min_growth, monkeypatch):
    from safe_learning_amd.benchmarks import build_lyapunov
    if cfg is None:
        monkeypatch.delenv("SL_GP_CFG", raising=False)
    else:
        monkeypatch.setenv("SL_GP_CFG", cfg)
    case = cases.make_case(name, **kw)
    lyap, olyap = build_lyapunov(case), cases.oracle_lyapunov(case)
    values, neg, rec = _engine_records(lyap)
    ref_rec, ref_neg = _oracle_all(olyap)
    d = case["d"]
    assert_array_equal(values, olyap.values)
    # states are O(1): 1e-12 absolute is 1e-12 of the state scale (2000-term dot products)
    assert_allclose(rec[:, 2:2 + d], ref_rec[:, 2:2 + d], rtol=RTOL_GP, atol=1e-12)   # mean
    assert_allclose(rec[:, 2 + d:], ref_rec[:, 2 + d:], rtol=1e-7, atol=1e-12)        # beta*sigma
    var, ref_var = (rec[:, 2 + d:] / 2.0) ** 2, (ref_rec[:, 2 + d:] / 2.0) ** 2
    assert_allclose(var, ref_var, rtol=1e-6, atol=1e-16)                              # variance
    assert_allclose(rec[:, :2], ref_rec[:, :2], rtol=1e-7, atol=1e-12)
    flips, _ = _check_masks(neg, ref_neg, rec, ref_rec)
    _compare_safe_sets(lyap, olyap, flips, neg)
    _assert_non_degenerate(case, ref_neg, olyap, min_growth)
    if flips == 0:
        # the level set the engine produced really is larger than the initial set
        init = np.zeros(len(neg), dtype=bool)
        init[cases.initial_safe_mask(case)] = True
        assert int((lyap.safe_set & ~init).sum()) >= min_growth
        assert neg[lyap.safe_set & ~init].all()


@pytest.mark.parametrize("name,kw", [
    ("cartpole", dict(num_points=12, n_gp=300, tau_scale=0.0, stack=False)),
    ("cartpole", dict(num_points=11, n_gp=120, tau_scale=0.0, stack=True)),
    ("pendulum", dict(num_points=48, n_gp=300, tau_scale=0.01)),
])
def test_gp_can_shrink_false_and_batches(sl, name, kw, small_batches):
    """The batch-granular quirks of lyapunov.py:507-510, 585-587 under GP dynamics: scattered
    previously-safe cells, a stricter threshold, then a looser one."""
    from gp_cases import INFORMED, TIGHT
    from safe_learning_amd.benchmarks import build_lyapunov
    case = cases.make_case(name, **dict(kw, **(TIGHT if name == "cartpole" else INFORMED)))
    lyap, olyap = build_lyapunov(case), cases.oracle_lyapunov(case)
    _, neg, rec = _engine_records(lyap)
    ref_rec, ref_neg = _oracle_all(olyap)
    flips, _ = _check_masks(neg, ref_neg, rec, ref_rec)
    assert flips == 0
    rng = np.random.default_rng(3)
    sizes = []
    for step in range(4):
        if step == 1:
            extra = rng.choice(lyap.discretization.nindex, 300, replace=False)
            lyap.safe_set[extra] = True
            olyap.safe_set[extra] = True
        if step == 2:        # more conservative confidence scaling: nothing may be removed
            lyap.tau = olyap.tau = case["tau"] + 2e-4
        if step == 3:
            lyap.tau = olyap.tau = case["tau"]
        lyap.update_safe_set(can_shrink=(step == 0))
        olyap.update_safe_set(can_shrink=(step == 0))
        assert_array_equal(lyap.safe_set, olyap.safe_set)
        assert lyap.c_max == olyap.c_max
        sizes.append(int(olyap.safe_set.sum()))
    init = int(np.count_nonzero(cases.initial_safe_mask(case)))
    assert sizes[0] >= init + 100 and sizes[1] >= sizes[0] and sizes[2] >= sizes[1]


def test_gp_ties_in_values(sl, small_batches):
    """Equal-valued cells under GP dynamics.  A quadratic V on a symmetric grid is bit-identical
    at x and -x while the GP (random training inputs) is not symmetric: here the smaller-index
    twin of the first failing value passes the check and the larger-index one fails, so the
    prefix is cut INSIDE a run of equal values - the (V, flat index) order decides the mask."""
    from gp_cases import TIGHT
    from safe_learning_amd.benchmarks import build_lyapunov
    case = cases.make_case("cartpole", num_points=9, n_gp=150, tau_scale=0.0, seed=0, **TIGHT)
    lyap, olyap = build_lyapunov(case), cases.oracle_lyapunov(case)
    _, neg, rec = _engine_records(lyap)
    ref_rec, ref_neg = _oracle_all(olyap)
    flips, _ = _check_masks(neg, ref_neg, rec, ref_rec)
    assert flips == 0 and ref_neg.any() and (~ref_neg).any()
    init = np.zeros(len(neg), dtype=bool)
    init[cases.initial_safe_mask(case)] = True
    ok = ref_neg | init
    order = np.argsort(olyap.values, kind="stable")
    v_star = olyap.values[order[np.argmin(ok[order])]]           # value of the first failing cell
    run = olyap.values == v_star
    for shrink in (True, False):
        lyap.update_safe_set(can_shrink=shrink); olyap.update_safe_set(can_shrink=shrink)
        assert_array_equal(lyap.safe_set, olyap.safe_set)
        assert lyap.c_max == olyap.c_max
    assert run.sum() >= 2 and olyap.safe_set[run].any() and not olyap.safe_set[run].all()
    assert olyap.safe_set.sum() >= init.sum() + 100


# ---------------------------------------------------------------------------------------------
# network / table Lyapunov functions with gradient-based L_v (configs C3 and the NIPS-17 loop)
# ---------------------------------------------------------------------------------------------
def _network_case(name, lv_kind, dims=None, acts=None, **kw):
    from safe_learning_amd.benchmarks import network_weights
    case = cases.make_case(name, **kw)
    if dims is None:
        dims = [8, 8, 12] if case["d"] == 2 else [6, 8]
    acts = ["tanh"] * len(dims) if acts is None else acts
    case["V"] = {"kind": "network", "layer_dims": dims, "activations": acts,
                 "eps": 1e-8, "weights": network_weights(case["d"], dims, seed=1)}
    case["lv"] = (lv_kind,)
    return case


@pytest.mark.parametrize("name,lv_kind,kw", [
    ("pendulum", "norm_grad", dict(num_points=40, dynamics="analytic", tau_scale=0.0)),
    ("pendulum", "norm_grad", dict(num_points=40, dynamics="analytic", tau_scale=0.01)),
    ("pendulum", "abs_grad", dict(num_points=32, n_gp=100, tau_scale=0.0)),
    ("cartpole", "norm_grad", dict(num_points=6, dynamics="linear", tau_scale=0.0)),
    # several 16-wide feature blocks per layer, widths that are not multiples of 4 or 16
    ("pendulum", "norm_grad", dict(num_points=24, n_gp=60, tau_scale=0.0, dims=[20, 33, 64])),
    ("pendulum", "abs_grad", dict(num_points=30, dynamics="analytic", tau_scale=0.01, dims=[64])),
    ("pendulum", "norm_grad", dict(num_points=30, dynamics="linear", tau_scale=0.0, dims=[18, 40],
                                   acts=["relu", "tanh"])),
    ("cartpole", "abs_grad", dict(num_points=5, n_gp=80, tau_scale=0.0, dims=[16, 17, 40, 64],
                                  acts=["tanh", "relu", "tanh", "tanh"])),
])
def test_network_lyapunov_function(sl, name, lv_kind, kw):
    """LyapunovNetwork V with L_v from its input gradient (lyapunov_function_learning.ipynb c.19)."""
    from safe_learning_amd.benchmarks import build_lyapunov
    case = _network_case(name, lv_kind, **kw)
    lyap, olyap = build_lyapunov(case), cases.oracle_lyapunov(case)
    assert_allclose(lyap.values, olyap.values, rtol=1e-12, atol=1e-15)        # V within 1e-5 req.
    values, neg, rec = _engine_records(lyap)
    ref_rec, ref_neg = _oracle_all(olyap)
    assert_allclose(rec, ref_rec, rtol=1e-8, atol=1e-13)
    flips, _ = _check_masks(neg, ref_neg, rec, ref_rec, allowed=4)
    if flips == 0 and np.array_equal(lyap.values, olyap.values):
        _compare_safe_sets(lyap, olyap, 0)


@pytest.mark.parametrize("kw", [
    dict(num_points=60, dynamics="analytic", tau_scale=0.0),
    dict(num_points=48, n_gp=150, tau_scale=0.0, signal_std=0.001, noise_std=0.0002, lengthscale=1.0),
])
def test_network_level_set_grows(sl, kw):
    """A LyapunovNetwork that is a Lyapunov candidate (V ~ x^T P x near the origin, tanh layers,
    L_v from its input gradient): the level set grows by more than 1000 cells and the safe set,
    c_max and masks equal the oracle's - a randomly initialised network (config C3) cannot show
    this, its sublevel sets are not invariant."""
    from safe_learning_amd.benchmarks import build_lyapunov
    case = cases.make_case("pendulum", **kw)
    dims = [16, 16, 24]
    case["V"] = {"kind": "network", "layer_dims": dims, "activations": ["tanh"] * 3, "eps": 1e-8,
                 "weights": cases.lyapunov_like_network_weights(case["P"], dims)}
    case["lv"] = ("norm_grad",)
    lyap, olyap = build_lyapunov(case), cases.oracle_lyapunov(case)
    assert_allclose(lyap.values, olyap.values, rtol=1e-12, atol=1e-18)
    values, neg, rec = _engine_records(lyap)
    ref_rec, ref_neg = _oracle_all(olyap)
    assert_allclose(rec, ref_rec, rtol=1e-8, atol=1e-13)
    flips, _ = _check_masks(neg, ref_neg, rec, ref_rec, allowed=4)
    olyap.update_safe_set()
    init = np.count_nonzero(cases.initial_safe_mask(case))
    assert ref_neg.any() and (~ref_neg).any() and olyap.safe_set.sum() >= init + 1000
    if flips == 0 and np.array_equal(lyap.values, olyap.values):
        lyap.update_safe_set()
        assert_array_equal(lyap.safe_set, olyap.safe_set)
        assert lyap.c_max == olyap.c_max


@pytest.mark.parametrize("lv_kind", ["abs_grad", "norm_grad"])
def test_table_lyapunov_function(sl, lv_kind):
    """Triangulation V (e.g. -value_function of the RL loop) with |gradient| as L_v
    (inverted_pendulum.ipynb cell 14)."""
    from safe_learning_amd.benchmarks import build_lyapunov
    case = cases.make_case("pendulum", num_points=33, dynamics="linear", tau_scale=0.0)
    g = oracle.GridWorld(case["limits"], case["num_points"])
    pts = g.all_points
    vals = np.einsum("ij,jk,ik->i", pts, case["P"], pts) + 0.05 * np.sin(3 * pts[:, 0]) * pts[:, 1]
    case["V"] = {"kind": "table", "values": vals[:, None], "project": True}
    case["lv"] = (lv_kind,)
    lyap, olyap = build_lyapunov(case), cases.oracle_lyapunov(case)
    values, neg, rec = _engine_records(lyap)
    ref_rec, ref_neg = _oracle_all(olyap)
    # The cell's own state is a grid vertex, where the gradient of a piecewise-linear table (and
    # with it the reference's L_v(x), hence the threshold for tau > 0) depends on the simplex
    # scipy happens to return; tau = 0 here, so the threshold is exactly -0.0 for every choice.
    # Successor states on cell faces are excluded for the same reason.
    from test_gpu_rl import ambiguous_points
    otri = olyap.lyapunov_function
    nxt = ref_rec[:, 2:4]
    frac = (g._center_states(nxt, clip=True) % g.unit_maxes) / g.unit_maxes
    on_face = (np.abs(frac) < 1e-9).any(axis=1) | (np.abs(frac - 1) < 1e-9).any(axis=1)
    on_face |= np.abs(frac.sum(axis=1) - 1) < 1e-9
    on_face |= ambiguous_points(otri, nxt)
    ok = ~on_face
    import exclusions
    # the table's GRADIENT (L_v at the successor) is what is ambiguous on a face, not its value
    exclusions.report("test_table_lyapunov_function[%s]" % lv_kind, ok, "successor", limit=0.10)   # measured 4.1 %
    assert ok.sum() > 50
    assert_allclose(values, olyap.values, rtol=1e-12, atol=1e-14)
    assert np.all(rec[:, 1] == 0.0) and np.all(ref_rec[:, 1] == 0.0)
    assert_allclose(rec[ok][:, [0, 2, 3]], ref_rec[ok][:, [0, 2, 3]], rtol=1e-9, atol=1e-12)
    assert np.array_equal(neg[ok], ref_neg[ok])


def _on_table_face(otri, pts):
    from test_gpu_rl import ambiguous_points
    g = otri.discretization
    frac = (g._center_states(pts, clip=True) % g.unit_maxes) / g.unit_maxes
    on_face = (np.abs(frac) < 1e-9).any(axis=1) | (np.abs(frac - 1) < 1e-9).any(axis=1)
    on_face |= np.abs(frac.sum(axis=1) - 1) < 1e-9
    return on_face | ambiguous_points(otri, pts)


def test_table_value_and_table_policy_with_gp(sl):
    """The sweep of inverted_pendulum.ipynb cell 14 (bench config C2-table): V and the policy are
    piecewise-linear tables on a coarser grid than the Lyapunov discretization, the dynamics a
    GP, L_v = |grad V| at the cell's own state, tau > 0."""
    from safe_learning_amd.benchmarks import build_lyapunov, table_case
    case = table_case(num_points=(45, 37), table_points=(11, 9), n_gp=60, tau_scale=0.01)
    lyap, olyap = build_lyapunov(case), cases.oracle_lyapunov(case)
    values, neg, rec = _engine_records(lyap)
    ref_rec, ref_neg = _oracle_all(olyap)
    otri = olyap.lyapunov_function
    states = olyap.discretization.all_points
    # gradients (hence thresholds) are simplex dependent on faces of the table grid
    opol = olyap.policy.fun if hasattr(olyap.policy, "fun") else olyap.policy
    ok_x = ~(_on_table_face(otri, states) | _on_table_face(opol, states))
    ok_n = ~_on_table_face(otri, ref_rec[:, 2:4])
    assert ok_x.sum() > 800 and (ok_x & ok_n).sum() > 800
    # (cells on table grid lines: the reference's value there depends on scipy's search history)
    assert_allclose(values[ok_x], olyap.values[ok_x], rtol=1e-12, atol=1e-14)
    assert_allclose(rec[ok_x][:, 2:], ref_rec[ok_x][:, 2:], rtol=RTOL_GP, atol=1e-12)  # mean, error
    assert_allclose(rec[ok_x][:, 1], ref_rec[ok_x][:, 1], rtol=1e-9, atol=1e-14)
    both = ok_x & ok_n
    assert_allclose(rec[both][:, 0], ref_rec[both][:, 0], rtol=1e-7, atol=1e-12)
    assert (ref_rec[:, 1] < 0).all() and 10 < ref_neg.sum() < len(ref_neg) - 10
    _check_masks(neg[both], ref_neg[both], rec[both], ref_rec[both])


def test_table_policy_with_quadratic_value_on_a_large_training_set(sl):
    """Only the POLICY is a table (quadratic V, linear L_v): the same three passes, and here every
    number has a bit-exact or tight counterpart in the oracle."""
    from safe_learning_amd.benchmarks import build_lyapunov, table_case
    case = table_case(num_points=(45, 40), table_points=(11, 9), n_gp=300, tau_scale=0.01)
    del case["V"]
    case["lv"] = ("abs_linear", 2 * case["P"])
    lyap, olyap = build_lyapunov(case), cases.oracle_lyapunov(case)
    values, neg, rec = _engine_records(lyap)
    kernel = lyap._ctx.last_kernel()
    assert "k_gp_sweep4" in kernel and "k_policy_table" in kernel and "k_check_records" in kernel, kernel
    ref_rec, ref_neg = _oracle_all(olyap)
    opol = olyap.policy.fun if hasattr(olyap.policy, "fun") else olyap.policy
    ok = ~_on_table_face(opol, olyap.discretization.all_points)
    assert ok.sum() > 800
    assert_array_equal(values, olyap.values)
    assert_allclose(rec[ok][:, 2:], ref_rec[ok][:, 2:], rtol=RTOL_GP, atol=1e-12)
    assert_allclose(rec[ok][:, :2], ref_rec[ok][:, :2], rtol=1e-7, atol=1e-12)
    _check_masks(neg[ok], ref_neg[ok], rec[ok], ref_rec[ok])
    lyap.update_safe_set()
    olyap.update_safe_set()
    if (neg == ref_neg).all():
        assert_array_equal(lyap.safe_set, olyap.safe_set)
        assert lyap.c_max == olyap.c_max


@pytest.mark.parametrize("closed_form_policy", [False, True], ids=["table_policy", "closed_form_policy"])
def test_table_flavours_on_a_large_training_set(sl, closed_form_policy):
    """The same sweep with more than 256 training points: the interpolated policy becomes a
    per-cell action table (``k_policy_table``), ``k_gp_sweep4`` writes the posterior records of
    that closed loop and ``k_check_records`` runs the check with the real V and L_v - instead of
    ``k_gp_sweep``'s 16x16x4 structure.  Same comparisons as above, and whole level sets."""
    from safe_learning_amd.benchmarks import build_lyapunov, table_case
    case = table_case(num_points=(45, 40), table_points=(11, 9), n_gp=300, tau_scale=0.01)
    if closed_form_policy:
        del case["policy_table"]
    lyap, olyap = build_lyapunov(case), cases.oracle_lyapunov(case)
    values, neg, rec = _engine_records(lyap)
    kernel = lyap._ctx.last_kernel()
    assert "k_gp_sweep4" in kernel and "k_check_records" in kernel, kernel
    assert ("k_policy_table" in kernel) == (not closed_form_policy), kernel
    ref_rec, ref_neg = _oracle_all(olyap)
    otri = olyap.lyapunov_function
    states = olyap.discretization.all_points
    opol = olyap.policy.fun if hasattr(olyap.policy, "fun") else olyap.policy
    ok_x = ~_on_table_face(otri, states)
    if not closed_form_policy:
        ok_x &= ~_on_table_face(opol, states)
    ok_n = ~_on_table_face(otri, ref_rec[:, 2:4])
    assert ok_x.sum() > 800 and (ok_x & ok_n).sum() > 800
    assert_allclose(values[ok_x], olyap.values[ok_x], rtol=1e-12, atol=1e-14)
    assert_allclose(rec[ok_x][:, 2:], ref_rec[ok_x][:, 2:], rtol=RTOL_GP, atol=1e-12)  # mean, error
    assert_allclose(rec[ok_x][:, 1], ref_rec[ok_x][:, 1], rtol=1e-9, atol=1e-14)
    both = ok_x & ok_n
    assert_allclose(rec[both][:, 0], ref_rec[both][:, 0], rtol=1e-7, atol=1e-12)
    assert 10 < ref_neg.sum() < len(ref_neg) - 10
    _check_masks(neg[both], ref_neg[both], rec[both], ref_rec[both])
    # a shard that does not start at cell 0 (the action table and the records are shard-relative)
    from test_gpu_reference_gp import sweep_records
    idx = np.arange(1088, 1800)
    part, kernels = sweep_records(lyap, idx)
    assert all("k_check_records" in k for k in kernels)
    assert_array_equal(part, rec[idx])
    # the 16x16x4 kernel computes the same records (SL_GP_CFG=3 at upload time)
    import os
    os.environ["SL_GP_CFG"] = "3"
    try:
        other = build_lyapunov(case)
        _, neg3, rec3 = _engine_records(other)
        assert other._ctx.last_kernel().startswith("k_gp_sweep<")
    finally:
        del os.environ["SL_GP_CFG"]
    assert_allclose(rec[ok_x][:, 2:], rec3[ok_x][:, 2:], rtol=1e-9, atol=1e-13)
    assert (neg[both] != neg3[both]).sum() == 0


def test_gp_known_answer_through_engine(sl, golden):
    """tests/test_functions.py:237-261 evaluated by the MFMA kernel (explicit points)."""
    import torch
    g = golden["gp_known_answer"]
    grid = sl.GridWorld([[-4, 4], [-4, 4]], 5)
    X, Y = np.array(g["X"], dtype=float), np.array(g["Y"], dtype=float)
    # GP over (x0, x1): model it as 1 state + 1 action so that the engine's input is [x, u]
    grid1 = sl.GridWorld([[-4, 4]], 5)
    gp = sl.GPRCached(X, Y, sl.RBF(2), None)
    dyn = sl.GaussianProcess(gp, g["beta"])
    pts = np.array(g["test_points"], dtype=float)
    for row, (mean_ref, err_ref) in enumerate(zip(g["expected_mean"], g["expected_error"])):
        policy = sl.ConstantFunction([pts[row, 1]])
        lyap = sl.Lyapunov(grid1, sl.QuadraticFunction([[1.0]]), dyn, 0.0, 1.0, 0.0, policy)
        lyap._upload_model()
        d_pts = torch.tensor([[pts[row, 0]]], dtype=torch.float64, device=lyap._ctx.torch_device)
        out = torch.zeros((1, 4), dtype=torch.float64, device=lyap._ctx.torch_device)
        lyap._ctx.eval_points(3, 1, d_pts, out)
        rec = out.cpu().numpy()[0]
        assert_allclose(rec[2], mean_ref[0], rtol=g["rtol"])
        assert_allclose(rec[3], err_ref[0], rtol=g["rtol"])


# ---------------------------------------------------------------------------------------------
# prefix-rule semantics: batches, can_shrink=False, c_max quirks, ties
# ---------------------------------------------------------------------------------------------
@pytest.fixture
def small_batches(sl):
    old = (sl.config.gp_batch_size, oracle.config.gp_batch_size)
    sl.config.gp_batch_size = oracle.config.gp_batch_size = 100
    yield 100
    sl.config.gp_batch_size, oracle.config.gp_batch_size = old


def test_can_shrink_false_and_batches(sl, small_batches):
    from safe_learning_amd.benchmarks import build_lyapunov
    case = cases.make_case("pendulum", num_points=50, dynamics="linear", tau_scale=0.02)
    lyap, olyap = build_lyapunov(case), cases.oracle_lyapunov(case)
    rng = np.random.default_rng(3)
    for step in range(4):
        if step == 1:        # pretend earlier verification marked scattered far-away cells safe
            extra = rng.choice(lyap.discretization.nindex, 300, replace=False)
            lyap.safe_set[extra] = True
            olyap.safe_set[extra] = True
        if step == 2:        # a stricter threshold: the safe set may not shrink
            lyap.tau = olyap.tau = case["tau"] * 4
        if step == 3:
            lyap.tau = olyap.tau = 0.0
        lyap.update_safe_set(can_shrink=(step == 0))
        olyap.update_safe_set(can_shrink=(step == 0))
        assert_array_equal(lyap.safe_set, olyap.safe_set)
        assert lyap.c_max == olyap.c_max


def test_c_max_quirks(sl, small_batches):
    from safe_learning_amd.benchmarks import build_lyapunov
    # (a) nothing fails, several batches: c_max = value just before the last batch (lyapunov.py:590)
    case = cases.make_case("pendulum", num_points=30, dynamics="linear", tau_scale=0.0)
    case["K"] = case["K"] * 0.0
    case["saturate"] = None
    case["dynamics"] = {"kind": "linear", "matrix": np.hstack((0.5 * np.eye(2), np.zeros((2, 1))))}
    case["initial_radius"] = 0.05          # the origin cell must be initial (decrease == 0 there)
    num = case["num_points"]
    case["num_points"] = [31, 31]          # odd: the origin is a grid point
    lyap, olyap = build_lyapunov(case), cases.oracle_lyapunov(case)
    lyap.update_safe_set(); olyap.update_safe_set()
    assert olyap.safe_set.all()
    assert_array_equal(lyap.safe_set, olyap.safe_set)
    assert lyap.c_max == olyap.c_max
    # (b) the very first cell fails: c_max = max(values)
    case = cases.make_case("pendulum", num_points=20, dynamics="linear", tau_scale=50.0)
    case["initial_radius"] = -1.0          # empty initial set
    lyap, olyap = build_lyapunov(case), cases.oracle_lyapunov(case)
    lyap.update_safe_set(); olyap.update_safe_set()
    assert not olyap.safe_set.any()
    assert_array_equal(lyap.safe_set, olyap.safe_set)
    assert lyap.c_max == olyap.c_max == olyap.values.max()


def test_deferred_c_max_is_the_level_of_its_own_update(sl, small_batches):
    """update_safe_set() defers the host's read of c_max; when nothing fails, that read selects an
    order statistic of the ordering keys (lyapunov.py:590-595 sets c_max inside update_safe_set from
    the values of THAT moment).  update_values() with another V in between - a new function object,
    an in-place edit of the matrix - must not move it."""
    from safe_learning_amd.benchmarks import build_lyapunov
    case = cases.make_case("pendulum", num_points=30, dynamics="linear", tau_scale=0.0)
    case["K"] = case["K"] * 0.0
    case["saturate"] = None
    case["dynamics"] = {"kind": "linear", "matrix": np.hstack((0.5 * np.eye(2), np.zeros((2, 1))))}
    case["initial_radius"] = 0.05
    case["num_points"] = [31, 31]
    other = np.array([[0.3, 0.1], [0.1, 2.0]])
    for how in ("new object", "in place"):
        lyap, olyap = build_lyapunov(case), cases.oracle_lyapunov(case)
        lyap.update_safe_set(); olyap.update_safe_set()
        assert olyap.safe_set.all() and lyap.discretization.nindex > small_batches
        if how == "new object":
            lyap.lyapunov_function = sl.QuadraticFunction(other)
        else:
            lyap.lyapunov_function.matrix[...] = other
        lyap.update_values()
        olyap.lyapunov_function = oracle.QuadraticFunction(other)
        c_before = olyap.c_max
        olyap.update_values()
        assert lyap.c_max == c_before == olyap.c_max, how
        assert_array_equal(lyap.values, olyap.values)
        lyap.update_safe_set(); olyap.update_safe_set()
        assert_array_equal(lyap.safe_set, olyap.safe_set)
        assert lyap.c_max == olyap.c_max


def test_frozen_initial_mask_is_never_hashed(sl):
    """A read-only initial_safe_set is identified by object identity from its first use on: no
    digest, no RuntimeWarning about a large writable mask (benchmarks.build_lyapunov freezes its)."""
    import warnings
    from safe_learning_amd import lyapunov as lyap_module
    from safe_learning_amd.benchmarks import build_lyapunov
    case = cases.make_case("cartpole", num_points=72, dynamics="linear", tau_scale=0.004)   # 26.9 MB of bool
    calls = []
    real = lyap_module._digest
    lyap_module._digest = lambda arr: calls.append(arr.nbytes) or real(arr)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            lyap = build_lyapunov(case)
            lyap.update_safe_set()
            lyap.update_safe_set()
            assert lyap.safe_count > 0
    finally:
        lyap_module._digest = real
    assert calls == []


def test_ties_in_values(sl, small_batches):
    """P = 0 in one direction: whole grid lines share a value; ties resolve by flat index."""
    from safe_learning_amd.benchmarks import build_lyapunov
    case = cases.make_case("pendulum", num_points=24, dynamics="linear", tau_scale=0.01)
    case["P"] = np.array([[1.0, 0.0], [0.0, 0.0]])
    case["lv"] = ("const", 0.05)
    lyap, olyap = build_lyapunov(case), cases.oracle_lyapunov(case)
    for shrink in (True, False, False):
        lyap.update_safe_set(can_shrink=shrink); olyap.update_safe_set(can_shrink=shrink)
        assert_array_equal(lyap.safe_set, olyap.safe_set)
        assert lyap.c_max == olyap.c_max
        olyap.tau = lyap.tau = lyap.tau * 3


def test_select_kth(sl):
    """The device-resident radix select (sl_select_begin / _hist / _digit) on explicit values with
    ties, NaNs and signed zeros; k given by the caller, k derived on the device from a folded
    record (the batch behind the first failure, lyapunov.py:585-587), and k beyond the grid."""
    import torch
    from safe_learning_amd import _hip
    from safe_learning_amd.benchmarks import build_lyapunov
    from safe_learning_amd.distributed import u64
    case = cases.make_case("pendulum", num_points=37, dynamics="linear")
    lyap = build_lyapunov(case)
    rng = np.random.default_rng(5)
    n = lyap.discretization.nindex
    vals = rng.normal(size=n).round(1)          # many ties
    vals[rng.choice(len(vals), 10)] = np.nan
    vals[rng.choice(len(vals), 10)] = -0.0
    lyap._values_implicit = False
    lyap._d_values.copy_(torch.from_numpy(vals))
    order = np.argsort(vals, kind="stable")
    from safe_learning_amd.lyapunov import vbits_to_float, select_kth, _HipShardEngine
    engine = _HipShardEngine(lyap)

    def key_of(state):
        words = state.cpu().numpy()
        return u64(words[_hip.S_KEY_V]), int(words[_hip.S_KEY_I]), int(words[_hip.S_NONE])

    for k in [0, 1, 17, 500, len(vals) // 2, len(vals) - 11, len(vals) - 1]:
        vbits, index, none = key_of(select_kth(engine, k, 1, lyap._d_folded, n))
        assert index == order[k] and not none
        got, ref = vbits_to_float(vbits), vals[order[k]]
        assert (np.isnan(got) and np.isnan(ref)) or got == ref
    # k from the device: (count_below // batch + 1) * batch
    record = torch.zeros(_hip.RESULT_WORDS, dtype=torch.int64, device=lyap._ctx.torch_device)
    for below, batch in ((0, 7), (123, 50), (n - 30, 100), (n - 1, 10), (n, 13)):
        record[_hip.R_BELOW] = below
        k = (below // batch + 1) * batch
        vbits, index, none = key_of(select_kth(engine, -1, batch, record, n))
        if k >= n:
            assert none and vbits == (1 << 64) - 1 and index == (1 << 63) - 1
        else:
            assert not none and index == order[k]


def test_implicit_values_are_bit_identical(sl, small_batches):
    """Quadratic V: the sweep and the streaming passes recompute the ordering keys from the cell
    index (sl_values_implicit; 8 cells of a grid row per thread) instead of reading the values
    array.  Masks, safe sets, c_max, counters and the radix select must be bit for bit those of the
    explicit path, for can_shrink on and off, on grids with and without whole bytes per row."""
    from safe_learning_amd.benchmarks import build_lyapunov
    shapes = [("1d", dict(num_points=1000)), ("pendulum", dict(num_points=[17, 43], dynamics="linear", tau_scale=0.02)),
              ("pendulum", dict(num_points=64, dynamics="analytic", tau_scale=0.01)),
              ("cartpole", dict(num_points=[5, 6, 7, 16], dynamics="linear", tau_scale=0.01)),
              ("cartpole", dict(num_points=9, n_gp=60, tau_scale=0.0))]
    for name, kw in shapes:
        case = cases.make_case(name, **kw)
        implicit, explicit = build_lyapunov(case), build_lyapunov(case)
        # rows of whole bytes: a thread's 8 cells share the row prefix (else V stays explicit)
        expected = case["num_points"][-1] % 8 == 0
        assert implicit._values_implicit == expected
        assert implicit._d_values_buffer is None or not expected
        explicit._values_implicit = False
        olyap = cases.oracle_lyapunov(case)
        rng = np.random.default_rng(1)
        for step, shrink in enumerate((True, False, False, True)):
            if step == 1:                          # hand-marked cells beyond the level set
                extra = rng.choice(implicit.discretization.nindex, 40, replace=False)
                for ly in (implicit, explicit, olyap):
                    ly.safe_set[extra] = True
                    ly.tau = case["tau"] * 3 if case["tau"] else 0.0
            for ly in (implicit, explicit, olyap):
                ly.update_safe_set(can_shrink=shrink)
            assert implicit._d_values_buffer is None or not expected       # never materialised
            assert_array_equal(implicit.safe_set, explicit.safe_set)
            assert implicit.c_max == explicit.c_max and implicit.safe_count == explicit.safe_count
            if case["dynamics"]["kind"] != "gp":
                assert_array_equal(implicit.safe_set, olyap.safe_set)
                assert implicit.c_max == olyap.c_max
        # reading the attribute materialises the very numbers the kernels used
        assert_array_equal(implicit.values, olyap.values)
    # a grid whose last np.linspace point is not index_to_state's: the keys stay explicit
    case = cases.make_case("pendulum", num_points=[17, 43], dynamics="linear")
    case["limits"] = [[-1.0, 1.03], [-0.97, 1.0]]
    grid = sl.GridWorld(case["limits"], case["num_points"])
    exact = all((n - 1) * u + o == hi for n, u, o, (_, hi) in
                zip(grid.num_points, grid.unit_maxes, grid.offset, grid.limits))
    lyap = build_lyapunov(case)
    assert lyap._values_implicit == exact
    olyap = cases.oracle_lyapunov(case)
    lyap.update_safe_set()
    olyap.update_safe_set()
    assert_array_equal(lyap.safe_set, olyap.safe_set)
    assert lyap.c_max == olyap.c_max


def test_bits_bytes_roundtrip(sl):
    import torch
    from safe_learning_amd import _hip
    ctx = _hip.Context()
    rng = np.random.default_rng(0)
    for n in (1, 7, 8, 63, 64, 65, 1000, 4099):
        mask = rng.random(n) < 0.4
        d_bytes = torch.from_numpy(mask.view(np.uint8)).to(ctx.torch_device)
        d_bits = torch.zeros((n + 63) // 64, dtype=torch.int64, device=ctx.torch_device)
        ctx.bytes_to_bits(n, d_bytes, d_bits)
        ref = np.packbits(mask, bitorder="little")
        got = d_bits.cpu().numpy().view(np.uint8)[:len(ref)]
        assert_array_equal(got, ref)
        out = torch.zeros(((n + 7) // 8) * 8, dtype=torch.uint8, device=ctx.torch_device)
        ctx.bits_to_bytes(n, d_bits, out)
        assert_array_equal(out.cpu().numpy()[:n].astype(bool), mask)


def test_smallest_boundary_value(sl, golden):
    g = golden["smallest_boundary_value"]
    # the reference's literal uses 2*sum|x| (not representable as a spec); use a quadratic with
    # the oracle as the checker on the same grid
    grid = sl.GridWorld(g["limits"], g["num_points"])
    P = np.array([[2.0, 0.3], [0.1, 1.0]])
    got = sl.smallest_boundary_value(sl.QuadraticFunction(P), grid)
    ref = oracle.smallest_boundary_value(oracle.QuadraticFunction(P),
                                         oracle.GridWorld(g["limits"], g["num_points"]))
    assert got == ref


def test_errors_are_loud(sl):
    from safe_learning_amd import _hip
    grid = sl.GridWorld([[-1, 1]], 5)
    with pytest.raises(TypeError):
        sl.Lyapunov(grid, sl.QuadraticFunction([[1.0]]), sl.LinearSystem((np.array([[1., 1.]]),)),
                    0.4, lambda x: x, 0.1, sl.LinearSystem((np.array([[-0.1]]),)))
    with pytest.raises(sl.DimensionError):
        sl.GridWorld([[0, 1]], 1)
    ctx = _hip.Context()
    with pytest.raises(_hip.HipEngineError):
        ctx.values(0, 10, None)                        # model not set


# ---------------------------------------------------------------------------------------------
# evaluation at explicit points (Function.__call__, Lyapunov.threshold / v_decrease_bound)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw", [
    ("pendulum", dict(num_points=20, dynamics="linear")),
    ("pendulum", dict(num_points=20, dynamics="analytic")),
    ("pendulum", dict(num_points=20, n_gp=90)),
    ("cartpole", dict(num_points=5, n_gp=120)),
    ("cartpole", dict(num_points=5, n_gp=60, stack=True)),
])
def test_point_evaluation_api(sl, name, kw):
    from safe_learning_amd.benchmarks import build_lyapunov
    case = cases.make_case(name, **kw)
    lyap, olyap = build_lyapunov(case), cases.oracle_lyapunov(case)
    rng = np.random.default_rng(11)
    d = case["d"]
    x = rng.uniform(-1, 1, (37, d))
    u = rng.uniform(-1, 1, (37, 1))
    assert_allclose(lyap.lyapunov_function(x), olyap.lyapunov_function(x), rtol=1e-13)
    assert_allclose(lyap.policy(x), olyap.policy(x), rtol=1e-13, atol=1e-15)
    got, ref = lyap.dynamics(x, u), olyap.dynamics(x, u)
    if isinstance(ref, tuple):
        assert_allclose(got[0], ref[0], rtol=1e-9, atol=1e-13)
        assert_allclose(got[1], ref[1], rtol=1e-7, atol=1e-12)
        nxt, onxt = got, ref
    else:
        assert_allclose(got, ref, rtol=1e-12, atol=1e-15)
        nxt, onxt = got, ref
    assert_allclose(lyap.lipschitz_lyapunov(x), olyap.lipschitz_lyapunov(x), rtol=1e-13)
    assert_allclose(lyap.threshold(x), olyap.threshold(x), rtol=1e-13)
    assert_allclose(lyap.threshold(x, 0.3), olyap.threshold(x, 0.3), rtol=1e-13)
    assert_allclose(lyap.v_decrease_bound(x, nxt), olyap.v_decrease_bound(x, onxt),
                    rtol=1e-7, atol=1e-12)
    grad = sl.LinearSystem((2 * case["P"],))
    assert_allclose(grad(x), oracle.LinearSystem((2 * case["P"],))(x), rtol=1e-13)


# ---------------------------------------------------------------------------------------------
# adaptive branch (lyapunov.py:445-487, 540-582), bug-compatible restatement
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw", [
    ("pendulum", dict(num_points=61, dynamics="analytic", tau_scale=1.0)),
    ("pendulum", dict(num_points=61, dynamics="analytic", tau_scale=0.05)),
    ("pendulum", dict(num_points=45, n_gp=80, tau_scale=0.3, noise_std=0.001)),
    ("pendulum", dict(num_points=45, dynamics="linear", tau_scale=0.02)),
])
def test_adaptive_branch(sl, name, kw, small_batches):
    from safe_learning_amd.benchmarks import build_specs
    case = cases.make_case(name, **kw)
    init = np.zeros(int(np.prod(case["num_points"])), dtype=bool)
    init[cases.initial_safe_mask(case)] = True
    policy, dynamics, value, lv = build_specs(case)
    lyap = sl.Lyapunov(sl.GridWorld(case["limits"], case["num_points"]), value, dynamics, case["lf"],
                       lv, case["tau"], policy, initial_set=init, adaptive=True)
    opolicy, odynamics, ovalue, olv = cases.oracle_specs(case)
    olyap = oracle.Lyapunov(oracle.GridWorld(case["limits"], case["num_points"]), ovalue, odynamics,
                            case["lf"], olv, case["tau"], opolicy, initial_set=init, adaptive=True)
    for shrink, factor in ((True, 1.0), (False, 1.5), (True, 1.0)):
        lyap.update_safe_set(can_shrink=shrink, max_refinement=16, safety_factor=factor)
        olyap.update_safe_set(can_shrink=shrink, max_refinement=16, safety_factor=factor)
        assert_array_equal(lyap.safe_set, olyap.safe_set)
        assert_array_equal(lyap._refinement, olyap._refinement)
        assert lyap.c_max == olyap.c_max
        lyap.tau = olyap.tau = lyap.tau * 0.5


@pytest.mark.parametrize("name,kw", [
    # oracle side, cells with N(x) > 1 after the first three steps: 2, 2, 2 / 4, 4, 0 / 2, 2, 0
    ("pendulum", dict(num_points=61, dynamics="analytic", tau_scale=1.0)),
    ("pendulum", dict(num_points=61, dynamics="analytic", tau_scale=0.05)),
    ("pendulum", dict(num_points=45, dynamics="linear", tau_scale=0.02)),
])
def test_refinement_survives_a_plain_update_that_must_not_shrink(sl, name, kw, small_batches):
    """``lyapunov.py:507-510``: with ``can_shrink=False`` the loop starts from the previous
    ``_refinement``; a NON-adaptive update writes 1 where the decrease condition holds, 0 from the
    first failure to the end of its batch, and leaves N(x) > 1 of an earlier adaptive update alone
    elsewhere (``:531, 585-587, 601-606``) - carried on the device by ``sl_refinement_carry``."""
    from safe_learning_amd.benchmarks import build_specs
    case = cases.make_case(name, **kw)
    init = np.zeros(int(np.prod(case["num_points"])), dtype=bool)
    init[cases.initial_safe_mask(case)] = True
    policy, dynamics, value, lv = build_specs(case)
    lyap = sl.Lyapunov(sl.GridWorld(case["limits"], case["num_points"]), value, dynamics, case["lf"],
                       lv, case["tau"], policy, initial_set=init, adaptive=True)
    opolicy, odynamics, ovalue, olv = cases.oracle_specs(case)
    olyap = oracle.Lyapunov(oracle.GridWorld(case["limits"], case["num_points"]), ovalue, odynamics,
                            case["lf"], olv, case["tau"], opolicy, initial_set=init, adaptive=True)
    steps = [dict(can_shrink=True, max_refinement=16, safety_factor=1.5),     # adaptive: some N(x) > 1
             dict(can_shrink=False),                                          # plain, stricter tau
             dict(can_shrink=False),                                          # plain, looser tau
             dict(can_shrink=False, max_refinement=16, safety_factor=1.5),    # adaptive on top of it
             dict(can_shrink=True)]                                           # plain reset: N = safe
    t0 = 0.4 * case["tau"]
    taus = [t0, 1.5 * t0, 0.5 * t0, 0.5 * t0, t0]
    seen_large = False
    for step, tau in zip(steps, taus):
        lyap.tau = olyap.tau = tau
        lyap.update_safe_set(**step)
        olyap.update_safe_set(**step)
        assert_array_equal(lyap.safe_set, olyap.safe_set)
        assert_array_equal(lyap._refinement, olyap._refinement)
        assert lyap.c_max == olyap.c_max
        if "max_refinement" not in step and not step["can_shrink"]:
            seen_large = seen_large or bool((olyap._refinement > 1).any())
    assert seen_large, "no N(x) > 1 was carried through a plain update: the scenario tests nothing"


def test_get_lyapunov_region(sl):
    """Flood fill of lyapunov.py:59-139 on engine values vs the oracle."""
    limits, num = [[-1, 1], [-1, 1]], [21, 25]
    P = np.array([[1.0, 0.3], [0.3, 0.5]])
    region = sl.get_lyapunov_region(sl.QuadraticFunction(P), sl.GridWorld(limits, num), (10, 12))
    ref = oracle.get_lyapunov_region(oracle.QuadraticFunction(P), oracle.GridWorld(limits, num),
                                     (10, 12))
    assert ref.sum() > 20
    assert_array_equal(region, ref)
    # a table with a local bump: the fill must stop where the values decrease (grid spacing is a
    # binary fraction so that the reference's vertex lookup is free of the `%` wrap-around glitch)
    num = [17, 33]
    grid, ogrid = sl.GridWorld(limits, num), oracle.GridWorld(limits, num)
    pts = ogrid.all_points
    vals = np.einsum("ij,jk,ik->i", pts, P, pts) - 0.2 * np.exp(-200 * ((pts[:, 0] - 0.5) ** 2 + pts[:, 1] ** 2))
    region = sl.get_lyapunov_region(sl.Triangulation(grid, vals), grid, (8, 16))
    ref = oracle.get_lyapunov_region(oracle.Triangulation(ogrid, vals), ogrid, (8, 16))
    assert ref.sum() > 20
    assert_array_equal(region, ref)


def test_safety_constraint(sl):
    """Lyapunov.safety_constraint(policy) (lyapunov.py:378-406, as documented there): the decrease
    mask under another policy, given per vertex or as a spec; the object's own policy and safe
    set are left alone."""
    from safe_learning_amd.benchmarks import build_lyapunov
    case = cases.make_case("pendulum", num_points=40, n_gp=120, tau_scale=0.0)
    lyap, olyap = build_lyapunov(case), cases.oracle_lyapunov(case)
    lyap.update_safe_set()
    safe_before, c_before = lyap.safe_set.copy(), lyap.c_max
    x = olyap.discretization.index_to_state(np.arange(olyap.discretization.nindex))
    init = np.zeros(len(x), dtype=bool)
    init[cases.initial_safe_mask(case)] = True
    # the own policy, handed over as a per-vertex table
    own = olyap.policy(x)
    ref = olyap.negative(x)
    assert ref.any()
    assert_array_equal(lyap.safety_constraint(own, include_initial=False), ref)
    assert_array_equal(lyap.safety_constraint(own), ref | init)
    # a different one: no control at all
    zero = sl.ConstantFunction(np.zeros(1))
    opolicy = olyap.policy
    olyap.policy = lambda states: np.zeros((len(states), 1))
    ref0 = olyap.negative(x)
    olyap.policy = opolicy
    assert_array_equal(lyap.safety_constraint(zero, include_initial=False), ref0)
    assert not np.array_equal(ref0, ref)
    lyap.update_safe_set()
    assert_array_equal(lyap.safe_set, safe_before)
    assert lyap.c_max == c_before


@pytest.mark.parametrize("name,kw", [
    ("pendulum", dict(num_points=40, dynamics="linear", tau_scale=0.02)),
    ("pendulum", dict(num_points=48, n_gp=300, tau_scale=0.01, signal_std=0.03, noise_std=0.0005,
                      lengthscale=1.5)),
    ("cartpole", dict(num_points=9, dynamics="analytic", tau_scale=0.002)),
])
def test_state_dependent_lipschitz_dynamics(sl, name, kw):
    """lipschitz_dynamics as a function of the state (lyapunov.py:227-244 accepts a callable):
    the spec c + ||M x||_1 in the kernels against a Python callable in the oracle."""
    from safe_learning_amd.benchmarks import build_specs
    case = cases.make_case(name, **kw)
    d = case["d"]
    rng = np.random.default_rng(12)
    mat = rng.uniform(-1.5, 1.5, (d, d))
    const = 0.3 * case["lf"]
    init = cases.initial_safe_mask(case)
    policy, dynamics, value, lv = build_specs(case)
    lf_spec = const + sl.Norm1Function(sl.LinearSystem((mat,)))
    lyap = sl.Lyapunov(sl.GridWorld(case["limits"], case["num_points"]), value, dynamics, lf_spec,
                       lv, case["tau"], policy, initial_set=init)
    opolicy, odynamics, ovalue, olv = cases.oracle_specs(case)
    olf = lambda x: const + oracle.np_functions.ordered_rowsum(np.abs(oracle.ordered_matmul(x, mat.T)))   # noqa: E731
    olyap = oracle.Lyapunov(oracle.GridWorld(case["limits"], case["num_points"]), ovalue, odynamics,
                            olf, olv, case["tau"], opolicy, initial_set=init)
    values, neg, rec = _engine_records(lyap)
    ref_rec, ref_neg = _oracle_all(olyap)
    deterministic = case["dynamics"]["kind"] == "linear"
    if deterministic:
        assert_array_equal(rec[:, 1], ref_rec[:, 1])               # thresholds bit for bit
    assert_allclose(rec, ref_rec, rtol=1e-9, atol=1e-12)
    flips, _ = _check_masks(neg, ref_neg, rec, ref_rec)
    assert ref_neg.any() and (~ref_neg).any()
    x = olyap.discretization.index_to_state(np.arange(0, len(rec), 7))
    assert_allclose(lyap.lipschitz_dynamics(x), olf(x), rtol=0, atol=0)
    assert_allclose(lyap.threshold(x), olyap.threshold(x), rtol=1e-13)
    _compare_safe_sets(lyap, olyap, flips, neg)


@pytest.mark.parametrize("noise_std,cond_min,var_rtol", [
    (3e-5, 5e8, 1e-5),        # cond(K) ~ 9e8: measured agreement ~2e-7
    (1e-5, 5e9, 1e-5),        # cond(K) ~ 8e9: ~1e-6, still inside the north-star tolerance
    (1e-6, 5e11, 1e-3),       # cond(K) ~ 8e11: ~1e-4 - where the explicit inverse stops meeting 1e-5
])
def test_ill_conditioned_gp(sl, noise_std, cond_min, var_rtol):
    """The engine multiplies by an explicit L^-1 where the reference solves with L
    (functions.py:441).  With nearly noise-free data the kernel matrix is ill conditioned and the
    two lose digits differently in var = k(x,x) - |a|^2 (which also cancels by up to 1e-9 here):
    the posterior mean / variance must still agree to the north-star tolerance 1e-5 up to
    cond(K) ~ 1e10; the last row documents where that stops."""
    from safe_learning_amd.benchmarks import build_lyapunov
    case = cases.make_case("pendulum", num_points=24, n_gp=400, noise_std=noise_std,
                           signal_std=0.05, lengthscale=2.0, tau_scale=0.0)
    dyn = case["dynamics"]
    gram = oracle.RBF(3, dyn["variance"], dyn["lengthscales"], ARD=True).K(dyn["X"])
    cond = np.linalg.cond(gram + dyn["noise_variance"] * np.eye(len(gram)))
    assert cond > cond_min
    lyap, olyap = build_lyapunov(case), cases.oracle_lyapunov(case)
    _, neg, rec = _engine_records(lyap)
    ref_rec, ref_neg = _oracle_all(olyap)
    d = case["d"]
    assert_allclose(rec[:, 2:2 + d], ref_rec[:, 2:2 + d], rtol=1e-5, atol=1e-9)
    var, ref_var = (rec[:, 2 + d:] / 2.0) ** 2, (ref_rec[:, 2 + d:] / 2.0) ** 2
    assert np.all(ref_var > 0) and ref_var.min() < 1e-6 * dyn["variance"]     # heavy cancellation
    assert_allclose(var, ref_var, rtol=var_rtol, atol=0)


def test_short_lengthscale_takes_the_direct_path(sl):
    """A lengthscale 25x below the cell spacing (scaled step 25, a^2 = 625): the Gaussian
    recurrence of k_gp_sweep4 would form 0 * inf for training points the run passes close to; the
    kernel must switch to one exponential per (point, cell) there.  Posterior and mask against the
    oracle, nothing NaN."""
    from safe_learning_amd.benchmarks import build_lyapunov
    case = cases.make_case("cartpole", num_points=12, n_gp=300, tau_scale=0.0,
                           signal_std=0.03, noise_std=0.0005, lengthscale=2.0 / 11 / 25)
    lyap, olyap = build_lyapunov(case), cases.oracle_lyapunov(case)
    values, neg, rec = _engine_records(lyap)
    assert "k_gp_sweep4" in lyap._ctx.last_kernel()
    ref_rec, ref_neg = _oracle_all(olyap)
    assert np.isfinite(rec).all()
    d = case["d"]
    assert_allclose(rec[:, 2:2 + d], ref_rec[:, 2:2 + d], rtol=RTOL_GP, atol=1e-12)
    assert_allclose(rec[:, 2 + d:], ref_rec[:, 2 + d:], rtol=1e-7, atol=1e-12)
    _check_masks(neg, ref_neg, rec, ref_rec)
    # a lengthscale between the two regimes (scaled step 0.8 < 1: recurrence; 1.6 > 1: direct)
    for ratio in (0.8, 1.6):
        case = cases.make_case("cartpole", num_points=12, n_gp=300, tau_scale=0.0,
                               signal_std=0.03, noise_std=0.0005, lengthscale=2.0 / 11 / ratio)
        lyap, olyap = build_lyapunov(case), cases.oracle_lyapunov(case)
        values, neg, rec = _engine_records(lyap)
        ref_rec, ref_neg = _oracle_all(olyap)
        assert_allclose(rec[:, 2:2 + d], ref_rec[:, 2:2 + d], rtol=RTOL_GP, atol=1e-12)
        assert_allclose(rec[:, 2 + d:], ref_rec[:, 2 + d:], rtol=1e-7, atol=1e-12)


def test_last_kernel_names_what_ran(sl, monkeypatch):
    """sl_last_kernel: the library itself reports which kernel a sweep launched."""
    from safe_learning_amd.benchmarks import build_lyapunov
    monkeypatch.delenv("SL_GP_CFG", raising=False)
    lyap = build_lyapunov(cases.make_case("pendulum", num_points=50, dynamics="linear", tau_scale=0.02))
    assert lyap._ctx.last_kernel() == ""
    lyap.update_safe_set()
    assert lyap._ctx.last_kernel().startswith("k_det_sweep<")
    lyap = build_lyapunov(cases.make_case("cartpole", num_points=8, n_gp=300, tau_scale=0.0))
    lyap.update_safe_set()
    assert lyap._ctx.last_kernel().startswith("k_gp_sweep4<d=4")
    lyap = build_lyapunov(cases.make_case("pendulum", num_points=32, n_gp=100, tau_scale=0.0))
    lyap.update_safe_set()
    assert lyap._ctx.last_kernel().startswith("k_gp_small<")          # <= 256 points, one head
    # (environment switches are read when a context is created, never per launch)
    monkeypatch.setenv("SL_GP_SMALL", "0")
    lyap.update_safe_set()
    assert lyap._ctx.last_kernel().startswith("k_gp_small<")
    lyap = build_lyapunov(cases.make_case("pendulum", num_points=32, n_gp=100, tau_scale=0.0))
    lyap.update_safe_set()
    assert lyap._ctx.last_kernel().startswith("k_gp_sweep<")
    # SL_GP_CFG=1 (a configuration that no longer exists) leaves the engine's choice alone
    monkeypatch.delenv("SL_GP_SMALL")
    monkeypatch.setenv("SL_GP_CFG", "1")
    lyap = build_lyapunov(cases.make_case("cartpole", num_points=8, n_gp=300, tau_scale=0.0))
    lyap.update_safe_set()
    assert lyap._ctx.last_kernel().startswith("k_gp_sweep4<d=4")
    lyap = build_lyapunov(cases.make_case("pendulum", num_points=32, n_gp=100, tau_scale=0.0))
    lyap.update_safe_set()
    assert lyap._ctx.last_kernel().startswith("k_gp_small<")


def _neg_mask_of_update(lyap):
    lyap.update_safe_set()
    n = lyap._hi - lyap._lo
    bits = lyap._d_neg.cpu().numpy().view(np.uint8)
    return np.unpackbits(bits, bitorder="little")[:n].astype(bool)


@pytest.mark.parametrize("name,kw", [
    ("1d", dict(num_points=1000)),                                                  # scalar L_v
    ("1d", dict(num_points=64, tau_scale=0.0)),
    ("pendulum", dict(num_points=[17, 40], dynamics="linear", tau_scale=0.02)),
    ("pendulum", dict(num_points=128, dynamics="linear", tau_scale=0.0)),
    ("pendulum", dict(num_points=[50, 72], dynamics="linear", tau_scale=0.01)),
    ("cartpole", dict(num_points=8, dynamics="linear", tau_scale=0.0)),
    ("cartpole", dict(num_points=[5, 6, 7, 16], dynamics="linear", tau_scale=0.01)),
    ("cartpole", dict(num_points=24, dynamics="linear", tau_scale=0.004)),
])
def test_row_kernel_is_bit_identical(sl, name, kw, monkeypatch):
    """k_det_rows (8 cells of a grid row per thread, shared prefixes of the ordered sums) against
    k_det_sweep (every cell from scratch) and against the oracle: decrease mask, safe set and c_max
    bit for bit."""
    from safe_learning_amd.benchmarks import build_lyapunov
    case = cases.make_case(name, **kw)
    monkeypatch.delenv("SL_DET_ROWS", raising=False)
    lyap = build_lyapunov(case)
    neg_rows = _neg_mask_of_update(lyap)
    assert lyap._ctx.last_kernel().startswith("k_det_rows<"), lyap._ctx.last_kernel()
    monkeypatch.setenv("SL_DET_ROWS", "0")
    ref = build_lyapunov(case)
    neg_cells = _neg_mask_of_update(ref)
    assert ref._ctx.last_kernel().startswith("k_det_sweep<")
    olyap = cases.oracle_lyapunov(case)
    _, ref_neg = _oracle_all(olyap)
    olyap.update_safe_set()
    assert_array_equal(neg_rows, neg_cells)
    assert_array_equal(neg_rows, ref_neg)
    if kw.get("num_points") in (128, 24):         # the larger grids: both outcomes occur
        assert neg_rows.any() and (~neg_rows).any()
    assert_array_equal(lyap.safe_set, olyap.safe_set)
    assert_array_equal(ref.safe_set, olyap.safe_set)
    assert lyap.c_max == olyap.c_max == ref.c_max


@pytest.mark.parametrize("m", [2, 1])
def test_six_dimensional_stack_of_six_heads_falls_back_to_the_wide_kernel(sl, m):
    """A 6-D FunctionStack of six single-output GPs with 250 training points each (padded capacity
    256).  Two actions (p = 8): the heads' inputs and alpha' (110.6 KB) plus the check's scratch of
    eight wavefronts (53.2 KB) exceed the 160 KB of LDS k_gp_small needs them in, so the sweep must
    take k_gp_sweep instead of failing (advisor finding, round 3) - and agree with the oracle.  One
    action (p = 7, 98 KB + 53 KB): fits since the scaled inputs left the scratch (round 6; it was
    82 KB), k_gp_small takes it."""
    d, n_gp = 6, 250
    rng = np.random.default_rng(5)
    limits, num_points = [[-1.0, 1.0]] * d, [4] * d
    A = np.eye(d) * 0.9 + 0.02 * rng.normal(size=(d, d))
    B = 0.1 * rng.normal(size=(d, m))
    K = -0.2 * rng.normal(size=(m, d))
    P = np.eye(d)
    X = rng.uniform(-1, 1, (n_gp, d + m))
    prior = np.hstack((A, B))
    Y = X @ prior.T + 1e-3 * np.sin(3 * X[:, :d]) + rng.normal(0, 2e-4, (n_gp, d))
    models = {}
    for ns in (sl, oracle):
        heads = []
        for k in range(d):
            kern = ns.RBF(d + m, 1e-6, np.full(d + m, 1.0 + 0.1 * k), ARD=True)
            gp = ns.GPRCached(X, Y[:, [k]], kern, ns.LinearSystem((prior[[k], :],)),
                              likelihood_variance=4e-8)
            heads.append(ns.GaussianProcess(gp, 2.0))
        models[ns] = ns.FunctionStack(heads)
    init = np.zeros(4 ** d, dtype=bool)
    lyaps = {}
    for ns in (sl, oracle):
        grid = ns.GridWorld(limits, num_points)
        lv = ns.AbsFunction(ns.LinearSystem((2 * P,)))
        lyaps[ns] = ns.Lyapunov(grid, ns.QuadraticFunction(P), models[ns], 1.0, lv, 0.0,
                                ns.Saturation(ns.LinearSystem((K,)), -1.0, 1.0), initial_set=init)
    lyap, olyap = lyaps[sl], lyaps[oracle]
    values, neg, rec = _engine_records(lyap)
    assert lyap._ctx.last_kernel().startswith("k_gp_sweep<" if m == 2 else "k_gp_small<"), lyap._ctx.last_kernel()
    ref_rec, ref_neg = _oracle_all(olyap)
    assert_array_equal(values, olyap.values)
    assert_allclose(rec[:, 2:2 + d], ref_rec[:, 2:2 + d], rtol=RTOL_GP, atol=1e-12)
    assert_allclose(rec[:, 2 + d:], ref_rec[:, 2 + d:], rtol=1e-7, atol=1e-12)
    assert_allclose(rec[:, :2], ref_rec[:, :2], rtol=1e-7, atol=1e-12)
    _check_masks(neg, ref_neg, rec, ref_rec)
    # four heads (1 + 1 + 2 + 2 outputs) of the same size still fit: the small kernel keeps them
    def head(cols):
        return sl.GaussianProcess(sl.GPRCached(X, Y[:, cols], sl.RBF(d + m, 1e-6, np.ones(d + m), ARD=True),
                                               sl.LinearSystem((prior[cols, :],)),
                                               likelihood_variance=4e-8), 2.0)
    stack4 = sl.FunctionStack([head([0]), head([1]), head([2, 3]), head([4, 5])])
    lyap4 = sl.Lyapunov(sl.GridWorld(limits, num_points), sl.QuadraticFunction(P), stack4, 1.0,
                        sl.AbsFunction(sl.LinearSystem((2 * P,))), 0.0,
                        sl.Saturation(sl.LinearSystem((K,)), -1.0, 1.0), initial_set=init)
    lyap4.update_safe_set()
    assert lyap4._ctx.last_kernel().startswith("k_gp_small<"), lyap4._ctx.last_kernel()


def test_gp4_sequence_seeds_are_bit_identical(sl, monkeypatch):
    """k_gp_sweep4 keeps the seeds (e_0, rho_0) of a chunk's Gaussian sequences between the panels
    of a tile and draws its tiles from a counter.  With SL_GP4_SEEDS=0 every generation starts from
    the exponentials again: masks, failing keys and the per-cell records (decrease, threshold,
    posterior mean and error) must be bit for bit the same - on a grid whose rows cross the
    saturation kinks of the policy (several runs per wavefront) and with 2 and 3 panels."""
    import torch
    from safe_learning_amd.benchmarks import GP_VARIANTS, build_lyapunov
    for n_gp in (300, 520):
        case = cases.make_case("cartpole", num_points=[6, 6, 6, 64], n_gp=n_gp, tau_scale=0.0,
                               **GP_VARIANTS["tight"])
        n = int(np.prod(case["num_points"]))
        out = []
        for seeds in ("1", "0"):
            monkeypatch.setenv("SL_GP4_SEEDS", seeds)
            lyap = build_lyapunov(case)
            d = case["d"]
            dbg = torch.zeros((n, 2 + 2 * d), dtype=torch.float64, device="cuda:0")
            lyap._ctx.lyap_sweep(0, n, lyap._d_init, lyap._d_values, lyap._d_neg, lyap._d_result, dbg)
            assert lyap._ctx.last_kernel().startswith("k_gp_sweep4")
            out.append((dbg.cpu().numpy(), lyap._d_neg.cpu().numpy().copy(), lyap._d_result.cpu().numpy().copy()))
        for a, b in zip(out[0], out[1]):
            assert_array_equal(a, b)
        # kinks inside the rows: the policy saturates on a part of every row of 64 cells
        states = np.stack(np.meshgrid(*[np.linspace(-1, 1, k) for k in case["num_points"]], indexing="ij"), -1)
        u = states.reshape(-1, case["d"]) @ np.asarray(case["K"]).T
        assert (np.abs(u) > 1).any() and (np.abs(u) < 1).any()


@pytest.mark.parametrize("name,kw", [
    ("pendulum", dict(num_points=48, n_gp=225, tau_scale=0.01)),
    ("pendulum", dict(num_points=[40, 64], n_gp=256, tau_scale=0.01)),
    ("cartpole", dict(num_points=[5, 6, 5, 32], n_gp=230, tau_scale=0.0)),
    ("cartpole", dict(num_points=7, n_gp=240, tau_scale=0.0, stack=True)),
])
def test_one_panel_training_sets_run_on_the_4x4x4_kernel(sl, name, kw, monkeypatch):
    """225 ... 256 training points per head = one 256-row panel that is nearly full: k_gp_sweep4 (whose
    factor fragments are prefetched from L2) instead of k_gp_small (whose factor no longer fits LDS;
    up to 224 points it is the faster one all the same, round 6) - the same records as the oracle's
    and, bit for bit in the masks, as k_gp_small's."""
    from gp_cases import INFORMED, TIGHT
    from safe_learning_amd.benchmarks import build_lyapunov
    case = cases.make_case(name, **dict(kw, **(TIGHT if name == "cartpole" else INFORMED)))
    lyap, olyap = build_lyapunov(case), cases.oracle_lyapunov(case)
    _, neg, rec = _engine_records(lyap)
    assert lyap._ctx.last_kernel().startswith("k_gp_sweep4<"), lyap._ctx.last_kernel()
    ref_rec, ref_neg = _oracle_all(olyap)
    assert_allclose(rec[:, 2:], ref_rec[:, 2:], rtol=1e-7, atol=1e-12)
    assert_allclose(rec[:, :2], ref_rec[:, :2], rtol=1e-7, atol=1e-12)
    flips, _ = _check_masks(neg, ref_neg, rec, ref_rec)
    _compare_safe_sets(lyap, olyap, flips, neg)
    monkeypatch.setenv("SL_GP4_ONE_PANEL", "0")          # (read when the context is created)
    lyap = build_lyapunov(case)
    _, neg_small, rec_small = _engine_records(lyap)
    assert lyap._ctx.last_kernel().startswith("k_gp_small<"), lyap._ctx.last_kernel()
    assert_allclose(rec, rec_small, rtol=1e-9, atol=1e-13)
    _check_masks(neg, neg_small, rec, rec_small, allowed=0)


def test_up_to_224_training_points_stay_on_the_small_kernel(sl):
    """193 ... 224 points: the padded capacity is one 256-row panel, but k_gp_small - which pays for the
    row blocks that hold training points - is the faster kernel (``sl_gp.hip``)."""
    from gp_cases import INFORMED
    from safe_learning_amd.benchmarks import build_lyapunov
    for n_gp in (193, 224):
        lyap = build_lyapunov(cases.make_case("pendulum", num_points=48, n_gp=n_gp, tau_scale=0.01, **INFORMED))
        lyap.update_safe_set()
        assert lyap._ctx.last_kernel().startswith("k_gp_small<"), (n_gp, lyap._ctx.last_kernel())


def test_bounded_streaming_pass_equals_the_plain_one(sl):
    """``sl_lyap_finalize_dev`` with ``can_shrink = True`` and a quadratic V bounds whole spans of a
    row and evaluates one cell of those far above the level (``SlRowValues::span_bounded``); with a
    previous set given (all zeros here: nothing to keep) it evaluates every cell.  Same safe words,
    same record (last safe key, largest key, counters) bit for bit - over row lengths from 8 to 256
    cells, ranges that start and end inside rows, levels from below the minimum to above the maximum
    and matrices that are not positive definite; and both equal NumPy on the exact values."""
    import torch
    from np_shard_engine import np_vbits
    from safe_learning_amd import _hip
    from safe_learning_amd.benchmarks import build_lyapunov
    rng = np.random.default_rng(12)
    shapes = [("1d", dict(num_points=1000)), ("pendulum", dict(num_points=[37, 8], dynamics="linear")),
              ("pendulum", dict(num_points=[33, 136], dynamics="linear")),
              ("pendulum", dict(num_points=[300, 256], dynamics="linear")),
              ("cartpole", dict(num_points=[5, 6, 7, 24], dynamics="linear")),
              ("cartpole", dict(num_points=[9, 8, 12, 128], dynamics="linear"))]
    for name, kw in shapes:
        for trial in range(3):
            case = cases.make_case(name, **kw)
            d = len(case["num_points"])
            if trial:
                A = rng.normal(size=(d, d))
                case["P"] = A @ A.T if trial == 1 else A          # trial 2: indefinite, not symmetric
            lyap = build_lyapunov(case)
            lyap.update_safe_set()                                  # uploads the model and the initial set
            assert lyap._values_implicit
            ctx, dev, n = lyap._ctx, lyap._ctx.torch_device, lyap.discretization.nindex
            values = lyap.values
            keys = np_vbits(values)
            init_words = lyap._d_init.clone()
            init = np.unpackbits(init_words.cpu().numpy().view(np.uint8), bitorder="little")[:n].astype(bool)
            ranges = [(0, n)]
            if n > 4096:
                ranges += [(64 * 3, n - 8 * 5), (64 * int(rng.integers(1, n // 128)), n)]
            picks = [int(np.argmin(values)), int(np.argmax(values))] + [int(j) for j in rng.choice(n, 4)]
            for lo, hi in ranges:
                words = (hi - lo + 63) // 64
                shard_init = None
                if lo == 0:
                    shard_init = init_words
                for star in [(keys[j], j) for j in picks] + [(np.uint64(0), -1), (~np.uint64(0), (1 << 63) - 1)]:
                    folded = torch.zeros(_hip.RESULT_WORDS, dtype=torch.int64, device=dev)
                    folded[_hip.R_FAIL_V] = int(np.uint64(star[0]).view(np.int64))
                    folded[_hip.R_FAIL_I] = int(star[1])
                    outs = []
                    for prev in (None, torch.zeros(words + 1, dtype=torch.int64, device=dev)):
                        safe = torch.full((words + 1,), -1, dtype=torch.int64, device=dev)
                        record = torch.zeros(_hip.RESULT_WORDS, dtype=torch.int64, device=dev)
                        ctx.lyap_finalize_dev(lo, hi, None, shard_init, prev, folded, None, safe, record)
                        outs.append((safe[:words].cpu().numpy(), record.cpu().numpy()))
                    assert_array_equal(outs[0][0], outs[1][0])
                    assert_array_equal(outs[0][1], outs[1][1])
                    # ... and NumPy on the exact values
                    idx = np.arange(lo, hi)
                    below = (keys[lo:hi] < star[0]) | ((keys[lo:hi] == star[0]) & (idx < star[1]))
                    want = below | (init[lo:hi] if shard_init is not None else False)
                    got = np.unpackbits(outs[0][0].view(np.uint8), bitorder="little")[:hi - lo].astype(bool)
                    assert_array_equal(got, want)
                    rec = outs[0][1]
                    assert rec[_hip.R_BELOW] == below.sum() and rec[_hip.R_SAFE] == want.sum()
                    order = np.lexsort((idx, keys[lo:hi]))
                    assert rec[_hip.R_MAX_I] == idx[order[-1]]
                    assert np.uint64(rec[_hip.R_MAX_V].view(np.uint64)) == keys[idx[order[-1]]]
                    if below.any():
                        last = idx[below][np.lexsort((idx[below], keys[lo:hi][below]))[-1]]
                        assert rec[_hip.R_LAST_I] == last


# ---------------------------------------------------------------------------------------------
# three state dimensions: the d = 3 instantiations (the benchmark families are 1-D, 2-D and 4-D)
# ---------------------------------------------------------------------------------------------
# cases.make_case_3d on a 9 x 10 x 16 grid (1440 cells, rows of whole bytes).  On the oracle: linear
# dynamics, tau-scale 0: 1052 cells pass, the level set grows by 770; tau-scale 0.01: 874 pass, it
# grows by 12; 300-point GP: 1006 pass, it grows by 730; 40-point GP: 870 pass, it grows by 481.
@pytest.mark.parametrize("tau_scale,min_growth", [(0.0, 500), (0.01, 10)])
def test_three_dimensions_deterministic_bit_exact(sl, tau_scale, min_growth, monkeypatch):
    """test_deterministic_bit_exact on a 3-D grid: records from k_det_sweep<d=3>, the update's mask
    from k_det_rows<3> and (SL_DET_ROWS=0) from k_det_sweep<false, 3, 1, linear>."""
    from safe_learning_amd.benchmarks import build_lyapunov
    monkeypatch.delenv("SL_DET_ROWS", raising=False)
    case = cases.make_case_3d(dynamics="linear", tau_scale=tau_scale)
    lyap, olyap = build_lyapunov(case), cases.oracle_lyapunov(case)
    assert_array_equal(lyap.values, olyap.values)
    values, neg, rec = _engine_records(lyap)
    assert lyap._ctx.last_kernel().startswith("k_det_sweep<general=0, d=3,"), lyap._ctx.last_kernel()
    ref_rec, ref_neg = _oracle_all(olyap)
    assert_array_equal(values, olyap.values)
    assert_array_equal(rec, ref_rec)
    assert_array_equal(neg, ref_neg)
    _compare_safe_sets(lyap, olyap, 0)
    assert lyap._ctx.last_kernel().startswith("k_det_rows<d=3>"), lyap._ctx.last_kernel()
    _assert_non_degenerate(case, ref_neg, olyap, min_growth)
    monkeypatch.setenv("SL_DET_ROWS", "0")
    cells = build_lyapunov(case)
    assert_array_equal(_neg_mask_of_update(cells), ref_neg)
    assert cells._ctx.last_kernel().startswith("k_det_sweep<general=0, d=3,"), cells._ctx.last_kernel()
    assert_array_equal(cells.safe_set, olyap.safe_set)
    assert cells.c_max == olyap.c_max


def test_three_dimensions_can_shrink_false_and_batches(sl, small_batches):
    """test_can_shrink_false_and_batches on the 3-D grid: quadratic V on rows of whole bytes, so the
    streaming passes (k_select_hist<3>, k_finalize_dev<3>) recompute the keys from the cell index."""
    from safe_learning_amd.benchmarks import build_lyapunov
    case = cases.make_case_3d(dynamics="linear", tau_scale=0.01)
    lyap, olyap = build_lyapunov(case), cases.oracle_lyapunov(case)
    assert lyap._values_implicit
    rng = np.random.default_rng(3)
    sizes = []
    for step in range(4):
        if step == 1:        # pretend earlier verification marked scattered far-away cells safe
            extra = rng.choice(lyap.discretization.nindex, 300, replace=False)
            lyap.safe_set[extra] = True
            olyap.safe_set[extra] = True
        if step == 2:        # a stricter threshold: the safe set may not shrink
            lyap.tau = olyap.tau = case["tau"] * 4
        if step == 3:
            lyap.tau = olyap.tau = 0.0
        lyap.update_safe_set(can_shrink=(step == 0))
        olyap.update_safe_set(can_shrink=(step == 0))
        assert_array_equal(lyap.safe_set, olyap.safe_set)
        assert lyap.c_max == olyap.c_max
        sizes.append(int(olyap.safe_set.sum()))
    # (oracle: 28, 310, 310, 933 safe cells)
    assert sizes[0] > 16 and sizes[1] >= sizes[0] + 200 and sizes[2] == sizes[1] and sizes[3] >= sizes[2] + 500


def test_three_dimensions_refinement_survives_a_plain_update(sl, small_batches):
    """test_refinement_survives_a_plain_update_that_must_not_shrink on the 3-D grid
    (k_refinement_carry<3>)."""
    from safe_learning_amd.benchmarks import build_specs
    case = cases.make_case_3d(dynamics="linear", tau_scale=0.01)
    init = np.zeros(int(np.prod(case["num_points"])), dtype=bool)
    init[cases.initial_safe_mask(case)] = True
    policy, dynamics, value, lv = build_specs(case)
    lyap = sl.Lyapunov(sl.GridWorld(case["limits"], case["num_points"]), value, dynamics, case["lf"],
                       lv, case["tau"], policy, initial_set=init, adaptive=True)
    opolicy, odynamics, ovalue, olv = cases.oracle_specs(case)
    olyap = oracle.Lyapunov(oracle.GridWorld(case["limits"], case["num_points"]), ovalue, odynamics,
                            case["lf"], olv, case["tau"], opolicy, initial_set=init, adaptive=True)
    steps = [dict(can_shrink=True, max_refinement=16, safety_factor=1.5),     # adaptive: some N(x) > 1
             dict(can_shrink=False),                                          # plain, stricter tau
             dict(can_shrink=False),                                          # plain, looser tau
             dict(can_shrink=False, max_refinement=16, safety_factor=1.5),    # adaptive on top of it
             dict(can_shrink=True)]                                           # plain reset: N = safe
    t0 = 0.4 * case["tau"]
    taus = [t0, 1.5 * t0, 0.5 * t0, 0.5 * t0, t0]
    seen_large = False
    for step, tau in zip(steps, taus):
        lyap.tau = olyap.tau = tau
        lyap.update_safe_set(**step)
        olyap.update_safe_set(**step)
        assert_array_equal(lyap.safe_set, olyap.safe_set)
        assert_array_equal(lyap._refinement, olyap._refinement)
        assert lyap.c_max == olyap.c_max
        if "max_refinement" not in step and not step["can_shrink"]:
            seen_large = seen_large or bool((olyap._refinement > 1).any())
    assert seen_large, "no N(x) > 1 was carried through a plain update: the scenario tests nothing"


@pytest.mark.parametrize("n_gp,cfg,kernel", [
    (40, None, "k_gp_small<"),
    (300, None, "k_gp_sweep4<"),
    (300, "3", "k_gp_sweep<"),
])
def test_three_dimensions_gp_dynamics(sl, n_gp, cfg, kernel, monkeypatch):
    """test_gp_dynamics (same comparisons, tolerances and flip allowance) on the 3-D grid, one case
    per GP kernel family."""
    from safe_learning_amd.benchmarks import build_lyapunov
    min_growth = 100
    if cfg is None:
        monkeypatch.delenv("SL_GP_CFG", raising=False)
    else:
        monkeypatch.setenv("SL_GP_CFG", cfg)
    case = cases.make_case_3d(dynamics="gp", n_gp=n_gp, tau_scale=0.0005)
    lyap, olyap = build_lyapunov(case), cases.oracle_lyapunov(case)
    values, neg, rec = _engine_records(lyap)
    ran = lyap._ctx.last_kernel()
    assert ran.startswith(kernel) and "d=3, m=1" in ran and "general=1" not in ran, ran
    ref_rec, ref_neg = _oracle_all(olyap)
    d = case["d"]
    assert_array_equal(values, olyap.values)
    assert_allclose(rec[:, 2:2 + d], ref_rec[:, 2:2 + d], rtol=RTOL_GP, atol=1e-12)   # mean
    assert_allclose(rec[:, 2 + d:], ref_rec[:, 2 + d:], rtol=1e-7, atol=1e-12)        # beta*sigma
    var, ref_var = (rec[:, 2 + d:] / 2.0) ** 2, (ref_rec[:, 2 + d:] / 2.0) ** 2
    assert_allclose(var, ref_var, rtol=1e-6, atol=1e-16)                              # variance
    assert_allclose(rec[:, :2], ref_rec[:, :2], rtol=1e-7, atol=1e-12)
    flips, _ = _check_masks(neg, ref_neg, rec, ref_rec)
    _compare_safe_sets(lyap, olyap, flips, neg)
    ran = lyap._ctx.last_kernel()
    assert ran.startswith(kernel) and "d=3, m=1" in ran and "general=1" not in ran, ran
    _assert_non_degenerate(case, ref_neg, olyap, min_growth)
    if flips == 0:
        init = np.zeros(len(neg), dtype=bool)
        init[cases.initial_safe_mask(case)] = True
        assert int((lyap.safe_set & ~init).sum()) >= min_growth
        assert neg[lyap.safe_set & ~init].all()
