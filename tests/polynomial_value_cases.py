"""The polynomial Lyapunov functions of the polynomial-value tests (host shim, NumPy truth, GPU kernels), with
the conditions on the INPUTS asserted here so that a change of a case cannot hide a failure.  Shared, not a
test module.  The NumPy truth of every spec is ``np_polynomial_value.NumpyPolynomialValue(spec)``.

Specs (``spec(key)``; every one also runs negated, through ``-V``):

* sos / sos-plain: the notebook's sixth-order candidate ``m(z)^T Q m(z)`` (``Q`` and ``state_norm`` from
  tests/golden/reference_sos.npz) with ``z = state_norm * x`` and with ``z = x``;
* quartic4 / quartic4-plain: every monomial of degree 1..4 in four variables (69 terms, 69 + 4 * 35 entries);
* sextic3: every monomial of degree 1..6 in three variables (83 terms, 83 + 3 * 56 entries), normalised;
* const: the single term 2.5;  empty: no term at all (d = 3);  deg8: ``0.75 x^3 y^5 - 1.25 x^8 + x``, normalised.
"""

import functools
import os

import numpy as np

import np_polynomial_value as NPV
import polynomial_cases as PC
from conftest import GOLDEN_DIR
from safe_learning_amd import _hip
from safe_learning_amd import functions as F

KEYS = ("sos", "sos-plain", "quartic4", "quartic4-plain", "sextic3", "const", "empty", "deg8")
POINT_COUNTS = (1, 63, 64, 65, 1000)


@functools.lru_cache(maxsize=None)
def sos_fixture():
    data = np.load(os.path.join(GOLDEN_DIR, "reference_sos.npz"))
    return {k: data[k] for k in data.files}


def all_monomials(d, degree):
    """Every exponent tuple of total degree 1..degree, graded, descending lexicographic inside a degree."""
    return [tuple(int(v) for v in row) for row in NPV.monomial_exponents(d, degree)]


def _dense_terms(d, degree, seed, dyadic=False):
    rng = np.random.default_rng(seed)
    exps = all_monomials(d, degree)
    if dyadic:
        coef = rng.integers(-12, 13, size=len(exps)) / 4.0
    else:
        coef = rng.uniform(-1.0, 1.0, size=len(exps))
    return [(float(c), e) for c, e in zip(coef, exps)]


@functools.lru_cache(maxsize=None)
def spec(key):
    """The engine-side spec of a case."""
    if key in ("sos", "sos-plain"):
        fx = sos_fixture()
        return F.PolynomialFunction.from_gram(fx["Q"], int(fx["degree"]), 2, fx["state_norm"] if key == "sos" else None)
    if key == "quartic4":
        return F.PolynomialFunction(_dense_terms(4, 4, 41), 4, [1.5, 2.0, 0.5, 1.25])
    if key == "quartic4-plain":
        return F.PolynomialFunction(_dense_terms(4, 4, 41), 4)
    if key == "sextic3":
        return F.PolynomialFunction(_dense_terms(3, 6, 63), 3, [0.75, 1.5, 1.1])
    if key == "const":
        return F.PolynomialFunction([(2.5, (0, 0))], 2)
    if key == "empty":
        return F.PolynomialFunction([], 3)
    if key == "deg8":
        return F.PolynomialFunction([(0.75, (3, 5)), (-1.25, (8, 0)), (1.0, (1, 0))], 2, [1.25, 0.9])
    raise KeyError(key)


@functools.lru_cache(maxsize=None)
def truth(key, negate=False):
    t = NPV.NumpyPolynomialValue(spec(key))
    return -t if negate else t


def check_specs():
    """Input-side conditions on the specs themselves."""
    q4, s3 = spec("quartic4"), spec("sextic3")
    assert len(q4.terms) == 69 and len(s3.terms) == 83
    assert 69 + 4 * 35 == len(q4.terms) + sum(1 for _, e in q4.terms for v in e if v) <= _hip.POLYV_MAX_ENTRIES
    assert 83 + 3 * 56 == len(s3.terms) + sum(1 for _, e in s3.terms for v in e if v) <= _hip.POLYV_MAX_ENTRIES
    assert max(sum(e) for _, e in q4.terms) == 4 and max(sum(e) for _, e in s3.terms) == 6
    assert q4.normalization is not None and spec("quartic4-plain").normalization is None
    sos = spec("sos")
    assert len(sos.terms) == 27 - 2 and max(sum(e) for _, e in sos.terms) == 6 and min(sum(e) for _, e in sos.terms) == 2
    assert spec("empty").terms == [] and spec("const").terms == [(2.5, (0, 0))]
    assert max(sum(e) for _, e in spec("deg8").terms) == _hip.POLY_MAX_DEGREE


def points(key, n, seed=5):
    """``n`` seeded states in [-1, 1]^d with, from 16 points on, signed zeros, subnormals, infinities, NaN and
    a value whose powers overflow: ordinary IEEE values that must come through."""
    d = spec(key).input_dim
    x = np.random.default_rng(seed + 7 * n + d).uniform(-1.0, 1.0, size=(n, d))
    if n >= 16:
        x[2, :] = 1e200
        x[3, 0] = np.nan
        x[4, -1] = np.inf
        x[5, 0] = -np.inf
        x[6, :] = -0.0
        x[7, :] = 0.0
        x[8, 0] = 5e-324
        x[9, -1] = -2.5e-310
        x[10, :] = 1e-160                     # its square is subnormal, its cube zero
        x[11, 0], x[11, -1] = np.inf, 0.0     # inf * 0
    return x


# ---- exactness -----------------------------------------------------------------------------------------------
EXACT = {
    # key -> (d, degree, normalization): dyadic coefficients k / 4, |k| <= 12; dyadic scales
    "quartic4": (4, 4, None),
    "quartic4-norm": (4, 4, [2.0, 0.5, 1.0, 0.25]),
    "sextic3": (3, 6, None),
    "sextic3-norm": (3, 6, [0.5, 2.0, 1.0]),
}


def exact_case(key):
    d, degree, norm = EXACT[key]
    return _dense_terms(d, degree, 1000 + d * degree, dyadic=True), d, norm


def exact_points(d, n=200, seed=3):
    """Multiples of 1/8 in [-2, 2]^d."""
    return np.random.default_rng(seed + d).integers(-16, 17, size=(n, d)) / 8.0


def fraction_value_and_gradient(terms, d, norm, x):
    """V and dV/dx of one point in exact rational arithmetic."""
    from fractions import Fraction
    z = [Fraction(float(v)) * (Fraction(float(norm[q])) if norm is not None else 1) for q, v in enumerate(x)]
    value, grad = Fraction(0), [Fraction(0)] * d
    for c, e in terms:
        prod = Fraction(float(c))
        for q in range(d):
            prod *= z[q] ** e[q]
        value += prod
        for k in range(d):
            if e[k] >= 1:
                g = Fraction(float(c)) * e[k]
                for q in range(d):
                    g *= z[q] ** (e[q] - (1 if q == k else 0))
                grad[k] += g * (Fraction(float(norm[k])) if norm is not None else 1)
    return value, grad


# ---- Lyapunov verification -------------------------------------------------------------------------------------
QUARTIC_C = 0.5


def quartic_terms(P, c):
    """V = x^T P x + c (sum_q x_q^4 + x_0^2 x_1^2) as a term table: the quadratic part one term per pair
    i <= j (P_ii, P_ij + P_ji), then the quartic part."""
    d = len(P)
    terms = []
    for i in range(d):
        for j in range(i, d):
            e = [0] * d
            e[i] += 1
            e[j] += 1
            terms.append((float(P[i, i]) if i == j else float(P[i, j] + P[j, i]), tuple(e)))
    for q in range(d):
        e = [0] * d
        e[q] = 4
        terms.append((float(c), tuple(e)))
    e = [0] * d
    e[0], e[1] = 2, 2
    terms.append((float(c), tuple(e)))
    return terms


# linear4: an open loop of spectral radius 0.99 under a saturated linear policy (closed loop 0.96 where the
# policy is not saturated): the quartic V decreases on part of [-1, 1]^4 only
LINEAR4_A = np.array([[0.99, 0.22, 0.0, 0.0],
                      [-0.22, 0.935, 0.11, 0.0],
                      [0.0, -0.11, 0.88, 0.275],
                      [0.055, 0.0, -0.275, 0.99]])
LINEAR4_B = np.array([[0.0], [0.1], [0.0], [0.2]])
LINEAR4_K = np.array([[0.203, -0.257, -0.115, -1.221]])
LINEAR4_SATURATION = 0.4

# key -> (grid limits, points per axis, radius of the initial set)
LYAPUNOV = dict(PC.LYAPUNOV)
LYAPUNOV["linear4"] = ("linear4", [[-1, 1]] * 4, [9, 9, 9, 9], 0.3)
# tau > 0 of a case: large enough to take cells out of the tau = 0 safe set, small enough to leave some
TAU = {"vdp": 0.002, "vdp-pow2": 0.002, "chain3": 0.01, "linear4": 0.004}
# (L_v mode, tau > 0?): tau = 0 makes the threshold 0 whatever L_v is
MODES = (("norm1", False), ("norm1", True), ("abs", True))
LF = 0.5


def lyapunov_matrix(key):
    if key == "linear4":
        import scipy.linalg
        closed = LINEAR4_A + LINEAR4_B.dot(LINEAR4_K)
        assert np.abs(np.linalg.eigvals(closed)).max() < 1.0
        return scipy.linalg.solve_discrete_lyapunov(closed.T, np.eye(4))
    return PC.lyapunov_matrix(key)


@functools.lru_cache(maxsize=None)
def lyapunov_value(key):
    """The engine-side V of a Lyapunov case."""
    P = lyapunov_matrix(key)
    return F.PolynomialFunction(quartic_terms(P, QUARTIC_C), len(P))


def engine_pair(key):
    """(dynamics, policy) specs of the engine."""
    if key == "linear4":
        return (F.LinearSystem((LINEAR4_A, LINEAR4_B)),
                F.Saturation(F.LinearSystem((LINEAR4_K,)), -LINEAR4_SATURATION, LINEAR4_SATURATION))
    name = LYAPUNOV[key][0]
    return PC.system(name), PC.engine_policy(name)


def oracle_pair(key):
    import oracle
    if key == "linear4":
        return (oracle.LinearSystem((LINEAR4_A, LINEAR4_B)),
                oracle.Saturation(oracle.LinearSystem((LINEAR4_K,)), -LINEAR4_SATURATION, LINEAR4_SATURATION))
    name = LYAPUNOV[key][0]
    return PC.truth(name), PC.oracle_policy(name)


def engine_lv(sl, value, mode):
    return sl.Norm1Function(sl.Gradient(value)) if mode == "norm1" else sl.AbsGradient(value)


def check_oracle(olyap, initial, value, dynamics, policy, what):
    """The conditions every mask comparison rests on, on the oracle side: a safe set strictly between the
    initial set and the grid, and no cell off the initial set whose V changes by less than 1e-6 relative."""
    grid = olyap.discretization
    x = grid.all_points
    nxt = dynamics(x, policy(x))
    if isinstance(nxt, tuple):
        nxt = nxt[0]
    vx = np.asarray(value(x)).ravel()
    change = np.asarray(value(nxt)).ravel() - vx
    off = ~initial
    relative = (np.abs(change[off]) / vx[off]).min()
    print("polynomial V, %s: %d initial cells, %d of %d safe, smallest relative change off the initial set %.3g, "
          "c_max %.10g" % (what, initial.sum(), olyap.safe_set.sum(), grid.nindex, relative, olyap.c_max))
    assert np.isfinite(nxt).all() and relative > 1e-6, relative
    assert initial.sum() < olyap.safe_set.sum() < grid.nindex
    return relative


@functools.lru_cache(maxsize=None)
def lyapunov_truth(key, mode="norm1", tau=0.0):
    """The oracle's ``Lyapunov`` with the NumPy restatement as V and L_v, after ``update_safe_set`` ->
    (oracle object, initial set)."""
    import oracle
    _, limits, num_points, radius = LYAPUNOV[key]
    grid = oracle.GridWorld(limits, num_points)
    initial = np.linalg.norm(grid.all_points, axis=1) <= radius
    value = NPV.NumpyPolynomialValue(lyapunov_value(key))
    dynamics, policy = oracle_pair(key)
    lv = value.norm1_gradient if mode == "norm1" else value.abs_gradient
    olyap = oracle.Lyapunov(grid, value, dynamics, LF, lv, tau, policy, initial_set=initial.copy())
    olyap.update_safe_set()
    relative = check_oracle(olyap, initial, value, dynamics, policy, "%s, L_v %s, tau %g" % (key, mode, tau))
    if tau > 0.0:
        zero = lyapunov_truth(key, mode, 0.0)[0]
        assert olyap.safe_set.sum() < zero.safe_set.sum()              # the threshold decides cells
    if tau == 0.0:
        # what the issue's table records for c = 0.5; the safe sets differ from the quadratic's alone
        if key == "vdp":
            assert (initial.sum(), olyap.safe_set.sum(), grid.nindex) == (21, 467, 2601) and 1.5e-4 < relative < 1.7e-4
        if key == "chain3":
            assert (initial.sum(), olyap.safe_set.sum(), grid.nindex) == (2, 221, 990) and 3.7e-4 < relative < 3.9e-4
    return olyap, initial


# ---- the notebook's candidate on the notebook's system -----------------------------------------------------------
PENDULUM = dict(mass=0.15, length=0.5, friction=0.1, dt=0.01)


def notebook_norms():
    state_norm = sos_fixture()["state_norm"]
    u_max = 9.81 * PENDULUM["mass"] * PENDULUM["length"] * np.sin(np.deg2rad(60))
    return [list(state_norm), [u_max]]


def notebook_system(ns):
    """(dynamics, saturated LQR policy) of the notebook from the classes of ``ns`` (``oracle`` or the engine)."""
    from safe_learning_amd.utilities import dlqr
    dyn = ns.InvertedPendulum(PENDULUM["mass"], PENDULUM["length"], PENDULUM["friction"], PENDULUM["dt"],
                              notebook_norms())
    A, B = dyn.linearize()
    K, _ = dlqr(A, B, np.eye(2), np.eye(1))                      # cell 11
    return dyn, ns.Saturation(ns.LinearSystem((-K,)), -1, 1)


@functools.lru_cache(maxsize=None)
def notebook_truth(num_points):
    """The oracle's ``Lyapunov`` of the notebook's system under the SOS candidate, tau = 0, the notebook's
    initial set (cell 9: a ball of radius 0.1) -> (oracle object, initial set)."""
    import oracle
    grid = oracle.GridWorld([[-1, 1]] * 2, num_points)
    initial = np.linalg.norm(grid.all_points, ord=2, axis=1) <= 0.1
    value = truth("sos")
    dynamics, policy = notebook_system(oracle)
    olyap = oracle.Lyapunov(grid, value, dynamics, LF, value.norm1_gradient, 0.0, policy, initial_set=initial.copy())
    olyap.update_safe_set()
    relative = check_oracle(olyap, initial, value, dynamics, policy, "notebook, %d^2" % num_points)
    # what the issue records
    if num_points == 51:
        assert (initial.sum(), olyap.safe_set.sum(), grid.nindex) == (21, 129, 2601)
        assert abs(olyap.c_max - 3.0391805839) < 1e-9 and 4.0e-5 < relative < 4.2e-5
    if num_points == 101:
        assert (initial.sum(), olyap.safe_set.sum(), grid.nindex) == (75, 439, 10201) and 9.7e-6 < relative < 9.9e-6
    return olyap, initial


def same_bits(a, b):
    return PC.same_bits(a, b)


assert_same_bits = PC.assert_same_bits


# ---- GP dynamics ---------------------------------------------------------------------------------------------------
GP_QUARTIC_C = 0.5


def gp_case(kind):
    """-> (case, engine dynamics, oracle dynamics): ``rbf`` is the smallest plain-RBF case of tests/gp_cases.py
    (pendulum, 40^2 cells, 3 observations), ``notebook`` its smallest ``Linear + Matern32 x Linear`` case
    (65 x 48 cells, 40 observations)."""
    import cases
    import gp_cases
    import oracle
    import safe_learning_amd as sl
    from safe_learning_amd.benchmarks import build_specs
    if kind == "rbf":
        family, kw, _, _ = gp_cases.GP_CASES[0]
        assert (family, kw["num_points"], kw["n_gp"]) == ("pendulum", 40, 3)
        case = cases.make_case(family, **kw)
        return case, build_specs(case)[1], cases.oracle_specs(case)[1]
    spec = gp_cases.kernel_case_list()[0]
    assert spec["name"] == "notebook_n40"
    fixture = np.load(os.path.join(GOLDEN_DIR, "reference_gp_kernels.npz"))
    case = gp_cases.kernel_build_case(spec)
    return case, gp_cases.kernel_model(sl, spec, case, fixture), gp_cases.kernel_model(oracle, spec, case, fixture)


def gp_lyapunovs(kind):
    """(engine Lyapunov, oracle Lyapunov, initial mask) of a GP case under the quartic V with
    ``L_v = AbsGradient(V)``; the oracle-side conditions are asserted."""
    import cases
    import oracle
    import safe_learning_amd as sl
    from safe_learning_amd.benchmarks import build_specs, initial_safe_mask
    case, dynamics, odynamics = gp_case(kind)
    policy = build_specs(case)[0]
    opolicy = cases.oracle_specs(case)[0]
    value = F.PolynomialFunction(quartic_terms(np.asarray(case["P"]), GP_QUARTIC_C), case["d"])
    ovalue = NPV.NumpyPolynomialValue(value)
    initial = np.zeros(int(np.prod(case["num_points"])), dtype=bool)
    initial[initial_safe_mask(case)] = True
    lyap = sl.Lyapunov(sl.GridWorld(case["limits"], case["num_points"]), value, dynamics, case["lf"],
                       sl.AbsGradient(value), case["tau"], policy, initial_set=initial.copy())
    olyap = oracle.Lyapunov(oracle.GridWorld(case["limits"], case["num_points"]), ovalue, odynamics, case["lf"],
                            ovalue.abs_gradient, case["tau"], opolicy, initial_set=initial.copy())
    return lyap, olyap, initial, (ovalue, odynamics, opolicy)


def check_gp_oracle(olyap, initial, ref_rec, ref_neg, parts, what):
    """Non-degenerate, no cell off the initial set with a relative change of V below 1e-6, and no cell within
    1e-7 relative of the threshold (so that not one mask bit may differ)."""
    ovalue, odynamics, opolicy = parts
    olyap.update_safe_set()
    check_oracle(olyap, initial, ovalue, odynamics, opolicy, what)
    margin = np.abs(ref_rec[:, 0] - ref_rec[:, 1]) / np.maximum(np.maximum(np.abs(ref_rec[:, 0]), np.abs(ref_rec[:, 1])),
                                                               1e-300)
    print("%s: smallest relative distance from the threshold %.3g, %d of %d cells negative"
          % (what, margin.min(), ref_neg.sum(), len(ref_neg)))
    assert margin.min() > 1e-7 and ref_neg.any() and not ref_neg.all()
