"""CPU checks of the polynomial Lyapunov function (safe_learning_amd/csrc/sl_poly_value.h).

The header is compiled with g++ into a test-only shim (tests/hostsim/poly_value.cpp) and compared BIT FOR BIT
with the NumPy restatement (tests/np_polynomial_value.py): the arithmetic is multiplications and additions in
one stated order, without contraction, so there is nothing to round differently.  The restatement in turn is
held against exact rational arithmetic and against a run of the reference's own functions
(tests/golden/reference_sos.npz).  The GPU tests (tests/test_gpu_polynomial_value.py) repeat the bit
comparisons through the kernels.
"""

import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import hostsim_build
import np_polynomial_value as NPV
import polynomial_value_cases as PVC
from conftest import GOLDEN_DIR, ROOT
from safe_learning_amd import _hip
from safe_learning_amd import functions as F
from safe_learning_amd._model import ModelBuilder


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return hostsim_build.shared("poly_value.cpp", tmp_path_factory.mktemp("poly_value"), hostsim_build.SHIM_FLAGS)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _table_arguments(spec):
    coef = np.ascontiguousarray(spec._coef, dtype=np.float64)
    expo = np.zeros((len(coef), _hip.MAX_STATE_DIM), dtype=np.uint8)
    expo[:, :spec.input_dim] = spec._expo
    tx = np.ones(_hip.MAX_STATE_DIM)
    if spec.normalization is not None:
        tx[:spec.input_dim] = spec.normalization
    return coef, expo, 0 if spec.normalization is None else 1, tx


def _shim_eval(shim, spec, states, negate=None):
    coef, expo, normalize, tx = _table_arguments(spec)
    states = np.ascontiguousarray(states, dtype=np.float64)
    n, d = states.shape
    value, grad = np.full(n, np.nan), np.full((n, d), np.nan)
    rc = shim.polyv_eval(d, len(coef), _p(coef), _p(expo), normalize, _p(tx), int(spec.negate if negate is None else negate),
                         C.c_int64(n), _p(states), _p(value), _p(grad))
    assert rc == 0
    return value[:, None], grad


# ---- 1. the header against the restatement, bit for bit ---------------------------------------------------------
@pytest.mark.parametrize("negate", [False, True])
@pytest.mark.parametrize("key", PVC.KEYS)
def test_header_equals_restatement_bit_for_bit(shim, key, negate):
    PVC.check_specs()
    spec = -PVC.spec(key) if negate else PVC.spec(key)
    assert spec.negate == negate
    truth = NPV.NumpyPolynomialValue(spec)
    for n in PVC.POINT_COUNTS:
        x = PVC.points(key, n)
        value, grad = _shim_eval(shim, spec, x)
        PVC.assert_same_bits(value, truth(x), "%s V, %d points" % (key, n))
        PVC.assert_same_bits(grad, truth.gradient(x), "%s gradient, %d points" % (key, n))
    x = PVC.points(key, 1000)
    with np.errstate(all="ignore"):
        v = truth(x)
    if key not in ("const", "empty"):
        assert np.isnan(v).any() and (~np.isfinite(v)).sum() >= 4 and np.isfinite(v).sum() > 900   # the special rows bite
    if key == "empty":
        assert not v.any() and np.array_equal(np.signbit(v), np.full(v.shape, negate))     # +0.0, or -0.0 negated
    if key == "const":
        assert np.array_equal(v, np.full(v.shape, -2.5 if negate else 2.5)) and not truth.gradient(x).any()


def test_table_builder_program(tmp_path):
    """The table builder and a few hand-computed values in the header's own program, under the address and
    undefined-behaviour sanitizers where the toolchain has them."""
    exe = hostsim_build.sanitized_program_or_plain("poly_value.cpp", tmp_path, hostsim_build.SHIM_FLAGS)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout


def test_uploaded_table_is_the_spec(shim):
    """What the model builder hands to ``sl_value_polynomial_set`` and how the header lays it out: value
    row in the caller's order, then the gradient rows (coefficient c * e_k, exponent e_k - 1)."""
    class Recording(object):
        def __init__(self):
            self.tables = []

        def model_set(self, desc):
            self.desc = desc

        def value_polynomial_set(self, d, coef, exponents, normalization=None):
            self.tables.append((d, np.array(coef), np.array(exponents), normalization))

    spec = PVC.spec("deg8")
    ctx = Recording()
    builder = ModelBuilder(ctx, F.GridWorld([[0., 1.]] * 2, 2))
    policy, dynamics = F.LinearSystem((np.zeros((1, 2)),)), F.LinearSystem((np.eye(2), np.zeros((2, 1))))
    builder.upload(policy, dynamics, -spec, F.Norm1Function(F.Gradient(spec)))
    assert (ctx.desc.value.kind, ctx.desc.value.negate, ctx.desc.lipschitz.lv_kind) == (_hip.V_POLYNOMIAL, 1,
                                                                                       _hip.LIP_NORM_GRAD)
    builder.upload(policy, dynamics, spec, F.AbsGradient(spec))                # the same table: no second upload
    assert len(ctx.tables) == 1 and ctx.desc.value.negate == 0 and ctx.desc.lipschitz.lv_kind == _hip.LIP_ABS_GRAD
    builder.upload(policy, dynamics, PVC.spec("const"), 0.5)                    # a new table
    assert len(ctx.tables) == 2 and ctx.desc.lipschitz.lv_kind == _hip.LIP_CONST
    d, coef, expo, norm = ctx.tables[0]
    assert d == 2 and coef.tolist() == [0.75, -1.25, 1.0] and expo.tolist() == [[3, 5], [8, 0], [1, 0]]
    assert_array_equal(norm, [1.25, 0.9])
    coef, expo, normalize, tx = _table_arguments(spec)
    row_start = np.zeros(_hip.MAX_STATE_DIM + 2, dtype=np.int32)
    out_coef, out_expo = np.zeros(_hip.POLYV_MAX_ENTRIES), np.zeros(_hip.POLYV_MAX_ENTRIES, dtype=np.uint64)
    assert shim.polyv_build(2, 3, _p(coef), _p(expo), normalize, _p(tx), _p(row_start), _p(out_coef), _p(out_expo),
                            None) == 0
    assert row_start.tolist() == [0, 3, 6, 7, 7, 7, 7, 7]
    assert out_coef[:7].tolist() == [0.75, -1.25, 1.0, 0.75 * 3, -1.25 * 8, 1.0, 0.75 * 5]
    assert out_expo[:7].tolist() == [0x0503, 0x0008, 0x0001, 0x0502, 0x0007, 0x0000, 0x0403]
    rows = NPV.gradient_rows(spec.terms, 2)
    assert rows == [[(2.25, (2, 5)), (-10.0, (7, 0)), (1.0, (0, 0))], [(3.75, (3, 4))]]


def test_from_gram_and_the_basis():
    """``from_gram`` against the restatement's expansion, and against the Gram form itself."""
    assert F.monomial_exponents(2, 3).tolist() == [[1, 0], [0, 1], [2, 0], [1, 1], [0, 2], [3, 0], [2, 1], [1, 2], [0, 3]]
    for d, degree in ((1, 4), (2, 3), (3, 2), (4, 2), (6, 1)):
        assert_array_equal(F.monomial_exponents(d, degree), NPV.monomial_exponents(d, degree))
    assert F.monomial_exponents(3, 2).tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 1], [2, 0, 0], [1, 1, 0], [1, 0, 1],
                                                   [0, 2, 0], [0, 1, 1], [0, 0, 2]]
    rng = np.random.default_rng(12)
    for d, degree in ((2, 3), (3, 2), (4, 1)):
        n = len(F.monomial_exponents(d, degree))
        Q = rng.normal(size=(n, n))                                           # not symmetric, not definite
        spec = F.PolynomialFunction.from_gram(Q, degree, d)
        assert spec.terms == NPV.gram_terms(Q, degree, d)
        exps = [e for _, e in spec.terms]
        assert len(set(exps)) == len(exps)                                    # one term per distinct monomial
        x = rng.uniform(-1, 1, size=(50, d))
        m = np.prod(x[:, None, :] ** F.monomial_exponents(d, degree)[None, :, :], axis=2)
        np.testing.assert_allclose(NPV.NumpyPolynomialValue(spec)(x)[:, 0], np.einsum("ni,ij,nj->n", m, Q, m),
                                   rtol=1e-12, atol=1e-12)
    # first appearance over (i, j) row-major, summed in that order: x * x, then x * y and y * x
    spec = F.PolynomialFunction.from_gram([[1.0, 0.1], [0.2, 3.0]], 1, 2)
    assert spec.terms == [(1.0, (2, 0)), (0.1 + 0.2, (1, 1)), (3.0, (0, 2))]
    with pytest.raises(ValueError, match="9 monomials"):
        F.PolynomialFunction.from_gram(np.eye(8), 3, 2)


# ---- 2. exactness -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(PVC.EXACT))
def test_exact_against_rational_arithmetic(shim, key):
    """Dyadic coefficients, dyadic scales and points on multiples of 1/8 in [-2, 2]^d: every product and sum
    is exact in double up to degree 6, so value and gradient EQUAL the rational evaluation - which pins the
    gradient rows (coefficients c e_k, reduced exponents, chain factor) without a tolerance."""
    from fractions import Fraction
    terms, d, norm = PVC.exact_case(key)
    assert max(sum(e) for _, e in terms) <= 6 and all(c * 4 == int(c * 4) for c, _ in terms)
    spec = F.PolynomialFunction(terms, d, norm)
    truth = NPV.NumpyPolynomialValue(spec)
    x = PVC.exact_points(d)
    assert np.array_equal(x * 8, np.round(x * 8)) and np.abs(x).max() == 2.0
    value, grad = truth(x), truth.gradient(x)
    shim_value, shim_grad = _shim_eval(shim, spec, x)
    differs = 0
    for i in range(len(x)):
        want_value, want_grad = PVC.fraction_value_and_gradient(terms, d, norm, x[i])
        assert Fraction(float(value[i, 0])) == want_value and Fraction(float(shim_value[i, 0])) == want_value
        for k in range(d):
            assert Fraction(float(grad[i, k])) == want_grad[k] and Fraction(float(shim_grad[i, k])) == want_grad[k]
        differs += any(g != 0 for g in want_grad)
    assert differs > 190                                                     # gradients that say something
    neg_value, neg_grad = _shim_eval(shim, spec, x, negate=1)
    assert np.array_equal(neg_value, -value) and np.array_equal(neg_grad, -grad)


# ---- 3. the reference's own functions --------------------------------------------------------------------------
def test_restatement_against_the_reference_run():
    fx = PVC.sos_fixture()
    Q, T = fx["Q"], fx["state_norm"]
    assert Q.shape == (9, 9) and np.linalg.eigvalsh((Q + Q.T) / 2).min() < -0.02      # not definite as printed
    # the basis is the reference's monomials(x, 3), column for column
    assert_array_equal(F.monomial_exponents(2, 3), fx["exponents"])
    truth = PVC.truth("sos")
    basis = F.monomial_exponents(2, 3).astype(np.float64)
    u = 2.0 ** -53
    for key in ("states", "grid"):
        x = fx[key if key == "states" else "grid_points"]
        assert len(x) == (500 if key == "states" else 41 * 41) and np.abs(x).max() <= 1.0
        z = x * T
        m = np.abs(np.prod(z[:, None, :] ** basis[None, :, :], axis=2))                    # |m_i|
        # 128 roundings is more than either evaluation order has on any path; the sum is the condition of the
        # cancellation
        bound = 128 * u * np.einsum("ni,ij,nj->n", m, np.abs(Q), m)
        error = np.abs(truth(x)[:, 0] - fx["value_" + key][:, 0])
        print("SOS value, %s: largest error / bound %.3g" % (key, (error / np.maximum(bound, 1e-300)).max()))
        assert (error <= bound).all()
        # gradient: |d m_j / d z_k|, the reference's derivative multiplied by T_k - and by 2: its
        # lyapunov_sos_derivative returns (m^T Q) dm/dz, one of the two equal halves of d(m^T Q m)/dz for the
        # symmetric Q it is given (the notebook reads only the sign of dV/dt); central differences of the
        # fixture's own values confirm the factor below
        assert np.array_equal(Q, Q.T)
        got = truth.gradient(x)
        for k in range(2):
            reduced = basis.copy()
            reduced[:, k] = np.maximum(reduced[:, k] - 1, 0)
            dm = basis[None, :, k] * np.abs(np.prod(z[:, None, :] ** reduced[None, :, :], axis=2))
            gbound = 128 * u * (np.einsum("ni,ij,nj->n", m, np.abs(Q), dm) + np.einsum("ni,ij,nj->n", dm, np.abs(Q), m))
            gbound = gbound * T[k]
            gerror = np.abs(got[:, k] - 2.0 * fx["dvdz_" + key][:, k] * T[k])
            print("SOS gradient %d, %s: largest error / bound %.3g" % (k, key, (gerror / np.maximum(gbound, 1e-300)).max()))
            assert (gerror <= gbound).all()
        assert np.abs(got).max() > 1.0 and truth(x).max() > 10.0
        if key == "grid":
            # the factor 2, from the reference's VALUES: central differences along the first axis of the grid
            n, h = int(fx["grid_num_points"]), 2.0 / (int(fx["grid_num_points"]) - 1)
            v = fx["value_grid"].reshape(n, n)
            central = ((v[2:, :] - v[:-2, :]) / (2 * h))[:, 1:-1].ravel()
            ref = (2.0 * fx["dvdz_grid"][:, 0] * T[0]).reshape(n, n)[1:-1, 1:-1].ravel()
            big = np.abs(ref) > 0.1 * np.abs(ref).max()
            assert np.abs(central[big] / ref[big] - 1.0).max() < 0.1


# ---- 4. constructor errors --------------------------------------------------------------------------------------
def test_constructor_errors_name_the_limit():
    with pytest.raises(ValueError, match="3 exponents, input_dim = 2"):
        F.PolynomialFunction([(1.0, (1, 0, 0))], 2)
    with pytest.raises(ValueError, match="negative exponent"):
        F.PolynomialFunction([(1.0, (1, -1))], 2)
    with pytest.raises(ValueError, match="non-integer exponent"):
        F.PolynomialFunction([(1.0, (1, 0.5))], 2)
    F.PolynomialFunction([(1.0, (1.0, 2.0))], 2)                                   # integral floats are integers
    with pytest.raises(ValueError, match="total degree 9.*POLY_MAX_DEGREE = 8"):
        F.PolynomialFunction([(1.0, (4, 5))], 2)
    F.PolynomialFunction([(1.0, (4, 4))], 2)
    with pytest.raises(ValueError, match="MAX_STATE_DIM = 6"):
        F.PolynomialFunction([], 7)
    with pytest.raises(ValueError, match="normalization holds 3 scales"):
        F.PolynomialFunction([], 2, [1.0, 2.0, 3.0])
    # the device table: a full quartic in four states fits (209 entries), a full quintic does not
    quintic = [(1.0, e) for e in PVC.all_monomials(4, 5)]
    with pytest.raises(ValueError, match="POLYV_MAX_ENTRIES = 256"):
        F.PolynomialFunction(quintic, 4)
    F.PolynomialFunction([(1.0, e) for e in PVC.all_monomials(4, 4)], 4)
    F.PolynomialFunction([(1.0, (0, 0))] * 256, 2)                                 # constants: no gradient entries
    with pytest.raises(ValueError, match="POLYV_MAX_ENTRIES"):
        F.PolynomialFunction([(1.0, (0, 0))] * 255 + [(1.0, (1, 1))], 2)
    # a grid of another dimension, before anything is uploaded
    builder = ModelBuilder(None, F.GridWorld([[-1, 1]] * 3, 3))
    with pytest.raises(ValueError, match="takes 2 inputs, the grid has 3 dimensions"):
        builder._write_value(_hip.ValueDesc(), PVC.spec("sos"))
    with pytest.raises(TypeError, match="PolynomialFunction"):
        builder._write_value(_hip.ValueDesc(), object())
    # refusals that need no device
    with pytest.raises(NotImplementedError, match="polynomial_function.*reward_function"):
        builder.upload(F.LinearSystem((np.zeros((1, 3)),)), F.LinearSystem((np.eye(3), np.zeros((3, 1)))),
                       F.QuadraticFunction(np.eye(3)), reward=F.PolynomialFunction([], 3))


def test_lipschitz_specs_accepted_and_refused():
    """``AbsGradient(V)`` and ``Norm1Function(Gradient(V))`` are the two gradient forms of L_v; a bare ``Gradient(V)``
    is refused by name with the two forms, and a gradient of another function than V is refused too."""
    V, W = PVC.spec("sos"), PVC.spec("sos-plain")
    table = F.Triangulation(F.GridWorld([[-1, 1]] * 2, 3), np.zeros((9, 1)))
    builder = ModelBuilder(None, F.GridWorld([[-1, 1]] * 2, 5))
    for lv, kind in ((F.AbsGradient(V), _hip.LIP_ABS_GRAD), (F.AbsFunction(F.Gradient(-V)), _hip.LIP_ABS_GRAD),
                     (F.Norm1Function(F.Gradient(V)), _hip.LIP_NORM_GRAD), (0.25, _hip.LIP_CONST),
                     (F.Norm1Function(F.LinearSystem((np.eye(2),))), _hip.LIP_NORM_LINEAR)):
        desc = _hip.LipschitzDesc()
        builder._write_lipschitz(desc, lv, 0.5, 0.0, V)
        assert desc.lv_kind == kind
    with pytest.raises(TypeError, match=r"bare Gradient\(V\) \(of a PolynomialFunction\).*AbsGradient\(V\).*"
                                        r"Norm1Function\(Gradient\(V\)\)"):
        builder._write_lipschitz(_hip.LipschitzDesc(), F.Gradient(V), 0.5, 0.0, V)
    with pytest.raises(TypeError, match=r"bare Gradient\(V\) \(of a Triangulation\)"):
        builder._write_lipschitz(_hip.LipschitzDesc(), F.Gradient(table), 0.5, 0.0, table)
    # the gradient of another function than the Lyapunov function
    for source, value in ((W, V), (table, V), (V, table), (V, F.QuadraticFunction(np.eye(2)))):
        with pytest.raises(ValueError, match="must be built on the Lyapunov function itself"):
            builder._write_lipschitz(_hip.LipschitzDesc(), F.AbsGradient(source), 0.5, 0.0, value)
    builder._write_lipschitz(_hip.LipschitzDesc(), F.AbsGradient(table), 0.5, 0.0, table)      # tables: as before


def test_roa_classification_refuses_a_subclass_by_name(monkeypatch):
    from safe_learning_amd import training

    class Mine(F.PolynomialFunction):
        pass

    class Holder(object):
        lyapunov_function = Mine([(1.0, (2, 0))], 2, name="mine")

    monkeypatch.setattr(training, "_check_single_process", lambda: None)
    with pytest.raises(NotImplementedError, match="roa_classification_step.*PolynomialFunction \\(mine\\)"):
        training.roa_classification_step(Holder(), np.zeros((3, 2)), np.ones(3), np.ones(3), 1.0, 1.0, 0.01)


# ---- 5. kernel resources against the parent commit --------------------------------------------------------------
def test_existing_kernels_keep_their_resources():
    """No kernel that existed before this feature changed its registers, scratch or LDS - except
    ``k_eval_simple``, the one kernel the feature edits (profiles/polynomial_value.md has its numbers) - and every
    new kernel is free of scratch.

    Both sides are the AMDGPU metadata of the code objects (``tools/kernel_resources.py``): SGPRs, the unified
    VGPR count, AGPRs, scratch, LDS - what the compiler's ``kernel-resource-usage`` remarks report
    (``tools/resource_summary.sh``), as recorded in the library, so that the comparison needs no second
    compilation inside a test.  This build: the library, brought up to date with the sources first (a no-op where
    ``build()`` has run).  The parent: tests/golden/kernel_resources_parent.json, the figures of a build of the
    commit this feature was made on.

    Refreshing the file: it states the baseline of ONE change.  The next change that moves a register on purpose,
    or retires a kernel, builds ITS parent commit (``git worktree add DIR HEAD~ && python -m safe_learning_amd._build``
    there), runs ``python tools/kernel_resources.py DIR/safe_learning_amd/libslhip.so --json
    tests/golden/kernel_resources_parent.json`` and names the kernels it edits in EDITED below; a change that only
    adds kernels passes as it is (a kernel the file does not know must be free of scratch, nothing else)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from safe_learning_amd._build import build
    build()                                                   # up to date with the sources, or rebuilt
    with open(os.path.join(GOLDEN_DIR, "kernel_resources_parent.json")) as handle:
        parent = json.load(handle)
    now = kernel_resources.resources(_hip.LIB_PATH)
    EDITED = ("_Z13k_eval_simple",)                           # mangled prefixes of the kernels this change edits

    def edited(name):
        return name.startswith(EDITED)
    assert len(parent) > 400 and sum(edited(name) for name in parent) == 1
    changed = {name: (parent[name], now.get(name)) for name in parent if not edited(name) and now.get(name) != parent[name]}
    assert not changed, changed
    new = sorted(name for name in now if name not in parent)
    with_scratch = {name: now[name] for name in new if not edited(name) and now[name]["scratch"] != 0}
    assert not with_scratch, with_scratch
    assert sum("k_poly_" in name for name in new) >= 7 and sum(edited(name) for name in new) == 1, new
    (old_eval,) = [parent[n] for n in parent if edited(n)]
    (new_eval,) = [now[n] for n in new if edited(n)]
    print("k_eval_simple: %r -> %r" % (old_eval, new_eval))
    assert new_eval["scratch"] == old_eval["scratch"] and new_eval["lds"] == old_eval["lds"]
