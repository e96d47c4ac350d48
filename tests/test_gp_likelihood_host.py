"""CPU checks of the GP marginal likelihood: (a) the long-double restatement (tests/np_gp_likelihood.py) against
difference quotients of itself - this pins the formulas; (b) the per-element arithmetic and the tile / slot
reduction of csrc/sl_gp_likelihood.h, run on the host by tests/hostsim/gp_likelihood.cpp, against the restatement
handed the same float64 W; (c) the Python layer (names, chain rule, ``optimize``) on a stand-in engine that computes
with the restatement."""

import ctypes
import subprocess

import numpy as np
import pytest
import scipy.linalg
import scipy.optimize

import np_gp_likelihood as NL
import np_gp_truth as T
import safe_learning_amd as sl
from hostsim_build import SHIM_FLAGS, sanitized_program_or_plain
from safe_learning_amd import _hip, functions

LD = T.LD
U = 2.0 ** -53
SIZES = (1, 2, 63, 64, 65, 129)


# ---- (a) --------------------------------------------------------------------------------------------------------
def _ld_lml(fam, X, R, noise):
    return NL.evaluate(fam.factors(LD), X, R, noise, "ld")


@pytest.mark.parametrize("name", NL.FAMILY_NAMES)
def test_restatement_against_difference_quotients(name):
    """Allowance per entry: 4 |D_h - D_(h/2)|, the quotient's own error estimate, plus one float64 rounding."""
    fam = NL.family(name)
    X, Y, M = NL.data(fam, 12, 2, True)
    R, noise = NL.residuals(X, Y, M), LD(1e-2)
    for leaf in fam.leaves:                                  # the parameters themselves move in long double
        leaf.variance = leaf.variance.astype(LD)
        if leaf.lengthscales is not None:
            leaf.lengthscales = leaf.lengthscales.astype(LD)
    result = _ld_lml(fam, X, R, noise)
    gradient = fam.natural_gradient(result["gv"], result["gl"], result["gn"])

    def quotient(move, h):
        values = []
        for sign in (1, -1):
            undo = move(sign * h)
            values.append(_ld_lml(fam, X, R, noise)["lml"])
            undo()
        return (values[0] - values[1]) / (2 * h)

    checked = 0
    for i, leaf in enumerate(fam.leaves):
        for what in ("variance", "lengthscales"):
            array = getattr(leaf, what)
            if array is None:
                continue
            vector = leaf.ARD and (what == "lengthscales" or leaf.kind == NL.LINEAR)
            for k in (range(array.size) if vector else [None]):
                def move(step, array=array, k=k):
                    saved = array.copy()
                    if k is None:
                        array[...] = array + step
                    else:
                        array[k] = array[k] + step
                    return lambda: array.__setitem__(Ellipsis, saved)
                h = LD(1e-3) * (np.ravel(array)[0] if k is None else array[k])
                d1, d2 = quotient(move, h), quotient(move, h / 2)
                analytic = np.ravel(gradient["kern.%d.%s" % (i, what)])[0 if k is None else k]
                allowance = 4 * abs(d1 - d2) + U * abs(analytic)
                print("%s kern.%d.%s[%s]: analytic %.12g, quotient %.12g, allowance %.3g"
                      % (name, i, what, k, float(analytic), float(d2), float(allowance)))
                assert abs(analytic - d2) <= allowance
                checked += 1
    h = LD(1e-3) * noise
    d1, d2 = [(_ld_lml(fam, X, R, noise + s)["lml"] - _ld_lml(fam, X, R, noise - s)["lml"]) / (2 * s) for s in (h, h / 2)]
    assert abs(gradient["likelihood_variance"] - d2) <= 4 * abs(d1 - d2) + U * abs(gradient["likelihood_variance"])
    assert checked == sum(np.size(v) for k, v in fam.natural(0.0).items()) - 1


# ---- (b) --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return sanitized_program_or_plain("gp_likelihood.cpp", tmp_path_factory.mktemp("gp_likelihood"), SHIM_FLAGS)


def _host_run(program, tmp_path, factors, X, B, Kinv):
    n, p = X.shape
    spec = _hip.Context._kernel_spec(factors, p)
    source, out = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(source, "wb") as f:
        f.write(np.array([n, p, B.shape[1]], dtype=np.int64).tobytes())
        f.write(ctypes.string_at(ctypes.addressof(spec), ctypes.sizeof(spec)))
        for array in (X, B, Kinv):
            f.write(np.ascontiguousarray(array, dtype=np.float64).tobytes())
    subprocess.check_call([program, str(source), str(out)])
    values = np.fromfile(out, dtype=np.float64)
    assert values.size == 130
    return int(values[0]), values[1:65].reshape(8, 8), values[65:129].reshape(8, 8), values[129]


def check_against_summation_bound(n, factors, X, B, Kinv, gv, gl, gn, label):
    """The rule of (b), shared with the GPU stage test: every slot within 2 (n^2 + 64) 2^-53 sum |W| |dK| of the
    long-double sum over the same float64 W."""
    p = X.shape[1]
    (tv, tl, tn), (av, al, an) = NL.gradient_from_w(factors, X, NL.device_w(B, Kinv))
    for what, got, truth, scale in (("variance", gv, tv, av), ("inv_ls", gl, tl, al), ("noise", gn, tn, an)):
        distance = np.abs(T.ld(got) - truth)
        allowance = NL.summation_allowance(n, scale)
        print("%s n=%d %s: distance %.3g, allowance %.3g" % (label, n, what, float(np.max(distance)),
                                                             float(np.max(allowance))))
        assert np.all(distance <= allowance), (label, n, what)
        assert np.all(np.asarray(got)[np.asarray(scale, dtype=np.float64) == 0] == 0)
    assert np.any(av > 0) or np.any(al > 0)
    return len(factors), p


@pytest.mark.parametrize("n", SIZES)
def test_header_arithmetic_on_the_host(program, tmp_path, n):
    for k, name in enumerate(NL.FAMILY_NAMES):
        fam = NL.family(name)
        D = 1 + (k + n) % 2
        X, Y, M = NL.data(fam, n, D, bool(k % 2))
        factors = fam.factors()
        ref = NL.evaluate(factors, X, NL.residuals(X, Y, M), 1e-2, "scipy")
        nslots, gv, gl, gn = _host_run(program, tmp_path, factors, X, ref["B"], ref["Kinv"])
        nf = len(factors)
        assert nslots == sum(int(np.count_nonzero(v if kind == NL.LINEAR else v[:1]) + np.count_nonzero(a))
                             for kind, _, v, a in factors)
        assert not gv[nf:].any() and not gl[nf:].any() and not gv[:, fam.p:].any() and not gl[:, fam.p:].any()
        check_against_summation_bound(n, factors, X, ref["B"], ref["Kinv"], gv[:nf, :fam.p], gl[:nf, :fam.p], gn, name)


# ---- (c) --------------------------------------------------------------------------------------------------------
@pytest.fixture
def stand_in(monkeypatch):
    """``functions._likelihood_engine`` answered by the float64 restatement; ``calls`` counts, ``reject`` holds the
    numbers of the calls to answer with a failed pivot."""
    state = dict(calls=0, reject=set())

    def engine(X, R, factors, noise, gradient):
        state["calls"] += 1
        if state["calls"] in state["reject"]:
            return None, None, None, None, 3
        result = NL.evaluate(factors, X, R, noise, "scipy")
        if result is None:
            return None, None, None, None, 1
        if not gradient:
            return float(result["lml"]), None, None, None, 0
        return float(result["lml"]), result["gv"], result["gl"], float(result["gn"]), 0

    monkeypatch.setattr(functions, "_likelihood_engine", engine)
    return state


def _model(name, n=20, D=2, noise=1e-2, with_mean=True):
    fam = NL.family(name)
    X, Y, M = NL.data(fam, n, D, with_mean)
    return fam, NL.package_model(sl, fam, X, Y, M, noise), NL.residuals(X, Y, M)


@pytest.mark.parametrize("name", NL.FAMILY_NAMES)
def test_names_and_chain_rule(stand_in, name):
    fam, model, R = _model(name)
    expected = fam.natural(1e-2)
    listed = model.hyperparameters()
    assert [n for n, _ in listed] == fam.names()
    for n, value in listed:
        assert np.shape(value) == np.shape(expected[n]) and np.array_equal(value, expected[n]), n
    assert model.kern._factors(fam.p)[0][1] == 0 and len(model.kern._factors(fam.p)) == len(fam.factors())
    for (k1, p1, v1, a1), (k2, p2, v2, a2) in zip(model.kern._factors(fam.p), fam.factors()):
        assert (k1, p1) == (k2, p2) and np.array_equal(v1, v2) and np.array_equal(a1, a2)
    ref = NL.evaluate(fam.factors(), model.X, R, 1e-2, "scipy")
    want = fam.natural_gradient(ref["gv"], ref["gl"], ref["gn"])
    got = model.log_likelihood_gradient()
    assert sorted(got) == sorted(want)
    for n in want:
        assert np.shape(got[n]) == np.shape(expected[n]), n
        np.testing.assert_allclose(got[n], want[n], rtol=4 * U, atol=0)
    assert model.compute_log_likelihood() == float(ref["lml"])


def test_shared_leaf_sums_over_both_products(stand_in):
    fam, model, R = _model("shared_leaf")
    ref = NL.evaluate(fam.factors(), model.X, R, 1e-2, "scipy")
    assert fam.factor_leaf() == [0, 1, 2, 1]
    got = model.log_likelihood_gradient()["kern.1.variance"]
    np.testing.assert_allclose(got, ref["gv"][1, 1] + ref["gv"][3, 1], rtol=4 * U)
    assert ref["gv"][1, 1] != 0 and ref["gv"][3, 1] != 0


def test_log_space_gradient_fixed_and_bounds(stand_in, monkeypatch):
    """``optimize`` hands SciPy the objective over the logarithms of the free parameters: its gradient against
    central differences of the objective itself (h and h / 2, allowance 4 |D_h - D_(h/2)| plus float64 noise of the
    objective, 2^-53 |f| / h per evaluation), the fixed names left out, the bounds in logarithms."""
    fam, model, _ = _model("notebook")
    seen = {}

    def fake_minimize(fun, x0, jac, method, tol, bounds, callback, options):
        seen.update(x0=x0.copy(), bounds=bounds, method=method, options=options)
        f0, g0 = fun(x0)
        for k in range(len(x0)):
            quotients = []
            for h in (1e-3, 5e-4):
                e = np.zeros_like(x0)
                e[k] = h
                quotients.append((fun(x0 + e)[0] - fun(x0 - e)[0]) / (2 * h))
            allowance = 4 * abs(quotients[0] - quotients[1]) + 4 * U * abs(f0) / 5e-4
            print("log-space entry %d: gradient %.10g, quotient %.10g, allowance %.3g" % (k, g0[k], quotients[1], allowance))
            assert abs(g0[k] - quotients[1]) <= allowance
        return scipy.optimize.OptimizeResult(x=x0, fun=f0, success=True)

    monkeypatch.setattr(scipy.optimize, "minimize", fake_minimize)
    model.optimize(fixed=("kern.1.lengthscales",), bounds={"likelihood_variance": (1e-4, 1.0),
                                                           "kern.0.variance": (None, 2.0)}, maxiter=7)
    natural = fam.natural(1e-2)
    free = [n for n in fam.names() if n != "kern.1.lengthscales"]
    np.testing.assert_array_equal(seen["x0"], np.log(np.concatenate([np.atleast_1d(natural[n]) for n in free])))
    assert seen["bounds"] == [(None, np.log(2.0))] * 2 + [(None, None)] * 2 + [(np.log(1e-4), 0.0)]
    assert seen["method"] == "L-BFGS-B" and seen["options"] == {"maxiter": 7}
    with pytest.raises(ValueError, match="kern.9.variance"):
        model.optimize(fixed=("kern.9.variance",))


def test_optimize_raises_the_likelihood_and_refreshes_the_cache(stand_in):
    fam, model, _ = _model("notebook", n=30, D=1)
    before, version = model.compute_log_likelihood(), model._version
    fixed_value = dict(model.hyperparameters())["kern.1.lengthscales"]
    result = model.optimize(fixed=("kern.1.lengthscales",), bounds={"likelihood_variance": (1e-6, 1.0)})
    after = model.compute_log_likelihood()
    print("lml %.6f -> %.6f in %d evaluations" % (before, after, stand_in["calls"]))
    assert result.success and after > before and after == -result.fun
    assert model._version != version
    values = dict(model.hyperparameters())
    assert values["kern.1.lengthscales"] == fixed_value
    assert 1e-6 <= values["likelihood_variance"] <= 1.0
    assert any(values[n].tolist() != fam.natural(1e-2)[n].tolist() for n in values)
    gram = model.kern.K(model.X) + model.likelihood_variance * np.eye(len(model.X))
    chol = scipy.linalg.cholesky(gram, lower=True)
    np.testing.assert_array_equal(model.cholesky, chol)
    np.testing.assert_array_equal(model.cholesky_inverse,
                                  np.tril(scipy.linalg.solve_triangular(chol, np.eye(len(chol)), lower=True)))


_UNDISTURBED = {}


@pytest.mark.parametrize("rejected", [(1,), (2,), (3,), (4,), (7,), (1, 2)])
@pytest.mark.parametrize("method", ["L-BFGS-B", "BFGS"])
def test_a_rejected_point_does_not_end_the_search(stand_in, method, rejected):
    """``rejected``: which evaluations after the start are rejected (one inside the first line search, later ones,
    two in a row).  BFGS backs off from a rejected point; the default L-BFGS-B stops on it or one
    evaluation later, and ``optimize`` takes the search up again from the best point seen: more evaluations follow,
    ``success`` is true and the fit ends where an undisturbed search ends (SciPy's ``ftol``, 2.2e-9 relative for
    L-BFGS-B; 1e-6 allows for two different paths to the same optimum)."""
    if method not in _UNDISTURBED:
        _, undisturbed, _ = _model("matern_shared", n=25, D=1)
        _UNDISTURBED[method] = undisturbed.optimize(method=method)
    wanted = _UNDISTURBED[method]
    _, model, _ = _model("matern_shared", n=25, D=1)
    before = model.compute_log_likelihood()
    first = stand_in["calls"] + 1
    stand_in["reject"] = {first + k for k in rejected}
    result = model.optimize(method=method)
    after = model.compute_log_likelihood()
    print("%s, rejected %s: lml %.9f -> %.9f (undisturbed %.9f), %d evaluations, %d rejected, success %s"
          % (method, rejected, before, after, -wanted.fun, stand_in["calls"] - first, result.rejected, result.success))
    assert result.rejected == len(rejected) and stand_in["calls"] - first > max(rejected) + 3
    assert result.success and np.isfinite(result.fun) and after == -result.fun and after > before
    assert abs(after - -wanted.fun) <= 1e-6 * abs(wanted.fun)


def test_a_search_that_ends_on_a_rejected_point_says_so(stand_in):
    """Every evaluation but the start is rejected: the best point is the start, the cache is rebuilt there, and the
    result does not claim success."""
    _, model, _ = _model("matern_shared", n=25, D=1)
    before = model.compute_log_likelihood()
    values = model.hyperparameters()
    stand_in["reject"] = set(range(stand_in["calls"] + 2, stand_in["calls"] + 400))
    result = model.optimize()
    assert not result.success and "cannot be factored" in result.message and result.rejected >= 1
    assert -result.fun == before and stand_in["calls"] < 100
    for (name, old), (_, new) in zip(values, model.hyperparameters()):
        np.testing.assert_allclose(new, old, rtol=4 * U, err_msg=name)


def test_a_model_that_cannot_be_factored_at_the_start_raises(stand_in):
    _, model, _ = _model("matern_shared", n=10, D=1)
    stand_in["reject"] = {stand_in["calls"] + 1, stand_in["calls"] + 2}
    with pytest.raises(np.linalg.LinAlgError, match="pivot 3"):
        model.compute_log_likelihood()
    version, values = model._version, model.hyperparameters()
    with pytest.raises(np.linalg.LinAlgError, match="pivot 3"):
        model.optimize()
    assert model._version == version                     # (never factored: the cache is left as it was)
    for (name, old), (_, new) in zip(values, model.hyperparameters()):
        np.testing.assert_allclose(new, old, rtol=4 * U, err_msg=name)


def test_stack_and_process_delegate(stand_in):
    fam, model, _ = _model("matern_shared", n=15, D=1)
    _, other, _ = _model("rbf_ard", n=15, D=1)
    stack = sl.FunctionStack([sl.GaussianProcess(model), sl.GaussianProcess(other)])
    results = stack.optimize(maxiter=3)
    assert len(results) == 2 and all(isinstance(r, scipy.optimize.OptimizeResult) for r in results)


def test_single_process_only(stand_in, monkeypatch):
    from safe_learning_amd import distributed
    _, model, _ = _model("matern_shared", n=5, D=1)
    monkeypatch.setattr(distributed, "rank_and_world", lambda: (0, 2))
    with pytest.raises(NotImplementedError):
        model.compute_log_likelihood()
    with pytest.raises(NotImplementedError):
        model.optimize()
