"""GPU tests of the GP marginal likelihood and its gradient (``sl_gp_likelihood``, ``GPRCached.optimize``): the
stage ``k_lml_grad`` on the restatement's ``B`` and ``K^-1`` against the derived summation bound, and the whole call
against the long-double truth with the restatement's own distance as the unit (tests/np_gp_likelihood.py) - the
rule of tests/test_gpu_gp_truth.py.  Every test prints its figures before it asserts."""

import numpy as np
import pytest
import scipy.optimize

import np_gp_likelihood as NL
import np_gp_sample as S
import np_gp_truth as T
import safe_learning_amd as sl
from safe_learning_amd import _evaluate
from test_gp_likelihood_host import check_against_summation_bound

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 129, 200)
NOISES = (1e-2, 1e-6)


def _plan():
    """(size, family) -> output columns, mean function, noise variance: every size meets every family, and over a
    size (and over a family) both column counts, both mean settings and both noise variances occur."""
    out = []
    for i, n in enumerate(SIZES):
        for j, name in enumerate(NL.FAMILY_NAMES):
            out.append((n, name, 1 + (i + j) % 2, bool((i + j // 2) % 2), NOISES[(i // 2 + j) % 2]))
    return out


PLAN = _plan()
_REFERENCES = {}


def reference(n, name, D, with_mean, noise):
    """Data, truth and the two float64 variants of one case: computed once per process, shared, left unchanged."""
    key = (n, name, D, with_mean, noise)
    if key not in _REFERENCES:
        fam = NL.family(name)
        X, Y, M = NL.data(fam, n, D, with_mean)
        R = NL.residuals(X, Y, M)
        factors = fam.factors()
        truth = NL.evaluate(factors, X, R, noise, "ld")
        variants = [NL.evaluate(factors, X, R, noise, v) for v in NL.VARIANTS]
        assert truth is not None and all(v is not None for v in variants)
        _REFERENCES[key] = dict(fam=fam, X=X, Y=Y, M=M, R=R, factors=factors, truth=truth, variants=variants)
    return _REFERENCES[key]


def _natural_vector(fam, result):
    gradient = fam.natural_gradient(result["gv"], result["gl"], result["gn"])
    return np.concatenate([np.atleast_1d(gradient[name]) for name in fam.names()])


def _allowance(own, truth):
    return S.FACTOR * max(float(own), S.ROUNDING * float(np.max(np.abs(truth))))


def test_plan_covers_the_issue():
    for n in SIZES:
        rows = [r for r in PLAN if r[0] == n]
        assert {r[1] for r in rows} == set(NL.FAMILY_NAMES)
        assert {r[2] for r in rows} == {1, 2} and {r[3] for r in rows} == {True, False} and {r[4] for r in rows} == set(NOISES)
    for name in NL.FAMILY_NAMES:
        rows = [r for r in PLAN if r[1] == name]
        assert {r[2] for r in rows} == {1, 2} and {r[3] for r in rows} == {True, False} and {r[4] for r in rows} == set(NOISES)


@pytest.mark.parametrize("n,name,D,with_mean,noise", PLAN)
def test_stage_k_lml_grad(n, name, D, with_mean, noise):
    """``k_lml_grad`` and ``k_lml_reduce`` on the restatement's float64 ``B`` and ``K^-1``: every slot within
    ``2 (n^2 + 64) 2^-53 sum |W| |dK|`` of the long-double sum over the same float64 ``W``."""
    ref = reference(n, name, D, with_mean, noise)
    given = ref["variants"][0]
    gv, gl, gn = _evaluate._ctx().gp_lml_grad_stage(ref["X"], given["B"], given["Kinv"], ref["factors"])
    check_against_summation_bound(n, ref["factors"], ref["X"], given["B"], given["Kinv"], gv, gl, gn, name)


@pytest.mark.parametrize("n,name,D,with_mean,noise", PLAN)
def test_end_to_end_against_the_truth(n, name, D, with_mean, noise):
    ref = reference(n, name, D, with_mean, noise)
    fam, truth = ref["fam"], ref["truth"]
    model = NL.package_model(sl, fam, ref["X"], ref["Y"], ref["M"], noise)
    lml = model.compute_log_likelihood()
    gradient = model.log_likelihood_gradient()
    assert list(gradient) == fam.names()
    got = np.concatenate([np.atleast_1d(gradient[k]) for k in fam.names()])
    want = _natural_vector(fam, truth)
    own_lml = max(abs(T.ld(v["lml"]) - truth["lml"]) for v in ref["variants"])
    own_grad = max(S.distance(_natural_vector(fam, v), want) for v in ref["variants"])
    rows = (("lml", abs(T.ld(lml) - truth["lml"]), own_lml, _allowance(own_lml, truth["lml"])),
            ("gradient", S.distance(got, want), own_grad, _allowance(own_grad, want)))
    for what, engine, own, allowance in rows:
        print("gp likelihood [%s n=%d D=%d mean=%s noise=%g] %s: engine %.3g, restatement %.3g, allowance %.3g"
              % (name, n, D, with_mean, noise, what, float(engine), float(own), allowance))
    for what, engine, own, allowance in rows:
        assert engine <= allowance, what
    # the value alone (no gradient pointers) is the same number
    assert _evaluate._ctx().gp_likelihood(ref["X"], ref["R"], ref["factors"], noise, gradient=False)[0] == lml


def test_n_1025_second_column_chunk():
    """n = 1025: the first size whose ``L^-1`` needs a second column chunk.  The long-double routines take 17 s on
    the CPU at this size (more than the ten a test may spend), so the engine is held to 32 x the distance between
    the two float64 restatement variants (floor: one rounding of the largest entry), not to the truth."""
    fam = NL.family("matern_shared")
    X, Y, _ = NL.data(fam, 1025, 1, False)
    a, b = [NL.evaluate(fam.factors(), X, Y, 1e-2, v) for v in NL.VARIANTS]
    lml, gv, gl, gn, pivot = _evaluate._ctx().gp_likelihood(X, Y, fam.factors(), 1e-2)
    assert pivot == 0
    engine = NL.flat(dict(lml=lml, gv=gv, gl=gl, gn=gn))
    for what, sel in (("lml", slice(0, 1)), ("gradient", slice(1, None))):
        between = float(np.max(np.abs(NL.flat(a)[sel] - NL.flat(b)[sel])))
        allowance = S.FACTOR * max(between, S.ROUNDING * float(np.max(np.abs(NL.flat(a)[sel]))))
        distance = float(np.max(np.abs(engine[sel] - NL.flat(a)[sel])))
        print("gp likelihood n=1025 %s: engine - scipy %.3g, scipy - blocked %.3g, allowance %.3g"
              % (what, distance, between, allowance))
        assert distance <= allowance


def _bits(result):
    lml, gv, gl, gn, pivot = result
    assert pivot == 0
    return np.concatenate(([lml], gv.ravel(), gl.ravel(), [gn])).view(np.uint64)


def test_same_bits_at_every_call():
    ctx = _evaluate._ctx()
    ref = reference(129, "notebook", *[r[2:] for r in PLAN if r[:2] == (129, "notebook")][0])
    other = reference(65, "rbf_ard", *[r[2:] for r in PLAN if r[:2] == (65, "rbf_ard")][0])
    noise = [r[4] for r in PLAN if r[:2] == (129, "notebook")][0]
    first = _bits(ctx.gp_likelihood(ref["X"], ref["R"], ref["factors"], noise))
    np.testing.assert_array_equal(first, _bits(ctx.gp_likelihood(ref["X"], ref["R"], ref["factors"], noise)))
    ctx.gp_likelihood(other["X"], other["R"], other["factors"], 1e-2)
    np.testing.assert_array_equal(first, _bits(ctx.gp_likelihood(ref["X"], ref["R"], ref["factors"], noise)))


def test_no_observations():
    fam = NL.family("notebook")
    lml, gv, gl, gn, pivot = _evaluate._ctx().gp_likelihood(np.zeros((0, 2)), np.zeros((0, 1)), fam.factors(), 1e-2)
    assert (lml, gn, pivot) == (0.0, 0.0, 0) and not gv.any() and not gl.any()
    model = sl.GPRCached(np.zeros((0, 2)), np.zeros((0, 1)), fam.package_kernel(sl), likelihood_variance=1e-2)
    assert model.compute_log_likelihood() == 0.0
    assert all(not np.any(v) for v in model.log_likelihood_gradient().values())


def test_identical_rows_without_noise_name_the_pivot():
    """Rows 0 and 1 are the same point of an RBF with variance 1/4: l_00 = 1/2, l_10 = 1/2 and the second pivot is
    1/4 - 1/4 = 0 in every arithmetic - the error return of ``sl_cholesky``, not a fault."""
    fam = NL.family("rbf_ard")
    fam.leaves[0].variance[...] = 0.25
    X, Y, _ = NL.data(fam, 10, 1, False)
    X[1] = X[0]
    model = NL.package_model(sl, fam, X[:1], Y[:1], None, 0.0)         # (the host cache cannot be built of all ten)
    model.X, model.Y = X, Y
    with pytest.raises(np.linalg.LinAlgError, match="pivot 2 "):
        model.compute_log_likelihood()
    with pytest.raises(np.linalg.LinAlgError, match="pivot 2 "):
        model.log_likelihood_gradient()
    # the context is as usable as before
    ref = reference(2, "rbf_ard", *[r[2:] for r in PLAN if r[:2] == (2, "rbf_ard")][0])
    assert _evaluate._ctx().gp_likelihood(ref["X"], ref["R"], ref["factors"], 1e-2)[4] == 0


def test_too_many_observations():
    fam = NL.family("matern_shared")
    with pytest.raises(ValueError, match="4096"):
        _evaluate._ctx().gp_likelihood(np.zeros((4097, 2)), np.zeros((4097, 1)), fam.factors(), 1e-2)
    model = sl.GPRCached(np.zeros((1, 2)), np.zeros((1, 1)), fam.package_kernel(sl))
    model.X, model.Y = np.zeros((4097, 2)), np.zeros((4097, 1))
    with pytest.raises(ValueError, match="4096"):
        model.compute_log_likelihood()


# ---- optimize() at the notebook's shape ---------------------------------------------------------------------------
# The engine is allowed 8 x the gap in final lml between the SciPy-Cholesky and the blocked-Cholesky restatement
# searches from the same start with the same options, measured on the CPU where the test runs (9.7e-13 at the time
# of writing, profiles/gp_likelihood.md).


def _notebook_problem():
    """n = 130, p = 2, ``Linear + Matern32 * Linear``: data drawn from the family's hyper-parameters (seed 5), the
    search started at twice (variances) / half (lengthscale, noise) of them."""
    fam = NL.family("notebook")
    rng = np.random.default_rng(5)
    X = rng.uniform(-1, 1, (130, 2))
    noise = 1e-3
    K, _ = NL.kernel_and_derivatives(fam.factors(), X)
    Y = np.linalg.cholesky(K + noise * np.eye(130)).dot(rng.standard_normal((130, 1)))
    start = NL.family("notebook")
    for leaf in start.leaves:
        leaf.variance *= 2.0
        if leaf.lengthscales is not None:
            leaf.lengthscales *= 0.5
    return fam, start, X, Y, 0.5 * noise


def restatement_search(variant):
    """``scipy.optimize.minimize`` on the float64 restatement: the same objective over logarithms, the same start
    and options as ``GPRCached.optimize``'s defaults -> final lml."""
    _, start, X, Y, noise0 = _notebook_problem()
    names = start.names()
    natural = start.natural(noise0)
    sizes = [np.size(natural[k]) for k in names]
    x0 = np.log(np.concatenate([np.atleast_1d(natural[k]) for k in names]))
    best = [np.inf]

    def objective(x):
        parts = dict(zip(names, np.split(np.exp(x), np.cumsum(sizes)[:-1])))
        for i, leaf in enumerate(start.leaves):
            leaf.variance[...] = parts["kern.%d.variance" % i] if leaf.variance.ndim else parts["kern.%d.variance" % i][0]
            if leaf.lengthscales is not None:
                leaf.lengthscales[...] = parts["kern.%d.lengthscales" % i]
        result = NL.evaluate(start.factors(), X, Y, parts["likelihood_variance"][0], variant)
        if result is None:
            return np.inf, np.zeros_like(x)
        gradient = start.natural_gradient(result["gv"], result["gl"], result["gn"])
        best[0] = min(best[0], -float(result["lml"]))
        return -float(result["lml"]), -np.concatenate([np.atleast_1d(gradient[k]) for k in names]) * np.exp(x)

    scipy.optimize.minimize(objective, x0, jac=True, method="L-BFGS-B", options=dict(maxiter=1000))
    return -best[0]


def test_optimize_notebook_shape_and_engines_follow():
    """The engine's optimum against the SciPy-Cholesky restatement search (8 x the measured gap between the two
    restatement searches), lml raised, ``success``; then a ``Lyapunov`` over the fitted ``GaussianProcess`` equals one
    built fresh from a ``GPRCached`` constructed with the optimum."""
    _, start, X, Y, noise0 = _notebook_problem()
    mean = sl.LinearSystem((np.array([[0.5, 0.1]]),))
    model = sl.GPRCached(X, Y + X.dot(mean.matrix.T), start.package_kernel(sl), mean, likelihood_variance=noise0)
    gp = sl.GaussianProcess(model)
    # One state, one action: the 41^2 cells lie on a line, three times as long as the data's interval, so that
    # beyond |x| = 1 the posterior deviation is the prior's and depends on the hyper-parameters.  With V = x^2,
    # L_v = 1.2 and the closed loop x -> about 0.5 x the start's kernel (twice the variances, half the lengthscale)
    # fails the decrease condition near |x| = 1.2, the fitted kernel nowhere (margins 1e-3 and 0.05 in float64 NumPy).
    grid = sl.GridWorld([[-3, 3]], 41 * 41)
    policy = sl.LinearSystem((np.array([[-0.5]]),))
    value = sl.QuadraticFunction([[1.0]])
    initial = np.abs(grid.all_points[:, 0]) < 0.5

    def lyapunov(dynamics):
        lyap = sl.Lyapunov(grid, value, dynamics, 0.1, 1.2, 6.0 / 1680, policy, initial_set=initial)
        lyap.update_safe_set()
        return lyap

    first = lyapunov(gp)
    set_before, c_before = np.array(first.safe_set, copy=True), first.c_max
    before = model.compute_log_likelihood()
    result = gp.optimize()
    after = model.compute_log_likelihood()
    reference_lml = restatement_search("scipy")
    gap = abs(reference_lml - restatement_search("blocked"))
    print("optimize: lml %.9f -> %.9f, restatement search %.9f, gap of the two restatement searches %.3g"
          % (before, after, reference_lml, gap))
    assert result.success and after > before and after == -result.fun
    # (floor: four roundings of lml, should the two restatement searches ever end on the same double)
    assert abs(after - reference_lml) <= max(8 * gap, 4 * S.ROUNDING * abs(reference_lml))
    first.update_safe_set()
    values = dict(model.hyperparameters())
    fresh_kern = NL.family("notebook")
    for i, leaf in enumerate(fresh_kern.leaves):
        leaf.variance[...] = values["kern.%d.variance" % i]
        if leaf.lengthscales is not None:
            leaf.lengthscales[...] = values["kern.%d.lengthscales" % i]
    fresh = lyapunov(sl.GaussianProcess(sl.GPRCached(model.X, model.Y, fresh_kern.package_kernel(sl), mean,
                                                     likelihood_variance=values["likelihood_variance"])))
    print("safe set: %d cells, c_max %.9g before the fit; %d cells, c_max %.9g after it; %d initial cells"
          % (set_before.sum(), c_before, np.asarray(first.safe_set).sum(), first.c_max, initial.sum()))
    np.testing.assert_array_equal(np.asarray(first.safe_set), np.asarray(fresh.safe_set))
    assert first.c_max == fresh.c_max
    # the fit moved the answer, so a Lyapunov that had kept the old kernel or the old factors would show here
    assert first.c_max != c_before and not np.array_equal(np.asarray(first.safe_set), set_before)
    assert np.asarray(first.safe_set).sum() > initial.sum() and set_before.sum() > initial.sum()
