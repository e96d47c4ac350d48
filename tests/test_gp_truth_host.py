"""The extended-precision GP posterior (``tests/np_gp_truth.py``) and the bounds built from it, on the CPU.

a. the long-double posterior is at least 100 times closer to an mpmath posterior (60 digits) than the oracle is;
b. a float64 NumPy restatement of the engine's formula (explicit ``L^-1``, then ``sigma^2 - |a|^2``) stays within
   the bound the GPU test gives the engine, with factors built by SciPy and with the package's own host factors
   (``GPRCached.update_cache`` and 64 ``append_data`` calls) - and leaves it when one row of ``L^-1`` is off by
   1e-9 relative, which the float64-against-float64 tolerances of the other tests do not notice;
c. the oracle's variance is positive at every compared cell and no cell is left out.
"""

import numpy as np
import pytest

import cases
import np_gp_truth as T
from oracle import np_functions as onp

DISTINCT = [name for name in T.CASES if T.CASES[name][1] is None]          # (the SL_GP_CFG rows share their case)
TABULATED = [name for name in T.TABULATED if name in DISTINCT]


# ---- a. the truth is trustworthy -----------------------------------------------------------------------------

def _mp_kernel(mp, kern, x, y, diag=False):
    """``k(x, y)`` of an oracle kernel object in mpmath (``diag``: the ``Kdiag`` definition)."""
    if isinstance(kern, onp.Prod):
        out = mp.mpf(1)
        for k in kern.kern_list:
            out *= _mp_kernel(mp, k, x, y, diag)
        return out
    if isinstance(kern, onp.Add):
        return mp.fsum(_mp_kernel(mp, k, x, y, diag) for k in kern.kern_list)
    dims = range(len(x)) if isinstance(kern, onp.RBF) else [int(q) for q in kern.active_dims]
    if isinstance(kern, onp.Linear):
        return mp.fsum(mp.mpf(float(v)) * x[q] * y[q] for v, q in zip(kern.variance, dims))
    if diag:
        return mp.mpf(kern.variance)
    sq = mp.fsum(((x[q] - y[q]) / mp.mpf(float(ell))) ** 2 for ell, q in zip(kern.lengthscales, dims))
    if isinstance(kern, onp.Matern32):
        r = mp.mpf(float(np.sqrt(3.))) * mp.sqrt(sq + mp.mpf(1e-12))
        return mp.mpf(kern.variance) * (1 + r) * mp.exp(-r)
    return mp.mpf(kern.variance) * mp.exp(-sq / 2)


def _mp_posterior(model, Z):
    """mean[q][d], var[q][d] at 60 digits: Cholesky and forward substitution written out."""
    import mpmath as mp
    mp.mp.dps = 60
    gps, _ = T.model_heads(model)
    means, variances = [[] for _ in Z], [[] for _ in Z]
    for gp in gps:
        n = len(gp.X)
        X = [[mp.mpf(float(v)) for v in row] for row in gp.X]
        prior = None if gp.mean_function is None else [[mp.mpf(float(v)) for v in row] for row in gp.mean_function.matrix]
        L = [[mp.mpf(0)] * n for _ in range(n)]
        for j in range(n):
            for i in range(j, n):
                s = _mp_kernel(mp, gp.kern, X[i], X[j]) + (mp.mpf(gp.likelihood_variance) if i == j else 0)
                s -= mp.fsum(L[i][k] * L[j][k] for k in range(j))
                L[i][j] = mp.sqrt(s) if i == j else s / L[j][j]

        def solve(b):
            out = []
            for i in range(n):
                out.append((b[i] - mp.fsum(L[i][k] * out[k] for k in range(i))) / L[i][i])
            return out

        cols = gp.Y.shape[1]
        alphas = []
        for c in range(cols):
            resid = [mp.mpf(float(gp.Y[i, c])) - (mp.fsum(p * x for p, x in zip(prior[c], X[i])) if prior else 0)
                     for i in range(n)]
            alphas.append(solve(resid))
        for q, z in enumerate(Z):
            z = [mp.mpf(float(v)) for v in z]
            a = solve([_mp_kernel(mp, gp.kern, X[i], z) for i in range(n)])
            var = _mp_kernel(mp, gp.kern, z, z, diag=True) - mp.fsum(v * v for v in a)
            for c in range(cols):
                mean = mp.fsum(u * v for u, v in zip(a, alphas[c]))
                if prior:
                    mean += mp.fsum(p * x for p, x in zip(prior[c], z))
                means[q].append(mean)
                variances[q].append(var)
    return means, variances


def _against_mpmath(case):
    """-> (long double's, the oracle's) largest relative variance error and largest mean error against mpmath."""
    import mpmath as mp
    cells = np.arange(int(np.prod(case["num_points"])))
    ref = T.oracle_error(case, cells)
    means, variances = _mp_posterior(ref.model, ref.Z)
    worst = dict(ld_var=0, oracle_var=0, ld_mean=0, oracle_mean=0)

    def to_mp(v):
        """A long double as an mpf, exactly: its float64 head plus the float64 rest."""
        head = np.float64(v)
        return mp.mpf(float(head)) + mp.mpf(float(np.float64(v - T.LD(head))))

    for q in range(len(ref.Z)):
        for c in range(ref.mean_true.shape[1]):
            v, m = variances[q][c], means[q][c]
            worst["ld_var"] = max(worst["ld_var"], abs(to_mp(ref.var_true[q, c]) - v) / v)
            worst["oracle_var"] = max(worst["oracle_var"], abs(mp.mpf(float(ref.var_oracle[q, c])) - v) / v)
            worst["ld_mean"] = max(worst["ld_mean"], abs(to_mp(ref.mean_true[q, c]) - m))
            worst["oracle_mean"] = max(worst["oracle_mean"], abs(mp.mpf(float(ref.mean_oracle[q, c])) - m))
    return {k: float(v) for k, v in worst.items()}


def _small_rbf_case():
    return cases.make_case("pendulum", num_points=6, n_gp=40, noise_std=1e-6, signal_std=0.05, lengthscale=2.0,
                           tau_scale=0.0)


def _small_kernel_case():
    """Every leaf kind, ARD lengthscales, active dimensions out of order, a product of three (gp_cases' mixed)."""
    from gp_cases import kernel_case_list
    case = cases.make_case("pendulum", num_points=6, n_gp=20, noise_std=0.001, tau_scale=0.0, stack=True)
    case["dynamics"]["kernels"] = kernel_case_list()[3]["kernels"]
    return case


@pytest.mark.parametrize("build", [_small_rbf_case, _small_kernel_case], ids=["rbf_n40_cond2e8", "matern_linear_rbf_n20"])
def test_long_double_is_a_hundred_times_closer_to_the_posterior_than_the_oracle(build):
    worst = _against_mpmath(build())
    print("gp truth [mpmath] %s: variance long double %.3g, oracle %.3g (relative); mean long double %.3g, oracle %.3g"
          % (build.__name__, worst["ld_var"], worst["oracle_var"], worst["ld_mean"], worst["oracle_mean"]))
    assert worst["oracle_var"] > 0 and worst["oracle_mean"] > 0
    assert worst["ld_var"] <= worst["oracle_var"] / 100
    assert worst["ld_mean"] <= worst["oracle_mean"] / 100


# ---- b. the bound is attainable (and it bites) -------------------------------------------------------------------

def _within(ref, mean, var, name, what):
    fig = ref.measure(mean, var)
    T.report(name, what, fig)
    assert fig["finite"]
    assert fig["var_over_bound"] <= 1.0, (name, what, fig)
    assert fig["mean_over_bound"] <= 1.0, (name, what, fig)
    return fig


def _package_factors(case):
    """``[(L^-1, alpha)]`` per head as the package's host code builds them, and the engine-side model."""
    from safe_learning_amd import functions as F
    from safe_learning_amd.benchmarks import build_specs
    dynamics = build_specs(case)[1]
    heads, _ = F._gp_heads(dynamics)
    return dynamics, [(gp.cholesky_inverse, gp.alpha) for gp, _, _ in heads]


@pytest.mark.parametrize("name", TABULATED)
def test_explicit_inverse_in_float64_stays_within_the_bound(name):
    """The engine's formula in plain NumPy, factors from SciPy: 1 to 8 times the oracle's error, so 32 is attainable."""
    case, cells, ref = T.case_reference(name)
    _within(ref, *T.explicit_inverse_posterior(ref.model, ref.Z), name, "NumPy explicit inverse")


@pytest.mark.parametrize("name", TABULATED)
def test_host_factors_of_the_package_stay_within_the_bound(name):
    """``GPRCached.update_cache``'s ``L^-1`` and ``alpha`` - the host half of the product - through the same formula."""
    case, cells, ref = T.case_reference(name)
    _, factors = _package_factors(case)
    _within(ref, *T.explicit_inverse_posterior(ref.model, ref.Z, factors), name, "GPRCached.update_cache")


def test_appended_host_factors_stay_within_the_bound():
    """64 rank-one extensions of ``L^-1`` (100 -> 164 points) against the posterior of all 164 points at once: the
    appended factors get the bound of any other, and are as close to the truth as a fresh ``update_cache``."""
    full, base = T.appended_case()
    cells = T.compared_cells(full)
    ref = T.oracle_error(full, cells)
    dynamics, _ = _package_factors(base)
    X, Y = full["dynamics"]["X"], full["dynamics"]["Y"]
    for i in range(100, 164):
        dynamics.add_data_point(X[[i]], Y[[i]])
    gp = dynamics.gaussian_process
    assert len(gp.X) == 164 and len(gp._append_log) == 64 and np.array_equal(gp.X, X)
    appended = _within(ref, *T.explicit_inverse_posterior(ref.model, ref.Z, [(gp.cholesky_inverse, gp.alpha)]),
                       "appended_100+64", "GPRCached.append_data")
    _, factors = _package_factors(full)
    fresh = _within(ref, *T.explicit_inverse_posterior(ref.model, ref.Z, factors), "appended_100+64", "fresh update_cache")
    print("gp truth [appended_100+64]: appended %.3g x oracle, fresh %.3g x oracle" % (appended["var_ratio"], fresh["var_ratio"]))


@pytest.mark.parametrize("name", ["ill_3e-5", "ill_1e-5", "ill_1e-6", "on_cells_5e-4", "on_cells_3e-5", "informed_n400"])
def test_a_perturbed_inverse_row_leaves_the_bound(name):
    """The bound bites: row 30 of ``L^-1`` off by 1e-9 relative (the early rows carry most of ``|a|^2``; row 0 would
    be 1e4 times the bound) leaves it in every case, while the variance stays within 2e-6 .. 1e-3 relative of the
    ORACLE's - 6e-8 at ``informed_n400`` - which float64-against-float64 tolerances of 1e-6 and wider do not see."""
    case, cells, ref = T.case_reference(name)
    _, factors = _package_factors(case)
    inverse, alpha = factors[0]
    broken = inverse.copy()
    broken[30] *= 1.0 + 1e-9
    mean, var = T.explicit_inverse_posterior(ref.model, ref.Z, [(broken, alpha)])
    fig = ref.measure(mean, var)
    T.report(name, "L^-1 row 30 x (1 + 1e-9)", fig)
    print("gp truth [%s]: the same against the oracle: %.3g relative" % (name, np.max(np.abs(var - ref.var_oracle) / ref.var_oracle)))
    assert fig["var_over_bound"] > 1.0


# ---- c. the conditions the comparison rests on -----------------------------------------------------------------------

@pytest.mark.parametrize("name", DISTINCT)
def test_every_compared_cell_has_a_positive_reference_variance(name):
    case, cells, ref = T.case_reference(name)
    n = int(np.prod(case["num_points"]))
    if case["d"] < 4:
        assert np.array_equal(cells, np.arange(n))                     # every cell of the grid
    else:
        assert len(cells) >= 1024 and np.all(np.isin(np.arange(64), cells)) and np.all(np.isin(np.arange(n - 64, n), cells))
    assert ref.Z.shape == (len(cells), case["d"] + 1)
    assert ref.var_true.shape == ref.var_oracle.shape == (len(cells), case["d"])      # nothing excluded
    assert np.all(ref.var_oracle > 0) and np.all(ref.var_true > 0)
    assert np.all(ref.variance_bound() > 0) and np.all(ref.mean_bound() > 0)
    print("gp truth [%s]: cond(K) %.3g, smallest var / prior var %.3g, oracle variance error %.3g relative, oracle mean "
          "error %.3g" % (name, T.condition_number(ref.model), float((ref.var_true / ref.prior_var).min()), ref.e_oracle,
                          float(ref.mean_err.max())))
