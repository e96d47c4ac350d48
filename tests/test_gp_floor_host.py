"""Host tests of the variance floor of k_gp_sweep4's early decision (no GPU): the constants of
safe_learning_amd/csrc/sl_gp_floor.h, computed by the stand-alone program tests/hostsim/gp_floor_sim.cpp
(built with g++ and the address and undefined-behaviour sanitizers, run directly) on factors written
here, against ``numpy.linalg.svd`` of the same blocks - and the inequality the kernel relies on,
``V_n(x) >= c_m V_m(x)``, against the long-double posterior of tests/np_gp_truth.py."""

import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg

import hostsim_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

# (n, p, noise std / signal std, panel height): ragged last panels (40 = 16 + 16 + 8, 300 = 18 x 16 + 12
# = 256 + 44, 600 = 2 x 256 + 88) and one-panel models (40 rows of 256)
MODELS = [(40, 2, 1e-1, 16), (40, 5, 1e-4, 256), (300, 2, 1e-2, 256), (300, 5, 1e-3, 16),
          (600, 2, 1e-4, 256), (600, 5, 1e-1, 256)]
SIGNAL_VARIANCE = 0.7


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("gp_floor")
    out = hostsim_build.program("gp_floor_sim.cpp", tmp, ["-O2"] + hostsim_build.SIM_FLAGS, sanitize=True)

    def run(linv, rp, variance):
        n = len(linv)
        stages = (n + rp - 1) // rp
        path = str(tmp / "factor.bin")
        np.concatenate(([n, rp, stages, variance], np.asarray(linv, dtype=np.float64).ravel())).tofile(path)
        res = subprocess.run([out, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert res.returncode == 0, res.stdout
        c = np.array([float(v) for v in res.stdout.split()])
        assert c.shape == (stages,), res.stdout
        return c
    return run


def _model(n, p, noise_rel, seed):
    """A random RBF model: inputs, lengthscales, noise variance, the float64 inverse factor of K + noise I."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.0, 1.0, (n, p))
    ell = rng.uniform(0.4, 1.2, p)
    noise = (noise_rel ** 2) * SIGNAL_VARIANCE
    diff = X[:, None, :] / ell - X[None, :, :] / ell
    K = SIGNAL_VARIANCE * np.exp(-0.5 * np.sum(diff * diff, axis=2))
    chol = scipy.linalg.cholesky(K + noise * np.eye(n), lower=True)
    linv = np.tril(scipy.linalg.solve_triangular(chol, np.eye(n), lower=True))
    return X, ell, noise, linv


_MODELS = {}


def model(k):
    if k not in _MODELS:
        n, p, noise_rel, _ = MODELS[k]
        _MODELS[k] = _model(n, p, noise_rel, 100 + k)
    return _MODELS[k]


def exact_constants(linv, noise, rp):
    """sigma_n^2 sigma_min(Linv[m:, m:])^2 for m = 0, rp, 2 rp, ..."""
    return np.array([noise * np.linalg.svd(linv[m:, m:], compute_uv=False)[-1] ** 2 for m in range(0, len(linv), rp)])


@pytest.mark.parametrize("k", range(len(MODELS)))
def test_constants_are_certified_and_tight(sim, k):
    """Every constant is at most the exact sigma_n^2 sigma_min^2 and at least 0.98 of it (the certificate's
    step is 1e-3 twice: a routine that is merely safe fails here)."""
    n, p, noise_rel, rp = MODELS[k]
    _, _, noise, linv = model(k)
    got = sim(linv, rp, SIGNAL_VARIANCE)
    exact = exact_constants(linv, noise, rp)
    print("n=%d p=%d noise/signal=%g panel=%d: exact %s, ratio %s" % (n, p, noise_rel, rp, exact, got / exact))
    assert (got <= exact).all()
    assert (got >= 0.98 * exact).all()


def test_non_finite_factor_gives_zeros(sim):
    _, _, _, linv = model(2)
    for bad in (np.nan, np.inf):
        broken = linv.copy()
        broken[200, 17] = bad
        assert (sim(broken, 256, SIGNAL_VARIANCE) == 0.0).all()
    # a pivot that leaves no positive noise: 1 / Linv[0][0]^2 <= the prior variance
    assert (sim(linv, 256, 2.0 * SIGNAL_VARIANCE) == 0.0).all()


@pytest.mark.parametrize("k", range(len(MODELS)))
def test_the_inequality_holds_in_long_double(sim, k):
    """V_n(x) >= c_m V_m(x) at 200 random inputs, inside and well outside the data, for every boundary m,
    with the posterior variances in long double (tests/np_gp_truth.py)."""
    import np_gp_truth as truth
    n, p, noise_rel, rp = MODELS[k]
    X, ell, noise, linv = model(k)
    c = sim(linv, rp, SIGNAL_VARIANCE)
    rng = np.random.default_rng(900 + k)
    Z = np.vstack((rng.uniform(-1.0, 1.0, (100, p)), rng.uniform(-4.0, 4.0, (100, p))))
    LD = truth.LD
    Xs, Zs = truth.ld(X) / truth.ld(ell), truth.ld(Z) / truth.ld(ell)

    def rbf(A, B):
        dist = np.zeros((len(A), len(B)), dtype=LD)
        for q in range(p):
            diff = A[:, q][:, None] - B[:, q][None, :]
            dist += diff * diff
        return LD(SIGNAL_VARIANCE) * np.exp(-dist / LD(2))

    chol = truth.cholesky(rbf(Xs, Xs) + LD(noise) * np.eye(n, dtype=LD))
    a = truth.forward_substitution(chol, rbf(Xs, Zs))
    sumsq = np.vstack((np.zeros((1, len(Z)), dtype=LD), np.cumsum(a * a, axis=0)))      # [m] = rows 0 .. m - 1
    v_n = LD(SIGNAL_VARIANCE) - sumsq[n]
    assert (v_n > 0).all()
    for s, m in enumerate(range(0, n, rp)):
        v_m = LD(SIGNAL_VARIANCE) - sumsq[m]
        ratio = v_n / v_m
        print("n=%d m=%d: c = %.4g, smallest V_n / V_m = %.4g" % (n, m, c[s], float(ratio.min())))
        assert (v_n >= LD(c[s]) * v_m).all()
