"""NumPy restatement of ``sample_gp_function`` (TEST INFRASTRUCTURE): float64, and long double built on
``np_gp_truth``'s ``ld``, ``kernel_matrix``, ``cholesky`` and ``forward_substitution``.

The float64 functions state the ENGINE's formulas with SciPy: the posterior with an explicit ``L^-1``
(``a = L^-1 K(X, Z)``, ``mean = a^T alpha + m(Z)``, ``cov = K(Z, Z) - a^T a + jitter I``), the Cholesky factor of
``cov``, the samples ``mean + L z``, ``alpha = cov^-1 sample`` by two triangular solves and the sample function
``m(x) + K(x, D) alpha`` with the prior kernel.  The long-double functions state the same mathematics with the
float64 inputs converted exactly; the distance between the two is the restatement's own error, and the engine is
allowed ``FACTOR`` times that (``bound``), with a floor of one rounding of the largest entry.

``blocked_cholesky`` / ``diag_factor`` restate the blocked algorithm of ``csrc/sl_gp_sample.h`` loop by loop: the
diagonal block in the device's order (bit for bit), the products between blocks with ``np.dot``.

The cases of the GPU tests are built here as well (``CASES``), one oracle ``GPRCached`` and one discretization each.
"""

import numpy as np
import scipy.linalg

import np_gp_truth as T
from oracle import np_functions as onp

LD = T.LD
FACTOR = T.FACTOR
ROUNDING = T.ROUNDING
JITTER = 1e-8
NB = 64


# ---- float64 ------------------------------------------------------------------------------------------------
def _factors(gp):
    """``(L^-1, alpha [n])`` of a one-output oracle GPRCached, as the package's host code builds them."""
    n = len(gp.X)
    if n == 0:
        return np.zeros((0, 0)), np.zeros(0)
    chol = scipy.linalg.cholesky(gp.kern.K(gp.X) + gp.likelihood_variance * np.eye(n), lower=True)
    inverse = np.tril(scipy.linalg.solve_triangular(chol, np.eye(n), lower=True))
    alpha = scipy.linalg.solve_triangular(chol, gp.Y - gp._mean(gp.X), lower=True)
    return inverse, alpha[:, 0]


def prior_mean(gp, Z):
    return gp._mean(np.atleast_2d(Z))[:, 0]


def posterior(gp, Z, jitter=JITTER):
    """``mean [N]``, ``cov [N, N]`` (jitter included) at ``Z`` by the engine's formula."""
    Z = np.atleast_2d(np.asarray(Z, dtype=np.float64))
    inverse, alpha = _factors(gp)
    cov = gp.kern.K(Z, Z)
    mean = prior_mean(gp, Z)
    if len(alpha):
        a = inverse.dot(gp.kern.K(gp.X, Z))
        mean = a.T.dot(alpha) + mean
        cov = cov - a.T.dot(a)
    cov = np.tril(cov) + np.tril(cov, -1).T           # the lower triangle, mirrored (BLAS products are not symmetric
    return mean, cov + jitter * np.eye(len(Z))        # to the last bit)


def cholesky(cov):
    return scipy.linalg.cholesky(cov, lower=True)


def samples(mean, chol, normal):
    """``[number, N]`` for ``normal [number, N]``."""
    return mean[None, :] + np.asarray(normal).dot(chol.T)


def alphas(chol, values):
    """``[N, number] = cov^-1 values^T`` for ``values [number, N]``."""
    half = scipy.linalg.solve_triangular(chol, np.asarray(values).T, lower=True)
    return scipy.linalg.solve_triangular(chol.T, half, lower=False)


def evaluate(gp, D, alpha, X):
    """``[M, number]``: the sample functions at ``X`` (prior kernel, as the reference evaluates them)."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    return prior_mean(gp, X)[:, None] + gp.kern.K(X, D).dot(alpha)


# ---- long double --------------------------------------------------------------------------------------------
def _prior_ld(gp, Z):
    if gp.mean_function is None:
        return np.zeros(len(Z), dtype=LD)
    return Z.dot(T.ld(gp.mean_function.matrix).T)[:, 0]


def posterior_ld(gp, Z, jitter=JITTER):
    Z = T.ld(np.atleast_2d(Z))
    cov = T.kernel_matrix(gp.kern, Z, Z)
    mean = _prior_ld(gp, Z)
    if len(gp.X):
        X = T.ld(gp.X)
        chol = T.cholesky(T.kernel_matrix(gp.kern, X, X) + LD(gp.likelihood_variance) * np.eye(len(X), dtype=LD))
        alpha = T.forward_substitution(chol, T.ld(gp.Y)[:, 0] - _prior_ld(gp, X))
        a = T.forward_substitution(chol, T.kernel_matrix(gp.kern, X, Z))
        mean = a.T.dot(alpha) + mean
        cov = cov - a.T.dot(a)
    return mean, cov + LD(jitter) * np.eye(len(Z), dtype=LD)


def backward_substitution(L, B):
    """``L^-T B``: the reversed system is lower triangular again."""
    return T.forward_substitution(L.T[::-1, ::-1], np.asarray(B, dtype=LD)[::-1])[::-1]


def samples_ld(mean, chol, normal):
    return mean[None, :] + T.ld(normal).dot(chol.T)


def alphas_ld(chol, values):
    return backward_substitution(chol, T.forward_substitution(chol, np.asarray(values, dtype=LD).T))


def evaluate_ld(gp, D, alpha, X):
    X = T.ld(np.atleast_2d(X))
    return _prior_ld(gp, X)[:, None] + T.kernel_matrix(gp.kern, X, T.ld(D)).dot(alpha)


def bound(restated, truth):
    """The engine's allowance for an array: FACTOR x max(the restatement's own largest error, one rounding of the
    largest entry of the truth) - from the restatement and the truth only."""
    own = float(np.max(np.abs(T.ld(restated) - truth))) if np.size(truth) else 0.0
    return FACTOR * max(own, ROUNDING * float(np.max(np.abs(truth)))), own


def distance(values, truth):
    return float(np.max(np.abs(T.ld(values) - truth)))


# ---- the blocked algorithm of csrc/sl_gp_sample.h -----------------------------------------------------------
def diag_factor(block):
    """Right-looking Cholesky of one block in the device's order: every entry loses ``l_ik l_ck`` with ascending
    ``k`` (one product, one subtraction each), then is divided by the square root of the pivot.
    -> ``(L, 0)`` or ``(partly factored block, 1-based failing column)``."""
    a = np.array(block, dtype=np.float64)
    nb = len(a)
    for j in range(nb):
        if not a[j, j] > 0.0:
            return np.tril(a), j + 1
        root = np.sqrt(a[j, j])
        a[j + 1:, j] = a[j + 1:, j] / root
        a[j, j] = root
        col = a[j + 1:, j]
        a[j + 1:, j + 1:] = a[j + 1:, j + 1:] - col[:, None] * col[None, :]
    return np.tril(a), 0


def panel_rows(panel, diag):
    """``X diag^T = panel`` row by row: ``x_j = (a_j - sum_{k<j} x_k l_jk) / l_jj`` with ascending ``k``."""
    x = np.array(panel, dtype=np.float64)
    for j in range(len(diag)):
        s = x[:, j].copy()
        for k in range(j):
            s = s - x[:, k] * diag[j, k]
        x[:, j] = s / diag[j, j]
    return x


def blocked_cholesky(matrix, nb=NB):
    """-> ``(L, info)``: the factorization block column by block column (diag_factor, panel_rows, the rest minus
    panel x panel^T); ``info`` as ``sl_cholesky`` reports it."""
    a = np.tril(np.array(matrix, dtype=np.float64))
    n = len(a)
    for r0 in range(0, n, nb):
        r1 = min(r0 + nb, n)
        a[r0:r1, r0:r1], fail = diag_factor(a[r0:r1, r0:r1])
        if fail:
            return a, r0 + fail
        if r1 < n:
            a[r1:, r0:r1] = panel_rows(a[r1:, r0:r1], a[r0:r1, r0:r1])
            a[r1:, r1:] = np.tril(a[r1:, r1:] - a[r1:, r0:r1].dot(a[r1:, r0:r1].T))
    return a, 0


# ---- cases ----------------------------------------------------------------------------------------------------
def notebook_gp(observations=0, seed=0):
    """The model of examples/1d_region_of_attraction_estimate.ipynb cell 5: inputs ``[x, u]``, ``Matern32 * Linear``
    on ``x``, prior mean ``0.25 x``, noise ``0.01^2`` - empty, or with observations of ``0.25 x + 0.1 sin(3 x)``."""
    kern = onp.Prod([onp.Matern32(1, variance=0.4 ** 2, lengthscales=1.0, active_dims=[0]),
                     onp.Linear(1, active_dims=[0])])
    rng = np.random.default_rng(seed)
    X = np.hstack((rng.uniform(-1, 1, (observations, 1)), np.zeros((observations, 1))))
    Y = 0.25 * X[:, :1] + 0.1 * np.sin(3 * X[:, :1])
    return onp.GPRCached(X, Y, kern, onp.LinearSystem((np.array([[0.25, 0.0]]),)), likelihood_variance=0.01 ** 2)


def notebook_points(n):
    return np.hstack((np.linspace(-1, 1, n)[:, None], np.zeros((n, 1))))


def grid_points(side):
    axis = np.linspace(-1, 1, side)
    mesh = np.meshgrid(axis, axis, indexing="ij")
    return np.stack([m.ravel() for m in mesh], axis=1)


def plane_gp(kind, lengthscale, observations, seed=1):
    """A 2-D GP without a mean function: RBF (sigma = 0.3, noise 1e-4) or Matern32 (sigma = 0.3, noise 1e-4)."""
    kern = (onp.RBF(2, variance=0.3 ** 2, lengthscales=lengthscale) if kind == "rbf"
            else onp.Matern32(2, variance=0.3 ** 2, lengthscales=lengthscale))
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1, 1, (observations, 2))
    Y = (0.2 * np.sin(2 * X[:, 0]) * np.cos(X[:, 1]))[:, None]
    return onp.GPRCached(X, Y, kern, None, likelihood_variance=1e-4)


def _cases():
    out = {}
    for obs in (0, 7):
        for n in (50, 129, 200):
            out["notebook_obs%d_n%d" % (obs, n)] = (lambda obs=obs: notebook_gp(obs), notebook_points(n), False)
    plan = [("rbf", ell, obs, side) for ell in (0.2, 0.5) for obs in (0, 5, 130) for side in (5, 8, 13, 17)]
    plan += [("matern", 0.5, obs, side) for obs in (0, 5, 130) for side in (8, 13, 17)]
    for kind, ell, obs, side in plan:
        out["%s_l%g_obs%d_n%d" % (kind, ell, obs, side * side)] = (
            lambda kind=kind, ell=ell, obs=obs: plane_gp(kind, ell, obs), grid_points(side), kind == "matern")
    out["single_point"] = (lambda: plane_gp("matern", 0.5, 5), np.array([[0.3, -0.2]]), True)
    return out


# name -> (builder of the oracle GPRCached, discretization [N, p], well conditioned: L itself is compared)
CASES = _cases()
# 33 x 33 points: only the backward error of the factorization is checked there, in float64
LARGE = {"matern_l0.5_obs%d_n1089" % obs: (lambda obs=obs: plane_gp("matern", 0.5, obs), grid_points(33))
         for obs in (0, 5, 130)}
RIGHT_HAND_SIDES = (1, 3, 10, 17)

_REFERENCES = {}


class Reference(object):
    """Restatement and truth of one case, computed once per process, shared and left unchanged."""

    def __init__(self, name):
        build, self.D, self.well_conditioned = CASES[name]
        self.name, self.gp = name, build()
        self.N = len(self.D)
        self.mean, self.cov = posterior(self.gp, self.D)
        self.mean_ld, self.cov_ld = posterior_ld(self.gp, self.D)
        self.chol = cholesky(self.cov)
        # every stage has the truth of ITS float64 input: the factor of the float64 covariance, the samples and
        # the alphas of the float64 factor - a stage is measured on what it is handed
        self.chol_ld = T.cholesky(T.ld(self.cov))
        self.normal = np.random.default_rng(11).standard_normal((max(RIGHT_HAND_SIDES), self.N))
        self.values = samples(self.mean, self.chol, self.normal)
        self.values_ld = samples_ld(T.ld(self.mean), T.ld(self.chol), self.normal)
        self.alpha = alphas(self.chol, self.values)
        self.alpha_ld = alphas_ld(T.ld(self.chol), T.ld(self.values))


def reference(name):
    if name not in _REFERENCES:
        _REFERENCES[name] = Reference(name)
    return _REFERENCES[name]


def package_gp(sl, gp):
    """The package's GaussianProcess of an oracle GPRCached (same kernel tree, same data)."""
    def convert(kern):
        if isinstance(kern, onp.Prod):
            return sl.functions.Prod([convert(k) for k in kern.kern_list])
        if isinstance(kern, onp.Add):
            return sl.functions.Add([convert(k) for k in kern.kern_list])
        if isinstance(kern, onp.RBF):
            return sl.RBF(kern.input_dim, variance=kern.variance, lengthscales=kern.lengthscales)
        if isinstance(kern, onp.Matern32):
            return sl.Matern32(kern.input_dim, variance=kern.variance, lengthscales=kern.lengthscales,
                               active_dims=kern.active_dims)
        if isinstance(kern, onp.Linear):
            return sl.Linear(kern.input_dim, variance=kern.variance, active_dims=kern.active_dims)
        raise TypeError(type(kern).__name__)
    mean = None if gp.mean_function is None else sl.LinearSystem((np.array(gp.mean_function.matrix),))
    model = sl.GPRCached(gp.X.reshape(-1, gp.X.shape[1]), gp.Y.reshape(-1, 1), convert(gp.kern), mean,
                         likelihood_variance=gp.likelihood_variance)
    return sl.GaussianProcess(model)
