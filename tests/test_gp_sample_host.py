"""Host tests of GP sampling: the blocked factorization of csrc/sl_gp_sample.h run on the host (a stand-alone
program under the sanitizers, tests/hostsim/gp_sample.cpp) against the NumPy restatement (tests/np_gp_sample.py),
the restatement against its own long-double version and against the oracle's posterior variance, and the Python
layer (``sample_gp_function``, ``GPSampleFunction``) on a stand-in engine that computes with NumPy.

The bounds are derived, not measured.  With u = 2^-53:
  * factorization (Higham, Accuracy and Stability of Numerical Algorithms, Thm 10.3): |L L^T - C|_ij <=
    gamma_(N+1) sqrt(c_ii c_jj) / (1 - gamma) for any order of the sums; the tests allow 2 (N + 1) u sqrt(c_ii c_jj);
  * substitution and products (Thm 8.5, Sec. 3.5): |L x - b| <= gamma_N |L| |x| and |y - L z| <= gamma_N |L| |z|
    componentwise, for any order of the sums; the tests allow 2 (N + 1) u times the right-hand sides.
"""

import os
import subprocess

import numpy as np
import pytest
import scipy.linalg

import np_gp_sample as S
import np_gp_truth as T
from conftest import ROOT
from hostsim_build import SHIM_FLAGS, sanitized_program_or_plain

U = 2.0 ** -53
SIZES = (1, 2, 63, 64, 65, 128, 129, 200)
RHS = 3


def _spd(n, seed=3):
    """A well-conditioned covariance: Matern32 (sigma = 0.3, l = 0.5) at n random points of the plane, plus 1e-8."""
    points = np.random.default_rng(seed).uniform(-1, 1, (n, 2))
    return S.plane_gp("matern", 0.5, 0).kern.K(points, points) + 1e-8 * np.eye(n)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return sanitized_program_or_plain("gp_sample.cpp", tmp_path_factory.mktemp("gp_sample"), SHIM_FLAGS)


def _run(program, tmp_path, A, B):
    n, k = B.shape
    src, dst = os.path.join(str(tmp_path), "in.bin"), os.path.join(str(tmp_path), "out.bin")
    with open(src, "wb") as handle:
        handle.write(np.array([n, k], dtype=np.int64).tobytes())
        handle.write(np.ascontiguousarray(A, dtype=np.float64).tobytes())
        handle.write(np.ascontiguousarray(B, dtype=np.float64).tobytes())
    subprocess.check_call([program, src, dst])
    flat = np.fromfile(dst, dtype=np.float64)
    assert flat.size == 1 + n * n + 3 * n * k
    info, rest = int(flat[0]), flat[1:]
    L = rest[:n * n].reshape(n, n)
    fwd, bwd, prod = (rest[n * n + i * n * k:n * n + (i + 1) * n * k].reshape(n, k) for i in range(3))
    return info, L, fwd, bwd, prod


@pytest.mark.parametrize("n", SIZES)
def test_blocked_algorithm_on_the_host(program, tmp_path, n):
    C = _spd(n)
    B = np.random.default_rng(n).standard_normal((n, RHS))
    info, L, fwd, bwd, prod = _run(program, tmp_path, C, B)
    assert info == 0
    assert np.array_equal(np.triu(L, 1), np.zeros((n, n)))
    restated, rinfo = S.blocked_cholesky(C)
    assert rinfo == 0
    # bit for bit where the order is the same: the first diagonal block (a NumPy loop in the device's order) and
    # the panel under it (substitution row by row)
    nb = min(n, S.NB)
    first, fail = S.diag_factor(C[:nb, :nb])
    assert fail == 0 and np.array_equal(L[:nb, :nb], first)
    assert np.array_equal(L[:, :nb], restated[:, :nb])
    # the rest differs in the order of the sums between blocks only: both within the backward-error bound
    scale = np.sqrt(np.outer(np.diag(C), np.diag(C)))
    for factor in (L, restated):
        residual = np.abs(T.ld(factor).dot(T.ld(factor).T) - T.ld(C))
        assert np.all(residual <= 2 * (n + 1) * U * scale)
    assert np.max(np.abs(L - restated)) <= 64 * n * U * np.max(np.abs(L)) * np.linalg.cond(C) ** 0.5
    # solves and product: componentwise residuals, in long double
    Ll, absL = T.ld(L), np.abs(T.ld(L))
    assert np.all(np.abs(Ll.dot(T.ld(fwd)) - T.ld(B)) <= 2 * (n + 1) * U * absL.dot(np.abs(T.ld(fwd))))
    assert np.all(np.abs(Ll.T.dot(T.ld(bwd)) - T.ld(B)) <= 2 * (n + 1) * U * absL.T.dot(np.abs(T.ld(bwd))))
    assert np.all(np.abs(T.ld(prod) - Ll.dot(T.ld(B))) <= 2 * (n + 1) * U * absL.dot(np.abs(T.ld(B))))
    # and against SciPy's solves of the same system: forward errors within cond(L) x the same allowance
    cond = np.linalg.cond(L)
    for got, want in ((fwd, scipy.linalg.solve_triangular(L, B, lower=True)),
                      (bwd, scipy.linalg.solve_triangular(L.T, B, lower=False)), (prod, L.dot(B))):
        assert np.max(np.abs(got - want)) <= 4 * (n + 1) * U * cond * np.max(np.abs(want))


@pytest.mark.parametrize("n, index", [(200, 10), (200, 63), (200, 64), (200, 199), (129, 128), (65, 0)])
def test_failing_pivot_index(program, tmp_path, n, index):
    """A negative diagonal entry at ``index`` makes pivot ``index + 1`` the first that is not positive: in the
    first block, at a block boundary (last column of a block, first column of the next), in the last block."""
    C = _spd(n)
    C[index, index] = -1.0
    info, L, _, _, _ = _run(program, tmp_path, C, np.ones((n, 1)))
    assert info == index + 1
    assert S.blocked_cholesky(C)[1] == index + 1
    with pytest.raises(np.linalg.LinAlgError, match="%d-th leading minor" % (index + 1)):
        scipy.linalg.cholesky(C, lower=True)
    # the columns before the pivot are the factor of the leading block
    # (two float64 factorizations of one matrix: apart by cond x the backward error at the most)
    if index:
        lead = C[:index, :index]
        good = scipy.linalg.cholesky(lead, lower=True)
        assert np.max(np.abs(L[:index, :index] - good)) <= 4 * (index + 1) * U * np.linalg.cond(lead) * np.max(good)


def test_nan_counts_as_a_failing_pivot(program, tmp_path):
    C = _spd(70)
    C[66, 66] = np.nan
    assert _run(program, tmp_path, C, np.ones((70, 1)))[0] == 67


# ---- the restatement ------------------------------------------------------------------------------------------
HOST_CASES = ("notebook_obs0_n50", "notebook_obs7_n129", "rbf_l0.2_obs5_n64", "rbf_l0.5_obs130_n169",
              "matern_l0.5_obs130_n289", "matern_l0.5_obs0_n64", "single_point")


def _shortest_lengthscale(kern):
    if hasattr(kern, "kern_list"):
        return min(_shortest_lengthscale(k) for k in kern.kern_list)
    return float(np.min(kern.lengthscales)) if hasattr(kern, "lengthscales") else 1.0


def _train_allowance(gp, D):
    """Allowance for the float64 posterior against long double.  A kernel entry carries the rounding of its squared
    distance - the oracle expands it as |x|^2 + |x'|^2 - 2 x.x', terms of size p / l^2 on [-1, 1]^p, so the entry is
    off by 64 u (1 + p / l^2) max|K| at the most - and with n observations the product a^T a (and a^T alpha)
    amplifies that, and the rounding of L^-1, by cond(K + sigma_n^2 I) per term: a factor 1 + 8 n cond."""
    kmax = float(np.max(np.abs(gp.kern.K(D, D))))
    n, p = len(gp.X), D.shape[1]
    entry = 64 * U * (1 + p / _shortest_lengthscale(gp.kern) ** 2) * kmax
    if n == 0:
        return entry
    cond = float(np.linalg.cond(gp.kern.K(gp.X) + gp.likelihood_variance * np.eye(n)))
    return entry * (1 + 8 * n * cond)


@pytest.mark.parametrize("name", HOST_CASES)
def test_restatement_against_long_double(name):
    ref = S.reference(name)
    allowance = _train_allowance(ref.gp, ref.D)
    ymax = max(1.0, float(np.max(np.abs(ref.gp.Y))) if len(ref.gp.Y) else 1.0)
    print("%s: cov error %.3g, mean error %.3g, allowance %.3g" % (name, S.distance(ref.cov, ref.cov_ld),
                                                                   S.distance(ref.mean, ref.mean_ld), allowance))
    assert S.distance(ref.cov, ref.cov_ld) <= allowance
    assert S.distance(ref.mean, ref.mean_ld) <= allowance * ymax / min(1.0, ref.gp.likelihood_variance ** 0.5)
    n, scale = ref.N, np.sqrt(np.outer(np.diag(ref.cov), np.diag(ref.cov)))
    Ll = T.ld(ref.chol)
    assert np.all(np.abs(Ll.dot(Ll.T) - T.ld(ref.cov)) <= 2 * (n + 1) * U * scale)
    # samples: a product; alphas: two substitutions (residuals of the float64 results, in long double)
    z = T.ld(ref.normal)
    assert np.all(np.abs(T.ld(ref.values) - (T.ld(ref.mean)[None, :] + z.dot(Ll.T)))
                  <= 2 * (n + 2) * U * (np.abs(T.ld(ref.mean))[None, :] + np.abs(z).dot(np.abs(Ll).T)))
    half = T.forward_substitution(Ll, T.ld(ref.values).T)
    assert np.all(np.abs(Ll.T.dot(T.ld(ref.alpha)) - half)
                  <= 4 * (n + 1) * U * (np.abs(Ll).T.dot(np.abs(T.ld(ref.alpha))) + np.abs(half)) * np.linalg.cond(ref.chol))
    # the sample functions return the sample values at the discretization of an empty GP
    if len(ref.gp.X) == 0:
        # (plus the prior mean once more: the reference's functions add it to K alpha, and alpha already
        # reproduces samples that contain it; K alpha = (cov - 1e-8 I) alpha = values - 1e-8 alpha)
        back = S.evaluate_ld(ref.gp, ref.D, ref.alpha_ld, ref.D)
        expected = ref.values_ld.T + T.ld(S.prior_mean(ref.gp, ref.D))[:, None]
        assert float(np.max(np.abs(back - expected))) <= 2 * 1e-8 * float(np.max(np.abs(ref.alpha_ld)))


@pytest.mark.parametrize("name", [n for n in HOST_CASES if "obs0" not in n])
def test_covariance_diagonal_is_the_oracles_variance(name):
    """``diag(cov) - 1e-8 = var`` of ``oracle/np_functions.py``'s ``build_predict`` (two float64 computations of the
    same number: twice the allowance; a Matern32 leaf's ``K(x, x)`` lies 1.5e-12 relative below its ``Kdiag``)."""
    ref = S.reference(name)
    _, var = ref.gp.build_predict(ref.D)
    kdiag = ref.gp.kern.Kdiag(ref.D)
    allowance = 2 * _train_allowance(ref.gp, ref.D) + 2e-12 * float(np.max(kdiag)) + 2 * U * 1e-8
    assert np.max(np.abs(np.diag(ref.cov) - S.JITTER - var[:, 0])) <= allowance


# ---- the Python layer on a stand-in engine --------------------------------------------------------------------
def _factor_kernel(factors, A, B):
    """``K(A, B)`` of a ``Kern._factors`` list, by the formulas of include/sl_hip.h."""
    total, prod, cur = 0.0, 1.0, 0
    for kind, product, variance, inv_ls in factors:
        if product != cur:
            total, prod, cur = total + prod, 1.0, product
        if kind == 2:
            v = (A * variance).dot(B.T)
        else:
            diff = (A[:, None, :] - B[None, :, :]) * inv_ls
            r2 = np.einsum("ijk,ijk->ij", diff, diff)
            if kind == 0:
                v = variance[0] * np.exp(-0.5 * r2)
            else:
                r = np.sqrt(3.0) * np.sqrt(r2 + 1e-12)
                v = variance[0] * (1.0 + r) * np.exp(-r)
        prod = prod * v
    return total + prod


class _FakeEngine(object):
    """The five engine calls of the sampling functions, computed with NumPy on CPU tensors."""

    def __init__(self):
        import torch
        self.torch_device, self.calls = torch.device("cpu"), []

    def gp_posterior_cov(self, X, Linv, alpha, factors, prior, d_Z, jitter, d_mean, d_cov):
        import torch
        self.calls.append("gp_posterior_cov")
        Z = d_Z.numpy()
        mean = np.zeros(len(Z)) if prior is None else Z.dot(prior)
        cov = _factor_kernel(factors, Z, Z)
        if len(X):
            a = np.asarray(Linv).dot(_factor_kernel(factors, np.asarray(X), Z))
            mean, cov = a.T.dot(np.reshape(alpha, -1)) + mean, cov - a.T.dot(a)
        d_mean.copy_(torch.from_numpy(mean))
        d_cov.copy_(torch.from_numpy(cov + jitter * np.eye(len(Z))))

    def cholesky(self, d_A):
        import torch
        self.calls.append("cholesky")
        L, info = S.blocked_cholesky(d_A.numpy())
        d_A.copy_(torch.from_numpy(L))
        return info

    def tri_solve(self, d_L, d_B, transpose=False):
        import torch
        self.calls.append("tri_solve")
        L = d_L.numpy()
        d_B.copy_(torch.from_numpy(scipy.linalg.solve_triangular(L.T if transpose else L, d_B.numpy(),
                                                                 lower=not transpose)))

    def tri_mult(self, d_L, d_Zn, d_mean, d_out):
        import torch
        self.calls.append("tri_mult")
        d_out.copy_(torch.from_numpy(d_mean.numpy()[:, None] + d_L.numpy().dot(d_Zn.numpy())))

    def gp_sample_eval(self, factors, prior, d_D, d_alpha, d_points, d_out):
        import torch
        self.calls.append("gp_sample_eval")
        X = d_points.numpy()
        mean = np.zeros(len(X)) if prior is None else X.dot(prior)
        d_out.copy_(torch.from_numpy(mean[:, None] + _factor_kernel(factors, X, d_D.numpy()).dot(d_alpha.numpy())))


@pytest.fixture
def fake_engine(monkeypatch):
    from safe_learning_amd import _evaluate
    engine = _FakeEngine()
    monkeypatch.setattr(_evaluate, "_ctx", lambda: engine)
    return engine


def _notebook(sl, observations=0):
    oracle_gp = S.notebook_gp(observations)
    return oracle_gp, S.package_gp(sl, oracle_gp)


def test_samples_alphas_and_functions(fake_engine):
    import safe_learning_amd as sl
    for observations in (0, 7):
        ogp, gpfun = _notebook(sl, observations)
        D = S.notebook_points(50)
        normal = np.random.default_rng(2).standard_normal((4, 50))
        values = sl.sample_gp_function(D, gpfun, number=4, return_function=False, standard_normal=normal)
        assert isinstance(values, np.ndarray) and values.shape == (4, 50)
        mean, cov = S.posterior(ogp, D)
        chol = S.cholesky(cov)
        np.testing.assert_allclose(values, S.samples(mean, chol, normal), rtol=0, atol=1e-12)
        funs = sl.sample_gp_function(D, gpfun, number=4, standard_normal=normal)
        assert len(funs) == 4 and all(isinstance(f, sl.GPSampleFunction) for f in funs)
        alpha = S.alphas(chol, values)
        for i, f in enumerate(funs):
            assert f.alpha.shape == (50,) and f.values.shape == (50,) and f.discretization.shape == (50, 2)
            np.testing.assert_array_equal(f.values, values[i])
            np.testing.assert_allclose(f.alpha, alpha[:, i], rtol=1e-6, atol=1e-6 * np.max(np.abs(alpha)))
        X = np.random.default_rng(4).uniform(-1, 1, (9, 2))
        out = funs[1](X, noise=False)
        assert isinstance(out, np.ndarray) and out.shape == (9, 1)
        np.testing.assert_allclose(out[:, 0], S.evaluate(ogp, D, funs[1].alpha[:, None], X)[:, 0], rtol=1e-12, atol=1e-12)
        # states and actions are concatenated; tensors in, tensors out
        import torch
        np.testing.assert_array_equal(funs[1](X[:, :1], X[:, 1:], noise=False), out)
        t_out = funs[1](torch.from_numpy(X[:, :1]), torch.from_numpy(X[:, 1:]), noise=False)
        assert isinstance(t_out, torch.Tensor) and np.array_equal(t_out.numpy(), out)
        # from given values: the same alphas
        again = sl.GPSampleFunction.from_values(D, gpfun, values)
        for f, g in zip(funs, again):
            np.testing.assert_array_equal(f.alpha, g.alpha)
        if observations == 0:      # empty GP: the functions return their values at the discretization - plus the
            # prior mean a second time, as the reference's do (alpha already reproduces samples that contain it)
            np.testing.assert_allclose(funs[0](D, noise=False)[:, 0], values[0] + S.prior_mean(ogp, D), rtol=0,
                                       atol=2e-8 * np.max(np.abs(funs[0].alpha)))
    assert set(fake_engine.calls) == {"gp_posterior_cov", "cholesky", "tri_solve", "tri_mult", "gp_sample_eval"}


def test_grid_world_discretization(fake_engine):
    import safe_learning_amd as sl
    gpfun = S.package_gp(sl, S.plane_gp("matern", 0.5, 5))
    grid = sl.GridWorld([[-1, 1], [-1, 1]], 4)
    funs = sl.sample_gp_function(grid, gpfun)
    assert len(funs) == 1 and np.array_equal(funs[0].discretization, grid.all_points)


def test_global_generator(fake_engine):
    import safe_learning_amd as sl
    _, gpfun = _notebook(sl)
    D = S.notebook_points(50)
    np.random.seed(5)
    first = sl.sample_gp_function(D, gpfun, number=10, return_function=False)
    second = sl.sample_gp_function(D, gpfun, number=10, return_function=False)
    np.random.seed(5)
    again = sl.sample_gp_function(D, gpfun, number=10, return_function=False)
    assert np.array_equal(first, again) and not np.array_equal(first, second)
    np.random.seed(5)
    normal = np.random.standard_normal((10, 50))
    assert np.array_equal(first, sl.sample_gp_function(D, gpfun, number=10, return_function=False,
                                                       standard_normal=normal))
    # the measurement noise comes from the same generator
    f = sl.sample_gp_function(D, gpfun, standard_normal=normal[:1])[0]
    X = D[:7]
    quiet = f(X, noise=False)
    assert np.array_equal(quiet, f(X, noise=False))
    np.random.seed(9)
    noisy = f(X)
    np.random.seed(9)
    expected = quiet + np.sqrt(gpfun.gaussian_process.likelihood_variance) * np.random.standard_normal((7, 1))
    assert np.array_equal(noisy, expected) and not np.array_equal(noisy, quiet)


def test_refusals(fake_engine, monkeypatch):
    import safe_learning_amd as sl
    from safe_learning_amd import distributed
    _, gpfun = _notebook(sl)
    D = S.notebook_points(50)
    with pytest.raises(ValueError, match=r"\[N, 2\]"):
        sl.sample_gp_function(D[:, :1], gpfun)
    with pytest.raises(ValueError, match="number"):
        sl.sample_gp_function(D, gpfun, number=0)
    with pytest.raises(ValueError, match="standard_normal"):
        sl.sample_gp_function(D, gpfun, number=2, standard_normal=np.zeros((2, 49)))
    with pytest.raises(TypeError, match="GaussianProcess"):
        sl.sample_gp_function(D, gpfun.gaussian_process)
    with pytest.raises(ValueError, match=r"from_values.*\[number, 50\]"):
        sl.GPSampleFunction.from_values(D, gpfun, np.zeros((1, 49)))
    f = sl.sample_gp_function(D, gpfun)[0]
    with pytest.raises(ValueError, match="2 inputs"):
        f(D[:, :1], noise=False)
    with pytest.raises(TypeError):
        f(D, noisy=False)
    # two outputs: the reference's squeeze(-1) only works for one
    two = sl.GPRCached(np.zeros((1, 2)), np.zeros((1, 2)), sl.RBF(2), likelihood_variance=0.1)
    with pytest.raises(ValueError, match="sample_gp_function.*output_dim 2"):
        sl.sample_gp_function(D, sl.GaussianProcess(two))
    # a covariance that cannot be factored
    bad = sl.GPRCached(np.empty((0, 2)), np.empty((0, 1)), sl.RBF(2, variance=-1.0), likelihood_variance=0.1)
    with pytest.raises(np.linalg.LinAlgError, match="pivot 1 "):
        sl.sample_gp_function(D, sl.GaussianProcess(bad))
    monkeypatch.setattr(distributed, "rank_and_world", lambda: (0, 2))
    with pytest.raises(NotImplementedError, match="sample_gp_function"):
        sl.sample_gp_function(D, gpfun)
    with pytest.raises(NotImplementedError, match="from_values"):
        sl.GPSampleFunction.from_values(D, gpfun, np.zeros((1, 50)))
