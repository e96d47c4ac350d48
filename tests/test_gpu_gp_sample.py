"""GP sample paths on the GPU (needs an MI355X): ``sl_gp_posterior_cov``, ``sl_cholesky``, ``sl_tri_solve``,
``sl_tri_mult``, ``sl_gp_sample_eval`` and ``sample_gp_function`` against the long-double truth of
``tests/np_gp_sample.py``.

The rule of ``tests/test_gpu_gp_truth.py``: the engine may be off by 32 times the float64 restatement's own distance
from the truth, with a floor of one rounding of the largest entry (``np_gp_sample.bound``: from the restatement and
the truth only, per case).  Every stage is handed the restatement's float64 input of that stage and measured against
the long-double evaluation of the same input.  The factorization and the solves are also held to the textbook
backward-error bounds, which hold for any order of the sums (Higham, Thm 10.3 and 8.5), times two:
``|L L^T - C|_ij <= 2 (N + 1) 2^-53 sqrt(c_ii c_jj)``, ``|L X - B| <= 2 (N + 1) 2^-53 |L| |X|``.
Every test prints its figures before it asserts.

A sample function adds the prior mean to ``K(x, D) alpha`` as the reference's does - although ``alpha`` already
reproduces samples that contain it - so at the discretization of an empty GP it returns the sample values plus the
prior mean (the values themselves where there is no mean function).
"""

import numpy as np
import pytest

import np_gp_sample as S
import np_gp_truth as T

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
NAMES = list(S.CASES)
EVAL_SIZES = (1, 63, 64, 65, 1001)


def _ctx():
    from safe_learning_amd import _evaluate
    return _evaluate._ctx()


def _dev(array):
    import torch
    return torch.from_numpy(np.ascontiguousarray(array, dtype=np.float64)).to(_ctx().torch_device)


def _package(ref):
    import safe_learning_amd as sl
    return S.package_gp(sl, ref.gp)


def _prior(gp):
    return None if gp.mean_function is None else np.asarray(gp.mean_function.matrix)[0]


def _within(what, name, values, restated, truth):
    """Print the engine's and the restatement's distance from the truth, then hold the engine to the bound."""
    allowed, own = S.bound(restated, truth)
    got = S.distance(values, truth)
    print("gp sample [%s] %s: engine %.3g, restatement %.3g, allowed %.3g" % (name, what, got, own, allowed))
    assert np.isfinite(np.asarray(values)).all()
    assert got <= allowed, (name, what, got, own, allowed)


def _factor(matrix):
    import torch
    d_a = _dev(matrix)
    info = _ctx().cholesky(d_a)
    torch.cuda.synchronize()
    return d_a.cpu().numpy(), info


def _backward_error(L, C, wide=True):
    n = len(C)
    scale = np.sqrt(np.outer(np.diag(C), np.diag(C)))
    if wide:
        residual = np.abs(T.ld(L).dot(T.ld(L).T) - T.ld(C))
    else:
        residual = np.abs(L.dot(L.T) - C)
    worst = float(np.max(residual / (2 * (n + 1) * U * scale)))
    return worst


@pytest.mark.parametrize("name", NAMES)
def test_posterior_covariance(name):
    import torch
    ref = S.reference(name)
    gp = _package(ref).gaussian_process
    ctx, n = _ctx(), ref.N
    d_mean = torch.empty(n, dtype=torch.float64, device=ctx.torch_device)
    d_cov = torch.empty((n, n), dtype=torch.float64, device=ctx.torch_device)
    ctx.gp_posterior_cov(gp.X, gp.cholesky_inverse, gp.alpha, gp.kern._factors(ref.D.shape[1]), _prior(gp), _dev(ref.D),
                         S.JITTER, d_mean, d_cov)
    mean, cov = d_mean.cpu().numpy(), d_cov.cpu().numpy()
    _within("mean", name, mean, ref.mean, ref.mean_ld)
    _within("cov", name, cov, ref.cov, ref.cov_ld)
    assert np.array_equal(cov, cov.T)


@pytest.mark.parametrize("name", NAMES)
def test_cholesky(name):
    ref = S.reference(name)
    L, info = _factor(ref.cov)
    assert info == 0
    worst = _backward_error(L, ref.cov)
    print("gp sample [%s] cholesky: backward error %.3g of the bound (SciPy: %.3g)"
          % (name, worst, _backward_error(ref.chol, ref.cov)))
    assert np.array_equal(np.triu(L, 1), np.zeros_like(L))
    assert worst <= 1.0
    if ref.well_conditioned:
        _within("L", name, L, ref.chol, ref.chol_ld)
    again, _ = _factor(ref.cov)
    assert np.array_equal(L.view(np.uint64), again.view(np.uint64))


@pytest.mark.parametrize("name", list(S.LARGE))
def test_cholesky_33x33_grid(name):
    build, D = S.LARGE[name]
    _, cov = S.posterior(build(), D)
    L, info = _factor(cov)
    assert info == 0 and np.array_equal(np.triu(L, 1), np.zeros_like(L))
    worst = _backward_error(L, cov, wide=False)
    print("gp sample [%s] cholesky: backward error %.3g of the bound, in float64" % (name, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("name", NAMES)
def test_solves_and_product(name):
    import torch
    ref = S.reference(name)
    ctx, n = _ctx(), ref.N
    d_L, d_mean = _dev(ref.chol), _dev(ref.mean)
    Ll, absL = T.ld(ref.chol), np.abs(T.ld(ref.chol))
    for k in S.RIGHT_HAND_SIDES:
        z = ref.normal[:k]
        d_out = torch.empty((n, k), dtype=torch.float64, device=ctx.torch_device)
        ctx.tri_mult(d_L, _dev(z.T), d_mean, d_out)
        values = d_out.cpu().numpy()
        _within("samples k=%d" % k, name, values.T, ref.values[:k], ref.values_ld[:k])
        exact = T.ld(ref.mean)[:, None] + Ll.dot(T.ld(z).T)
        assert np.all(np.abs(T.ld(values) - exact)
                      <= 2 * (n + 2) * U * (np.abs(T.ld(ref.mean))[:, None] + absL.dot(np.abs(T.ld(z)).T)))
        # alpha = L^-T L^-1 values, from the restatement's values
        B = np.ascontiguousarray(ref.values[:k].T)
        d_B = _dev(B)
        ctx.tri_solve(d_L, d_B, False)
        half = d_B.cpu().numpy()
        assert np.all(np.abs(Ll.dot(T.ld(half)) - T.ld(B)) <= 2 * (n + 1) * U * absL.dot(np.abs(T.ld(half))))
        ctx.tri_solve(d_L, d_B, True)
        alpha = d_B.cpu().numpy()
        assert np.all(np.abs(Ll.T.dot(T.ld(alpha)) - T.ld(half)) <= 2 * (n + 1) * U * absL.T.dot(np.abs(T.ld(alpha))))
        _within("alphas k=%d" % k, name, alpha, ref.alpha[:, :k], ref.alpha_ld[:, :k])


@pytest.mark.parametrize("name", NAMES)
def test_sample_function_values(name):
    import torch
    ref = S.reference(name)
    gp = _package(ref).gaussian_process
    ctx, p = _ctx(), ref.D.shape[1]
    k = max(S.RIGHT_HAND_SIDES)
    alpha = np.ascontiguousarray(ref.alpha[:, :k])
    d_D, d_alpha = _dev(ref.D), _dev(alpha)
    X = np.random.default_rng(21).uniform(-1, 1, (max(EVAL_SIZES), p))

    def run(points):
        d_out = torch.empty((len(points), k), dtype=torch.float64, device=ctx.torch_device)
        ctx.gp_sample_eval(gp.kern._factors(p), _prior(gp), d_D, d_alpha, _dev(points), d_out)
        return d_out.cpu().numpy()

    results = {}
    restated, exact = S.evaluate(ref.gp, ref.D, alpha, X), S.evaluate_ld(ref.gp, ref.D, T.ld(alpha), X)
    for m in EVAL_SIZES:
        results[m] = run(X[:m])
        _within("f on %d points" % m, name, results[m], restated[:m], exact[:m])
    full = results[max(EVAL_SIZES)]
    for m in EVAL_SIZES:                                 # the same point inside two launches: the same bits
        assert np.array_equal(results[m].view(np.uint64), full[:m].view(np.uint64))
    at_D = run(ref.D)
    truth = S.evaluate_ld(ref.gp, ref.D, T.ld(alpha), ref.D)
    _within("f on the discretization", name, at_D, S.evaluate(ref.gp, ref.D, alpha, ref.D), truth)
    if len(ref.gp.X) == 0:
        # an empty GP: K alpha = (cov - 1e-8 I) alpha = values - 1e-8 alpha, and the prior mean on top
        expected = ref.values[:k].T + S.prior_mean(ref.gp, ref.D)[:, None]
        # (alpha is the restatement's: cov alpha = values up to ITS residual `own`, computed here in float64)
        allowed, _ = S.bound(S.evaluate(ref.gp, ref.D, alpha, ref.D), truth)
        own = float(np.max(np.abs(ref.cov.dot(alpha) - ref.values[:k].T)))
        slack = allowed + 2e-8 * float(np.max(np.abs(alpha))) + own
        print("gp sample [%s] f(D) - values - prior: %.3g (allowed %.3g)"
              % (name, float(np.max(np.abs(at_D - expected))), slack))
        assert np.max(np.abs(at_D - expected)) <= slack


def test_indefinite_matrix_ends_cleanly():
    """A negative diagonal entry at index 70 of 129: pivot 71 is the first that is not positive.  An ordinary error
    path: the call returns the error and the context works on."""
    from safe_learning_amd import HipEngineError
    import ctypes as C
    ctx = _ctx()
    bad = S.reference("notebook_obs7_n129").cov.copy()
    bad[70, 70] = -1.0
    d_bad = _dev(bad)
    info = C.c_int32(0)
    with pytest.raises(HipEngineError, match="pivot 71 of 129"):
        ctx.lib.sl_cholesky(ctx.handle, 129, C.c_void_p(d_bad.data_ptr()), 129, C.byref(info))
    assert info.value == 71
    assert ctx.cholesky(_dev(bad)) == 71
    # the columns in front of the pivot's block are the factor's, the context is usable: the next case runs on it
    partly = d_bad.cpu().numpy()
    ref = S.reference("notebook_obs7_n129")
    lead = ref.cov[:64, :64]                     # (two float64 factors of one block: cond x the backward error apart)
    assert np.max(np.abs(partly[:64, :64] - ref.chol[:64, :64])) <= 4 * 65 * U * np.linalg.cond(lead) * np.max(ref.chol)
    L, ok = _factor(ref.cov)
    assert ok == 0 and _backward_error(L, ref.cov) <= 1.0


def test_nan_pivot_ends_cleanly():
    bad = S.reference("matern_l0.5_obs5_n169").cov.copy()
    bad[130, 130] = np.nan
    assert _factor(bad)[1] == 131
    ref = S.reference("single_point")
    L, ok = _factor(ref.cov)
    assert ok == 0 and L[0, 0] == np.sqrt(ref.cov[0, 0])


def test_limits_are_refused():
    import torch
    from safe_learning_amd import HipEngineError
    ctx = _ctx()
    tiny = torch.zeros((1, 1), dtype=torch.float64, device=ctx.torch_device)
    with pytest.raises(HipEngineError, match="at most 1024"):
        ctx.lib.sl_tri_solve(ctx.handle, 1, 1025, tiny.data_ptr(), 1, 0, tiny.data_ptr())
    with pytest.raises(HipEngineError, match="at most 16384"):
        ctx.lib.sl_cholesky(ctx.handle, 16385, tiny.data_ptr(), 16385, None)
    with pytest.raises(HipEngineError, match="ld = 0"):
        ctx.lib.sl_cholesky(ctx.handle, 1, tiny.data_ptr(), 0, None)


PYTHON_CASES = ("notebook_obs0_n50", "notebook_obs7_n200", "rbf_l0.5_obs5_n169", "matern_l0.5_obs130_n289",
                "single_point")


@pytest.mark.parametrize("name", PYTHON_CASES)
def test_sample_gp_function_matches_the_restatement(name):
    """The whole chain with the draws given: samples, alphas and function values against the long-double chain; the
    allowance is the float64 restatement's distance from it."""
    import safe_learning_amd as sl
    ref = S.reference(name)
    gpfun = _package(ref)
    number = 3
    normal = ref.normal[:number]
    chol_ld = T.cholesky(ref.cov_ld)
    values_ld = S.samples_ld(ref.mean_ld, chol_ld, normal)
    alpha_ld = S.alphas_ld(chol_ld, values_ld)
    values = sl.sample_gp_function(ref.D, gpfun, number=number, return_function=False, standard_normal=normal)
    assert values.shape == (number, ref.N)
    _within("sample_gp_function values", name, values, ref.values[:number], values_ld)
    funs = sl.sample_gp_function(ref.D, gpfun, number=number, standard_normal=normal)
    assert np.array_equal(np.stack([f.values for f in funs]), values)
    _within("sample_gp_function alphas", name, np.stack([f.alpha for f in funs], axis=1), ref.alpha[:, :number], alpha_ld)
    X = np.random.default_rng(3).uniform(-1, 1, (65, ref.D.shape[1]))
    out = np.hstack([f(X, noise=False) for f in funs])
    _within("sample functions", name, out, S.evaluate(ref.gp, ref.D, ref.alpha[:, :number], X),
            S.evaluate_ld(ref.gp, ref.D, alpha_ld, X))
    replay = sl.GPSampleFunction.from_values(ref.D, gpfun, values)
    assert all(np.array_equal(f.alpha, g.alpha) for f, g in zip(funs, replay))


def test_sample_statistics_and_noise():
    """512 samples at 64 points with a fixed seed: the sample mean within 5 standard errors of the mean,
    sqrt(c_ii / 512), the sample variance within 5 of its own, c_ii sqrt(2 / 511), at every point."""
    import safe_learning_amd as sl
    import torch
    ref = S.reference("matern_l0.5_obs5_n64")
    gpfun = _package(ref)
    np.random.seed(7)
    values = sl.sample_gp_function(ref.D, gpfun, number=512, return_function=False)
    assert values.shape == (512, 64)
    var = np.diag(ref.cov)
    mean_z = np.abs(values.mean(axis=0) - ref.mean) / np.sqrt(var / 512)
    var_z = np.abs(values.var(axis=0, ddof=1) - var) / (var * np.sqrt(2.0 / 511))
    print("gp sample statistics: mean off by %.3g standard errors at the most, variance by %.3g"
          % (mean_z.max(), var_z.max()))
    assert mean_z.max() <= 5 and var_z.max() <= 5
    np.random.seed(7)
    assert np.array_equal(values, sl.sample_gp_function(ref.D, gpfun, number=512, return_function=False))
    f = sl.sample_gp_function(ref.D, gpfun)[0]
    quiet = f(ref.D[:10], noise=False)
    assert quiet.shape == (10, 1) and np.array_equal(quiet, f(ref.D[:10], noise=False))
    assert not np.array_equal(quiet, f(ref.D[:10]))
    on_device = f(torch.from_numpy(ref.D[:10, :1]).to(_ctx().torch_device),
                  torch.from_numpy(ref.D[:10, 1:]).to(_ctx().torch_device), noise=False)
    assert isinstance(on_device, torch.Tensor) and on_device.is_cuda and np.array_equal(on_device.cpu().numpy(), quiet)


def test_sampling_leaves_a_lyapunov_on_the_same_context_alone(monkeypatch):
    import cases
    import safe_learning_amd as sl
    from safe_learning_amd import _evaluate
    from safe_learning_amd.benchmarks import GP_VARIANTS, build_lyapunov
    case = cases.make_case("pendulum", num_points=24, n_gp=60, tau_scale=0.01, **GP_VARIANTS["informed"])
    lyap = build_lyapunov(case)
    lyap.update_safe_set()
    before, c_before = lyap.safe_set.copy(), lyap.c_max
    assert before.any()
    monkeypatch.setattr(_evaluate, "_ctx", lambda: lyap._ctx)
    ref = S.reference("notebook_obs7_n129")
    f = sl.sample_gp_function(ref.D, _package(ref), standard_normal=ref.normal[:1])[0]
    f(ref.D, noise=False)
    lyap.update_safe_set()
    assert np.array_equal(lyap.safe_set, before) and lyap.c_max == c_before
    fresh = build_lyapunov(case)
    fresh.update_safe_set()
    assert np.array_equal(fresh.safe_set, before) and fresh.c_max == c_before


NOTEBOOK_SEED = 5


def test_notebook_exploration_loop():
    """examples/1d_region_of_attraction_estimate.ipynb cells 5-14 on the 1 001-point grid: draw the true dynamics,
    then four rounds of 'most uncertain safe state -> measure it with the sample function -> add_data_point ->
    update_safe_set', side by side with the oracle's Lyapunov driven by the NumPy restatement of the same sample
    function (same alphas).  Chosen states and safe sets must be equal, measurements agree to 1e-9 relative."""
    import oracle
    import safe_learning_amd as sl
    from oracle import np_functions as onp
    D = S.notebook_points(50)
    ogp = S.notebook_gp(0)
    gpfun, ogpfun = S.package_gp(sl, ogp), onp.GaussianProcess(ogp)
    np.random.seed(NOTEBOOK_SEED)
    sl.sample_gp_function(D, gpfun, number=10, return_function=False)          # cell 6 draws these first
    true_dynamics = sl.sample_gp_function(D, gpfun)[0]
    alpha = true_dynamics.alpha[:, None]
    prior_gp = S.notebook_gp(0)                                                 # the sample function: prior kernel

    def restated(state, action):
        return S.evaluate(prior_gp, D, alpha, np.hstack((state, action)))

    tau = 1.0 / 1001
    policy, opolicy = sl.LinearSystem(np.array([[0.0]])), onp.LinearSystem((np.array([[0.0]]),))
    value = sl.Triangulation(sl.GridWorld([[-1.0, 1.0]], 3), np.array([[1.0], [0.0], [1.0]]))
    ovalue = onp.Triangulation(oracle.GridWorld([[-1.0, 1.0]], 3), np.array([[1.0], [0.0], [1.0]]))
    lyap = sl.Lyapunov(sl.GridWorld([[-1.0, 1.0]], 1001), value, gpfun, 0.25, 1.0, tau, policy)
    olyap = oracle.Lyapunov(oracle.GridWorld([[-1.0, 1.0]], 1001), ovalue, ogpfun, 0.25, 1.0, tau, opolicy)
    grid = lyap.discretization.all_points
    lyap.update_safe_set()
    olyap.update_safe_set()
    assert np.array_equal(lyap.safe_set, olyap.safe_set)
    initial = np.abs(grid.squeeze()) < 0.2
    lyap.initial_safe_set, olyap.initial_safe_set = initial, initial.copy()
    lyap.update_safe_set()
    olyap.update_safe_set()
    assert np.array_equal(lyap.safe_set, olyap.safe_set)
    sizes = [int(lyap.safe_set.sum())]
    for stage in range(4):
        safe_grid = grid[lyap.safe_set]
        _, std = gpfun(safe_grid, policy(safe_grid))
        _, ostd = ogpfun(safe_grid, opolicy(safe_grid))
        # The prior's uncertainty is symmetric in x, so the oracle's largest value can belong to x and -x EXACTLY (the
        # notebook's np.argmax then takes the first): the engine must choose one of those states, and both sides go on
        # with the first.  Any other state within 1e-9 of the largest is a near-tie: take another NOTEBOOK_SEED.
        largest = ostd[:, 0].max()
        tie = np.flatnonzero(ostd[:, 0] == largest)
        rest = np.delete(ostd[:, 0], tie)
        assert rest.size == 0 or largest - rest.max() > 1e-9 * largest, "near-tie of the most uncertain state"
        assert int(np.argmax(std)) in tie, (int(np.argmax(std)), tie)
        max_id = int(tie[0])
        state = safe_grid[[max_id], :].copy()
        action = policy(state)
        measurement = true_dynamics(state, action, noise=False)
        omeasurement = restated(state, opolicy(state))
        print("notebook loop, stage %d: state %.6g, measurement %.17g (restatement %.17g), %d safe"
              % (stage, state[0, 0], measurement[0, 0], omeasurement[0, 0], sizes[-1]))
        np.testing.assert_allclose(measurement, omeasurement, rtol=1e-9, atol=0)
        gpfun.add_data_point(np.hstack((state, action)), measurement)
        ogpfun.add_data_point(np.hstack((state, action)), omeasurement)
        lyap.update_safe_set()
        olyap.update_safe_set()
        assert np.array_equal(lyap.safe_set, olyap.safe_set)
        sizes.append(int(lyap.safe_set.sum()))
    assert len(gpfun.X) == 4 and sizes[-1] >= sizes[0] > 0, sizes
