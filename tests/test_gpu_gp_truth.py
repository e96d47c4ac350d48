"""The sweep kernels' GP posterior against the posterior in extended precision (needs an MI355X).

Every other GP test compares the engine (explicit ``L^-1`` on the matrix cores) with another float64 computation
under tolerances that grow with ``cond(K)``.  Here the yardstick is ``tests/np_gp_truth.py``: the posterior in long
double, which measures the oracle's OWN error per case; the engine gets 32 times that,

    |v - v_true| <= 32 max(e_oracle v_true, 2^-53 k(z, z))         per cell and column,
    |m - m_true| <= 32 max(max |m_oracle - m_true|, 2^-53 max |m_true|)   per column,

with ``e_oracle`` the oracle's largest relative variance error on the compared cells (the floor: one rounding of
``k(z, z) - |a|^2``, for cases the oracle gets exactly right).  The bounds come from the oracle and the truth only.
Variances are recovered from the records as ``(error / beta)^2``; every cell of a grid up to 3-D is compared, of a
4-D grid 1024 drawn cells plus the first and the last 64-cell block.  Every test prints the engine's error in units
of the oracle's and the share of variances below the truth (the unsafe side) before it asserts, and asserts which
kernel ran.  Figures of the last run: ``profiles/gp_posterior_truth.md``.
"""

import numpy as np
import pytest

import np_gp_truth as T
from test_gpu_reference_gp import sweep_records

pytestmark = pytest.mark.gpu


def _set_cfg(monkeypatch, cfg):
    if cfg is None:
        monkeypatch.delenv("SL_GP_CFG", raising=False)
    else:
        monkeypatch.setenv("SL_GP_CFG", cfg)


def _records(lyap, cells):
    lyap._upload_model()
    lyap._refresh_init_bits()
    rec, kernels = sweep_records(lyap, cells)
    assert rec.shape[0] == len(cells)
    return rec, kernels


def _check(name, ref, mean, err, kernels, expected):
    """Print the figures, then assert the kernel, the variance bound at every cell and the mean bound per column."""
    var = (np.asarray(err, dtype=np.float64) / ref.beta) ** 2
    fig = ref.measure(mean, var)
    T.report(name, " | ".join(sorted(kernels)), fig)
    for kernel in kernels:
        assert kernel.startswith(expected[0]) and all(part in kernel for part in expected), (kernel, expected)
    assert fig["finite"]
    assert fig["var_over_bound"] <= 1.0, (name, fig)
    assert fig["mean_over_bound"] <= 1.0, (name, fig)
    return fig


@pytest.mark.parametrize("name", list(T.CASES))
def test_sweep_posterior_against_the_truth(name, monkeypatch):
    from safe_learning_amd.benchmarks import build_lyapunov
    _, cfg, family, also = T.CASES[name]
    _set_cfg(monkeypatch, cfg)
    case, cells, ref = T.case_reference(name)
    d = case["d"]
    rec, kernels = _records(build_lyapunov(case), cells)
    _check(name, ref, rec[:, 2:2 + d], rec[:, 2 + d:], kernels, (family, also))


POINT_CASES = [("ill_1e-5", "k_gp_sweep4<"), ("informed_n400", "k_gp_sweep4<"), ("informed_n224", "k_gp_small<"),
               ("cartpole_run64_informed", "k_gp_sweep4<"), ("chain3_n300", "k_gp_sweep4<"),
               ("notebook_kernels_n130", "k_gp_small<")]


@pytest.mark.parametrize("name,family", POINT_CASES, ids=[n for n, _ in POINT_CASES])
def test_explicit_points_against_the_truth(name, family, monkeypatch):
    """``sl_eval_points``: 64 query points equal to training inputs bit for bit (the variance is as close to the noise
    floor as it gets) and 64 points far outside the data (the posterior is the prior)."""
    from safe_learning_amd import _evaluate
    from safe_learning_amd.benchmarks import build_specs
    _set_cfg(monkeypatch, None)
    case, _, grid_ref = T.case_reference(name)
    d, dyn = case["d"], case["dynamics"]
    dynamics = build_specs(case)[1]
    far = dyn["X"][:64] + 100.0 * np.where(np.arange(64)[:, None] % 2, 1.0, -1.0)
    points = [("training inputs", dyn["X"][:64].copy())]
    if "kernels" not in dyn:              # (a Linear leaf grows with |z|: only an RBF model returns to its prior)
        points.append(("far points", far))
    for what, Z in points:
        ref = T.Reference(grid_ref.model, Z, truth=grid_ref.truth)
        if what == "far points":          # the reference itself is at the prior: var = sigma^2, mean = m(z)
            assert np.all(ref.var_true == ref.prior_var) and np.all(ref.var_oracle == dyn["variance"])
            assert np.all(ref.mean_true == T.ld(Z).dot(T.ld(dyn["prior"]).T))
        else:
            assert np.all(ref.var_oracle > 0) and np.all(ref.var_true < 0.1 * ref.prior_var)
        mean, err = _evaluate.dynamics(dynamics, Z[:, :d], Z[:, d:])
        kernel = _evaluate._ctx().last_kernel()
        assert mean.shape == (64, d) and err.shape == (64, d)
        _check("%s, %s" % (name, what), ref, mean, err, {kernel}, (family,))


def test_appended_observations_against_the_truth(monkeypatch):
    """64 ``add_data_point`` calls on an uploaded 100-point head (it grows across 128 points), one upload after each
    as the exploration loop does it: the engine extends ``L^-1`` by rank-one rows.  Truth and oracle are built from
    all 164 points at once; the appended model gets the bound of any other, and a model built from scratch in a
    fresh object is measured beside it."""
    import safe_learning_amd as sl
    from safe_learning_amd.benchmarks import build_lyapunov, build_specs, initial_safe_mask
    _set_cfg(monkeypatch, None)
    full, base = T.appended_case()
    cells = T.compared_cells(full)
    ref = T.oracle_error(full, cells)
    d = full["d"]
    policy, dynamics, value, lv = build_specs(base)
    lyap = sl.Lyapunov(sl.GridWorld(base["limits"], base["num_points"]), value, dynamics, base["lf"], lv,
                       base["tau"], policy, initial_set=initial_safe_mask(base))
    lyap._upload_model()
    rows = []
    append = lyap._ctx.gp_append_point
    monkeypatch.setattr(lyap._ctx, "gp_append_point", lambda *args: rows.append(append(*args)) or rows[-1])
    X, Y = full["dynamics"]["X"], full["dynamics"]["Y"]
    for i in range(100, 164):
        dynamics.add_data_point(X[[i]], Y[[i]])
        lyap._upload_model()
    print("gp truth [appended_100+64]: %d of 64 observations reached the device as rank-one rows" % sum(rows))
    assert sum(rows) >= 48                # (the head is re-packed when its padded capacity is exhausted)
    rec, kernels = _records(lyap, cells)
    appended = _check("appended_100+64", ref, rec[:, 2:2 + d], rec[:, 2 + d:], kernels, ("k_gp_small<",))
    rec, kernels = _records(build_lyapunov(full), cells)
    fresh = _check("fresh_164", ref, rec[:, 2:2 + d], rec[:, 2 + d:], kernels, ("k_gp_small<",))
    print("gp truth [appended_100+64]: appended %.3g x oracle, fresh %.3g x oracle"
          % (appended["var_ratio"], fresh["var_ratio"]))
