"""The variance floor of ``k_gp_sweep4``'s early decision: the lower bound of a cell's decrease uses
``err = beta sqrt(c_s var - 2 delta)`` instead of ``err = 0``, with constants ``c_s`` of the model
that ``sl_gp_set_head`` certifies on the host (safe_learning_amd/csrc/sl_gp_floor.h).  Cells that fail
because of their uncertainty are then decided before the last panel - and every mask word and the
64-byte sweep record must stay what ``SL_GP4_EARLY=0`` (every panel of every tile) gives, compared
with ``assert_array_equal``: no tolerance.  Needs an MI355X."""

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import cases
from test_gpu_gp4_blocks import _blocks_vs_plain
from test_gpu_gp4_early import RP, SLAB_HI, SLAB_LO, _informed, _slab_case
from test_gpu_gp4_mean_kernel import _split_vs_plain

pytestmark = pytest.mark.gpu


def _exact_floor(gp):
    """sigma_n^2 sigma_min(Linv[m:, m:])^2 at the panel boundaries m = 0, 256, ... of a host model."""
    linv = gp.cholesky_inverse
    return np.array([gp.likelihood_variance * np.linalg.svd(linv[m:, m:], compute_uv=False)[-1] ** 2
                     for m in range(0, len(linv), RP)])


def _raw_sweep(lyap):
    """One sl_lyap_sweep over the whole grid on the model's own context: (mask words, record)."""
    import torch
    n = lyap.discretization.nindex
    lyap._upload_model()                                         # (follows add_data_point with row uploads)
    lyap._refresh_init_bits()
    bits = torch.zeros((n + 63) // 64, dtype=torch.int64, device=lyap._ctx.torch_device)
    record = torch.zeros_like(lyap._d_result)
    lyap._ctx.lyap_sweep(0, n, lyap._d_init, lyap._values_arg(), bits, record, None)
    return bits.cpu().numpy().copy(), record.cpu().numpy().copy()


def test_headline_slab(monkeypatch):
    """The slab of tests/test_gpu_gp4_blocks.py, the launch's own workgroups and one."""
    _blocks_vs_plain(_slab_case(), monkeypatch, (None, 1), lo=SLAB_LO, hi=SLAB_HI)


def test_survey_hyper_parameters_at_the_headline_tau_in_three_segments(monkeypatch):
    """The case the floor decides most of (profiles/floor_cpu_counts.txt): the `survey` model of 1024
    points on the headline's discretisation constant, 2048 tiles of an 8 x 8 x 16 x 128 grid, in
    segments of 700 source tiles."""
    from safe_learning_amd.benchmarks import headline_case
    case = headline_case(variant="survey")
    case["tau"] = headline_case()["tau"]
    case["num_points"] = [8, 8, 16, 128]
    _, note = _split_vs_plain(case, monkeypatch, 700, caps=(None, 1))
    assert "3 segment(s)" in note, note


@pytest.mark.parametrize("n_gp", [257, 600])
def test_two_and_three_panels_with_a_ragged_last_one(monkeypatch, n_gp):
    """257 points: the second panel holds one row.  600 points: three panels, the last of 88 rows."""
    case = cases.make_case("cartpole", num_points=[6, 6, 6, 64], n_gp=n_gp, **_informed(tau_scale=0.0005))
    _blocks_vs_plain(case, monkeypatch, (None, 1))
    _split_vs_plain(case, monkeypatch, 100, caps=(None,))


def test_two_and_three_dimensions_with_kinked_rows_and_a_ragged_end(monkeypatch):
    """Pendulum 64 x 24 (rows end inside the 16-cell blocks and cross the saturation kinks of the
    policy) and a 16 x 16 x 24 grid, 300 points, both ending 23 cells into a tile."""
    pendulum = cases.make_case("pendulum", num_points=[64, 24], n_gp=300, **_informed(tau_scale=0.0005))
    hi = 64 * 20 + 23
    plain = _blocks_vs_plain(pendulum, monkeypatch, (None, 1), lo=0, hi=hi)
    assert plain[3].startswith("k_gp_sweep4<d=2"), plain[3]
    _split_vs_plain(pendulum, monkeypatch, 8, plain=plain, lo=0, hi=hi)
    chain = cases.make_case_3d(num_points=[16, 16, 24], dynamics="gp", n_gp=300, tau_scale=0.0005)
    hi = 64 * 90 + 23
    plain = _blocks_vs_plain(chain, monkeypatch, (None, 1), lo=0, hi=hi)
    assert plain[3].startswith("k_gp_sweep4<d=3"), plain[3]
    _split_vs_plain(chain, monkeypatch, 40, plain=plain, lo=0, hi=hi)


def test_constants_in_use_are_the_certified_ones(monkeypatch):
    """The getter (it reads the device words back) against NumPy: at most the exact sigma_n^2 sigma_min^2
    of every block, at least 0.98 of it (the window of tests/test_gp_floor_host.py), zero behind the last
    boundary - and all zero, at no cost, where the early decision is off at upload."""
    from safe_learning_amd.benchmarks import build_lyapunov
    monkeypatch.delenv("SL_GP4_EARLY", raising=False)
    for case in (_slab_case(), cases.make_case("cartpole", num_points=[6, 6, 6, 64], n_gp=600,
                                                **_informed(tau_scale=0.0005))):
        lyap = build_lyapunov(case)
        lyap.update_safe_set()                                   # uploads the head
        exact = _exact_floor(lyap.dynamics.gaussian_process)
        got = lyap._ctx.gp_variance_floor(0, len(exact) + 1)
        print("exact", exact, "in use", got)
        assert (got[:-1] <= exact).all() and (got[:-1] >= 0.98 * exact).all()
        assert got[-1] == 0.0
    # a context whose early decision is off when the head is uploaded does not pay for the constants
    monkeypatch.setenv("SL_GP4_EARLY", "0")
    lyap = build_lyapunov(case)
    lyap.update_safe_set()
    assert_array_equal(lyap._ctx.gp_variance_floor(0, 4), np.zeros(4))
    with pytest.raises(Exception, match="sl_gp_variance_floor"):
        lyap._ctx.gp_variance_floor(0, 33)


def test_an_appended_head_has_no_floor_and_sweeps_like_a_fresh_upload(monkeypatch):
    """sl_gp_append_point: a new row grows the Schur complements, so the constants are zero until the
    next full upload - and the sweep equals the one after a fresh upload of the same points and
    factors, which has its floor again."""
    from safe_learning_amd.benchmarks import _true_dynamics_numpy, build_lyapunov
    monkeypatch.delenv("SL_GP4_EARLY", raising=False)
    case = cases.make_case("cartpole", num_points=[6, 6, 6, 64], n_gp=300, **_informed(tau_scale=0.0005))
    lyap = build_lyapunov(case)
    ctx = lyap._ctx
    _raw_sweep(lyap)                                             # uploads the head
    assert (ctx.gp_variance_floor(0, 2) > 0.0).all()
    uploads = {"rows": 0}
    rows = ctx.gp_append_point
    ctx.gp_append_point = lambda *a, **k: (uploads.__setitem__("rows", uploads["rows"] + 1), rows(*a, **k))[1]
    x_new = np.random.default_rng(21).uniform(-1, 1, (3, case["d"] + 1))
    lyap.dynamics.add_data_point(x_new, _true_dynamics_numpy(case, x_new))
    appended = _raw_sweep(lyap)
    assert uploads["rows"] == 3
    assert "early decision" in ctx.last_kernel()
    assert_array_equal(ctx.gp_variance_floor(0, 4), np.zeros(4))
    gp = lyap.dynamics.gaussian_process
    ctx.gp_set_head(0, gp.X, gp.cholesky_inverse, gp.alpha, 0, gp.kern.variance, gp.kern.lengthscales)
    ctx.gp_configure(1, lyap.dynamics.beta)
    exact = _exact_floor(gp)
    got = ctx.gp_variance_floor(0, 2)
    assert (got <= exact).all() and (got >= 0.98 * exact).all()
    fresh = _raw_sweep(lyap)
    assert "early decision" in ctx.last_kernel()
    assert_array_equal(appended[0], fresh[0])
    assert_array_equal(appended[1], fresh[1])
