"""``k_gp_sweep4`` decides a tile from bounds of the decrease (the posterior mean first, then
``err = 0`` from below and ``err = beta sqrt(variance - partial |a|^2)`` from above) and skips the
variance panels the bounds make superfluous.  That must not change one bit: every case here runs
with the early decision (default) and with ``SL_GP4_EARLY=0`` (every panel of every tile, the mean
interleaved with the first generation of each chunk) and compares mask words and the 64-byte sweep
record (failing key, counters) with ``assert_array_equal`` - no tolerance.  Needs an MI355X."""

import numpy as np
import pytest
import scipy.linalg
from numpy.testing import assert_array_equal

import cases

pytestmark = pytest.mark.gpu

EARLY_NOTE = "early decision"        # what sl_last_kernel adds when the launch may decide early
RP = 256                             # rows per panel of k_gp_sweep4


def _sweep(case, monkeypatch, early, lo=0, hi=None, dbg=False, init_cells=None):
    """One sl_lyap_sweep over [lo, hi) on a fresh context: (mask words, record, records, kernel)."""
    import torch
    from safe_learning_amd.benchmarks import build_lyapunov
    if early:
        monkeypatch.delenv("SL_GP4_EARLY", raising=False)
    else:
        monkeypatch.setenv("SL_GP4_EARLY", "0")          # (read when the context is created)
    lyap = build_lyapunov(case)
    n = lyap.discretization.nindex
    hi = n if hi is None else hi
    d = case["d"]
    dev = lyap._ctx.torch_device
    if init_cells is not None:
        mask = np.zeros(n, dtype=bool)
        mask[init_cells] = True
        lyap._upload_mask(mask, lyap._d_init)
    else:
        lyap._refresh_init_bits()
    bits = torch.zeros((hi - lo + 63) // 64, dtype=torch.int64, device=dev)
    record = torch.zeros_like(lyap._d_result)
    rec = torch.zeros((hi - lo, 2 + 2 * d), dtype=torch.float64, device=dev) if dbg else None
    values = lyap._values_arg()
    lyap._ctx.lyap_sweep(lo, hi, lyap._d_init[lo // 64:], None if values is None else values[lo:],
                         bits, record, rec)
    kernel = lyap._ctx.last_kernel()
    return (bits.cpu().numpy().copy(), record.cpu().numpy().copy(),
            None if rec is None else rec.cpu().numpy().copy(), kernel)


def _both(case, monkeypatch, expect_early=True, **kw):
    on = _sweep(case, monkeypatch, True, **kw)
    off = _sweep(case, monkeypatch, False, **kw)
    assert on[3].startswith("k_gp_sweep4<") and off[3].startswith("k_gp_sweep4<"), (on[3], off[3])
    assert (EARLY_NOTE in on[3]) == expect_early, on[3]
    assert EARLY_NOTE not in off[3], off[3]
    assert_array_equal(on[0], off[0])
    assert_array_equal(on[1], off[1])
    if on[2] is not None:
        assert_array_equal(on[2].view(np.int64), off[2].view(np.int64))
    return on


def _neg(words, n):
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)


def oracle_tile_kinds(case, lo, hi):
    """What the bounds decide for the 64-cell tiles of [lo, hi), computed with the oracle alone:
    per tile the stage (0 = from the mean, s = after s panels of 256 rows, -1 = never before the
    last panel), the final mask of its cells, and which cells are clear of the threshold (further
    than the 1e-7 relative agreement of the engine's records with the oracle's)."""
    ol = cases.oracle_lyapunov(case, compute_values=False)
    grid, G = ol.discretization, ol.dynamics
    gp = G.gaussian_process
    L = gp.cholesky
    npan = (L.shape[0] + RP - 1) // RP
    idx = np.arange(lo, hi)
    x = grid.index_to_state(idx)
    Xn = np.hstack((x, ol.policy(x)))
    a = scipy.linalg.solve_triangular(L, gp.kern.K(gp.X, Xn), lower=True)
    mean = a.T.dot(gp.alpha) + gp._mean(Xn)
    var0 = gp.kern.Kdiag(Xn)
    thr = np.broadcast_to(ol.threshold(x, ol.tau), (len(idx), 1))[:, 0]

    def negative(sumsq):
        err = G.beta * np.sqrt(np.maximum(var0 - sumsq, 0))[:, None] * np.ones((1, mean.shape[1]))
        return ol.v_decrease_bound(x, (mean, err))[:, 0] < thr

    final = negative(np.sum(a ** 2, 0))
    err = G.beta * np.sqrt(np.maximum(var0 - np.sum(a ** 2, 0), 0))[:, None] * np.ones((1, mean.shape[1]))
    dec = ol.v_decrease_bound(x, (mean, err))[:, 0]
    clear = np.abs(dec - thr) > 1e-7 * (np.abs(dec) + np.abs(thr)) + 1e-12
    sure_fail = ~negative(var0)                          # err = 0
    stage = np.full(len(idx) // 64, -1)
    part = np.zeros_like(var0)
    for s in range(npan):
        if s:
            part = part + np.sum(a[(s - 1) * RP:s * RP] ** 2, 0)
        done = (sure_fail | negative(part)).reshape(-1, 64).all(1)
        stage[(stage < 0) & done] = s
    return stage, final.reshape(-1, 64), clear.reshape(-1, 64)


@pytest.mark.parametrize("n_gp,num_points", [(300, [6, 6, 6, 64]), (520, [6, 6, 6, 64]),
                                             (1024, [4, 4, 4, 64])])
def test_early_decision_is_bit_identical_across_kinks(monkeypatch, n_gp, num_points):
    """Rows that cross the saturation kinks of the policy (several runs per wavefront), 2, 3 and 4
    panels: the shape of test_gp4_sequence_seeds_are_bit_identical."""
    from safe_learning_amd.benchmarks import GP_VARIANTS
    case = cases.make_case("cartpole", num_points=num_points, n_gp=n_gp, tau_scale=0.0,
                           **GP_VARIANTS["tight"])
    _both(case, monkeypatch)
    monkeypatch.setenv("SL_GP4_SEEDS", "0")              # the mean phase without the seed scratch
    _both(case, monkeypatch)


# A slab of the headline grid itself: whole rows (128 cells) of the 128^4 cart-pole grid at 5 x 4 x 4
# positions of the three leading axes (index = first + stride * k), the `informed` hyper-parameters,
# 1024 training points, the headline's tau.  Chosen on the oracle (oracle_tile_kinds) so that the
# 160 tiles hold every kind: 26 fail from the mean alone, 42 / 28 / 6 pass after one / two / three
# panels, 58 stay open to the last panel.
SLAB_FIRST, SLAB_STRIDE, SLAB_COUNT = (10, 20, 40), (13, 14, 7), (5, 4, 4)
SLAB_LO, SLAB_HI = 0, 5 * 4 * 4 * 128


def _slab_case():
    from safe_learning_amd.benchmarks import headline_case
    case = headline_case()
    unit = 2.0 / 127
    case["limits"] = [[-1 + unit * f, -1 + unit * (f + s * (k - 1))]
                      for f, s, k in zip(SLAB_FIRST, SLAB_STRIDE, SLAB_COUNT)] + [[-1., 1.]]
    case["num_points"] = list(SLAB_COUNT) + [128]
    return case


def test_headline_slab_has_every_kind_of_tile_and_keeps_its_bits(monkeypatch):
    """160 tiles of the headline grid.  On the oracle side: tiles that the mean alone decides as
    failing, tiles decided as passing after a panel (with the prior variance as the upper bound no
    cell of this workload passes: nothing is decided as passing before the first panel) and tiles
    that stay open to the last panel all occur; the engine's words equal the oracle's wherever the
    oracle's decrease is clear of the threshold, and are bit-identical with and without the early
    decision."""
    case = _slab_case()
    stage, final, clear = oracle_tile_kinds(case, SLAB_LO, SLAB_HI)
    assert ((stage == 0) & ~final.any(1)).sum() >= 10    # decided failing from the mean
    assert ((stage > 0) & final.all(1)).sum() >= 10      # decided passing after a panel
    assert (stage < 0).sum() >= 10                       # undecided to the end
    assert clear.mean() > 0.999
    words, _, _, _ = _both(case, monkeypatch, lo=SLAB_LO, hi=SLAB_HI)
    neg = _neg(words, SLAB_HI - SLAB_LO).reshape(-1, 64)
    assert_array_equal(neg[clear], final[clear])


def test_ragged_end_init_bits_and_shards(monkeypatch):
    """``hi`` not a multiple of 64, initial-set bits among the failing cells, a range cut into two
    shards, and update_safe_set(can_shrink=False) as a whole."""
    from safe_learning_amd.benchmarks import build_lyapunov
    case = _slab_case()
    lo, hi = 64 * 20, 64 * 60 + 23
    plain = _both(case, monkeypatch, lo=lo, hi=hi)
    first_failing = int(plain[1][1])                     # the record's key: (V bits, cell index)
    assert lo <= first_failing < hi
    init = np.union1d(np.arange(lo + 5, hi, 7), [first_failing])
    full = _both(case, monkeypatch, lo=lo, hi=hi, init_cells=init)
    assert_array_equal(full[0], plain[0])                # the mask does not depend on the initial set
    assert not np.array_equal(full[1], plain[1])         # the failing key does
    mid = lo + 64 * 17
    a = _both(case, monkeypatch, lo=lo, hi=mid, init_cells=init)
    b = _both(case, monkeypatch, lo=mid, hi=hi, init_cells=init)
    assert_array_equal(np.concatenate((a[0], b[0])), full[0])
    out = []
    for early in (True, False):
        if early:
            monkeypatch.delenv("SL_GP4_EARLY", raising=False)
        else:
            monkeypatch.setenv("SL_GP4_EARLY", "0")
        lyap = build_lyapunov(cases.make_case("cartpole", num_points=[4, 4, 4, 64], n_gp=520,
                                              **_informed(tau_scale=0.0005)))
        lyap.update_safe_set()
        lyap.update_safe_set(can_shrink=False)
        assert (EARLY_NOTE in lyap._ctx.last_kernel()) == early
        out.append((lyap._d_neg.cpu().numpy().copy(), lyap.safe_set.copy(), lyap.c_max,
                    lyap._d_result.cpu().numpy().copy()))
    assert_array_equal(out[0][0], out[1][0])
    assert_array_equal(out[0][1], out[1][1])
    assert out[0][2] == out[1][2]
    assert_array_equal(out[0][3], out[1][3])


def _informed(**kw):
    from safe_learning_amd.benchmarks import GP_VARIANTS
    return dict(GP_VARIANTS["informed"], **kw)


def test_function_stack_and_records_keep_the_plain_path(monkeypatch):
    """A FunctionStack model (one head per output) and a sweep that writes per-cell records do not
    decide early: the kernel reports the plain path, and the bits are those of SL_GP4_EARLY=0."""
    from safe_learning_amd.benchmarks import GP_VARIANTS
    stack = cases.make_case("cartpole", num_points=[4, 4, 4, 64], n_gp=300, tau_scale=0.0, stack=True,
                            **GP_VARIANTS["tight"])
    _both(stack, monkeypatch, expect_early=False)
    shared = cases.make_case("cartpole", num_points=[4, 4, 4, 64], n_gp=300, tau_scale=0.0,
                             **GP_VARIANTS["tight"])
    rec = _both(shared, monkeypatch, expect_early=False, dbg=True)
    plain = _both(shared, monkeypatch)
    assert_array_equal(rec[0], plain[0])                 # with and without records: the same words
    assert_array_equal(rec[1], plain[1])


def test_tiny_noise_trips_the_variance_guard(monkeypatch):
    """Noise variance tiny against the signal: variance - |a|^2 may round below zero (NaN error,
    'not negative'), which a bound could not reproduce - the launch keeps the plain path."""
    case = cases.make_case("cartpole", num_points=[4, 4, 4, 64], n_gp=300, tau_scale=0.0,
                           signal_std=0.03, noise_std=0.03 * 1e-6, lengthscale=0.3)
    _both(case, monkeypatch, expect_early=False)
