"""``k_gp_predecide`` decides, in front of ``k_gp_mean_blocks``, the 16-cell blocks that a
bound of the posterior mean (a first-order Taylor expansion about the nearest cell of a lattice,
with a rigorous remainder: DESIGN.md 4.1 "Deciding before the mean") shows to fail whatever their
variance; the mean kernel skips them.  That must not change one bit: every case compares mask
words and the 64-byte sweep record with ``SL_GP4_EARLY=0`` with ``assert_array_equal`` - no
tolerance - and the launch's note must report blocks decided before the mean.
``SL_GP4_PREDECIDE_SPACING=S`` sets the lattice spacing, ``SL_GP4_PREDECIDE=0`` switches the pass
off.  Needs an MI355X."""

import os
import re
import sys

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import cases
from test_gpu_gp4_early import EARLY_NOTE, SLAB_HI, SLAB_LO, _informed, _slab_case, _sweep
from test_gpu_gp4_floor import _raw_sweep
from test_gpu_gp4_mean_kernel import MEAN_NOTE, _split_vs_plain

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

pytestmark = pytest.mark.gpu

PRE_NOTE = re.compile(r"(\d+) block\(s\) decided before the mean")


def _decided(note):
    """Blocks the note reports as decided before the mean; None when the pass did not run."""
    m = PRE_NOTE.search(note)
    return None if m is None else int(m.group(1))


@pytest.fixture(autouse=True)
def _switches(monkeypatch):
    monkeypatch.delenv("SL_GP4_PREDECIDE", raising=False)
    monkeypatch.delenv("SL_GP4_PREDECIDE_SPACING", raising=False)


def _cpu_blocks(case, lo, hi, spacing):
    """The 16-cell blocks of [lo, hi) the rule decides, on the CPU (tools/early_block_counts.py)."""
    from early_block_counts import mean_lattice_sure
    sure = mean_lattice_sure(case, np.arange(lo, hi), spacing)
    sure = np.concatenate((sure, np.ones(-len(sure) % 16, dtype=bool)))      # (a ragged last block: its valid cells decide)
    return sure.reshape(-1, 16).all(1)


@pytest.fixture(scope="module")
def slab_plain():
    """The slab with SL_GP4_EARLY=0, once for the tests that share it."""
    mp = pytest.MonkeyPatch()
    try:
        return _sweep(_slab_case(), mp, False, lo=SLAB_LO, hi=SLAB_HI)
    finally:
        mp.undo()


def test_headline_slab_in_segments_of_64(monkeypatch, slab_plain):
    """160 tiles in three segments, the launch's own workgroups and one; S = 8.  CPU: 55 of 640 blocks
    decided by the bound, 155 by the exact mean."""
    _, note = _split_vs_plain(_slab_case(), monkeypatch, 64, caps=(None, 1), plain=slab_plain, lo=SLAB_LO, hi=SLAB_HI)
    assert "3 segment(s)" in note, note
    print(note)
    assert _decided(note) is not None and 0 < _decided(note) < 640, note


@pytest.mark.parametrize("n_gp", [257, 600])
def test_clamped_last_lattice_index(monkeypatch, n_gp):
    """6 x 6 x 6 x 64 at S = 2: the axis length is no multiple of S and the last lattice index (5) is
    clamped; 257 points (two panels, the second nearly empty) and 600.  CPU: 281 / 229 of 864 blocks."""
    monkeypatch.setenv("SL_GP4_PREDECIDE_SPACING", "2")
    case = cases.make_case("cartpole", num_points=[6, 6, 6, 64], n_gp=n_gp, **_informed(tau_scale=0.0005))
    _, note = _split_vs_plain(case, monkeypatch, 64, caps=(None, 1))
    print(note)
    assert _decided(note) is not None and 0 < _decided(note) < 864, note


def test_two_and_three_dimensions(monkeypatch):
    """Pendulum 64 x 24 (rows end inside the 16-cell blocks and cross the saturation kinks of the
    policy; `hi` inside a block) and the 16 x 16 x 24 chain (`tau_scale` 0.1), S = 2.  CPU: 30 of 96 and 235 of
    384 blocks (the exact mean: 48 and 272)."""
    monkeypatch.setenv("SL_GP4_PREDECIDE_SPACING", "2")
    pendulum = cases.make_case("pendulum", num_points=[64, 24], n_gp=300, **_informed(tau_scale=0.1))
    _, note = _split_vs_plain(pendulum, monkeypatch, 8, caps=(None, 1), lo=0, hi=64 * 24 - 9)
    assert note.startswith("k_gp_sweep4<d=2"), note
    print(note)
    assert _decided(note) is not None and 0 < _decided(note) < 96, note
    chain = cases.make_case_3d(num_points=[16, 16, 24], dynamics="gp", n_gp=300, tau_scale=0.1)
    _, note = _split_vs_plain(chain, monkeypatch, 40, caps=(None, 1))
    assert note.startswith("k_gp_sweep4<d=3"), note
    print(note)
    assert _decided(note) is not None and 0 < _decided(note) < 384, note


def test_shard_that_does_not_start_at_zero(monkeypatch, slab_plain):
    """A shard [64 k, hi) with hi 23 cells into a tile: its words are the slice of the full sweep's."""
    lo, hi = 64 * 37, 64 * 120 + 23
    part, note = _split_vs_plain(_slab_case(), monkeypatch, 24, lo=lo, hi=hi)
    assert _decided(note) is not None and _decided(note) > 0, note
    words = part[0]
    assert_array_equal(words[:-1], slab_plain[0][lo // 64:hi // 64])
    assert words[-1] == slab_plain[0][hi // 64] & np.int64((1 << 23) - 1)


def test_initial_set_inside_predecided_blocks(monkeypatch, slab_plain):
    """The key fold of a predecided block honours the initial bits.  Initial set: every cell outside
    the blocks the bound decides (CPU), and every seventh cell inside them - so the record's key, the
    failing cell outside the initial set with the least V, lies in a predecided block, and it moves
    when the initial set takes that cell too."""
    case = _slab_case()
    blocks = _cpu_blocks(case, SLAB_LO, SLAB_HI, 8)
    assert 0 < blocks.sum() < len(blocks)
    inside = np.repeat(blocks, 16)
    cells = np.arange(SLAB_LO, SLAB_HI)
    init = np.union1d(cells[~inside], cells[5::7])
    first, note = _split_vs_plain(case, monkeypatch, 64, caps=(None, 1), lo=SLAB_LO, hi=SLAB_HI, init_cells=init)
    assert _decided(note) > 0, note
    assert_array_equal(first[0], slab_plain[0])              # the mask does not depend on the initial set
    key = int(first[1][1])
    assert inside[key - SLAB_LO] and key not in init, key
    second, _ = _split_vs_plain(case, monkeypatch, 64, lo=SLAB_LO, hi=SLAB_HI, init_cells=np.union1d(init, [key]))
    assert int(second[1][1]) != key


def test_whole_update_against_the_oracle(monkeypatch):
    """update_safe_set() as a whole on 4 x 4 x 4 x 64 cells, 520 points, S = 2 (CPU: 85 of 256 blocks):
    values, safe set and c_max are the oracle's, the mask equals SL_GP4_EARLY=0."""
    from safe_learning_amd.benchmarks import build_lyapunov
    case = cases.make_case("cartpole", num_points=[4, 4, 4, 64], n_gp=520, **_informed(tau_scale=0.0005))
    monkeypatch.setenv("SL_GP4_PREDECIDE_SPACING", "2")
    monkeypatch.setenv("SL_GP4_SEGMENT_TILES", "40")
    monkeypatch.delenv("SL_GP4_EARLY", raising=False)
    lyap = build_lyapunov(case)
    lyap.update_safe_set()
    note = lyap._ctx.last_kernel()
    assert MEAN_NOTE in note and _decided(note) is not None and _decided(note) > 0, note
    olyap = cases.oracle_lyapunov(case)
    olyap.update_safe_set()
    assert_array_equal(lyap.values, olyap.values)
    assert_array_equal(lyap.safe_set, olyap.safe_set)
    assert lyap.c_max == olyap.c_max
    monkeypatch.setenv("SL_GP4_EARLY", "0")
    monkeypatch.delenv("SL_GP4_SEGMENT_TILES", raising=False)
    plain = build_lyapunov(case)
    plain.update_safe_set()
    assert EARLY_NOTE not in plain._ctx.last_kernel()
    assert_array_equal(lyap._d_neg.cpu().numpy(), plain._d_neg.cpu().numpy())
    assert_array_equal(lyap._d_result.cpu().numpy(), plain._d_result.cpu().numpy())


def test_switched_off_is_the_parent(monkeypatch, slab_plain):
    """SL_GP4_PREDECIDE=0: the note ends where it did before this pass existed, and the bits are the same."""
    monkeypatch.setenv("SL_GP4_PREDECIDE", "0")
    _, note = _split_vs_plain(_slab_case(), monkeypatch, 64, plain=slab_plain, lo=SLAB_LO, hi=SLAB_HI)
    assert _decided(note) is None, note
    assert re.search(r"3 segment\(s\), \d+ paired composite\(s\), \d+ lone half slot\(s\)$", note), note


def test_an_appended_head_switches_the_pass_off(monkeypatch):
    """sl_gp_append_point changes alpha' and with it the RKHS norm: no deciding pass until the next full
    upload, after which it runs again - with the same bits."""
    from safe_learning_amd.benchmarks import _true_dynamics_numpy, build_lyapunov
    monkeypatch.delenv("SL_GP4_EARLY", raising=False)
    monkeypatch.setenv("SL_GP4_PREDECIDE_SPACING", "2")
    monkeypatch.setenv("SL_GP4_SEGMENT_TILES", "64")
    case = cases.make_case("cartpole", num_points=[6, 6, 6, 64], n_gp=300, **_informed(tau_scale=0.0005))
    lyap = build_lyapunov(case)
    ctx = lyap._ctx
    _raw_sweep(lyap)                                             # uploads the head
    assert _decided(ctx.last_kernel()) > 0
    x_new = np.random.default_rng(21).uniform(-1, 1, (3, case["d"] + 1))
    lyap.dynamics.add_data_point(x_new, _true_dynamics_numpy(case, x_new))
    appended = _raw_sweep(lyap)
    note = ctx.last_kernel()
    assert MEAN_NOTE in note and _decided(note) is None, note
    gp = lyap.dynamics.gaussian_process
    ctx.gp_set_head(0, gp.X, gp.cholesky_inverse, gp.alpha, 0, gp.kern.variance, gp.kern.lengthscales)
    ctx.gp_configure(1, lyap.dynamics.beta)
    fresh = _raw_sweep(lyap)
    assert _decided(ctx.last_kernel()) > 0
    assert_array_equal(appended[0], fresh[0])
    assert_array_equal(appended[1], fresh[1])


def test_a_network_policy_keeps_the_pass_off(monkeypatch):
    """The lattice pass evaluates the policy at cells of the whole grid, and a network policy is served
    during a sweep from a table of the shard's cells alone: the pass takes closed-form policies only.
    A saturated network policy on a shard inside the grid: segments and the mean kernel run, the note
    reports no deciding pass, and the bits are those of SL_GP4_EARLY=0."""
    import torch
    import safe_learning_amd as sl
    from safe_learning_amd.benchmarks import build_lyapunov
    from test_gpu_network_policy import _network_pair
    case = cases.make_case("cartpole", num_points=[6, 6, 6, 64], n_gp=300, **_informed(tau_scale=0.0005))
    lo, hi = 64 * 30, 64 * 150 + 23
    monkeypatch.setenv("SL_GP4_PREDECIDE_SPACING", "2")
    out = []
    for early in (True, False):
        if early:
            monkeypatch.delenv("SL_GP4_EARLY", raising=False)
            monkeypatch.setenv("SL_GP4_SEGMENT_TILES", "64")
        else:
            monkeypatch.setenv("SL_GP4_EARLY", "0")
            monkeypatch.delenv("SL_GP4_SEGMENT_TILES", raising=False)
        lyap = build_lyapunov(case)
        net, _ = _network_pair(sl, case["d"], [16, 16, 1], ["relu", "tanh", "tanh"], 1.2, True, seed=5)
        lyap.policy = sl.Saturation(net, -1.0, 1.0)
        lyap._upload_model()
        lyap._refresh_init_bits()
        bits = torch.zeros((hi - lo + 63) // 64, dtype=torch.int64, device=lyap._ctx.torch_device)
        record = torch.zeros_like(lyap._d_result)
        values = lyap._values_arg()
        lyap._ctx.lyap_sweep(lo, hi, lyap._d_init[lo // 64:], None if values is None else values[lo:], bits, record, None)
        note = lyap._ctx.last_kernel()
        assert note.startswith("k_gp_sweep4<"), note
        if early:
            assert MEAN_NOTE in note and _decided(note) is None, note
        out.append((bits.cpu().numpy().copy(), record.cpu().numpy().copy()))
    assert_array_equal(out[0][0], out[1][0])
    assert_array_equal(out[0][1], out[1][1])
