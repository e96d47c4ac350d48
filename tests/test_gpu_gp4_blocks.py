"""``k_gp_sweep4`` decides 16-cell blocks, keeps the open ones in per-workgroup queues and runs
every variance panel on composite tiles of four queued blocks, which may come from four source
tiles and land in any slot.  A block's slot only selects registers: every case here compares the
default path with ``SL_GP4_EARLY=0`` (every panel of every 64-cell tile) with
``assert_array_equal`` on the mask words and the 64-byte sweep record - no tolerance.
``SL_GP4_WORKGROUPS=N`` caps the workgroups, so that on these small grids one workgroup draws many
tiles and its queues fill (unset, every workgroup gets one or two tiles and mostly flushes).
Needs an MI355X."""

import os
import sys

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import cases
from test_gpu_gp4_early import EARLY_NOTE, SLAB_HI, SLAB_LO, _informed, _neg, _slab_case, _sweep

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

pytestmark = pytest.mark.gpu

BLOCK_NOTE = "16-cell blocks"


def _blocks_vs_plain(case, monkeypatch, caps, plain=None, **kw):
    """The default path at every workgroup cap of ``caps`` (None: unset) against the plain path
    (computed once, uncapped); returns the plain result."""
    monkeypatch.delenv("SL_GP4_WORKGROUPS", raising=False)
    if plain is None:
        plain = _sweep(case, monkeypatch, False, **kw)
    assert plain[3].startswith("k_gp_sweep4<") and EARLY_NOTE not in plain[3], plain[3]
    for cap in caps:
        if cap is None:
            monkeypatch.delenv("SL_GP4_WORKGROUPS", raising=False)
        else:
            monkeypatch.setenv("SL_GP4_WORKGROUPS", str(cap))     # (read when the context is created)
        on = _sweep(case, monkeypatch, True, **kw)
        assert on[3].startswith("k_gp_sweep4<") and EARLY_NOTE in on[3] and BLOCK_NOTE in on[3], on[3]
        assert_array_equal(on[0], plain[0], err_msg="mask words, workgroup cap %s" % cap)
        assert_array_equal(on[1], plain[1], err_msg="sweep record, workgroup cap %s" % cap)
    monkeypatch.delenv("SL_GP4_WORKGROUPS", raising=False)
    return plain


def test_headline_slab_blocks_leave_at_every_stage_and_mix_in_composites(monkeypatch):
    """160 tiles = 640 blocks of the headline grid, four panels.  On the oracle side: blocks finish
    at every stage, most tiles hold blocks that leave at different stages, and the numbers of blocks
    that enter the panels are not all multiples of four (one workgroup then runs partly filled
    composites, and each of its composites mixes source tiles).  The device words equal the oracle's
    wherever the oracle is clear of the threshold, and the plain path's everywhere, with one
    workgroup, two, and the launch's own number."""
    from early_block_counts import cell_stages, granule_stages
    case = _slab_case()
    stage, final, clear, npan = cell_stages(case, np.arange(SLAB_LO, SLAB_HI))
    assert npan == 4
    blocks = granule_stages(stage, 16)
    finished = np.bincount(blocks, minlength=npan + 1)          # [stage 0 .. 3, never]
    print("blocks finished at stage 0/1/2/3/never:", finished)
    assert (finished >= 10).all(), finished
    per_tile = blocks.reshape(-1, 4)
    mixed = int((per_tile.min(1) != per_tile.max(1)).sum())
    entering = [int((blocks > p).sum()) for p in range(npan)]
    print("tiles with blocks leaving at different stages:", mixed, "blocks entering panel 0..3:", entering)
    assert mixed >= 50
    assert any(n % 4 for n in entering), entering
    assert clear.mean() > 0.999
    plain = _blocks_vs_plain(case, monkeypatch, (1, 2, None), lo=SLAB_LO, hi=SLAB_HI)
    neg = _neg(plain[0], SLAB_HI - SLAB_LO)
    assert_array_equal(neg[clear], final[clear])


@pytest.mark.parametrize("with_init", [False, True])
def test_ragged_end_blocks(monkeypatch, with_init):
    """``hi`` ends 23 cells into a tile: its last tile has one full block, one block with 7 valid
    cells and two blocks without any (their bytes of the word are written as zeros); with and
    without initial-set bits, whole and cut into two shards."""
    case = _slab_case()
    lo, hi = 64 * 20, 64 * 60 + 23
    init = None
    if with_init:
        bare = _sweep(case, monkeypatch, False, lo=lo, hi=hi)
        first_failing = int(bare[1][1])
        assert lo <= first_failing < hi
        init = np.union1d(np.arange(lo + 5, hi, 7), [first_failing])
    full = _blocks_vs_plain(case, monkeypatch, (1, None), lo=lo, hi=hi, init_cells=init)
    assert not (full[0][-1] >> 23)                          # nothing set beyond hi
    mid = lo + 64 * 17
    a = _blocks_vs_plain(case, monkeypatch, (1, None), lo=lo, hi=mid, init_cells=init)
    b = _blocks_vs_plain(case, monkeypatch, (1, None), lo=mid, hi=hi, init_cells=init)
    assert_array_equal(np.concatenate((a[0], b[0])), full[0])


@pytest.mark.parametrize("n_gp,num_points", [(300, [6, 6, 6, 64]), (520, [6, 6, 6, 64]),
                                             (1024, [4, 4, 4, 64])])
def test_kinked_blocks_are_regenerated_in_another_slot(monkeypatch, n_gp, num_points):
    """Rows that cross the saturation kinks of the policy: blocks with two to four affine runs are
    queued and regenerated in whatever slot they land in (one workgroup), against the plain path
    with its sequence seeds and with ``SL_GP4_SEEDS=0``."""
    from safe_learning_amd.benchmarks import GP_VARIANTS
    case = cases.make_case("cartpole", num_points=num_points, n_gp=n_gp, tau_scale=0.0,
                           **GP_VARIANTS["tight"])
    plain = _blocks_vs_plain(case, monkeypatch, (1,))
    monkeypatch.setenv("SL_GP4_SEEDS", "0")
    unseeded = _blocks_vs_plain(case, monkeypatch, (1,))
    assert_array_equal(unseeded[0], plain[0])
    assert_array_equal(unseeded[1], plain[1])


def test_row_ends_inside_blocks(monkeypatch):
    """A last axis of 24 cells: grid rows end inside the 16-cell blocks (a new affine run there),
    864 cells are 13.5 tiles."""
    from safe_learning_amd.benchmarks import GP_VARIANTS
    case = cases.make_case("cartpole", num_points=[3, 3, 4, 24], n_gp=300, tau_scale=0.0,
                           **GP_VARIANTS["tight"])
    _blocks_vs_plain(case, monkeypatch, (1, None))


def test_whole_update_with_one_workgroup(monkeypatch):
    """update_safe_set() and update_safe_set(can_shrink=False) as a whole."""
    from safe_learning_amd.benchmarks import build_lyapunov
    out = []
    for early in (True, False):
        if early:
            monkeypatch.delenv("SL_GP4_EARLY", raising=False)
            monkeypatch.setenv("SL_GP4_WORKGROUPS", "1")
        else:
            monkeypatch.setenv("SL_GP4_EARLY", "0")
            monkeypatch.delenv("SL_GP4_WORKGROUPS", raising=False)
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
