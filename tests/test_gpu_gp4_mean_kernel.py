"""``k_gp_mean_blocks`` computes the posterior mean and the first decision of every 16-cell block in
a kernel of its own, segment by segment of source tiles; ``k_gp_sweep4`` then draws its stage-0
composite tiles from the list of open blocks each segment leaves and only runs panels.  That must
not change one bit: every case compares mask words and the 64-byte sweep record with
``SL_GP4_EARLY=0`` (every panel of every 64-cell tile, the mean interleaved with the first
generation) with ``assert_array_equal`` - no tolerance.  ``SL_GP4_SEGMENT_TILES=N`` sets the
segment size (and makes these small launches take the two-kernel path at all),
``SL_GP4_WORKGROUPS=N`` caps the panel kernel's workgroups.  Needs an MI355X."""

import os
import sys

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import cases
from test_gpu_gp4_early import EARLY_NOTE, SLAB_HI, SLAB_LO, _informed, _slab_case, _sweep

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

pytestmark = pytest.mark.gpu

MEAN_NOTE = "k_gp_mean_blocks"


def _split_vs_plain(case, monkeypatch, segment, caps=(None,), plain=None, **kw):
    """The two-kernel path with segments of ``segment`` source tiles, at every workgroup cap of
    ``caps`` (None: unset), against the plain path (computed once); returns (plain, last note)."""
    monkeypatch.delenv("SL_GP4_WORKGROUPS", raising=False)
    monkeypatch.delenv("SL_GP4_SEGMENT_TILES", raising=False)
    if plain is None:
        plain = _sweep(case, monkeypatch, False, **kw)
    assert plain[3].startswith("k_gp_sweep4<") and EARLY_NOTE not in plain[3] and MEAN_NOTE not in plain[3], plain[3]
    monkeypatch.setenv("SL_GP4_SEGMENT_TILES", str(segment))      # (read when the context is created)
    note = None
    for cap in caps:
        if cap is None:
            monkeypatch.delenv("SL_GP4_WORKGROUPS", raising=False)
        else:
            monkeypatch.setenv("SL_GP4_WORKGROUPS", str(cap))
        on = _sweep(case, monkeypatch, True, **kw)
        note = on[3]
        assert note.startswith("k_gp_sweep4<") and EARLY_NOTE in note and "16-cell blocks" in note, note
        assert MEAN_NOTE in note, note
        assert_array_equal(on[0], plain[0], err_msg="mask words, segment %s, workgroup cap %s" % (segment, cap))
        assert_array_equal(on[1], plain[1], err_msg="sweep record, segment %s, workgroup cap %s" % (segment, cap))
    monkeypatch.delenv("SL_GP4_WORKGROUPS", raising=False)
    monkeypatch.delenv("SL_GP4_SEGMENT_TILES", raising=False)
    return plain, note


@pytest.fixture(scope="module")
def slab_blocks():
    """Stage at which every 16-cell block of the headline slab is decided (CPU, the oracle)."""
    from early_block_counts import cell_stages, granule_stages
    stage, _, _, npan = cell_stages(_slab_case(), np.arange(SLAB_LO, SLAB_HI))
    assert npan == 4
    return granule_stages(stage, 16)


def test_headline_slab_in_three_segments(monkeypatch, slab_blocks):
    """160 tiles in segments of 64: three segments, the last of 32 tiles; one workgroup and the
    launch's own number.  The open blocks of at least one segment are no multiple of four (as one
    segment the slab has 485): a partly filled stage-0 draw."""
    open_per_segment = [int((slab_blocks[4 * t:4 * (t + 64)] > 0).sum()) for t in range(0, 160, 64)]
    print("open blocks per segment:", open_per_segment)
    assert sum(open_per_segment) == 485
    assert any(n % 4 for n in open_per_segment), open_per_segment
    _, note = _split_vs_plain(_slab_case(), monkeypatch, 64, caps=(1, None), lo=SLAB_LO, hi=SLAB_HI)
    assert "3 segment(s)" in note, note


def test_odd_list_lengths_in_many_segments(monkeypatch, slab_blocks):
    """Segments of 24 tiles (seven, the last of 16): lists of many lengths, with every remainder
    modulo four among them on the CPU side, and one segment of the whole slab (485 records)."""
    lengths = [int((slab_blocks[4 * t:4 * (t + 24)] > 0).sum()) for t in range(0, 160, 24)]
    print("open blocks per segment:", lengths)
    assert len({n % 4 for n in lengths}) >= 3, lengths
    plain, _ = _split_vs_plain(_slab_case(), monkeypatch, 24, caps=(1, None), lo=SLAB_LO, hi=SLAB_HI)
    _, note = _split_vs_plain(_slab_case(), monkeypatch, 160, caps=(2,), plain=plain, lo=SLAB_LO, hi=SLAB_HI)
    assert "1 segment(s)" in note, note


def test_segments_whose_list_is_empty(monkeypatch):
    """The `survey` hyper-parameters on a 16^4 grid: the mean decides every block (checked on the
    CPU), every list is empty and the panel kernel has nothing to write."""
    from early_block_counts import cell_stages, granule_stages
    from safe_learning_amd.benchmarks import GP_VARIANTS
    case = cases.make_case("cartpole", num_points=16, n_gp=300, **GP_VARIANTS["survey"])
    n = 16 ** 4
    stage, _, _, _ = cell_stages(case, np.arange(n))
    assert (granule_stages(stage, 16) == 0).all()
    _, note = _split_vs_plain(case, monkeypatch, 256, caps=(None, 1))
    assert "4 segment(s)" in note, note


@pytest.mark.parametrize("with_init", [False, True])
def test_ragged_end_in_segments_of_eight(monkeypatch, with_init):
    """``hi`` ends 23 cells into a tile (one full block, one with 7 valid cells, two without any:
    their bytes of the word are zeros), with and without initial-set bits, whole and as two shards."""
    case = _slab_case()
    lo, hi = 64 * 20, 64 * 60 + 23
    init = None
    if with_init:
        bare = _sweep(case, monkeypatch, False, lo=lo, hi=hi)
        first_failing = int(bare[1][1])
        assert lo <= first_failing < hi
        init = np.union1d(np.arange(lo + 5, hi, 7), [first_failing])
    full, _ = _split_vs_plain(case, monkeypatch, 8, caps=(1, None), lo=lo, hi=hi, init_cells=init)
    assert not (full[0][-1] >> 23)                          # nothing set beyond hi
    mid = lo + 64 * 17
    a, _ = _split_vs_plain(case, monkeypatch, 8, lo=lo, hi=mid, init_cells=init)
    b, _ = _split_vs_plain(case, monkeypatch, 8, lo=mid, hi=hi, init_cells=init)
    assert_array_equal(np.concatenate((a[0], b[0])), full[0])


def test_kinked_blocks_and_row_ends_inside_blocks(monkeypatch):
    """A last axis of 24 cells: grid rows end inside the 16-cell blocks (a new affine run there) and
    cross the saturation kinks of the policy; 864 cells are 13.5 tiles."""
    from safe_learning_amd.benchmarks import GP_VARIANTS
    case = cases.make_case("cartpole", num_points=[3, 3, 4, 24], n_gp=300, tau_scale=0.0,
                           **GP_VARIANTS["tight"])
    _split_vs_plain(case, monkeypatch, 5, caps=(1, None))


def test_two_and_three_dimensions(monkeypatch):
    """The kernels of the other dimensions: pendulum 64^2 and a 16^3 grid, 300 points."""
    pendulum = cases.make_case("pendulum", num_points=64, n_gp=300, **_informed(tau_scale=0.0005))
    _, note = _split_vs_plain(pendulum, monkeypatch, 24, caps=(1, None))
    assert note.startswith("k_gp_sweep4<d=2"), note
    chain = cases.make_case_3d(num_points=16, dynamics="gp", n_gp=300, tau_scale=0.0005)
    _, note = _split_vs_plain(chain, monkeypatch, 24, caps=(1, None))
    assert note.startswith("k_gp_sweep4<d=3"), note


def test_whole_update_in_segments(monkeypatch):
    """update_safe_set() and update_safe_set(can_shrink=False) as a whole: safe set, c_max and the
    record equal SL_GP4_EARLY=0; the note names both kernels."""
    from safe_learning_amd.benchmarks import build_lyapunov
    out = []
    for early in (True, False):
        if early:
            monkeypatch.delenv("SL_GP4_EARLY", raising=False)
            monkeypatch.setenv("SL_GP4_SEGMENT_TILES", "40")
        else:
            monkeypatch.setenv("SL_GP4_EARLY", "0")
            monkeypatch.delenv("SL_GP4_SEGMENT_TILES", raising=False)
        lyap = build_lyapunov(cases.make_case("cartpole", num_points=[4, 4, 4, 64], n_gp=520,
                                              **_informed(tau_scale=0.0005)))
        lyap.update_safe_set()
        lyap.update_safe_set(can_shrink=False)
        note = lyap._ctx.last_kernel()
        assert (EARLY_NOTE in note) == early and (MEAN_NOTE in note) == early, note
        assert note.startswith("k_gp_sweep4<"), note
        out.append((lyap._d_neg.cpu().numpy().copy(), lyap.safe_set.copy(), lyap.c_max,
                    lyap._d_result.cpu().numpy().copy(), int(lyap.safe_set.sum())))
    monkeypatch.delenv("SL_GP4_SEGMENT_TILES", raising=False)
    assert_array_equal(out[0][0], out[1][0])
    assert_array_equal(out[0][1], out[1][1])
    assert out[0][2] == out[1][2]
    assert_array_equal(out[0][3], out[1][3])
    assert out[0][4] == out[1][4]
