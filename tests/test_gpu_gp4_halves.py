"""``k_gp_sweep4``'s block mode decides and queues the 8-cell HALVES of its 16-cell blocks: a half the
bounds decide leaves at once, and the variance panels run on slots that hold one whole block or the
low half of one block beside the high half of another (two generations feed such a slot's columns).
That must not change one bit: every case compares mask words and the 64-byte sweep record with
``SL_GP4_EARLY=0`` (every panel of every 64-cell tile) with ``assert_array_equal`` - no tolerance -
and must really run paired composites: the launch's note (``sl_last_kernel``) reports how many, and
how many of their slots held one half only (that count is printed, not asserted: the mean kernel
appends to its list in any order, so which halves meet in a slot differs from run to run).  ``SL_GP4_HALVES=0`` goes back to whole blocks.

The open halves per stage of every case were counted on the CPU with the oracle before it was chosen
(``tools/early_block_counts.cell_stages`` with the variance floor, 8-cell granule): per stage
(blocks with an open half, both halves open, low half only, high half only) - every stage leaves
halves of both kinds without a sibling, so every stage runs paired slots and, the counts being
unequal, lone halves.  Needs an MI355X."""

import re

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import cases
from test_gpu_gp4_blocks import _blocks_vs_plain
from test_gpu_gp4_early import EARLY_NOTE, SLAB_HI, SLAB_LO, _informed, _slab_case, _sweep
from test_gpu_gp4_mean_kernel import _split_vs_plain

pytestmark = pytest.mark.gpu

HALVES_NOTE = "in 8-cell halves"


def _pairs(note):
    """(paired composites, lone-half slots) of a launch's note."""
    m = re.search(r"(\d+) paired composite\(s\), (\d+) lone half slot\(s\)", note)
    assert m, note
    return int(m.group(1)), int(m.group(2))


def _halves_vs(plain, case, monkeypatch, cap=None, segment=None, **kw):
    """One default sweep (halves on) at a workgroup cap / segment size against the plain result:
    equal bits, and the note must report paired composites.  Returns (result, paired, lone)."""
    monkeypatch.delenv("SL_GP4_HALVES", raising=False)
    for name, value in (("SL_GP4_WORKGROUPS", cap), ("SL_GP4_SEGMENT_TILES", segment)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(value))
    on = _sweep(case, monkeypatch, True, **kw)
    monkeypatch.delenv("SL_GP4_WORKGROUPS", raising=False)
    monkeypatch.delenv("SL_GP4_SEGMENT_TILES", raising=False)
    note = on[3]
    assert note.startswith("k_gp_sweep4<") and EARLY_NOTE in note and HALVES_NOTE in note, note
    assert_array_equal(on[0], plain[0], err_msg="mask words, cap %s, segment %s" % (cap, segment))
    assert_array_equal(on[1], plain[1], err_msg="sweep record, cap %s, segment %s" % (cap, segment))
    paired, lone = _pairs(note)
    print(note)
    assert paired > 0, note
    return on, paired, lone


def test_headline_slab_capped_and_uncapped(monkeypatch):
    """The 640 blocks of the headline slab.  CPU count per stage: (485, 463, 4, 18), (203, 154, 20, 29),
    (101, 59, 14, 28), (79, 31, 23, 25).  One workgroup meets them all: its half rings pair across
    source tiles and the surplus of high halves runs alone; uncapped in segments of 64 source tiles,
    every workgroup flushes a few.  (Without a cap or a segment size this launch is a small one: its
    source pass runs in the panel kernel, on whole blocks.)"""
    plain = _blocks_vs_plain(_slab_case(), monkeypatch, (None, 1), lo=SLAB_LO, hi=SLAB_HI)
    _halves_vs(plain, _slab_case(), monkeypatch, cap=1, lo=SLAB_LO, hi=SLAB_HI)
    _halves_vs(plain, _slab_case(), monkeypatch, segment=64, lo=SLAB_LO, hi=SLAB_HI)
    monkeypatch.delenv("SL_GP4_HALVES", raising=False)
    small = _sweep(_slab_case(), monkeypatch, True, lo=SLAB_LO, hi=SLAB_HI)
    assert EARLY_NOTE in small[3] and HALVES_NOTE not in small[3] and _pairs(small[3]) == (0, 0), small[3]


@pytest.mark.parametrize("n_gp", [257, 600])
def test_two_and_three_panels_with_a_ragged_last_one(monkeypatch, n_gp):
    """Cart-pole 6 x 6 x 6 x 64, 864 blocks.  257 points (the second panel holds one row): (217, 177, 23,
    17), (81, 28, 27, 26).  600 points (three panels, the last of 88 rows): (207, 170, 19, 18), (147,
    81, 34, 32), (113, 40, 34, 39).  In the panel kernel itself and in segments of 100 source tiles."""
    case = cases.make_case("cartpole", num_points=[6, 6, 6, 64], n_gp=n_gp, **_informed(tau_scale=0.0005))
    plain = _blocks_vs_plain(case, monkeypatch, (None,))
    _halves_vs(plain, case, monkeypatch, cap=1)
    _halves_vs(plain, case, monkeypatch, cap=2, segment=100)
    _split_vs_plain(case, monkeypatch, 100, caps=(None,), plain=plain)


def test_pendulum_with_kinked_rows_and_a_ragged_end_inside_a_half(monkeypatch):
    """Pendulum 64 x 24, 300 points, hi = 64 * 20 + 23: rows of 24 cells end inside the halves, cross the
    saturation kinks of the policy (several runs per block: the replay of a half starts at its block's
    first cell), and the grid ends seven cells into a high half.  (82, 48, 17, 17), (13, 2, 5, 6)."""
    pendulum = cases.make_case("pendulum", num_points=[64, 24], n_gp=300, **_informed(tau_scale=0.0005))
    hi = 64 * 20 + 23
    plain = _blocks_vs_plain(pendulum, monkeypatch, (None,), lo=0, hi=hi)
    assert plain[3].startswith("k_gp_sweep4<d=2"), plain[3]
    _halves_vs(plain, pendulum, monkeypatch, cap=1, lo=0, hi=hi)
    _halves_vs(plain, pendulum, monkeypatch, cap=1, segment=8, lo=0, hi=hi)


def test_three_dimensions(monkeypatch):
    """The 16 x 16 x 24 chain, 300 points, ending 23 cells into a tile: (359, 262, 50, 47), (87, 0, 45,
    42) - before the second panel no block has both halves open, every slot is a pair or a lone half."""
    chain = cases.make_case_3d(num_points=[16, 16, 24], dynamics="gp", n_gp=300, tau_scale=0.0005)
    hi = 64 * 90 + 23
    plain = _blocks_vs_plain(chain, monkeypatch, (None,), lo=0, hi=hi)
    assert plain[3].startswith("k_gp_sweep4<d=3"), plain[3]
    _halves_vs(plain, chain, monkeypatch, cap=1, lo=0, hi=hi)
    _halves_vs(plain, chain, monkeypatch, cap=2, segment=40, lo=0, hi=hi)


def test_survey_hyper_parameters_at_the_headline_tau_in_three_segments(monkeypatch):
    """The `survey` model of 1024 points on the headline's discretisation constant, 8 x 8 x 16 x 128 in
    segments of 700 source tiles: (3619, 3099, 297, 223), (1350, 976, 197, 177), (1131, 809, 177, 145),
    (733, 486, 130, 117)."""
    from safe_learning_amd.benchmarks import headline_case
    case = headline_case(variant="survey")
    case["tau"] = headline_case()["tau"]
    case["num_points"] = [8, 8, 16, 128]
    plain, note = _split_vs_plain(case, monkeypatch, 700, caps=(None,))
    assert "3 segment(s)" in note and HALVES_NOTE in note, note
    assert _pairs(note)[0] > 0, note
    _halves_vs(plain, case, monkeypatch, cap=4, segment=700)


def test_halves_off_is_the_same_bits_and_pairs_nothing(monkeypatch):
    """SL_GP4_HALVES=0: whole blocks as before - no paired composite, the note says so, and mask words
    and record equal the default's (both equal the plain path's)."""
    case = _slab_case()
    plain = _blocks_vs_plain(case, monkeypatch, (), lo=SLAB_LO, hi=SLAB_HI)
    on, paired, _ = _halves_vs(plain, case, monkeypatch, cap=1, lo=SLAB_LO, hi=SLAB_HI)
    monkeypatch.setenv("SL_GP4_HALVES", "0")
    monkeypatch.setenv("SL_GP4_WORKGROUPS", "1")
    off = _sweep(case, monkeypatch, True, lo=SLAB_LO, hi=SLAB_HI)
    monkeypatch.delenv("SL_GP4_HALVES", raising=False)
    monkeypatch.delenv("SL_GP4_WORKGROUPS", raising=False)
    assert EARLY_NOTE in off[3] and HALVES_NOTE not in off[3], off[3]
    assert _pairs(off[3]) == (0, 0), off[3]
    assert_array_equal(off[0], on[0])
    assert_array_equal(off[1], on[1])


def test_a_whole_update_safe_set_against_the_oracle(monkeypatch):
    """Cart-pole 4 x 4 x 4 x 64, 520 points, one workgroup: (46, 32, 7, 7), (37, 22, 6, 9), (26, 9, 8, 9).
    The mask, the safe set and c_max of update_safe_set equal the oracle's."""
    from safe_learning_amd.benchmarks import build_lyapunov
    monkeypatch.delenv("SL_GP4_EARLY", raising=False)
    monkeypatch.delenv("SL_GP4_HALVES", raising=False)
    monkeypatch.setenv("SL_GP4_WORKGROUPS", "1")
    case = cases.make_case("cartpole", num_points=[4, 4, 4, 64], n_gp=520, **_informed(tau_scale=0.0005))
    lyap = build_lyapunov(case)
    lyap.update_safe_set()
    note = lyap._ctx.last_kernel()
    monkeypatch.delenv("SL_GP4_WORKGROUPS", raising=False)
    assert note.startswith("k_gp_sweep4<") and HALVES_NOTE in note and _pairs(note)[0] > 0, note
    olyap = cases.oracle_lyapunov(case)
    olyap.update_safe_set()
    assert_array_equal(lyap.safe_set, olyap.safe_set)
    assert lyap.c_max == olyap.c_max
    assert lyap.safe_set.any() and not lyap.safe_set.all()
