"""Behind ``k_gp_predecide`` the blocks it left open are compacted into an ascending list of block
numbers (``k_gp_open_count``, ``k_gp_open_scatter``), and the mean pass works through that list
(``k_gp_mean_open``) instead of walking every tile (``k_gp_mean_blocks``): a segment of source tiles
``[t0, t1)`` then stands for the list positions ``[4 t0, 4 t1)``.  That must not change one bit: every
case compares mask words and the 64-byte sweep record with ``SL_GP4_EARLY=0`` AND with
``SL_GP4_PREDECIDE=0`` (segments, ``k_gp_mean_blocks``) with ``assert_array_equal`` - no tolerance -
and requires that the mean pass ran from the list (``sl_gp4_open_list``: ``used``).  The counts are
those of the CPU rule (``tools/early_block_counts.py --mean-lattice``, profiles/predecide.md).
Needs an MI355X."""

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import cases
from test_gpu_gp4_early import EARLY_NOTE, SLAB_HI, SLAB_LO, _informed, _slab_case
from test_gpu_gp4_mean_kernel import MEAN_NOTE
from test_gpu_gp4_predecide import _cpu_blocks, _decided

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _switches(monkeypatch):
    for name in ("SL_GP4_PREDECIDE", "SL_GP4_PREDECIDE_SPACING", "SL_GP4_SEGMENT_TILES", "SL_GP4_WORKGROUPS",
                 "SL_GP4_EARLY"):
        monkeypatch.delenv(name, raising=False)


def _sweep(case, monkeypatch, mode, segment=None, spacing=None, lo=0, hi=None, init_cells=None):
    """One sl_lyap_sweep over [lo, hi) on a fresh context.  mode "list": the deciding pass and its list;
    "bytes": SL_GP4_PREDECIDE=0; "plain": SL_GP4_EARLY=0.  -> dict(words, record, note, listed, used)."""
    import torch
    from safe_learning_amd.benchmarks import build_lyapunov
    with monkeypatch.context() as mp:
        if mode == "plain":
            mp.setenv("SL_GP4_EARLY", "0")
        else:
            mp.setenv("SL_GP4_SEGMENT_TILES", str(segment))
            if mode == "bytes":
                mp.setenv("SL_GP4_PREDECIDE", "0")
            if spacing is not None:
                mp.setenv("SL_GP4_PREDECIDE_SPACING", str(spacing))
        lyap = build_lyapunov(case)                          # (the switches are read when the context is created)
    n = lyap.discretization.nindex
    hi = n if hi is None else hi
    dev = lyap._ctx.torch_device
    if init_cells is not None:
        mask = np.zeros(n, dtype=bool)
        mask[init_cells] = True
        lyap._upload_mask(mask, lyap._d_init)
    else:
        lyap._refresh_init_bits()
    bits = torch.zeros((hi - lo + 63) // 64, dtype=torch.int64, device=dev)
    record = torch.zeros_like(lyap._d_result)
    values = lyap._values_arg()
    lyap._ctx.lyap_sweep(lo, hi, lyap._d_init[lo // 64:], None if values is None else values[lo:], bits, record, None)
    note = lyap._ctx.last_kernel()
    listed, used = lyap._ctx.gp4_open_list()
    return dict(words=bits.cpu().numpy().copy(), record=record.cpu().numpy().copy(), note=note, listed=listed,
                used=used)


def _three_ways(case, monkeypatch, segment, spacing=None, plain=None, **kw):
    """The sweep from the list against SL_GP4_EARLY=0 and SL_GP4_PREDECIDE=0 -> (list run, plain run)."""
    if plain is None:
        plain = _sweep(case, monkeypatch, "plain", **kw)
    assert plain["note"].startswith("k_gp_sweep4<") and EARLY_NOTE not in plain["note"], plain["note"]
    assert not plain["used"] and len(plain["listed"]) == 0
    walked = _sweep(case, monkeypatch, "bytes", segment=segment, **kw)
    assert MEAN_NOTE in walked["note"] and _decided(walked["note"]) is None, walked["note"]
    assert not walked["used"] and len(walked["listed"]) == 0
    on = _sweep(case, monkeypatch, "list", segment=segment, spacing=spacing, **kw)
    assert on["note"].startswith("k_gp_sweep4<") and EARLY_NOTE in on["note"] and MEAN_NOTE in on["note"], on["note"]
    assert _decided(on["note"]) is not None, on["note"]
    for other, name in ((plain, "SL_GP4_EARLY=0"), (walked, "SL_GP4_PREDECIDE=0")):
        assert_array_equal(on["words"], other["words"], err_msg="mask words against " + name)
        assert_array_equal(on["record"], other["record"], err_msg="sweep record against " + name)
    assert on["used"] is True
    return on, plain


def _check_list(on, nblocks_live, decided=None):
    """Strictly ascending entries below the live blocks, as many as the pass left open."""
    listed = on["listed"].astype(np.int64)
    if decided is not None:
        assert _decided(on["note"]) == decided, on["note"]
    assert len(listed) == nblocks_live - _decided(on["note"]), (len(listed), on["note"])
    assert (np.diff(listed) > 0).all()
    assert len(listed) == 0 or (0 <= listed[0] and listed[-1] < nblocks_live)


@pytest.fixture(scope="module")
def cart_case():
    return cases.make_case("cartpole", num_points=[6, 6, 6, 64], n_gp=257, **_informed(tau_scale=0.0005))


@pytest.fixture(scope="module")
def slab_plain():
    mp = pytest.MonkeyPatch()
    try:
        return _sweep(_slab_case(), mp, "plain", lo=SLAB_LO, hi=SLAB_HI)
    finally:
        mp.undo()


def test_cartpole_in_six_segments_with_a_partly_filled_last_draw(monkeypatch, cart_case):
    """6 x 6 x 6 x 64, 257 points, S = 2, segments of 40 tiles: 281 of 864 blocks decided, 583 listed - no
    multiple of four, the last draw holds three blocks; six segments of 160 positions, of which the list
    fills three and part of the fourth and the last two find nothing.  The entries are exactly the blocks
    the CPU rule leaves open: every one a clear bit, none beyond `hi`."""
    on, _ = _three_ways(cart_case, monkeypatch, 40, spacing=2)
    assert "6 segment(s)" in on["note"], on["note"]
    _check_list(on, 864, decided=281)
    assert len(on["listed"]) == 583 and 583 % 4 and 583 <= 4 * 160
    assert_array_equal(on["listed"], np.flatnonzero(~_cpu_blocks(cart_case, 0, 6 * 6 * 6 * 64, 2)))


def test_headline_slab_in_segments_of_64(monkeypatch, slab_plain):
    """160 tiles of the headline grid, S = 8: 55 of 640 blocks decided, 585 listed (segments of 256, 256
    and 128 positions: 256 + 256 + 73)."""
    on, _ = _three_ways(_slab_case(), monkeypatch, 64, plain=slab_plain, lo=SLAB_LO, hi=SLAB_HI)
    assert "3 segment(s)" in on["note"], on["note"]
    _check_list(on, 640, decided=55)
    assert len(on["listed"]) == 585
    assert_array_equal(on["listed"], np.flatnonzero(~_cpu_blocks(_slab_case(), SLAB_LO, SLAB_HI, 8)))


def test_shard_that_does_not_start_at_zero(monkeypatch, slab_plain):
    """The slab as a shard [64 k, hi) with hi 23 cells into a tile: block numbers count from the shard's
    `lo`, the two blocks wholly behind `hi` are not listed, and the words are the slice of the full sweep's."""
    lo, hi = 64 * 37, 64 * 120 + 23
    case = _slab_case()
    on, _ = _three_ways(case, monkeypatch, 24, lo=lo, hi=hi)
    live = (hi - lo + 15) // 16
    _check_list(on, live)
    assert _decided(on["note"]) > 0
    assert_array_equal(on["listed"], np.flatnonzero(~_cpu_blocks(case, lo, hi, 8)))
    assert_array_equal(on["words"][:-1], slab_plain["words"][lo // 64:hi // 64])
    assert on["words"][-1] == slab_plain["words"][hi // 64] & np.int64((1 << 23) - 1)


def test_pendulum_with_a_ragged_last_block(monkeypatch):
    """Pendulum 64 x 24, `hi` nine cells short (the last block has 7 valid cells), S = 2, segments of 8
    tiles: 30 of 96 blocks decided, 66 listed.  k_gp_mean_open<2, 1>."""
    case = cases.make_case("pendulum", num_points=[64, 24], n_gp=300, **_informed(tau_scale=0.1))
    hi = 64 * 24 - 9
    on, _ = _three_ways(case, monkeypatch, 8, spacing=2, lo=0, hi=hi)
    assert on["note"].startswith("k_gp_sweep4<d=2"), on["note"]
    _check_list(on, 96, decided=30)
    assert len(on["listed"]) == 66
    assert_array_equal(on["listed"], np.flatnonzero(~_cpu_blocks(case, 0, hi, 2)))
    assert not int(on["words"][-1]) >> (hi % 64)              # nothing set beyond hi


def test_three_dimensions_and_one(monkeypatch):
    """The 16 x 16 x 24 chain (k_gp_mean_open<3, 1>; CPU: 235 of 384 blocks) and a one-dimensional grid of
    1000 points (k_gp_mean_open<1, 1>), S = 2.  The deciding pass takes any dimension with a closed-form
    policy and a quadratic V, so d = 1 runs from the list like the others."""
    chain = cases.make_case_3d(num_points=[16, 16, 24], dynamics="gp", n_gp=300, tau_scale=0.1)
    on, _ = _three_ways(chain, monkeypatch, 40, spacing=2)
    assert on["note"].startswith("k_gp_sweep4<d=3"), on["note"]
    _check_list(on, 384, decided=235)
    from gp_sweep_matrix import gp_1d_case
    line = gp_1d_case([1000], 300, 0.1)
    on, _ = _three_ways(line, monkeypatch, 5, spacing=2)
    assert on["note"].startswith("k_gp_sweep4<d=1"), on["note"]
    _check_list(on, (1000 + 15) // 16)


def test_every_block_decided_before_the_mean(monkeypatch):
    """The `survey` hyper-parameters with their full tau on the 6 x 6 x 6 x 64 grid at S = 1 (every cell its
    own reference: the bound is the mean's): the pass decides all 864 blocks (CPU), the list is empty, every
    segment's mean launch ends at once - and the pass still counts as used."""
    from safe_learning_amd.benchmarks import GP_VARIANTS
    case = cases.make_case("cartpole", num_points=[6, 6, 6, 64], n_gp=257, **GP_VARIANTS["survey"])
    assert _cpu_blocks(case, 0, 6 * 6 * 6 * 64, 1).all()
    on, _ = _three_ways(case, monkeypatch, 40, spacing=1)
    _check_list(on, 864, decided=864)
    assert len(on["listed"]) == 0


def test_no_block_decided_before_the_mean(monkeypatch):
    """A negative tau (tau_scale -0.01: the threshold lies above zero) - no cell fails from a bound of the mean
    (CPU: 0 of 864 blocks), the list holds every block and the six segments are as full as without the pass."""
    case = cases.make_case("cartpole", num_points=[6, 6, 6, 64], n_gp=257, **_informed(tau_scale=-0.01))
    assert not _cpu_blocks(case, 0, 6 * 6 * 6 * 64, 2).any()
    on, _ = _three_ways(case, monkeypatch, 40, spacing=2)
    _check_list(on, 864, decided=0)
    assert_array_equal(on["listed"], np.arange(864))


def test_initial_set_inside_predecided_blocks(monkeypatch, slab_plain):
    """The key fold, as in test_gpu_gp4_predecide.py: with every cell outside the predecided blocks (and every
    seventh inside) in the initial set, the record's key lies in a predecided block - k_gp_mean_open folds
    its own keys into the slots the pass wrote and must keep it - and moves when that cell joins the set."""
    case = _slab_case()
    blocks = _cpu_blocks(case, SLAB_LO, SLAB_HI, 8)
    inside = np.repeat(blocks, 16)
    cells = np.arange(SLAB_LO, SLAB_HI)
    init = np.union1d(cells[~inside], cells[5::7])
    first, _ = _three_ways(case, monkeypatch, 64, lo=SLAB_LO, hi=SLAB_HI, init_cells=init)
    assert_array_equal(first["words"], slab_plain["words"])
    key = int(first["record"][1])
    assert inside[key - SLAB_LO] and key not in init, key
    second, _ = _three_ways(case, monkeypatch, 64, lo=SLAB_LO, hi=SLAB_HI, init_cells=np.union1d(init, [key]))
    assert int(second["record"][1]) != key


def test_step_wider_than_the_lengthscale(monkeypatch):
    """Lengthscale 0.02 on the 4 x 4 x 4 x 64 grid: neighbouring cells of a row are 1.59 lengthscales apart in the
    state alone (scaled step above 1: `wide`), and a block inside one row and one regime of the policy is still
    ONE affine run - it takes the recurrence from the constants of its first run, which k_gp_mean_open keeps in
    row 0 of `runc`.  The pass decides nothing here (CPU: 0 of 256 blocks), so the mean kernel forms every block."""
    kw = _informed(tau_scale=0.0005)
    kw["lengthscale"] = 0.02
    case = cases.make_case("cartpole", num_points=[4, 4, 4, 64], n_gp=257, **kw)
    unit = (case["limits"][-1][1] - case["limits"][-1][0]) / 63
    assert unit / np.asarray(case["dynamics"]["lengthscales"])[3] > 1.5
    on, _ = _three_ways(case, monkeypatch, 24, spacing=2)
    assert on["note"].startswith("k_gp_sweep4<d=4"), on["note"]
    _check_list(on, 256)
    assert len(on["listed"]) > 128                            # (CPU: all 256)


def test_whole_update_with_the_list_in_use(monkeypatch, cart_case):
    """update_safe_set() as a whole on the first case's model: safe set, c_max, mask and record equal
    SL_GP4_PREDECIDE=0."""
    from safe_learning_amd.benchmarks import build_lyapunov
    out = []
    for pre in (True, False):
        with monkeypatch.context() as mp:
            mp.setenv("SL_GP4_SEGMENT_TILES", "40")
            mp.setenv("SL_GP4_PREDECIDE_SPACING", "2")
            if not pre:
                mp.setenv("SL_GP4_PREDECIDE", "0")
            lyap = build_lyapunov(cart_case)
        lyap.update_safe_set()
        note = lyap._ctx.last_kernel()
        assert MEAN_NOTE in note and (_decided(note) is not None) == pre, note
        length, used = lyap._ctx.gp4_open_list(entries=False)
        assert used == pre and (length == 864 - _decided(note) if pre else length == 0)
        out.append((lyap._d_neg.cpu().numpy().copy(), lyap.safe_set.copy(), lyap.c_max,
                    lyap._d_result.cpu().numpy().copy()))
    assert_array_equal(out[0][0], out[1][0])
    assert_array_equal(out[0][1], out[1][1])
    assert out[0][2] == out[1][2]
    assert_array_equal(out[0][3], out[1][3])
