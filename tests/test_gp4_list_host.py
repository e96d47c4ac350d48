"""Host tests of the two-kernel block mode of k_gp_sweep4 (no GPU): the list of stage-0 records that
k_gp_mean_blocks leaves per segment and the draws of the panel kernel (sl_gp4_queue.h), driven
together with the queue functions by the stand-alone program tests/hostsim/gp4_list_sim.cpp (built
with g++ and, where the toolchain has them, the address and undefined-behaviour sanitizers)."""

import os
import re
import subprocess
import sys

import numpy as np
import pytest

import hostsim_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    out = hostsim_build.sanitized_program_or_plain("gp4_list_sim.cpp", tmp_path_factory.mktemp("gp4_list"),
                                                   ["-O1"] + hostsim_build.SIM_FLAGS)

    def run(*args):
        res = subprocess.run([out] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                             text=True, timeout=120)
        assert res.returncode == 0, res.stdout
        got = []
        for line in res.stdout.splitlines():
            m = re.match(r"ok tiles=(\d+) stages=(\d+) segments=(\d+) records=(\d+) draws=(\d+) partial_draws=(\d+) "
                         r"block_panels=(\d+) flush_partial=(\d+) composites=([\d,]+)$", line)
            assert m, res.stdout
            got.append(dict(zip(("tiles", "stages", "segments", "records", "draws", "partial_draws", "block_panels",
                                 "flush_partial"), (int(v) for v in m.groups()[:8])),
                            composites=[int(v) for v in m.group(9).split(",")]))
        return got
    return run


@pytest.mark.parametrize("stages", [1, 2, 4, 7, 32])
def test_random_patterns_segments_and_workgroups(sim, stages):
    """Every open block enters panel 0 once, runs its panels once and in order, no list or ring
    position is handed out twice, every segment's flush leaves nothing (the program exits with 1
    otherwise); a segment has at most one partly filled draw, its last."""
    for seed in range(3):
        for tiles, segment, workgroups in ((0, 4, 1), (1, 4, 2), (5, 2, 1), (40, 7, 3), (40, 64, 1), (1000, 256, 5),
                                           (1000, 33, 16)):
            got, = sim("random", seed, tiles, stages, segment, workgroups)
            assert got["tiles"] == tiles and got["stages"] == stages
            assert got["segments"] == (tiles + segment - 1) // segment
            assert got["partial_draws"] <= got["segments"]
            assert got["draws"] >= (got["records"] + 3) // 4
            assert got["composites"][0] == got["draws"]


def test_lists_of_zero_one_4k_and_4k_plus_one_records(sim):
    for stages in (1, 4):
        runs = sim("lengths", stages)
        assert [r["records"] for r in runs[::2]] == [0, 1, 2, 3, 4, 5, 8, 9, 64, 65]
        for r in runs:
            assert r["draws"] == (r["records"] + 3) // 4 and r["partial_draws"] == (r["records"] % 4 != 0)


@pytest.mark.parametrize("segment,workgroups", [(160, 1), (64, 1), (64, 4), (24, 2), (8, 3), (1, 1)])
def test_the_slab_pattern_of_the_oracle(sim, tmp_path, segment, workgroups):
    """The headline slab of tests/test_gpu_gp4_mean_kernel.py: 485 of its 640 blocks are open after
    the mean; every panel sees the blocks that enter it."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from early_block_counts import cell_stages, granule_stages
    from test_gpu_gp4_early import SLAB_HI, SLAB_LO, _slab_case
    stage, _, _, npan = _slab_stages(cell_stages, _slab_case, SLAB_LO, SLAB_HI)
    blocks = granule_stages(stage, 16)
    path = tmp_path / "slab.txt"
    path.write_text("%d %d\n%s\n" % (npan, len(blocks), " ".join(str(int(b)) for b in blocks)))
    got, = sim("file", path, segment, workgroups)
    entering = [int((blocks > p).sum()) for p in range(npan)]
    assert entering[0] == 485 and got["records"] == 485
    assert got["block_panels"] == sum(entering)
    assert got["segments"] == (160 + segment - 1) // segment
    assert got["composites"][0] == got["draws"]
    per_segment = [int((blocks[4 * t:4 * (t + segment)] > 0).sum()) for t in range(0, 160, segment)]
    assert got["draws"] == sum((n + 3) // 4 for n in per_segment)
    assert got["partial_draws"] == sum(n % 4 != 0 for n in per_segment)


_SLAB = {}


def _slab_stages(cell_stages, slab_case, lo, hi):
    if "stages" not in _SLAB:                              # (the oracle's pass over the slab: once per module)
        _SLAB["stages"] = cell_stages(slab_case(), np.arange(lo, hi))
    return _SLAB["stages"]
