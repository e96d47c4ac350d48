"""Host tests (no GPU) of the half-block bookkeeping of k_gp_sweep4's block mode: sl_gp4_halves.h
driven by the stand-alone program tests/hostsim/gp4_halves_sim.cpp, built with g++ and, where the
toolchain has them, the address and undefined-behaviour sanitizers.  The program itself checks that
every half runs each panel it reaches once and in order, that a slot never mixes kinds, that no ring
position is handed out twice, that no ring overflows and that the flush empties everything (exit
status 1 otherwise); the tests here add what the counts must be."""

import os
import re
import subprocess
import sys

import numpy as np
import pytest

import hostsim_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ROWS = ("full", "paired", "lone", "partial", "slots")


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    out = hostsim_build.sanitized_program_or_plain("gp4_halves_sim.cpp", tmp_path_factory.mktemp("gp4_halves"),
                                                   ["-O1"] + hostsim_build.SIM_FLAGS)

    def run(*args):
        res = subprocess.run([out] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                             text=True, timeout=120)
        assert res.returncode == 0, res.stdout
        m = re.match(r"ok tiles=(\d+) stages=(\d+) half_panels=(\d+)" + "".join(r" %s=([\d,]+)" % r for r in ROWS),
                     res.stdout)
        assert m, res.stdout
        got = dict(tiles=int(m.group(1)), stages=int(m.group(2)), half_panels=int(m.group(3)))
        for k, name in enumerate(ROWS):
            got[name] = [int(v) for v in m.group(4 + k).split(",")]
        return got
    return run


@pytest.mark.parametrize("stages", [1, 2, 3, 4, 7, 32])
def test_random_sequences_keep_the_ring_invariants(sim, stages):
    """Random leave-stages per half (phases: decided early, open, ragged, siblings together, low
    halves only) in the three modes.  Whole-block verdicts never pair; half verdicts never run more
    slot-panels than whole-block ones; only the flush leaves a composite partly filled - a stage at
    most one of full slots and, since the flush takes up to four halves of a kind a pass, at most
    three of paired ones (a half ring holds at most 11)."""
    for seed in range(4):
        for tiles in (0, 1, 2, 5, 40, 1000):
            kernel = sim("random", seed, tiles, stages, "kernel")
            listed = sim("random", seed, tiles, stages, "list")
            blocks = sim("random", seed, tiles, stages, "blocks")
            assert kernel["tiles"] == tiles and kernel["stages"] == stages
            assert sum(blocks["paired"]) == 0 and sum(blocks["lone"]) == 0
            assert kernel["half_panels"] <= listed["half_panels"] <= blocks["half_panels"]
            for got in (kernel, listed, blocks):
                assert max(got["partial"]) <= 4, got
            # the list only changes panel 0 (whole blocks there): every later panel sees the same halves
            if stages > 1:
                assert sum(listed["slots"][1:]) <= sum(blocks["slots"][1:])
            assert sum(kernel["slots"]) <= sum(blocks["slots"])


def _slab_halves():
    from early_block_counts import cell_stages, granule_stages
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_gp4_early import SLAB_HI, SLAB_LO, _slab_case
    stage, _, _, npan = cell_stages(_slab_case(), np.arange(SLAB_LO, SLAB_HI))
    return granule_stages(stage, 8), npan


def test_the_slab_sequence_of_the_oracle(sim, tmp_path):
    """The headline slab of tests/test_gpu_gp4_blocks.py in tile order, as ONE workgroup meets it,
    stages per half from the oracle.  Every half runs exactly its panels (the program checks it);
    the slot-panels are what the packing promises: at least the halves entering a panel over two, at
    most the blocks entering it, and fewer than those in total; list launches and in-kernel source
    passes agree on every panel behind the first."""
    halves, npan = _slab_halves()
    path = tmp_path / "slab.txt"
    path.write_text("%d %d\n%s\n" % (npan, len(halves) // 2, " ".join(str(int(h)) for h in halves)))
    kernel, listed, blocks = (sim("file", path, mode) for mode in ("kernel", "list", "blocks"))
    pairs = halves.reshape(-1, 2)
    entering_halves = [int((halves > p).sum()) for p in range(npan)]
    entering_blocks = [int((pairs.max(1) > p).sum()) for p in range(npan)]
    assert kernel["half_panels"] == sum(entering_halves)
    assert blocks["half_panels"] == 2 * sum(entering_blocks)
    assert blocks["slots"] == entering_blocks
    for p in range(npan):
        assert (entering_halves[p] + 1) // 2 <= kernel["slots"][p] <= entering_blocks[p], (p, kernel)
    assert listed["slots"][0] == entering_blocks[0]
    assert sum(kernel["paired"]) > 0 and sum(listed["paired"]) > 0
    assert sum(kernel["slots"]) < sum(blocks["slots"]) and sum(listed["slots"]) < sum(blocks["slots"])
    # the same halves enter every panel behind the first in both modes; the slots may differ by what
    # the different order leaves the flush to run alone
    for p in range(1, npan):
        assert abs(listed["slots"][p] - kernel["slots"][p]) <= 4, (p, listed, kernel)
    print("slab: blocks entering", entering_blocks, "halves entering", entering_halves, "kernel", kernel,
          "list", listed)
