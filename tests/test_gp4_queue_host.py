"""Host tests of k_gp_sweep4's block mode (no GPU): the queue bookkeeping of sl_gp4_queue.h, driven
by the stand-alone program tests/hostsim/gp4_queue_sim.cpp (built with g++ and, where the toolchain
has them, the address and undefined-behaviour sanitizers), and the CPU count of the panel work
(tools/early_block_counts.py) against the device count of the 64-cell kernel."""

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
    out = hostsim_build.sanitized_program_or_plain("gp4_queue_sim.cpp", tmp_path_factory.mktemp("gp4_queue"),
                                                   ["-O1"] + hostsim_build.SIM_FLAGS)

    def run(*args):
        res = subprocess.run([out] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                             text=True, timeout=120)
        assert res.returncode == 0, res.stdout
        m = re.match(r"ok tiles=(\d+) stages=(\d+) block_panels=(\d+) composites=([\d,]+) partial=([\d,]+)", res.stdout)
        assert m, res.stdout
        return dict(tiles=int(m.group(1)), stages=int(m.group(2)), block_panels=int(m.group(3)),
                    composites=[int(v) for v in m.group(4).split(",")],
                    partial=[int(v) for v in m.group(5).split(",")])
    return run


@pytest.mark.parametrize("stages", [1, 2, 3, 4, 7, 32])
def test_random_sequences_keep_the_queue_invariants(sim, stages):
    """Every pushed block runs each panel it reaches exactly once, no queue exceeds seven records,
    the flush leaves everything empty (the program exits with 1 otherwise)."""
    for seed in range(6):
        for tiles in (0, 1, 2, 5, 40, 1000):
            got = sim("random", seed, tiles, stages)
            assert got["tiles"] == tiles and got["stages"] == stages
            # Only the flush runs partly filled composites, and a stage at most one: it runs
            # partly filled as the shallowest stage that holds anything, and nothing feeds it after.
            assert max(got["partial"]) <= 1, got


def test_the_slab_sequence_of_the_oracle(sim, tmp_path):
    """The headline slab of tests/test_gpu_gp4_blocks.py in tile order, as ONE workgroup meets it:
    the composites per panel are the blocks entering it, four at a time."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from early_block_counts import cell_stages, granule_stages
    from test_gpu_gp4_early import SLAB_HI, SLAB_LO, _slab_case
    stage, _, _, npan = cell_stages(_slab_case(), np.arange(SLAB_LO, SLAB_HI))
    blocks = granule_stages(stage, 16)
    path = tmp_path / "slab.txt"
    path.write_text("%d %d\n%s\n" % (npan, len(blocks), " ".join(str(int(b)) for b in blocks)))
    got = sim("file", path)
    entering = [int((blocks > p).sum()) for p in range(npan)]
    assert got["block_panels"] == sum(entering)
    for made, n, partly in zip(got["composites"], entering, got["partial"]):
        assert (n + 3) // 4 <= made <= n // 4 + 1 and partly <= 1, got
    assert any(n % 4 for n in entering) and sum(got["partial"]) >= 1    # the flush is exercised


def test_cpu_count_reproduces_the_device_count_of_64_cell_tiles():
    """tools/early_block_counts.py, 64-cell granule, against the device count of the kernel that
    decided whole tiles (profiles/early_stage_counts.txt, headline): within the sampling error of
    its random tiles - 4 sigma of a binomial fraction over n tiles - and the 16-cell granule
    leaves clearly less panel work."""
    import early_block_counts
    with open(os.path.join(ROOT, "profiles", "early_stage_counts.txt")) as handle:
        text = handle.read()
    m = re.search(r"## headline informed 128\^4\nk_gp_sweep4 stages: tiles (\d+) decided before panel 0/1/2/3: "
                  r"(\d+) (\d+) (\d+) (\d+)", text)
    total = int(m.group(1))
    decided = np.cumsum([int(m.group(k)) for k in range(2, 6)])
    device_open = 1.0 - decided / total
    tiles = 400
    result, npan = early_block_counts.count(None, tiles=tiles, seed=1)
    assert npan == 4
    frac64, work64 = result[64]
    sigma = np.sqrt(device_open * (1 - device_open) / tiles)
    print("open before panel 0..3: device", device_open, "cpu", frac64, "sigma", sigma)
    assert (np.abs(frac64 - device_open) <= 4 * sigma).all()
    w = early_block_counts.panel_weights(npan)
    device_work = float(device_open.dot(w) / w.sum())
    assert abs(work64 - device_work) <= 4 * float(sigma.dot(w) / w.sum())
    works = [result[g][1] for g in early_block_counts.GRANULES]
    assert works == sorted(works, reverse=True)           # finer granules never execute more
    assert result[16][1] < 0.75 * work64
