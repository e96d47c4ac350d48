"""Host tests (no GPU) of the open-block list of a segmented block-mode GP sweep: the rule of
sl_gp4_open.h - which blocks the deciding pass left open, the count of a run of tile bytes, the rank
of a block inside its chunk - driven by the stand-alone program tests/hostsim/gp4_open_sim.cpp, which
runs the count and the scatter chunk by chunk as k_gp_open_count and k_gp_open_scatter do.  Built
with g++ and, where the toolchain has them, the address and undefined-behaviour sanitizers (the
program's buffers have exactly the device allocation's sizes).  The program itself checks that the
two passes agree, that every entry stands at its rank and that nothing leaves the list (exit status 1
otherwise); the tests here hold the list against NumPy."""

import re
import subprocess

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import hostsim_build

CHUNK = 4096
SIZES = [1, 3, 4095, 4096, 4097, 10001]


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    work = tmp_path_factory.mktemp("gp4_open")
    out = hostsim_build.sanitized_program_or_plain("gp4_open_sim.cpp", work, ["-O1"] + hostsim_build.SIM_FLAGS)

    def run(tile_bytes):
        tile_bytes = np.ascontiguousarray(tile_bytes, dtype=np.uint8)
        src, dst = work / "bytes.bin", work / "list.bin"
        tile_bytes.tofile(src)
        res = subprocess.run([out, str(src), str(len(tile_bytes)), str(dst)], stdout=subprocess.PIPE,
                             stderr=subprocess.STDOUT, text=True, timeout=120)
        assert res.returncode == 0, res.stdout
        m = re.match(r"ok ntiles=(\d+) chunks=(\d+) length=(\d+)", res.stdout)
        assert m, res.stdout
        assert int(m.group(1)) == len(tile_bytes) and int(m.group(2)) == -(-len(tile_bytes) // CHUNK)
        listed = np.fromfile(dst, dtype=np.uint32)
        assert len(listed) == int(m.group(3))
        return listed
    return run


def _expected(tile_bytes):
    """Block numbers 4 tile + jb of the clear bits 0 .. 3 of every byte, ascending."""
    bits = (np.asarray(tile_bytes, dtype=np.uint8)[:, None] >> np.arange(4)) & 1
    return np.flatnonzero(bits.reshape(-1) == 0).astype(np.uint32)


@pytest.mark.parametrize("ntiles", SIZES)
def test_random_tile_bytes(sim, ntiles):
    """Random decided bits at three densities; the high nibble of a byte is never looked at."""
    rng = np.random.default_rng(ntiles)
    for density in (0.1, 0.5, 0.9):
        low = (rng.random((ntiles, 4)) < density) @ (1 << np.arange(4))
        high = rng.integers(0, 16, ntiles) << 4
        tile_bytes = (low + high).astype(np.uint8)
        want = _expected(tile_bytes)
        got = sim(tile_bytes)
        assert len(got) == len(want) == int((((tile_bytes[:, None] >> np.arange(4)) & 1) == 0).sum())
        assert_array_equal(got, want)


@pytest.mark.parametrize("ntiles", SIZES)
def test_all_decided_and_none_decided(sim, ntiles):
    assert len(sim(np.full(ntiles, 15, dtype=np.uint8))) == 0
    assert_array_equal(sim(np.zeros(ntiles, dtype=np.uint8)), np.arange(4 * ntiles, dtype=np.uint32))


def test_runs_of_decided_tiles_and_a_ragged_last_tile(sim):
    """Long runs of wholly decided tiles across chunk boundaries (what the headline grid looks like), a last
    chunk that is not full, and a last tile whose blocks behind `hi` the pass has marked."""
    ntiles = 2 * CHUNK + 1234
    tile_bytes = np.zeros(ntiles, dtype=np.uint8)
    tile_bytes[100:CHUNK + 7] = 15
    tile_bytes[CHUNK + 900:2 * CHUNK + 1] = 15
    tile_bytes[-1] = 0b1100                                   # two live blocks, two behind hi
    tile_bytes[5] = 0b0101
    want = _expected(tile_bytes)
    got = sim(tile_bytes)
    assert_array_equal(got, want)
    assert got[-1] == 4 * (ntiles - 1) + 1 and (np.diff(got.astype(np.int64)) > 0).all()
