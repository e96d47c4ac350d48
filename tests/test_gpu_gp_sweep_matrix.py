"""Every instantiation of ``k_gp_small`` and ``k_gp_sweep`` that no other test identifies by its kernel note
(tests/gp_sweep_matrix.py; needs an MI355X).

Per ledger entry the sweep must NAME the instantiation in full - flavour, d, where the factor is read from, wavefront
count, head count - after every launch (a case that silently ran another kernel fails).  Then one of two comparisons:

* an ANCHOR (eight wavefronts under ``SL_GP_SMALL_WAVES=8``; every ``k_gp_sweep`` entry): records at the compared
  cells through ``sweep_records``; mean and variance against the long-double posterior of ``tests/np_gp_truth.py``
  with the bound of ``test_gpu_gp_truth._check`` (32 x the oracle's own error; the ``xs_global`` heads are too large
  for that and are held to the oracle under ``8 eps cond(K)``); decrease and threshold against the oracle at 1e-9; the
  mask under the margin rule.  ``k_gp_sweep`` entries also against the kernel one step down the chain;
* every other wavefront count: one full-range sweep whose records, mask words and result record equal, bit for bit,
  the eight-wavefront sweep of the same range and model.

The wavefront count is steered by the launcher's own round-cost rule through the length of the range (a function of
the device's compute units), never by a switch.  Figures of the last run: ``profiles/gp_sweep_matrix.md``."""

import time

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import gp_sweep_matrix as gm
import np_gp_truth as T
from gp_cases import reference_gp_tolerance
from test_gp_sweep_matrix_host import oracle_records
from test_gpu_gp_truth import _check
from test_gpu_lyapunov import _check_masks
from test_gpu_reference_gp import sweep_records

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def num_cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _build(c, monkeypatch, env=None):
    """The engine's Lyapunov object of a ledger case, uploaded (the switches are read when the context is created)."""
    from safe_learning_amd.benchmarks import build_lyapunov
    for name in gm.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in (c["env"] if env is None else env).items():
        monkeypatch.setenv(name, value)
    lyap = build_lyapunov(oracle_records(c)[0])
    lyap._upload_model()
    lyap._refresh_init_bits()
    return lyap


def _full_sweep(lyap, lo, hi):
    """One sweep of [lo, hi): per-cell records, mask words, the 64-byte result record, the kernel note."""
    import torch
    d = lyap.discretization.ndim
    dev = lyap._ctx.torch_device
    dbg = torch.zeros((hi - lo, 2 + 2 * d), dtype=torch.float64, device=dev)
    bits = torch.zeros((hi - lo + 63) // 64, dtype=torch.int64, device=dev)
    record = torch.zeros_like(lyap._d_result)
    lyap._ctx.lyap_sweep(lo, hi, lyap._d_init[lo // 64:], lyap._d_values[lo:], bits, record, dbg)
    return dbg, bits, record, lyap._ctx.last_kernel()


def _mask(bits, count):
    words = bits.cpu().numpy().view(np.uint8)
    return np.unpackbits(words, bitorder="little")[:count].astype(bool)


_REFERENCES, _CONDITION = {}, {}


def _model_key(c):
    return (c["family"], tuple(c["num_points"]), c["n_gp"], c["kernels"])


def _truth(c):
    """The long-double posterior and the oracle's own error at the compared cells: once per model, left unchanged."""
    key = _model_key(c)
    if key not in _REFERENCES:
        made, cells, _, _ = oracle_records(c)
        _REFERENCES[key] = T.oracle_error(made, cells)
    return _REFERENCES[key]


def _tolerance(c):
    key = _model_key(c)
    if key not in _CONDITION:
        _CONDITION[key] = T.condition_number(oracle_records(c)[0])
    return reference_gp_tolerance(_CONDITION[key]), _CONDITION[key]


def _close(label, got, want, d, tol):
    """Means within tol x the column's largest, error bounds within tol relative (tests/test_gpu_reference_gp.py)."""
    mean, bound = np.abs(got[:, 2:2 + d] - want[:, 2:2 + d]), np.abs(got[:, 2 + d:] - want[:, 2 + d:])
    scale = np.abs(want[:, 2:2 + d]).max(axis=0)
    print("%s: mean %.3g, error bound %.3g of the tolerance %.3g" % (
        label, (mean / scale).max() / tol, (bound / want[:, 2 + d:]).max() / tol, tol))
    assert np.all(mean <= tol * scale), label
    assert np.all(bound <= tol * want[:, 2 + d:]), label


@pytest.mark.parametrize("entry", [e for e in gm.entries("new") if e["anchor"] is True], ids=gm.entry_id)
def test_anchor_against_the_truth(entry, num_cu, monkeypatch):
    import exclusions
    import torch
    start = time.perf_counter()
    c, label = entry["case"], gm.entry_id(entry)
    made, cells, ref, ok = oracle_records(c)
    d = made["d"]
    lyap = _build(c, monkeypatch)
    rec, kernels = sweep_records(lyap, cells)
    assert all(k.startswith(entry["expect"]) for k in kernels), (label, kernels)
    # the full-range sweep: the same instantiation, the same bits at the compared cells, a mask that is its records'
    lo, hi = gm.sweep_range(c, num_cu)
    dbg, bits, _, kernel = _full_sweep(lyap, lo, hi)
    assert kernel.startswith(entry["expect"]), (label, kernel)
    full = dbg.cpu().numpy()
    inside = cells >= lo
    assert inside.sum() >= 64
    assert_array_equal(full[cells[inside] - lo].view(np.int64), rec[inside].view(np.int64))
    assert_array_equal(_mask(bits, hi - lo), full[:, 0] < full[:, 1])
    # mean and variance against the yardstick
    if entry["yardstick"] == "long double":
        _check(label, _truth(c), rec[:, 2:2 + d], rec[:, 2 + d:], kernels, (entry["expect"],))
    else:
        tol, cond = _tolerance(c)
        print("%s: cond(K) = %.3g" % (label, cond))
        _close(label + " against the oracle", rec, ref, d, tol)
    # decrease and threshold against the oracle, the mask under the margin rule
    states = np.asarray(lyap.discretization.index_to_state(cells))
    edge = (np.abs(np.abs(states) - 1.0) < 1e-12).any(axis=1)
    exclusions.report(label, ok, "table lines", limit=float((~ok & edge).mean()) + 0.02)
    print("%s: decrease and threshold within %.3g relative of the oracle's" % (
        label, np.max(np.abs(rec[ok][:, :2] - ref[ok][:, :2]) / np.maximum(np.abs(ref[ok][:, :2]), 1e-300))))
    assert_allclose(rec[ok][:, :2], ref[ok][:, :2], rtol=1e-9, atol=1e-12)
    neg, ref_neg = rec[ok, 0] < rec[ok, 1], ref[ok, 0] < ref[ok, 1]
    assert min(ref_neg.mean(), 1 - ref_neg.mean()) >= 0.05                  # a mask that is not vacuous
    _check_masks(neg, ref_neg, rec[ok], ref[ok])
    if entry["down"] is not None:
        env, family = entry["down"]
        other, others = sweep_records(_build(c, monkeypatch, env), cells)
        assert all(k.startswith(family) for k in others), (label, others)
        tol, _ = _tolerance(c)
        _close("%s against %s" % (label, sorted(others)[0].split(" ")[0]), rec, other, d, tol)
        margin = np.abs(other[ok, 0] - other[ok, 1]) / np.maximum(np.abs(other[ok, 0]), np.abs(other[ok, 1]))
        assert not np.any(((other[ok, 0] < other[ok, 1]) != neg) & (margin > 1e-9))
    torch.cuda.synchronize()
    print("%s: %.2f s" % (label, time.perf_counter() - start))


@pytest.mark.parametrize("entry", [e for e in gm.entries("new") if e["anchor"] is not True], ids=gm.entry_id)
def test_wavefront_count_against_its_anchor(entry, num_cu, monkeypatch):
    """4, 12 and 16 wavefronts per workgroup (chosen by the launcher's round-cost rule for this range) against eight:
    a tile's arithmetic depends neither on the workgroup it runs in nor on where the factor is read from."""
    import torch
    start = time.perf_counter()
    c, anchor, label = entry["case"], entry["anchor"], gm.entry_id(entry)
    lo, hi = gm.sweep_range(c, num_cu)
    assert (lo, hi) == gm.sweep_range(anchor, num_cu)
    want = _full_sweep(_build(anchor, monkeypatch), lo, hi)
    assert want[3].startswith(entry["expect"].split(", Linv")[0]) and ", 8 wavefronts>" in want[3], (label, want[3])
    got = _full_sweep(_build(c, monkeypatch), lo, hi)
    assert got[3].startswith(entry["expect"]), (label, got[3])
    print("%s: %s against %s, %d tiles on %d compute units" % (label, got[3], want[3], (hi - lo + 63) // 64, num_cu))
    assert torch.equal(got[1], want[1])
    assert torch.equal(got[2], want[2])
    assert torch.equal(got[0].view(torch.int64), want[0].view(torch.int64))
    passing = int((got[0][:, 0] < got[0][:, 1]).sum())
    assert passing > 1000 and (hi - lo) - passing > 1000                  # a mask that is not vacuous
    assert_array_equal(_mask(got[1], hi - lo), (got[0][:, 0] < got[0][:, 1]).cpu().numpy())
    torch.cuda.synchronize()
    print("%s: %.2f s" % (label, time.perf_counter() - start))
