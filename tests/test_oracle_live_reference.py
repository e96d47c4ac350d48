"""Reference and oracle side by side on random scenarios.

``tests/golden/make_reference_safe_sets.py --record-live`` ran the reference's own ``Lyapunov``
(behind ``tests/golden/numpy_tf.py``) on the seeded random scenarios of its ``LIVE_RUNS`` - grid
sizes and limits, tau, batch size, linear / Euler / GP / stacked-GP dynamics, the adaptive branch,
hand-marked cells, ``can_shrink`` on and off - and stored the scenarios with the value tables, safe
sets, ``c_max`` and refinement arrays after every call in
``tests/golden/reference_live_safe_sets.npz``.  Here ``oracle.Lyapunov`` replays them and has to
be equal bit for bit.  (``--check-live N SEED`` runs both sides on other seeds where the
reference checkout exists; a sweep of 200 scenarios, seeds 2-6, was clean when the fixtures were
committed.)
"""

import importlib.util
import os
import sys

import pytest

from conftest import GOLDEN_DIR


def _generator(name):
    sys.path.insert(0, GOLDEN_DIR)
    try:
        spec = importlib.util.spec_from_file_location(name, os.path.join(GOLDEN_DIR, name + ".py"))
        module = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(module)
    finally:
        sys.path.remove(GOLDEN_DIR)
    return module


SAFE_SETS = _generator("make_reference_safe_sets")
POLICY_ITERATION = _generator("make_reference_policy_iteration")


@pytest.fixture
def batch_size():
    from oracle import np_lyapunov
    saved = np_lyapunov.config.gp_batch_size
    yield
    np_lyapunov.config.gp_batch_size = saved


@pytest.mark.parametrize("seed", [11, 12])
def test_oracle_equals_the_reference_on_random_scenarios(seed, batch_size):
    runs = [(scenario, want) for s, scenario, want in SAFE_SETS.live_fixture() if s == seed]
    assert len(runs) == {s: count for count, s in SAFE_SETS.LIVE_RUNS}[seed]
    for scenario, want in runs:
        assert want is not None, "%s: recorded without a comparison (tied values)" % scenario["name"]
        SAFE_SETS.check_records(scenario, SAFE_SETS.oracle_run(scenario), want)


@pytest.mark.parametrize("seed", [21, 22])
def test_oracle_policy_iteration_equals_the_reference_on_random_scenarios(seed):
    """The same for ``PolicyIteration`` (``make_reference_policy_iteration.py --record-live``,
    ``tests/golden/reference_live_policy_iteration.npz``): random value / policy grids (equal or
    not), action sets, discounts, rewards, constraint callbacks, Lyapunov penalties,
    ``bellmann_error``.  (120 scenarios, seeds 1-4, were clean when committed; the first sweep found
    the one difference there was: ``bellmann_error`` summed pairwise.)"""
    runs = [(scenario, want) for s, scenario, want in POLICY_ITERATION.live_fixture() if s == seed]
    assert len(runs) == {s: count for count, s in POLICY_ITERATION.LIVE_RUNS}[seed]
    for scenario, want in runs:
        got = POLICY_ITERATION.oracle_run(scenario)
        assert len(got) == len(want), scenario["name"]
        for k, (a, b) in enumerate(zip(got, want)):
            assert POLICY_ITERATION.records_match(a, b, scenario["case"]), "%s record %d" % (scenario["name"], k)
