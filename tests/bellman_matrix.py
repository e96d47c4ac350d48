"""The ledger of the dynamic-programming kernels: every instantiation that the dispatch sites of
``sl_bellman.hip``, ``sl_bellman4.hip``, ``sl_succ.hip`` and ``sl_policy_solve.hip`` compile, and for
each one either the smallest case that selects it (or the existing test that already does) or the
reason why no call can select it.

Plain data and a few lines of arithmetic; imports without a GPU.  ``tests/test_bellman_matrix_host.py``
holds the ledger against the sources (the ``sl_with_dim<...>`` lists, the launchers' selection rules,
the constants the reasons name, the oracle-side well-posedness of every case).  The cases of the
entries that no other test reaches are run by ``tests/test_gpu_bellman_matrix.py``.

``sl_with_dim<D0, D1, ...>(v, f)`` calls ``f`` with the first listed value equal to ``v`` and with
the LAST listed value when none matches: a site's list is the set of instantiations it compiles.
"""

import itertools

# ---------------------------------------------------------------------------------------------
# The sl_with_dim lists, unit by unit in source order: (what the list chooses, its values).
# ---------------------------------------------------------------------------------------------
DISPATCH = {
    "sl_bellman.hip": [
        ("k_bellman_policy_mfma: d", ("4", "2")),
        ("k_bellman_mfma: d", ("4", "2")),
        ("k_bellman_mfma: column blocks (0: a FunctionStack, one block per head)", ("0", "1", "3", "6")),
        ("k_bellman: d", ("4", "2", "1", "0")),
        ("k_bellman: actions", ("3", "9", "SL_MAX_ACTIONS", "0")),
    ],
    "sl_bellman4.hip": [
        ("k_bellman4_policy_distinct: d", ("4", "2")),
        ("k_bellman4_policy: d", ("4", "2")),
        ("k_bellman4 / k_bellman4s: d", ("4", "2")),
        ("k_bellman4 / k_bellman4s: 2 * row blocks + quarter", ("3", "2", "5", "4", "6")),
        ("k_bellman_lookup: d", ("4", "2")),
        ("k_bellman_lookup: filling", ("1", "0")),
    ],
    "sl_succ.hip": [
        ("k_succ_select: d", ("4", "3", "2", "1")),
        ("k_bellman_cached: d", ("4", "3", "2", "1")),
        ("k_bellman_cached: policy", ("1", "0")),
        ("k_succ_policy_miss: d", ("4", "3", "2", "1")),
    ],
    "sl_policy_solve.hip": [
        ("k_policy_operator_rows: d", ("1", "2", "3", "4")),
        ("k_value_matvec: widest row", ("2", "3", "4", "5", "8", "SL_ROW_MAX_K")),
    ],
}
# k_value_matvec<MODE, kmax>: MODE is chosen by the `matvec<MODE>(` calls of the solver
# (0: y = x - gamma P x inside a GMRES cycle, 1: a Jacobi step, 2: the residual of an iterate)
MATVEC_MODES = (0, 1, 2)

# the constants the lists and the reasons name: header -> names
CONSTANTS = {"sl_common.h": ("SL_MAX_ACTIONS",), "sl_policy_rows.h": ("SL_ROW_MAX_K",)}

# the switches of the shipped library that step down the fallback chain of a max sweep
SWITCHES = ("SL_BELLMAN4", "SL_BELLMAN4_SHARED", "SL_BELLMAN4_POLICY", "SL_BELLMAN4_RAGGED", "SL_BELLMAN_MFMA",
            "SL_SUCC_CACHE")
SPLIT = {"SL_BELLMAN4_SHARED": "0"}          # k_bellman4s -> k_bellman4
NO_4X4X4 = {"SL_BELLMAN4": "0"}              # -> k_bellman_mfma
NO_MFMA = {"SL_BELLMAN_MFMA": "0"}           # -> k_bellman


# ---------------------------------------------------------------------------------------------
# The launchers' choices restated (sl_bellman4_launch, bellman_mfma, bellman_valu, Solver::matvec).
# ---------------------------------------------------------------------------------------------
def bellman4_blocks(rows):
    """(row blocks, quarter) of k_bellman4 / k_bellman4s for `rows` = n_actions * d (action, output)
    rows: full blocks of 16 rows, a quarter block behind them for a remainder of 1 to 4 rows; None
    beyond 48 rows (the launcher declines)."""
    if rows < 1 or rows > 48:
        return None
    quarter = rows > 16 and 1 <= rows % 16 <= 4
    return (rows // 16 if quarter else -(-rows // 16)), int(quarter)


def mfma_column_blocks(n_actions, dout):
    """Column blocks of k_bellman_mfma for one head with `dout` outputs: 1, 3 or 6 blocks of 16
    (action, output) columns; None beyond 6 (the launcher declines)."""
    ncb = -(-n_actions * dout // 16)
    return None if ncb > 6 else (1 if ncb <= 1 else (3 if ncb <= 3 else 6))


def valu_actions(n_actions, max_actions):
    """The action bucket of k_bellman<actions<=A, d>; 0 is policy evaluation."""
    return 0 if n_actions == 0 else (3 if n_actions <= 3 else (9 if n_actions <= 9 else max_actions))


def matvec_bucket(k, row_max):
    """The row-width bucket of k_value_matvec: the smallest compiled width that holds k entries."""
    return 2 if k <= 2 else (k if k <= 5 else (8 if k <= 8 else row_max))


def instantiations(constants):
    """kernel -> set of parameter tuples: what the DISPATCH lists compile, macros resolved."""
    def values(unit, index):
        return [int(constants.get(v, v)) for v in DISPATCH[unit][index][1]]
    b, b4, s, p = "sl_bellman.hip", "sl_bellman4.hip", "sl_succ.hip", "sl_policy_solve.hip"
    rq = [(v // 2, v % 2) for v in values(b4, 3)]
    return {
        "k_bellman_policy_mfma": {(d,) for d in values(b, 0)},
        "k_bellman_mfma": set(itertools.product(values(b, 1), values(b, 2))),        # (d, column blocks | 0)
        "k_bellman": set(itertools.product(values(b, 4), values(b, 3))),             # (actions, d)
        "k_bellman4_policy_distinct": {(d,) for d in values(b4, 0)},
        "k_bellman4_policy": {(d,) for d in values(b4, 1)},
        "k_bellman4": {(d,) + q for d in values(b4, 2) for q in rq},                 # (d, row blocks, quarter)
        "k_bellman4s": {(d,) + q for d in values(b4, 2) for q in rq},
        "k_bellman_lookup": set(itertools.product(values(b4, 4), values(b4, 5))),    # (d, filling)
        "k_succ_select": {(d,) for d in values(s, 0)},
        "k_bellman_cached": set(itertools.product(values(s, 1), values(s, 2))),      # (d, policy)
        "k_succ_policy_miss": {(d,) for d in values(s, 3)},
        "k_policy_operator_rows": {(d,) for d in values(p, 0)},
        "k_value_matvec": set(itertools.product(MATVEC_MODES, values(p, 1))),        # (mode, widest row)
    }


# ---------------------------------------------------------------------------------------------
# Cases.  `name` / `kw` / `nv` go to cases.make_case (chain3: cases.make_case_3d; two_actions:
# two_action_case below), `na` actions np.linspace(-1, 1, na) per action dimension, `env` the
# switches set before the context is created, `cache` the successor cache of the context.
# ---------------------------------------------------------------------------------------------
def case(name, kw, nv, na, env=None, cache=True):
    return dict(name=name, kw=dict(kw), nv=nv, na=na, env=dict(env or {}), cache=cache)


CP64 = ("cartpole", dict(n_gp=90), [3, 4, 3, 64])       # whole 64-cell tiles: the 4x4x4 kernels
CP5 = ("cartpole", dict(n_gp=90), [3, 3, 2, 5])         # ragged rows: k_bellman4s declines
CPA = ("cartpole", dict(dynamics="analytic"), [3, 4, 3, 5])
ONE = ("1d", dict(), 65)
CH3 = ("chain3", dict(dynamics="gp", n_gp=60), [5, 6, 7])
PEND = ("pendulum", dict(dynamics="analytic"), [5, 7])
TWO = ("two_actions", dict(), [5, 7])


def two_action_case(num_points):
    """The smallest model with two action dimensions (the Python surface takes up to
    _hip.MAX_ACTION_DIM = 2 and accepts this one): the linear pendulum of make_case on a 2-D grid
    with a second input column (half the first one's gain on the other state), a 2 x 2 linear
    policy, saturated like every policy of the cases."""
    import numpy as np
    from safe_learning_amd.benchmarks import make_case
    out = make_case("pendulum", num_points=num_points, dynamics="linear")
    a, b = out["A_true"], out["B_true"]
    b2 = np.hstack((b, 0.5 * b[::-1]))
    out.update(name="two_actions", m=2, K=np.vstack((out["K"], 0.3 * out["K"][:, ::-1])),
               B_true=b2, dynamics={"kind": "linear", "matrix": np.hstack((a, b2))})
    return out


def make(c):
    """The parameter dict of a ledger case (the same numbers for the engine and the oracle)."""
    import cases
    if c["name"] == "chain3":
        return cases.make_case_3d(num_points=c["nv"], **c["kw"])
    if c["name"] == "two_actions":
        return two_action_case(c["nv"])
    return cases.make_case(c["name"], num_points=c["nv"], **c["kw"])


def action_set(c, m=1):
    """np.linspace(-1, 1, na) as everywhere else; with two action dimensions the second column runs
    the other way at half the size (na distinct rows)."""
    import numpy as np
    col = np.linspace(-1, 1, c["na"])[:, None]
    return col if m == 1 else np.hstack((col, -0.5 * col))


# ---------------------------------------------------------------------------------------------
# Entries.
# ---------------------------------------------------------------------------------------------
ENTRIES = []


def _reach(kernel, params, expect, case=None, existing=None, down=None, role="max", shape=None):
    """`expect`: substring of Context.last_kernel() after the sweep.  `existing`: the test id that
    reaches the instantiation already (no new case), `shape` = (d, n_actions) of that test where the
    launchers' rules decide by them.  `down`: (switches, expected kernel, rtol, atol) of the kernel
    one step down the fallback chain, to be compared on the same inputs.  `role`: what the case is
    for (a max sweep, the successor cache, the solver)."""
    assert (case is None) != (existing is None)
    ENTRIES.append(dict(kind="reachable", kernel=kernel, params=tuple(params), expect=expect, case=case,
                        existing=existing, down=down, role=role, shape=shape))


def _unreachable(kernel, params, reason, check):
    """`reason`: a statement that `check(constants)` verifies by its own arithmetic."""
    ENTRIES.append(dict(kind="unreachable", kernel=kernel, params=tuple(params), reason=reason, check=check))


RL = "tests.test_gpu_rl::"
SC = "tests.test_gpu_successor_cache::"
PE = "tests.test_gpu_policy_evaluation::"


def _with_env(c, env):
    return dict(c, env=dict(env))


# ---- k_bellman4s / k_bellman4 <d, row blocks, quarter> (+ k_bellman_lookup) -------------------
def _b4_rows_reachable(d, max_actions):
    return {bellman4_blocks(na * d) for na in range(1, max_actions + 1)} - {None}


_B4_EXISTING = {(2, 1, 1): ("test_bellman_sweep_4x4x4_kernel[pendulum-kw0-nv0-9]", 9),
                (2, 1, 0): ("test_bellman_sweep_4x4x4_kernel[pendulum-kw1-nv1-2]", 2),
                (2, 2, 0): ("test_bellman_sweep_4x4x4_kernel[pendulum-kw2-nv2-16]", 16),
                (4, 2, 1): ("test_bellman_sweep_4x4x4_kernel[cartpole-kw3-nv3-9]", 9),
                (4, 3, 0): ("test_bellman_sweep_4x4x4_kernel[cartpole-kw4-nv4-12]", 12)}
_B4_NEW = {(4, 1, 0): 4, (4, 1, 1): 5, (4, 2, 0): 8}            # -> actions on the CP64 grid
for _key in sorted(set(_B4_EXISTING) | set(_B4_NEW)):
    _tail = "<d=%d, row blocks=%d, quarter=%d>" % _key
    if _key in _B4_EXISTING:
        _id, _na = _B4_EXISTING[_key]
        _reach("k_bellman4s", _key, "k_bellman4s" + _tail, existing=RL + _id, shape=(_key[0], _na))
        _reach("k_bellman4", _key, "k_bellman4" + _tail, existing=RL + _id, shape=(_key[0], _na))
    else:
        _c = case(*CP64, na=_B4_NEW[_key])
        _mfma = "k_bellman_mfma<d=4, column blocks=%d, heads=1>" % mfma_column_blocks(_c["na"], 4)
        _reach("k_bellman4s", _key, "k_bellman4s" + _tail, case=_c,
               down=(SPLIT, "k_bellman4" + _tail, 1e-12, 1e-14))
        _reach("k_bellman4", _key, "k_bellman4" + _tail, case=_with_env(_c, SPLIT),
               down=(NO_4X4X4, _mfma, 1e-11, 1e-13))
for _rb, _q in ((2, 1), (3, 0)):
    for _kernel in ("k_bellman4s", "k_bellman4"):
        _unreachable(_kernel, (2, _rb, _q),
                     "rows = 2 * n_actions <= 2 * SL_MAX_ACTIONS = 32 < 33: no action count of a 2-D sweep gives "
                     "(row blocks, quarter) = (%d, %d)" % (_rb, _q),
                     lambda c, _rq=(_rb, _q): 2 * c["SL_MAX_ACTIONS"] < 33 and
                     _rq not in _b4_rows_reachable(2, c["SL_MAX_ACTIONS"]))

# k_bellman_lookup<d, filling>: filling follows the successor cache of the context
_reach("k_bellman_lookup", (2, 1), "k_bellman_lookup<2>",
       existing=SC + "test_cached_max_sweeps_are_bit_identical[pendulum-kw0-nv0-9-k_bellman_lookup]")
_reach("k_bellman_lookup", (2, 0), "k_bellman_lookup<2>",
       existing=SC + "test_cached_max_sweeps_are_bit_identical[pendulum-kw0-nv0-9-k_bellman_lookup]")
_reach("k_bellman_lookup", (4, 1), "k_bellman_lookup<4>",
       existing=SC + "test_cached_max_sweeps_are_bit_identical[cartpole-kw1-nv1-9-k_bellman_lookup]")
_reach("k_bellman_lookup", (4, 0), "k_bellman_lookup<4>",
       existing=SC + "test_cached_max_sweeps_are_bit_identical[cartpole-kw1-nv1-9-k_bellman_lookup]")

# ---- k_bellman4_policy<d>, k_bellman4_policy_distinct<d>, k_bellman_policy_mfma<d> -----------
for _d, _id in ((2, "test_policy_evaluation_4x4x4_kernel[pendulum-kw0-nv0-9-greedy]"),
                (4, "test_policy_evaluation_4x4x4_kernel[cartpole-kw3-nv3-16-random]")):
    _reach("k_bellman4_policy", (_d,), "k_bellman4_policy<d=%d>" % _d, existing=RL + _id)
    _reach("k_bellman4_policy_distinct", (_d,), "k_bellman4_policy<d=%d>" % _d, existing=RL + _id)
    _reach("k_bellman_policy_mfma", (_d,), "k_bellman_policy_mfma<d=%d>" % _d, existing=RL + _id)

# ---- k_bellman_mfma<d, column blocks, heads> (0 column blocks: one block per head) ------------
_MFMA_EXISTING = {(2, 1): ("test_discrete_policy_optimization[pendulum-kw2-nv2-3]", 3),
                  (2, 3): ("test_discrete_policy_optimization[pendulum-kw1-15-9]", 9),
                  (4, 3): ("test_discrete_policy_optimization[cartpole-kw3-5-9]", 9),
                  (4, 6): ("test_discrete_policy_optimization[cartpole-kw4-nv4-16]", 16),
                  (4, 0): ("test_discrete_policy_optimization[cartpole-kw5-4-9]", 9),
                  (2, 0): ("test_discrete_policy_optimization[pendulum-kw6-nv6-9]", 9)}
for (_d, _n), (_id, _na) in sorted(_MFMA_EXISTING.items()):
    _reach("k_bellman_mfma", (_d, _n), "k_bellman_mfma<d=%d, column blocks=%d, heads=%d>"
           % (_d, _n or 1, _d if _n == 0 else 1), existing=RL + _id, shape=(_d, _na))
_reach("k_bellman_mfma", (4, 1), "k_bellman_mfma<d=4, column blocks=1, heads=1>", case=case(*CP5, na=4),
       down=(NO_MFMA, "k_bellman<actions<=9, d=4>", 1e-9, 1e-12))
_unreachable("k_bellman_mfma", (2, 6),
             "column blocks = ceil(2 * n_actions / 16) <= ceil(2 * SL_MAX_ACTIONS / 16) = 2: a 2-D sweep never "
             "needs more than 3 column blocks (6 start at 25 actions)",
             lambda c: all(mfma_column_blocks(na, 2) in (1, 3) for na in range(1, c["SL_MAX_ACTIONS"] + 1)) and
             mfma_column_blocks(25, 2) == 6 and c["SL_MAX_ACTIONS"] < 25)

# ---- k_bellman<actions<=A, d> ----------------------------------------------------------------
# d = 0 is the runtime-dimension flavour: a 3-D grid (the kernel note then says d=3) and every
# model with two action dimensions (note: d=0).
_VALU_EXISTING = {(0, 4): (RL + "test_value_iteration[cartpole-kw3-6]", 0),
                  (0, 2): (RL + "test_value_iteration[pendulum-kw0-21]", 0),
                  (0, 1): (RL + "test_value_iteration_1d_lqr", 0),
                  (0, 0): (PE + "test_rows_versus_sweep_and_oracle[chain3-nv6-kw6]", 0),
                  (3, 4): (SC + "test_cached_max_sweeps_are_bit_identical[cartpole-kw5-6-3-k_bellman<]", 3),
                  (3, 0): (SC + "test_three_dimensional_max_sweeps_recompute_and_commit_no_cache", 3),
                  (9, 2): (RL + "test_discrete_policy_optimization[pendulum-kw0-15-9]", 9),
                  (9, 4): (RL + "test_discrete_policy_optimization_with_a_lyapunov_constraint[cartpole-kw3-nv3-9]", 9),
                  (16, 2): (SC + "test_cached_max_sweeps_are_bit_identical[pendulum-kw6-nv6-16-k_bellman<]", 16)}
_VALU_NEW = {(3, 2): case(*PEND, na=3), (16, 4): case(*CPA, na=16),
             (3, 1): case(*ONE, na=3), (9, 1): case(*ONE, na=9), (16, 1): case(*ONE, na=16),
             (9, 0): case(*CH3, na=9), (16, 0): case(*CH3, na=16)}
for _a, _d in sorted(set(_VALU_EXISTING) | set(_VALU_NEW)):
    _note = "k_bellman<actions<=%d, d=%d>" % (_a, 3 if _d == 0 else _d)
    if (_a, _d) in _VALU_EXISTING:
        _reach("k_bellman", (_a, _d), _note, existing=_VALU_EXISTING[(_a, _d)][0],
               shape=(3 if _d == 0 else _d, _VALU_EXISTING[(_a, _d)][1]))
    else:
        _reach("k_bellman", (_a, _d), _note, case=_VALU_NEW[(_a, _d)])
# the same instantiation through its other door: two action dimensions
_reach("k_bellman", (3, 0), "k_bellman<actions<=3, d=0>", case=case(*TWO, na=3))

# ---- the successor cache: k_bellman_cached<d, policy>, k_succ_select<d>, k_succ_policy_miss<d> -
_CACHE_MAX = {2: "test_cached_max_sweeps_are_bit_identical[pendulum-kw0-nv0-9-k_bellman_lookup]",
              4: "test_cached_max_sweeps_are_bit_identical[cartpole-kw1-nv1-9-k_bellman_lookup]"}
_CACHE_POLICY = {2: "test_policy_evaluation_selects_cached_entries[pendulum-kw0-nv0-9]",
                 4: "test_policy_evaluation_selects_cached_entries[cartpole-kw1-nv1-9]"}
# (fill kernel, case) of the cache test: d = 1, and each fill kernel at the shapes of the cases above
CACHE_CASES = [("k_bellman<actions<=9, d=1>", case(*ONE, na=9)),
               ("k_bellman_lookup<4>", case(*CP64, na=4)),
               ("k_bellman_lookup<4>", case(*CP64, na=5)),
               ("k_bellman_lookup<4>", case(*CP64, na=8)),
               ("k_bellman_mfma<d=4, column blocks=1, heads=1>", case(*CP5, na=4)),
               ("k_bellman<actions<=9, d=4>", case(*CPA, na=9)),
               ("k_bellman<actions<=3, d=2>", case(*PEND, na=3))]
for _d in (4, 2):
    _reach("k_bellman_cached", (_d, 0), "k_bellman_cached<d=%d, max>" % _d, existing=SC + _CACHE_MAX[_d])
    _reach("k_bellman_cached", (_d, 1), "k_bellman_cached<d=%d, policy>" % _d, existing=SC + _CACHE_POLICY[_d])
    _reach("k_succ_select", (_d,), "k_bellman_cached<d=%d, policy>" % _d, existing=SC + _CACHE_POLICY[_d])
# (the greedy table read at its own vertices takes values between the actions at ambiguous vertices)
_reach("k_succ_policy_miss", (4,), "k_bellman_cached<d=4, policy> (successor cache, 9 actions, ",
       existing=RL + "test_discrete_policy_optimization[cartpole-kw13-nv13-9]")
_reach("k_succ_policy_miss", (2,), "k_bellman_cached<d=2, policy> (successor cache, 9 actions, ",
       existing=RL + "test_discrete_policy_optimization[pendulum-kw0-15-9]")
_reach("k_bellman_cached", (1, 0), "k_bellman_cached<d=1, max>", case=case(*ONE, na=9), role="cache")
_reach("k_bellman_cached", (1, 1), "k_bellman_cached<d=1, policy>", case=case(*ONE, na=9), role="cache")
_reach("k_succ_select", (1,), "k_bellman_cached<d=1, policy>", case=case(*ONE, na=9), role="cache")
_reach("k_succ_policy_miss", (1,), "one by one", case=case(*ONE, na=9), role="cache")


def _nothing_fills_three_dimensions(constants):
    lists = dict(DISPATCH["sl_bellman.hip"] + DISPATCH["sl_bellman4.hip"])
    return ("3" not in lists["k_bellman: d"] and "0" == lists["k_bellman: d"][-1] and
            all("3" not in lists[site] for site in ("k_bellman_mfma: d", "k_bellman4 / k_bellman4s: d",
                                                    "k_bellman_lookup: d")))


for _kernel, _params in (("k_bellman_cached", (3, 0)), ("k_bellman_cached", (3, 1)), ("k_succ_select", (3,)),
                         ("k_succ_policy_miss", (3,))):
    _unreachable(_kernel, _params,
                 "a cache serves sweeps only after a max sweep filled it; 3 is in no dimension list of a kernel that "
                 "fills (k_bellman_lookup <4, 2>, k_bellman_mfma <4, 2>, k_bellman <4, 2, 1, 0>): a 3-D sweep runs "
                 "k_bellman<A, 0>, the last listed, which has no located points to leave and commits nothing",
                 _nothing_fills_three_dimensions)

# ---- k_policy_operator_rows<d> ---------------------------------------------------------------
for _d, _id in ((1, "[1d-33-kw0]"), (2, "[pendulum-nv1-kw1]"), (3, "[chain3-nv6-kw6]"), (4, "[cartpole-nv3-kw3]")):
    _reach("k_policy_operator_rows", (_d,), "k_policy_operator_rows<d=%d>" % _d,
           existing=PE + "test_rows_versus_sweep_and_oracle" + _id)

# ---- k_value_matvec<mode, widest row> --------------------------------------------------------
# GMRES runs modes 2 and 0 (mode 1 too when its safeguard takes Jacobi cycles), Jacobi mode 1.
MATVEC_WIDTHS = (6, 8, 9, 16)                 # row widths of the solver test: buckets 8 and 16
_MATVEC_EXISTING = {2: {0: "test_diverging_solve_is_not_converged", 1: "test_diverging_solve_is_not_converged",
                        2: "test_diverging_solve_is_not_converged"},
                    3: dict.fromkeys((0, 1, 2), "test_safeguard_falls_back_to_jacobi_on_the_device"),
                    4: dict.fromkeys((0, 1, 2), "test_reference_known_answer"),
                    5: {0: "test_fixed_point[cartpole-nv8-kw8-greedy]", 2: "test_fixed_point[cartpole-nv8-kw8-greedy]",
                        1: "test_rows_versus_sweep_and_oracle[cartpole-nv3-kw3]"}}
for _kmax in (2, 3, 4, 5):
    for _mode in MATVEC_MODES:
        _reach("k_value_matvec", (_mode, _kmax), "k_value_matvec", existing=PE + _MATVEC_EXISTING[_kmax][_mode])
for _kmax, _k in ((8, 6), (16, 9)):
    for _mode in MATVEC_MODES:
        _reach("k_value_matvec", (_mode, _kmax), "k_value_matvec", case=dict(n=300, k=_k), role="solve")


def reachable(role=None, new=True):
    """The reachable entries (of one role) that name a case (new=True) or an existing test."""
    return [e for e in ENTRIES if e["kind"] == "reachable" and (role is None or e["role"] == role)
            and (e["case"] is not None) == new]


def entry_id(e):
    c = e.get("case")
    tail = "" if c is None or "name" not in c else "-%s-%s-%d%s" % (
        c["name"], "x".join(str(v) for v in (c["nv"] if isinstance(c["nv"], list) else [c["nv"]])), c["na"],
        "".join("-%s=%s" % kv for kv in sorted(c["env"].items())))
    return "%s<%s>%s" % (e["kernel"], ",".join(str(p) for p in e["params"]), tail)
