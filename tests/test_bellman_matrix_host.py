"""The ledger of tests/bellman_matrix.py against the sources and the oracle (no GPU).

* the ``sl_with_dim<...>`` lists of the four dispatching units are the lists the ledger declares, site
  by site: an instantiation added to or dropped from a dispatcher fails here until the ledger follows;
* every instantiation those lists compile has exactly the entries the ledger gives it, and the cases
  select what they claim by the launchers' own rules (restated in the ledger);
* the "unreachable" reasons hold by their own arithmetic against the constants they name;
* every case is well posed on the oracle alone: no more than the project's 2 % of its (vertex, action)
  successors are ambiguous points of the value table."""

import os
import re

import numpy as np
import pytest
import scipy.linalg

import bellman_matrix as bm
import cases
import exclusions
import oracle
from conftest import ROOT

CSRC = os.path.join(ROOT, "safe_learning_amd", "csrc")


def _source(name):
    with open(os.path.join(CSRC, name)) as handle:
        text = handle.read()
    return re.sub(r"//[^\n]*", "", text)                  # (comments speak of sl_with_dim too)


def dispatch_lists(text):
    """The template arguments of every ``sl_with_dim<...>(`` call, in source order."""
    return [tuple(v.strip() for v in m.group(1).split(","))
            for m in re.finditer(r"\bsl_with_dim\s*<([^<>]*)>\s*\(", text)]


@pytest.fixture(scope="module")
def constants():
    out = {}
    for header, names in bm.CONSTANTS.items():
        text = _source(header)
        for name in names:
            found = re.findall(r"^\s*#\s*define\s+%s\s+(\d+)\b" % name, text, flags=re.M)
            assert len(found) == 1, (header, name, found)
            out[name] = int(found[0])
    return out


@pytest.mark.parametrize("unit", sorted(bm.DISPATCH))
def test_ledger_lists_are_the_dispatchers_lists(unit):
    declared = [values for _, values in bm.DISPATCH[unit]]
    assert dispatch_lists(_source(unit)) == declared, \
        "%s: the sl_with_dim lists changed - update tests/bellman_matrix.py (DISPATCH and the entries)" % unit


def test_list_parser_sees_an_edited_list():
    """An instantiation added to, or dropped from, a dispatcher changes what the parser returns."""
    text = _source("sl_succ.hip")
    assert dispatch_lists(text.replace("sl_with_dim<4, 3, 2, 1>", "sl_with_dim<4, 2, 1>", 1))[0] == ("4", "2", "1")
    assert dispatch_lists(text.replace("sl_with_dim<1, 0>", "sl_with_dim<1, 0, 2>")) != dispatch_lists(text)


def test_matvec_modes_are_the_solvers(constants):
    text = _source("sl_policy_solve.hip")
    assert tuple(sorted({int(m) for m in re.findall(r"\bmatvec<(\d+)>\(", text)})) == bm.MATVEC_MODES
    widths = {bm.matvec_bucket(k, constants["SL_ROW_MAX_K"]) for k in range(1, constants["SL_ROW_MAX_K"] + 1)}
    assert widths == {p[1] for p in bm.instantiations(constants)["k_value_matvec"]}


def test_every_instantiation_has_its_entries(constants):
    compiled = bm.instantiations(constants)
    listed = {}
    for e in bm.ENTRIES:
        listed.setdefault(e["kernel"], {}).setdefault(e["params"], set()).add(e["kind"])
    assert set(listed) == set(compiled)
    for kernel, params in compiled.items():
        assert set(listed[kernel]) == params, (kernel, set(listed[kernel]) ^ params)
        for p, kinds in listed[kernel].items():
            assert len(kinds) == 1, "%s%s is listed as reachable AND unreachable" % (kernel, p)


def _c_expression(text, pattern):
    """The C++ expression that `pattern` (a regular expression with one group) captures in `text`, as
    Python source: nested `a ? b : c`, `&&`, integer `/`."""
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)

    def convert(s):
        s = s.strip()
        depth = 0
        for i, ch in enumerate(s):
            depth += ch == "("
            depth -= ch == ")"
            if ch == "?" and depth == 0:
                nested, level = 0, 0
                for j in range(i + 1, len(s)):
                    level += s[j] == "("
                    level -= s[j] == ")"
                    nested += s[j] == "?" and level == 0
                    if s[j] == ":" and level == 0:
                        if nested == 0:
                            return "((%s) if (%s) else (%s))" % (convert(s[i + 1:j]), convert(s[:i]), convert(s[j + 1:]))
                        nested -= 1
        if s.startswith("(") and s.endswith(")") and s.count("(") == s.count(")") and "?" in s:
            return "(%s)" % convert(s[1:-1])
        return s.replace("&&", " and ").replace("/", "//")
    return convert(found[0])


def test_the_launchers_rules_are_the_ledgers(constants):
    """The rules restated in the ledger against the C++ expressions of the launchers themselves,
    evaluated over every argument a sweep can pass."""
    b4, b, ps = _source("sl_bellman4.hip"), _source("sl_bellman.hip"), _source("sl_policy_solve.hip")
    top = constants["SL_MAX_ACTIONS"]
    quarter = _c_expression(b4, r"pk\.quarter\s*=\s*([^;]+);")
    nrb = _c_expression(b4, r"pk\.nrb\s*=\s*([^;]+);")
    limit = re.findall(r"if\s*\(rows\s*>\s*(\d+)\)\s*return SL_DECLINED;", b4)
    assert limit == ["48"] and re.search(r"const int rows\s*=\s*n_actions\s*\*\s*hh\.dout;", b4)
    assert re.search(r"if\s*\(hh\.dout\s*!=\s*d\s*\|\|", b4)
    for rows in range(1, 49):
        q = eval(quarter, {"rows": rows})
        class pk:
            quarter = q
        assert (eval(nrb, {"rows": rows, "pk": pk}), q) == bm.bellman4_blocks(rows), rows
    assert bm.bellman4_blocks(49) is None
    ncb_t = _c_expression(b, r"const int ncb_t\s*=\s*([^;]+);")
    assert re.search(r"if\s*\(ncb\s*>\s*6\)\s*return SL_DECLINED;", b)
    assert re.search(r"const int c\s*=\s*\(n_actions\s*\*\s*ctx->gp_heads\[h\]\.dout\s*\+\s*15\)\s*/\s*16;", b)
    for d in (2, 4):
        for na in range(1, top + 1):
            ncb = -(-na * d // 16)
            want = bm.mfma_column_blocks(na, d)
            assert (want is None) == (ncb > 6)
            if want is not None:
                assert eval(ncb_t, {"policy_mode": False, "ncb": ncb}) == want, (d, na)
    amax = _c_expression(b, r"const int amax\s*=\s*([^;]+);")
    for na in range(0, top + 1):
        assert eval(amax, {"n_actions": na, "SL_MAX_ACTIONS": top}) == bm.valu_actions(na, top), na
    assert re.search(r"n_actions\s*>\s*SL_MAX_ACTIONS", b)              # sl_bellman_sweep refuses more
    bucket = _c_expression(ps, r"const int bucket\s*=\s*([^;]+);")
    row_max = constants["SL_ROW_MAX_K"]
    for k in range(1, row_max + 1):
        assert eval(bucket, {"k": k, "SL_ROW_MAX_K": row_max}) == bm.matvec_bucket(k, row_max), k
    # the runtime-dimension flavour hands no cache over
    assert re.search(r"if constexpr\s*\(DT != 0\)\s*\{\s*if\s*\(ctx->succ\.filling\)", b)


def test_cases_select_what_they_claim(constants):
    top = constants["SL_MAX_ACTIONS"]
    for e in bm.reachable(new=True):
        c, p = e["case"], e["params"]
        if e["kernel"] in ("k_bellman4s", "k_bellman4"):
            assert bm.bellman4_blocks(c["na"] * p[0]) == p[1:] and bm.make(c)["d"] == p[0], e
            assert c["nv"][-1] % 64 == 0
            assert c["env"] == ({} if e["kernel"] == "k_bellman4s" else bm.SPLIT)
        elif e["kernel"] == "k_bellman_mfma":
            assert bm.mfma_column_blocks(c["na"], p[0]) == p[1] and bm.make(c)["d"] == p[0], e
            # ragged rows that fill less than 70 % of their tiles: the 4x4x4 kernels decline
            assert c["nv"][-1] % 64 != 0 and 10 * c["nv"][-1] < 7 * 64 * -(-c["nv"][-1] // 64)
        elif e["kernel"] == "k_bellman":
            made = bm.make(c)
            variant = made["d"] if made["m"] == 1 and made["d"] in (4, 2, 1) else 0
            assert (bm.valu_actions(c["na"], top), variant) == p, e
            assert made["dynamics"]["kind"] != "gp" or variant not in (4, 2)       # nothing takes it first
        elif e["kernel"] == "k_value_matvec":
            assert bm.matvec_bucket(c["k"], constants["SL_ROW_MAX_K"]) == p[1], e
        else:
            assert e["role"] == "cache" and bm.make(c)["d"] == p[0], e
        assert 1 <= c.get("na", 1) <= top
    assert {bm.matvec_bucket(k, constants["SL_ROW_MAX_K"]) for k in bm.MATVEC_WIDTHS} == {8, constants["SL_ROW_MAX_K"]}
    # the existing tests the ledger names, by the same rules at their (d, n_actions)
    for e in bm.reachable(new=False):
        if e["shape"] is None:
            continue
        (d, na), p = e["shape"], e["params"]
        if e["kernel"] in ("k_bellman4s", "k_bellman4"):
            assert (d,) + bm.bellman4_blocks(na * d) == p, e
        elif e["kernel"] == "k_bellman_mfma":
            assert p == (d, 0) or (d, bm.mfma_column_blocks(na, d)) == p, e       # (0: the stack cases, one output per head)
        else:
            assert e["kernel"] == "k_bellman" and (bm.valu_actions(na, top), d if d != 3 else 0) == p, e
    # every cache-role entry's case is one of the cache cases
    cache_cases = [c for _, c in bm.CACHE_CASES]
    for e in bm.reachable(role="cache"):
        assert e["case"] in cache_cases, e


def _parametrisations(function):
    """id -> {argument: value} of a test function's one parametrize mark, with pytest's default ids
    (text and numbers as they are, anything else the argument's name and the row's index)."""
    marks = [m for m in getattr(function, "pytestmark", []) if m.name == "parametrize"]
    if not marks:
        return {}
    assert len(marks) == 1, function.__name__
    names = [n.strip() for n in marks[0].args[0].split(",")]
    out = {}
    for index, row in enumerate(marks[0].args[1]):
        row = row if len(names) > 1 else (row,)
        parts = [str(v) if isinstance(v, (str, int, float, bool)) or v is None else "%s%d" % (n, index)
                 for n, v in zip(names, row)]
        out["-".join(parts)] = dict(zip(names, row))
    return out


def test_existing_tests_exist():
    """The tests the ledger names are real parametrisations, and where the ledger records their
    (d, n_actions) these are the ones of that parametrisation."""
    import importlib
    dims = {"1d": 1, "pendulum": 2, "chain3": 3, "cartpole": 4}
    for e in bm.reachable(new=False):
        module, _, name = e["existing"].partition("::")
        function, _, params = name.partition("[")
        test = getattr(importlib.import_module(module.split(".", 1)[1]), function, None)
        assert callable(test), e["existing"]
        rows = _parametrisations(test)
        if not params:
            assert not rows, e["existing"]
            continue
        assert params.rstrip("]") in rows, (e["existing"], sorted(rows))
        row = rows[params.rstrip("]")]
        if e["shape"] is not None and "na" in row:
            assert (dims[row["name"]], row["na"]) == e["shape"], e
        if e["kernel"] in ("k_bellman_lookup", "k_bellman_cached", "k_succ_select", "k_policy_operator_rows",
                           "k_bellman4_policy", "k_bellman4_policy_distinct", "k_bellman_policy_mfma"):
            assert dims[row["name"]] == e["params"][0], e


@pytest.mark.parametrize("entry", [e for e in bm.ENTRIES if e["kind"] == "unreachable"],
                         ids=lambda e: bm.entry_id(e))
def test_unreachable_reasons_hold(entry, constants):
    assert entry["check"](constants), entry["reason"]
    for name in re.findall(r"\bSL_[A-Z_]+\b", entry["reason"]):
        assert name in constants, "the reason names %s, which no header of bm.CONSTANTS defines" % name


def test_an_unreachable_reason_fails_when_its_constant_moves(constants):
    """With 32 actions a 2-D sweep would reach every instantiation the reasons rule out."""
    moved = dict(constants, SL_MAX_ACTIONS=32)
    for e in bm.ENTRIES:
        if e["kind"] == "unreachable" and "SL_MAX_ACTIONS" in e["reason"]:
            assert not e["check"](moved), e["reason"]


def oracle_pair(c):
    """The oracle's PolicyIteration of a ledger case, as tests/test_gpu_rl.py::_rl_pair builds it."""
    made = bm.make(c)
    d, m = made["d"], made["m"]
    grid = oracle.GridWorld(made["limits"], c["nv"])
    v0 = -np.random.default_rng(4).random((grid.nindex, 1))
    policy, dynamics, _, _ = cases.oracle_specs(made)
    vf = oracle.Triangulation(grid, v0, project=True)
    reward = oracle.QuadraticFunction(-scipy.linalg.block_diag(np.eye(d), 0.1 * np.eye(m)))
    return oracle.PolicyIteration(policy, dynamics, reward, vf, gamma=0.95), vf, bm.action_set(c, m)


def successor_mask(orl, ovf, actions):
    """ok[N, A]: the successor of (vertex, action) is no ambiguous point of the value table."""
    x = orl.state_space
    ok = np.ones((len(x), len(actions)), dtype=bool)
    for a, action in enumerate(actions):
        nxt = orl.dynamics(x, np.broadcast_to(action, (len(x), len(action))))
        ok[:, a] = ~exclusions.ambiguous_points(ovf, nxt[0] if isinstance(nxt, tuple) else nxt)
    return ok


def _sweep_cases():
    seen, out = set(), []
    for c in [e["case"] for e in bm.reachable(new=True) if "name" in e["case"]] + [c for _, c in bm.CACHE_CASES]:
        key = (c["name"], str(c["nv"]), c["na"])
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


@pytest.mark.parametrize("c", _sweep_cases(), ids=lambda c: "%s-%s-%d" % (c["name"], c["nv"], c["na"]))
def test_cases_are_well_posed_on_the_oracle(c):
    orl, ovf, actions = oracle_pair(c)
    assert len(np.unique(actions, axis=0)) == c["na"]
    ok = successor_mask(orl, ovf, actions)
    excluded = 1.0 - ok.mean()
    print("%s %s x %d: %d of %d (vertex, action) successors excluded" % (c["name"], c["nv"], c["na"],
                                                                         int((~ok).sum()), ok.size))
    assert excluded <= exclusions.LIMITS["successor"]
    # the oracle's sweep is defined and not degenerate: the actions differ in value somewhere
    orl.policy = oracle.Triangulation(ovf.discretization, np.zeros((ovf.discretization.nindex, actions.shape[1])))
    q, _ = orl.discrete_policy_optimization(actions)
    assert np.isfinite(q).all() and (np.ptp(q, axis=1) > 0).any()
