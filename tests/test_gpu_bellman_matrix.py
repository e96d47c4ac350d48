"""Every reachable instantiation of the dynamic-programming kernels that no other test selects
(tests/bellman_matrix.py; needs an MI355X).

Per ledger entry: the sweep must NAME the instantiation (a case that silently ran another kernel
fails), its action values, new table and greedy actions are held against the oracle's
``discrete_policy_optimization`` (``reinforcement_learning.py:266-279``) and against the kernel one
step down the fallback chain on the same inputs.  The successor cache at d = 1 and behind each newly
covered fill kernel; ``k_value_matvec`` at the row widths 6 to 16."""

import ctypes as C

import numpy as np
import pytest
import scipy.linalg
from numpy.testing import assert_allclose, assert_array_equal

import bellman_matrix as bm
import exclusions
import oracle
from test_bellman_matrix_host import oracle_pair, successor_mask

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sl():
    import safe_learning_amd
    return safe_learning_amd


def _key(c, env=None):
    return (c["name"], str(c["nv"]), c["na"], tuple(sorted((c["env"] if env is None else env).items())), c["cache"])


def _engine_pair(sl, c, monkeypatch, env=None, cache=None):
    """The engine's PolicyIteration of a ledger case with the same numbers as oracle_pair's (the
    switches are read when the context is created)."""
    from safe_learning_amd.benchmarks import build_specs
    for name in bm.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in (c["env"] if env is None else env).items():
        monkeypatch.setenv(name, value)
    made = bm.make(c)
    d, m = made["d"], made["m"]
    grid = sl.GridWorld(made["limits"], c["nv"])
    v0 = -np.random.default_rng(4).random((grid.nindex, 1))
    policy, dynamics, _, _ = build_specs(made)
    vf = sl.Triangulation(grid, v0, project=True)
    reward = sl.QuadraticFunction(-scipy.linalg.block_diag(np.eye(d), 0.1 * np.eye(m)))
    rl = sl.PolicyIteration(policy, dynamics, reward, vf, gamma=0.95)
    if not (c["cache"] if cache is None else cache):
        rl.successor_cache(0)
    return rl, vf, bm.action_set(c, m), v0


_SWEEPS, _ORACLE = {}, {}


def _max_sweep(sl, c, monkeypatch, env=None):
    """One max sweep: action values, new table, arg-max, residual, kernel note (once per case and
    switch setting: the cross-kernel partner of one entry is the subject of another)."""
    key = _key(c, env)
    if key not in _SWEEPS:
        rl, vf, actions, _ = _engine_pair(sl, c, monkeypatch, env)
        v_new, argmax, q, stats = rl._sweep(rl.policy, actions, want_q=True)
        n = rl._hi - rl._lo
        _SWEEPS[key] = dict(q=q[:n].cpu().numpy(), v=v_new[:n].cpu().numpy(), best=argmax[:n].cpu().numpy(),
                            residual=float(stats[0]), kernel=rl._ctx.last_kernel(),
                            cache=rl.successor_cache_info)
    return _SWEEPS[key]


def _oracle_sweep(c):
    """The oracle's action values of a case (computed once, never modified)."""
    key = _key(c, {})[:3]
    if key not in _ORACLE:
        orl, ovf, actions = oracle_pair(c)
        v0 = ovf.parameters.copy()
        ok = successor_mask(orl, ovf, actions)
        orl.policy = oracle.Triangulation(ovf.discretization,
                                          np.zeros((ovf.discretization.nindex, actions.shape[1])))
        oq, obest = orl.discrete_policy_optimization(actions)
        for array in (oq, obest, ok, v0):
            array.setflags(write=False)
        _ORACLE[key] = dict(q=oq, best=obest, ok=ok, v0=v0)
    return _ORACLE[key]


def _ties(oq):
    if oq.shape[1] < 2:
        return np.zeros(len(oq), dtype=bool)
    top2 = np.sort(oq, axis=1)[:, -2:]
    return np.abs(top2[:, 1] - top2[:, 0]) <= 1e-9 * np.abs(top2[:, 1])


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if a.size else 0.0


@pytest.mark.parametrize("entry", bm.reachable(role="max"), ids=bm.entry_id)
def test_max_sweep_instantiation(sl, entry, monkeypatch):
    c = entry["case"]
    label = "test_max_sweep_instantiation[%s]" % bm.entry_id(entry)
    got = _max_sweep(sl, c, monkeypatch)
    assert entry["expect"] in got["kernel"], "%s ran %s" % (label, got["kernel"])
    if entry["kernel"] == "k_bellman" and entry["params"][1] != 0 and c["cache"]:
        assert got["cache"]["fills"] == 1, got["cache"]
    ref = _oracle_sweep(c)
    ok_q, oq = ref["ok"], ref["q"]
    ok = ok_q.all(axis=1)
    exclusions.report(label, ok_q, "successor")
    print("%s: %s; oracle: max rel. difference of the action values %.3g, of the table %.3g" % (
        label, got["kernel"], _rel(got["q"][ok_q], oq[ok_q]), _rel(got["v"][ok], oq.max(axis=1)[ok])))
    assert_allclose(got["q"][ok_q], oq[ok_q], rtol=1e-9, atol=1e-12)
    assert_allclose(got["v"][ok], oq.max(axis=1)[ok], rtol=1e-9, atol=1e-12)
    tie = _ties(oq)
    assert not np.any((got["best"] != ref["best"]) & ok & ~tie)
    # the table is the row maximum of the action values, the arg-max its first maximiser: exactly
    assert_array_equal(got["v"], got["q"].max(axis=1))
    assert_array_equal(got["best"], got["q"].argmax(axis=1))
    if ok.all():
        assert_allclose(got["residual"], np.max(np.abs(oq.max(axis=1) - ref["v0"][:, 0])), rtol=1e-9)
    if entry["down"] is None:
        return
    env, expect, rtol, atol = entry["down"]
    other = _max_sweep(sl, c, monkeypatch, dict(c["env"], **env))
    assert expect in other["kernel"], "%s: one step down ran %s" % (label, other["kernel"])
    print("%s: against %s: max rel. difference %.3g (rtol %.0e)" % (label, other["kernel"],
                                                                    _rel(got["q"], other["q"]), rtol))
    assert_allclose(got["q"], other["q"], rtol=rtol, atol=atol)
    assert_array_equal(got["best"][~tie], other["best"][~tie])


def _loop(rl, vf, actions, sweeps, v0):
    vf.parameters = v0.copy()
    out = []
    for _ in range(sweeps):
        res = rl.value_iteration(actions)
        out.append((vf._host_parameters().copy(), rl.policy._host_parameters().copy(), res,
                    rl._ctx.last_kernel()))
    return out


@pytest.mark.parametrize("fill,c", bm.CACHE_CASES,
                         ids=["%s-%s-%d" % (c["name"], "x".join(map(str, np.atleast_1d(c["nv"]))), c["na"])
                              for _, c in bm.CACHE_CASES])
def test_successor_cache_behind_each_fill_kernel(sl, fill, c, monkeypatch):
    """Three cached against three recomputing max sweeps, bit for bit; then policy evaluation with a
    per-vertex table of cached actions (k_succ_select + k_bellman_cached<d, policy>) and with a few
    values outside the action set (k_succ_policy_miss), against the recomputing kernels and the
    oracle."""
    label = "test_successor_cache_behind_each_fill_kernel[%s-%s-%d]" % (c["name"], c["nv"], c["na"])
    rl, vf, actions, v0 = _engine_pair(sl, c, monkeypatch)
    rl_u, vf_u, _, _ = _engine_pair(sl, c, monkeypatch, cache=False)
    d = vf.discretization.ndim
    cached = _loop(rl, vf, actions, 3, v0)
    plain = _loop(rl_u, vf_u, actions, 3, v0)
    assert fill in cached[0][3] and "k_bellman_cached" not in cached[0][3], cached[0][3]
    for sweep, (got, want) in enumerate(zip(cached, plain)):
        assert_array_equal(got[0], want[0], err_msg="value table, sweep %d" % sweep)
        assert_array_equal(got[1], want[1], err_msg="greedy table, sweep %d" % sweep)
        assert got[2] == want[2], (sweep, got[2], want[2])
        assert "k_bellman_cached" not in want[3]
        if sweep:
            assert "k_bellman_cached<d=%d, max>" % d in got[3], got[3]
    assert not np.array_equal(cached[0][0], cached[2][0])          # the tables move
    info = rl.successor_cache_info
    assert info["valid"] == 1 and info["fills"] == 1 and info["hits"] == 2, info
    # the first sweep against the oracle (the later ones are bit for bit what recomputing gives)
    ref = _oracle_sweep(c)
    ok = ref["ok"].all(axis=1)
    exclusions.report(label, ref["ok"], "successor")
    assert_allclose(cached[0][0][ok, 0], ref["q"].max(axis=1)[ok], rtol=1e-9, atol=1e-12)
    # policy evaluation from identical inputs: a table of cached actions, then five values off the set
    orl, ovf, _ = oracle_pair(c)
    x = orl.state_space
    n = len(x)
    rng = np.random.default_rng(12)
    table = actions[rng.integers(0, c["na"], n)]
    off = table.copy()
    where = np.sort(rng.choice(n, 5, replace=False))
    off[where] = 0.0137 * (1 + np.arange(5))[:, None]
    assert not np.isin(off[where, 0], actions[:, 0]).any()
    for tab, nmiss in ((table, 0), (off, 5)):
        results = []
        for r, v in ((rl, vf), (rl_u, vf_u)):
            r.policy = np.ascontiguousarray(tab)
            v.parameters = v0.copy()
            res = r.value_iteration()
            results.append((v._host_parameters().copy(), res, r._ctx.last_kernel()))
        (got, res, kernel), (want, res_u, kernel_u) = results
        assert "k_bellman_cached<d=%d, policy>" % d in kernel and "k_bellman_cached" not in kernel_u, (kernel, kernel_u)
        assert ("one by one" in kernel) == (nmiss > 0), kernel
        if nmiss:
            assert "%d vertices" % nmiss in kernel, kernel
        print("%s: %s against %s: max rel. difference %.3g" % (label, kernel, kernel_u, _rel(got, want)))
        assert_allclose(got, want, rtol=1e-11, atol=1e-13)
        assert_allclose(res, res_u, rtol=1e-9)
        orl.policy = lambda states, _tab=tab: _tab
        ovf.parameters = v0.copy()
        nxt = orl.dynamics(x, tab)
        good = ~exclusions.ambiguous_points(ovf, nxt[0] if isinstance(nxt, tuple) else nxt)
        exclusions.report(label + " policy evaluation", good, "successor")
        orl.value_iteration()
        assert_allclose(got[good], ovf.parameters[good], rtol=1e-9, atol=1e-12)
    assert rl.successor_cache_info["policy_hits"] == 2


def _combine(cols, w, r, gamma, v):
    """r + gamma P v through the host shim of csrc/sl_policy_rows.h (the device's row combine)."""
    from test_policy_rows_host import load_shim
    k, n = cols.shape
    out = np.zeros(n)
    arrays = [np.ascontiguousarray(a) for a in (cols, w, r, v)]
    ptr = [a.ctypes.data_as(C.c_void_p) for a in arrays]
    assert load_shim().pr_combine(C.c_int64(n), k, ptr[0], ptr[1], ptr[2], C.c_double(gamma), ptr[3],
                                  out.ctypes.data_as(C.c_void_p)) == 0
    return out


@pytest.mark.parametrize("k", bm.MATVEC_WIDTHS)
def test_value_solve_wide_rows(sl, k):
    """k_value_matvec<mode, 8> and <mode, 16>: random row-stochastic ELL operators with 6 to 16
    entries per row through both solve methods against a dense solve, and one Jacobi step bit for
    bit against the host shim's row combine."""
    import torch
    from safe_learning_amd import _hip
    rng = np.random.default_rng(100 + k)
    n, gamma, m = 300, 0.98, 8
    cols = rng.integers(0, n, size=(n, k))
    w = rng.random((n, k))
    w /= w.sum(axis=1, keepdims=True)
    P = np.zeros((n, n))
    np.add.at(P, (np.repeat(np.arange(n), k), cols.ravel()), w.ravel())
    r = rng.normal(size=n)
    exact = np.linalg.solve(np.eye(n) - gamma * P, r)
    ctx = _hip.Context()
    dev = ctx.torch_device
    ell_cols = np.ascontiguousarray(cols.T, dtype=np.int32)
    ell_w = np.ascontiguousarray(w.T)
    d_cols, d_w, d_r = (torch.from_numpy(a).to(dev) for a in (ell_cols, ell_w, r))
    for method in (_hip.SOLVE_GMRES, _hip.SOLVE_JACOBI):
        v = torch.zeros(n, dtype=torch.float64, device=dev)
        out = ctx.value_solve(n, k, d_cols, d_w, d_r, gamma, v, 1e-10, 20000, m, method)
        assert "k_value_matvec" in ctx.last_kernel()
        error = np.abs(v.cpu().numpy() - exact).max()
        print("test_value_solve_wide_rows[%d] method %d: error %.3g, bound %.3g, %s" % (k, method, error,
                                                                                         out["bound"], out))
        assert out["converged"], out
        assert out["kappa"] <= gamma * (1 + 1e-12)
        assert error <= out["bound"] + 1e-12
    # two Jacobi steps, out of matvecs: the first step's iterate r + gamma P v, and its residual
    start = rng.normal(size=n)
    v = torch.from_numpy(start.copy()).to(dev)
    out = ctx.value_solve(n, k, d_cols, d_w, d_r, gamma, v, 0.0, 2, 2, _hip.SOLVE_JACOBI)
    assert out["matvecs"] == 2 and not out["converged"]
    first = _combine(ell_cols, ell_w, r, gamma, start)
    assert_array_equal(v.cpu().numpy(), first)
    assert out["residual_inf"] == np.abs(_combine(ell_cols, ell_w, r, gamma, first) - first).max()
    assert_allclose(first, r + gamma * P.dot(start), rtol=1e-12, atol=1e-13)
