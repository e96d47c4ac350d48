"""CPU checks of exact policy evaluation (safe_learning_amd/csrc/sl_policy_rows.h, DESIGN.md
"Exact policy evaluation").

The row header is compiled with g++ into a test-only shim (tests/hostsim/policy_rows.cpp) and
compared with the oracle's barycentric weights (Triangulation._get_weights, the matrix of the
reference's LP) and with the sweep's value lookup.  A NumPy model of the safeguarded GMRES(m) that
sl_value_solve runs is checked on the reference's 4-state known answer and on random operators.
"""

import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import hostsim_build
import oracle
from conftest import ROOT
from safe_learning_amd import functions as F


@functools.lru_cache(maxsize=None)
def load_shim():
    """The shim, compiled once per process (also used by tests/test_gpu_policy_evaluation.py and
    tests/test_gpu_bellman_matrix.py)."""
    return hostsim_build.shared("policy_rows.cpp", None, hostsim_build.SHIM_FLAGS)


@pytest.fixture(scope="module")
def shim():
    return load_shim()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class _Rows(object):
    """The shim with one value triangulation set (the arrays stay alive with this object)."""

    def __init__(self, shim, tri):
        grid = tri.discretization
        self.shim, self.d, self.n = shim, grid.ndim, grid.nindex
        self.desc = grid._desc()
        self.simp = np.ascontiguousarray(tri.unit_simplex_codes, dtype=np.int32)
        self.hyper = np.ascontiguousarray(tri.hyperplanes)
        self.dp = np.ascontiguousarray(np.concatenate(grid.discrete_points))
        self.table = np.ascontiguousarray(tri.parameters[:, 0])
        assert shim.pr_set_tri(C.byref(self.desc), len(self.simp), _p(self.simp), _p(self.hyper),
                               _p(self.dp), int(tri.project), _p(self.table)) == 0

    def rows(self, pts, negate=False):
        pts = np.ascontiguousarray(pts, dtype=np.float64)
        npts, k = len(pts), self.d + 1
        cols = np.zeros((k, npts), dtype=np.int32)
        w = np.zeros((k, npts))
        neg = np.zeros(npts, dtype=np.uint8)
        abs_sum = np.zeros(npts)
        assert self.shim.pr_rows(C.c_int64(npts), _p(pts), int(negate), _p(cols), _p(w), _p(neg),
                                 _p(abs_sum)) == 0
        return cols, w, neg.astype(bool), abs_sum

    def values(self, pts):
        pts = np.ascontiguousarray(pts, dtype=np.float64)
        out = np.zeros(len(pts))
        assert self.shim.pr_values(C.c_int64(len(pts)), _p(pts), _p(out)) == 0
        return out

    def combine(self, cols, w, r, gamma, v):
        k, n = cols.shape
        out = np.zeros(n)
        v = np.ascontiguousarray(v, dtype=np.float64)
        r = np.ascontiguousarray(r, dtype=np.float64)
        assert self.shim.pr_combine(C.c_int64(n), k, _p(np.ascontiguousarray(cols)),
                                    _p(np.ascontiguousarray(w)), _p(r), C.c_double(gamma), _p(v),
                                    _p(out)) == 0
        return out


def _dense(cols, w, n):
    """Rows as a dense [npts, n] matrix (entries of a repeated column add up)."""
    k, npts = cols.shape
    P = np.zeros((npts, n))
    for q in range(k):
        np.add.at(P, (np.arange(npts), cols[q]), w[q])
    return P


def _points(limits, rng, count):
    """Interior points, points on the upper limits and on the grid vertices, points outside."""
    lo, hi = limits[:, 0], limits[:, 1]
    d = len(lo)
    inside = lo + (hi - lo) * rng.random((count, d))
    upper = inside.copy()
    axis = rng.integers(0, d, count)
    upper[np.arange(count), axis] = hi[axis]
    corner = np.tile(hi, (3, 1))
    outside = lo - 0.3 * (hi - lo) + 1.6 * (hi - lo) * rng.random((count, d))
    return np.vstack([inside, upper, corner, outside])


GRIDS = [([[-1, 1]], [7]), ([[-1, 1], [-0.5, 2]], [5, 6]), ([[0, 1]] * 3, [4, 3, 5]),
         ([[-1, 1]] * 4, [4, 5, 3, 4])]


@pytest.mark.parametrize("limits,num", GRIDS, ids=["1d", "2d", "3d", "4d"])
@pytest.mark.parametrize("project", [True, False])
def test_rows_match_oracle_weights(shim, limits, num, project):
    rng = np.random.default_rng(3)
    grid = F.GridWorld(limits, num)
    values = rng.normal(size=(grid.nindex, 1))
    tri = F.Triangulation(grid, values, project=project)
    otri = oracle.Triangulation(oracle.GridWorld(limits, num), values, project=project)
    pts = _points(np.asarray(limits, dtype=np.float64), rng, 40)
    rows = _Rows(shim, tri)
    cols, w, neg, abs_sum = rows.rows(pts)
    ow, osimp = otri._get_weights(pts)
    # the same operator row: the oracle's unfused weights and the sweep's fused ones differ by
    # rounding only; a point on a shared face may pick another simplex with zero weight there.
    # Outside the grid without projection the clipped point can lie on a face shared by two
    # simplices whose extrapolations differ (the sweep picks by the largest smallest weight, the
    # oracle by its Delaunay walk): those rows are checked for reproducing the point instead.
    same = np.ones(len(pts), dtype=bool) if project else np.arange(len(pts)) < len(pts) - 40
    dense = _dense(cols, w, grid.nindex)
    assert_allclose(dense[same], _dense(osimp.T.astype(np.int32), ow.T, grid.nindex)[same],
                    rtol=0, atol=1e-13)
    assert_allclose(dense @ grid.all_points, np.clip(pts, grid.limits[:, 0], grid.limits[:, 1])
                    if project else pts, rtol=0, atol=1e-12)
    assert_allclose(w.sum(axis=0), 1.0, rtol=0, atol=1e-13)
    interior = np.all(ow > 1e-9, axis=1)
    assert_array_equal(np.sort(cols.T[interior], axis=1), np.sort(osimp[interior], axis=1))
    assert_array_equal(neg, np.any(w < 0, axis=0))
    assert_array_equal(abs_sum, np.abs(w).sum(axis=0))
    if not project:
        assert neg[len(pts) - 40:].any()       # outside the grid without projection: extrapolation


@pytest.mark.parametrize("limits,num", GRIDS, ids=["1d", "2d", "3d", "4d"])
@pytest.mark.parametrize("project", [True, False])
def test_row_combine_is_the_sweep_value(shim, limits, num, project):
    """r + gamma * (P V) through the rows equals r + gamma * V(next) of the sweep's lookup bit for
    bit, and for a negated value function r + gamma * (-V(next))."""
    rng = np.random.default_rng(5)
    grid = F.GridWorld(limits, num)
    values = rng.normal(size=(grid.nindex, 1))
    tri = F.Triangulation(grid, values, project=project)
    rows = _Rows(shim, tri)
    pts = _points(np.asarray(limits, dtype=np.float64), rng, 60)
    r = rng.normal(size=len(pts))
    gamma = 0.98
    v_next = rows.values(pts)
    cols, w, _, _ = rows.rows(pts)
    got = rows.combine(cols, w, r, gamma, values[:, 0])
    assert_array_equal(got, r + gamma * v_next)
    cols, w, _, _ = rows.rows(pts, negate=True)
    got = rows.combine(cols, w, r, gamma, values[:, 0])
    assert_array_equal(got, r + gamma * (v_next * -1.0))


def test_combine_of_an_explicit_operator(shim):
    """k = 4 rows of the reference's 4-state operator (any ELL operator, not only a grid's)."""
    tri = F.Triangulation(F.GridWorld([[0, 1]], 4), np.zeros((4, 1)))
    rows = _Rows(shim, tri)
    P, r, gamma = _known_answer()
    cols = np.tile(np.arange(4, dtype=np.int32)[:, None], (1, 4))
    w = np.ascontiguousarray(P.T)
    v = np.array([0.5, -1.0, 2.0, 3.0])
    expected = np.empty(4)
    for i in range(4):                            # corners 1..3 fused in turn, corner 0 last
        acc = 0.0
        for q in (1, 2, 3):
            acc = _fma(w[q, i], v[q], acc)
        acc = _fma(w[0, i], v[0], acc)
        expected[i] = r[i] + gamma * acc
    assert_array_equal(rows.combine(cols, w, r, gamma, v), expected)


def _fma(a, b, c):
    from fractions import Fraction
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _known_answer():
    with open(os.path.join(ROOT, "tests", "golden", "reference_policy_evaluation.json")) as f:
        case = json.load(f)
    return np.array(case["transition"]), np.array(case["reward"]), case["gamma"]


# ---- NumPy model of sl_value_solve ------------------------------------------------
def solve_model(P, r, gamma, v0, tol, m, max_matvecs, method="gmres", spoil=None):
    """Safeguarded restarted GMRES(m) / Jacobi as sl_value_solve runs it.  ``spoil(cycle, x_new)``
    may replace a GMRES cycle's iterate (to construct a bad cycle)."""
    n = len(r)
    kappa = gamma * np.abs(P).sum(axis=1).max()
    r_inf = np.abs(r).max()
    if r_inf == 0:
        return np.zeros(n), dict(converged=True, matvecs=0, jacobi_cycles=0, cycles=0, residual=0.0)
    tol_abs = tol * r_inf
    A = np.eye(n) - gamma * P
    resid = lambda x: r + gamma * (P @ x) - x            # noqa: E731
    stats = dict(matvecs=0, jacobi_cycles=0, cycles=0)
    x = np.array(v0, dtype=np.float64)

    def jacobi(x, steps):
        for _ in range(steps):
            x = r + gamma * (P @ x)
        return x

    if method == "jacobi":
        res = np.inf
        while stats["matvecs"] < max_matvecs:
            steps = min(m, max_matvecs - stats["matvecs"])
            before = jacobi(x, steps - 1)
            res = np.abs(resid(before)).max()
            after = r + gamma * (P @ before)
            stats["matvecs"] += steps
            stats["cycles"] += 1
            if res <= tol_abs or not np.isfinite(res) or stats["matvecs"] >= max_matvecs:
                x = before                               # its residual is known exactly
                break
            x = after
        stats.update(converged=res <= tol_abs, residual=res)
        return x, stats

    r0 = resid(x)
    res = np.abs(r0).max()
    stats["matvecs"] = 1
    while res > tol_abs and stats["matvecs"] < max_matvecs:
        steps = min(max_matvecs - stats["matvecs"] - 1, m)
        if steps < 1:
            break
        beta = np.sqrt(np.sum(r0 * r0))
        V = [r0 / beta]
        H = np.zeros((m + 1, m))
        cs, sn = np.zeros(m), np.zeros(m)
        g = np.zeros(m + 1)
        g[0] = beta
        done = 0
        for j in range(steps):
            w = A @ V[j]
            for _ in range(2):                           # classical Gram-Schmidt, twice
                h = np.array([np.dot(V[i], w) for i in range(j + 1)])
                H[:j + 1, j] += h
                w = w - np.array(V).T @ h
            hn = np.sqrt(np.sum(w * w))
            for i in range(j):
                h0, h1 = H[i, j], H[i + 1, j]
                H[i, j], H[i + 1, j] = cs[i] * h0 + sn[i] * h1, -sn[i] * h0 + cs[i] * h1
            rr = np.hypot(H[j, j], hn)
            cs[j], sn[j] = (H[j, j] / rr, hn / rr) if rr > 0 else (1.0, 0.0)
            H[j, j] = rr
            g[j], g[j + 1] = cs[j] * g[j], -sn[j] * g[j]
            done = j + 1
            if not hn > 1e-300 or abs(g[j + 1]) <= tol_abs:
                break
            V.append(w / hn)
        y = np.linalg.solve(np.triu(H[:done, :done]), g[:done])
        x_new = x + np.array(V[:done]).T @ y
        stats["cycles"] += 1
        if spoil is not None:
            x_new = spoil(stats["cycles"], x_new)
        stats["matvecs"] += done + 1
        r_new = resid(x_new)
        res_new = np.abs(r_new).max()
        if kappa >= 1 or res_new <= kappa ** done * res or res_new <= tol_abs:
            x, r0, res = x_new, r_new, res_new
            continue
        start = x_new if res_new < res else x           # the better of the two iterates
        js = min(m, max_matvecs - stats["matvecs"] - 1)
        if js < 1:
            x, res = start, min(res, res_new)
            break
        x = jacobi(start, js)
        stats["jacobi_cycles"] += 1
        stats["matvecs"] += js + 1
        r0 = resid(x)
        res = np.abs(r0).max()
    stats.update(converged=res <= tol_abs, residual=res)
    return x, stats


def test_model_known_answer():
    P, r, gamma = _known_answer()
    expected = np.linalg.solve(np.eye(4) - gamma * P, r)
    for method in ("gmres", "jacobi"):
        x, stats = solve_model(P, r, gamma, np.zeros(4), 1e-12, 4, 100000, method)
        assert stats["converged"]
        assert_allclose(x, expected, rtol=1e-10)
    _, gm = solve_model(P, r, gamma, np.zeros(4), 1e-12, 4, 100000, "gmres")
    assert gm["matvecs"] <= 12                          # 4 unknowns: one cycle is exact


@pytest.mark.parametrize("seed", range(4))
def test_model_random_convex_operators(seed):
    rng = np.random.default_rng(seed)
    n, k = 200, 3
    cols = rng.integers(0, n, size=(n, k))
    w = rng.random((n, k))
    w /= w.sum(axis=1, keepdims=True)
    P = np.zeros((n, n))
    np.add.at(P, (np.repeat(np.arange(n), k), cols.ravel()), w.ravel())
    r = rng.normal(size=n)
    gamma = 0.98
    expected = np.linalg.solve(np.eye(n) - gamma * P, r)
    x, stats = solve_model(P, r, gamma, np.zeros(n), 1e-10, 16, 20000)
    assert stats["converged"]
    bound = stats["residual"] / (1 - gamma)
    assert np.abs(x - expected).max() <= bound * (1 + 1e-6) + 1e-12
    # the safeguard bounds the work by about twice Jacobi's
    _, jac = solve_model(P, r, gamma, np.zeros(n), 1e-10, 16, 20000, "jacobi")
    assert jac["converged"]
    assert stats["matvecs"] <= 2 * jac["matvecs"] + 34


def test_model_bad_cycle_falls_back_to_jacobi():
    rng = np.random.default_rng(9)
    n = 60
    P = rng.random((n, n)) * (rng.random((n, n)) < 0.05)
    P[np.arange(n), rng.integers(0, n, n)] += 1.0
    P /= P.sum(axis=1, keepdims=True)
    r = rng.normal(size=n)
    gamma = 0.95
    expected = np.linalg.solve(np.eye(n) - gamma * P, r)

    def spoil(cycle, x_new):
        # the first cycle's iterate made worse than its start
        return x_new + (100.0 * np.sin(np.arange(n)) if cycle == 1 else 0.0)

    x, stats = solve_model(P, r, gamma, np.zeros(n), 1e-10, 8, 20000, spoil=spoil)
    assert stats["jacobi_cycles"] >= 1
    assert stats["converged"]
    assert_allclose(x, expected, rtol=1e-7, atol=1e-8)
