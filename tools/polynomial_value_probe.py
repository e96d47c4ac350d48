"""A polynomial Lyapunov function beside the quadratic form and the interpolated table in the same updates
(profiles/polynomial_value.md).

    python tools/polynomial_value_probe.py [--repeats 5] [--quick] [--out FILE.jsonl]

Two workloads, each warmed up once, then ``--repeats`` device-synchronised wall-clock runs in one process:

* pendulum  the notebooks' 2001 x 1501 grid under ``InvertedPendulum(0.15, 0.5, 0.1, 0.01, ...)`` and the saturated
            LQR policy, tau = 0, with three candidates: the sixth-order SOS polynomial of
            ``lyapunov_function_learning.ipynb`` (``PolynomialFunction.from_gram``; Q and state_norm from
            tests/golden/reference_sos.npz), the LQR quadratic form, and the quadratic form's values on a 101^2
            ``Triangulation``;
* cartpole  64^4 cells under the Euler cart-pole: ``x^T P x + 0.5 (sum x_q^4 + x_0^2 x_1^2)`` beside ``x^T P x``.

Per candidate: ``update_values()`` (with ``values`` materialised on the device), ``update_safe_set()``, and the
sweep kernel alone (the library's own events around ``sl_lyap_sweep``).  One JSON line per (workload, candidate,
measurement) with every repeat; ``--quick``: small shapes, a functional check of the tool (numbers meaningless)."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def quartic_terms(P, c):
    """x^T P x + c (sum_q x_q^4 + x_0^2 x_1^2) as a term table."""
    d = len(P)
    unit = np.eye(d, dtype=int)
    terms = [(float(P[i, i]) if i == j else float(P[i, j] + P[j, i]), tuple(unit[i] + unit[j]))
             for i in range(d) for j in range(i, d)]
    terms += [(float(c), tuple(4 * unit[q])) for q in range(d)]
    return terms + [(float(c), tuple(2 * unit[0] + 2 * unit[1]))]


def pendulum_candidates(sl, table_points):
    data = np.load(os.path.join(ROOT, "tests", "golden", "reference_sos.npz"))
    state_norm = data["state_norm"]
    u_max = 9.81 * 0.15 * 0.5 * np.sin(np.deg2rad(60))
    dynamics = sl.InvertedPendulum(0.15, 0.5, 0.1, 0.01, [list(state_norm), [u_max]])
    a, b = dynamics.linearize()
    k, p_lqr = sl.utilities.dlqr(a, b, np.eye(2), np.eye(1))
    policy = sl.Saturation(sl.LinearSystem((-k,)), -1, 1)
    sos = sl.PolynomialFunction.from_gram(data["Q"], int(data["degree"]), 2, state_norm)
    quadratic = sl.QuadraticFunction(p_lqr)
    tgrid = sl.GridWorld([[-1, 1]] * 2, table_points)
    pts = tgrid.all_points
    table = sl.Triangulation(tgrid, np.einsum("ni,ij,nj->n", pts, p_lqr, pts)[:, None], project=True)
    candidates = [("sos", sos, sl.Norm1Function(sl.Gradient(sos))),
                  ("quadratic", quadratic, sl.Norm1Function(sl.LinearSystem((p_lqr + p_lqr.T,)))),
                  ("table", table, sl.Norm1Function(sl.Gradient(table)))]
    return dynamics, policy, candidates


def cartpole_candidates(sl, num_points):
    from safe_learning_amd.benchmarks import build_specs, make_case
    case = make_case("cartpole", num_points=num_points, dynamics="analytic", tau_scale=0.0)
    policy, dynamics, quadratic, _ = build_specs(case)
    P = np.asarray(case["P"])
    quartic = sl.PolynomialFunction(quartic_terms(P, 0.5), 4)
    candidates = [("quartic", quartic, sl.Norm1Function(sl.Gradient(quartic))),
                  ("quadratic", quadratic, sl.Norm1Function(sl.LinearSystem((P + P.T,))))]
    return case, dynamics, policy, candidates


def measure(sl, torch, workload, grid, dynamics, policy, candidates, initial, repeats, lf):
    lines = []
    for name, value, lv in candidates:
        lyap = sl.Lyapunov(grid, value, dynamics, lf, lv, 0.0, policy, initial_set=initial)

        def values():
            lyap.update_values()
            return float(lyap._d_values[0])                     # (a quadratic V is materialised here)

        def sweep():
            lyap.update_safe_set()
            return int(lyap.safe_count)
        for what, fn in (("update_values", values), ("update_safe_set", sweep)):
            timed(fn, torch)
            runs = [timed(fn, torch) for _ in range(repeats)]
            lines.append(dict(workload=workload, candidate=name, measurement=what, cells=grid.nindex, result=runs[0][1],
                              kernel=lyap._ctx.last_kernel(), ms=[round(r[0], 3) for r in runs]))
        # the sweep kernel alone (the library's own events around sl_lyap_sweep)
        lyap._ctx.timing_configure(repeats)
        for _ in range(repeats):
            lyap._upload_model()
            lyap._refresh_init_bits()
            lyap._ctx.lyap_sweep(lyap._lo, lyap._hi, lyap._d_init, lyap._d_values, lyap._d_neg, lyap._d_result)
        lines.append(dict(workload=workload, candidate=name, measurement="sl_lyap_sweep", cells=grid.nindex,
                          kernel=lyap._ctx.last_kernel(), ms=[round(v, 4) for v in lyap._ctx.timing_collect(0)]))
        del lyap
        torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import safe_learning_amd as sl
    pend_points, table_points, cart_points = ([201, 151], 21, 12) if args.quick else ([2001, 1501], 101, 64)
    lines = []
    dynamics, policy, candidates = pendulum_candidates(sl, table_points)
    grid = sl.GridWorld([[-1, 1]] * 2, pend_points)
    initial = np.linalg.norm(grid.all_points, axis=1) <= 0.1
    lines += measure(sl, torch, "pendulum", grid, dynamics, policy, candidates, initial, args.repeats, 0.5)
    case, dynamics, policy, candidates = cartpole_candidates(sl, cart_points)
    grid = sl.GridWorld(case["limits"], case["num_points"])
    initial = np.linalg.norm(grid.all_points, axis=1) <= 0.2
    lines += measure(sl, torch, "cartpole", grid, dynamics, policy, candidates, initial, args.repeats, case["lf"])
    for line in lines:
        print(json.dumps(line))
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
