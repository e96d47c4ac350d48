"""Polynomial dynamics against the pendulum in the same kernels (profiles/polynomial_dynamics.md).

    python tools/polynomial_probe.py [--system vdp|pendulum|both] [--repeats 5] [--quick] [--out FILE.jsonl]

Two workloads, each warmed up once, then ``--repeats`` device-synchronised wall-clock runs in one process:

* sweep    ``Lyapunov.update_safe_set()`` on 2048 x 2048 cells (quadratic V, scalar L_f / L_v, tau = 0):
           k_det_sweep of the kind, plus the level-set passes that are the same for both systems;
* rollout  ``compute_roa`` on 1001 x 1001 cells, horizon 300: k_rollout of the kind.

``--system pendulum`` runs under a library of another revision too (SL_LIB_PATH: the comparator at the parent
commit).  One JSON line per (system, workload) with every repeat; ``--quick``: small shapes, a functional
check of the tool (numbers meaningless)."""

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


def specs(sl, system):
    """-> (dynamics, policy, P of V = x^T P x)."""
    import scipy.linalg
    if system == "vdp":
        dynamics = sl.VanDerPol(1, dt=0.1, normalization=[3, 3])
        closed = dynamics.linearize()
        policy = sl.LinearSystem((np.zeros((1, 2)),))
    else:
        dynamics = sl.InvertedPendulum(0.15, 0.5, 0.1, 0.01, [[np.deg2rad(30), 4.0], [0.15 * 9.81 * 0.5 * 0.5]])
        a, b = dynamics.linearize()
        k, _ = sl.utilities.dlqr(a, b, np.diag([1.0, 2.0]), np.array([[1.2]]))
        policy = sl.Saturation(sl.LinearSystem((-k,)), -1.0, 1.0)
        closed = a - b.dot(k)
    return dynamics, policy, scipy.linalg.solve_discrete_lyapunov(closed.T, np.eye(2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--system", default="both", choices=["vdp", "pendulum", "both"])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import safe_learning_amd as sl
    from safe_learning_amd import _evaluate
    sweep_points, roa_points, horizon = (256, 101, 30) if args.quick else (2048, 1001, 300)
    lines = []
    for system in (["vdp", "pendulum"] if args.system == "both" else [args.system]):
        dynamics, policy, pmat = specs(sl, system)
        grid = sl.GridWorld([[-1, 1]] * 2, sweep_points)
        initial = np.zeros(grid.nindex, dtype=bool)
        initial[grid.state_to_index(np.zeros((1, 2)))] = True

        def sweep():
            lyap.update_safe_set()
            return int(lyap.safe_set.sum())
        lyap = sl.Lyapunov(grid, sl.QuadraticFunction(pmat), dynamics, 0.5, 0.8, 0.0, policy, initial_set=initial)
        timed(sweep, torch)
        runs = [timed(sweep, torch) for _ in range(args.repeats)]
        lines.append(dict(system=system, workload="update_safe_set", cells=grid.nindex, safe=runs[0][1],
                          kernel=lyap._ctx.last_kernel(), ms=[round(r[0], 3) for r in runs]))
        # the sweep kernel alone (the library's own events around sl_lyap_sweep)
        lyap._ctx.timing_configure(args.repeats)
        for _ in range(args.repeats):
            lyap._upload_model()
            lyap._refresh_init_bits()
            lyap._ctx.lyap_sweep(lyap._lo, lyap._hi, lyap._d_init, lyap._d_values, lyap._d_neg, lyap._d_result)
        kernel = lyap._ctx.last_kernel()
        lines.append(dict(system=system, workload="sl_lyap_sweep", cells=grid.nindex, kernel=kernel,
                          ms=[round(v, 4) for v in lyap._ctx.timing_collect(0)]))
        roa_grid = sl.GridWorld([[-1, 1]] * 2, roa_points)

        def roa():
            return int(sl.compute_roa(roa_grid, (dynamics, policy), horizon=horizon, tol=0.01).sum())
        timed(roa, torch)
        runs = [timed(roa, torch) for _ in range(args.repeats)]
        lines.append(dict(system=system, workload="compute_roa", cells=roa_grid.nindex, horizon=horizon,
                          inside=runs[0][1], kernel=_evaluate._ctx().last_kernel(), ms=[round(r[0], 3) for r in runs]))
    for line in lines:
        line["library"] = os.environ.get("SL_LIB_PATH") or "shipped"
        print(json.dumps(line))
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
