"""Exact policy evaluation on the C5-policy shape: cost of the rows, GMRES vs Jacobi vs
value_iteration() to the same residual.

    python tools/policy_eval_probe.py [--num-points 64] [--n-gp 1024] [--tol 1e-10] [--out FILE]

The policy is the greedy table of three max sweeps from V = 0 (bench.py's C5-policy setup).
k_policy_operator_rows is timed with HIP events; each solve starts from the same table.  One JSON
line per run is appended to --out (default profiles/policy_eval_c5.jsonl)."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-points", type=int, default=64)
    ap.add_argument("--n-gp", type=int, default=1024)
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--restarts", default="8,16,32")
    ap.add_argument("--max-sweeps", type=int, default=4000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_eval_c5.jsonl"))
    args = ap.parse_args()
    import scipy.linalg
    import torch
    import safe_learning_amd as sl
    from safe_learning_amd.benchmarks import build_specs, headline_case
    case = headline_case(num_points=args.num_points, n_gp=args.n_gp)
    policy, dynamics, _, _ = build_specs(case)
    grid = sl.GridWorld(case["limits"], case["num_points"])
    vf = sl.Triangulation(grid, np.zeros((grid.nindex, 1)), project=True)
    d = case["d"]
    reward = sl.QuadraticFunction(-scipy.linalg.block_diag(0.1 * np.eye(d), 0.1 * np.eye(1)))
    rl = sl.PolicyIteration(policy, dynamics, reward, vf, gamma=0.98)
    actions = np.linspace(-1, 1, 9)[:, None]
    for _ in range(3):
        rl.value_iteration(actions)
    rl.discrete_policy_optimization(actions)
    start = vf._device(rl._ctx).clone()
    out = dict(shape="%d^%d" % (args.num_points, d), n_gp=args.n_gp, vertices=int(grid.nindex),
               tol=args.tol, gamma=rl.gamma, device=torch.cuda.get_device_name())

    # the rows: first call (allocation, network-free table policy upload) then timed calls
    rl.evaluate_policy(tol=args.tol, restart=16)
    r_inf = float(rl._rows[2].abs().max())
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(5):
        ev0.record()
        rl._ctx.policy_operator(0, grid.nindex, *rl._rows)
        ev1.record()
        torch.cuda.synchronize()
        times.append(ev0.elapsed_time(ev1))
    out["rows_ms"] = sorted(times)
    out["negative_rows"] = rl.last_solve["negative_rows"]
    out["kappa"] = rl.last_solve["kappa"]

    solves = []
    for method, restart in [("jacobi", 16)] + [("gmres", int(m)) for m in args.restarts.split(",")]:
        for rep in range(2):
            vf._adopt_device_table(start.clone())
            torch.cuda.synchronize()
            rl.evaluate_policy(tol=args.tol, restart=restart, method=method)
            s = dict(rl.last_solve)
            s.update(restart=restart, rep=rep)
            solves.append(s)
            print(json.dumps(s), flush=True)
        if method == "gmres" and restart == 16:
            solved16 = vf._host_parameters().copy()
    out["solves"] = solves

    # value_iteration() from the same start to the same residual (its residual is that of the
    # table it read, max |r + gamma P V - V|)
    vf._adopt_device_table(start.clone())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sweeps, res = 0, np.inf
    while sweeps < args.max_sweeps:
        res = rl.value_iteration()
        sweeps += 1
        if res <= args.tol * r_inf:
            break
    torch.cuda.synchronize()
    out["value_iteration"] = dict(sweeps=sweeps, ms=(time.perf_counter() - t0) * 1e3, residual=res,
                                  converged=bool(res <= args.tol * r_inf),
                                  max_diff_to_gmres16=float(np.abs(vf._host_parameters() - solved16).max()))
    print(json.dumps(out["value_iteration"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as handle:
        handle.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
