#!/usr/bin/env python
"""Time the policy-gradient path on the GPU (sl_action_gradient, sl_policy_param_grad):

* one ``policy_improvement_step`` at the shape of ``examples/inverted_pendulum.ipynb`` cells 9/12: 1000
  sampled states, a FunctionStack of two 130-point heads with the notebook's kernels (Linear + Matern32 x
  Linear), a ``[32, 32, 1]`` relu / relu / tanh ``NeuralNetwork`` policy, a Triangulation value function -
  wall clock per step (the host's share included: upload of the stepped parameters, the gradient's copy
  back) and the device time of its two engine calls;
* one ``sl_action_gradient`` over every vertex of a 64^4 value grid with the 1024-point RBF GP of the
  cart-pole case, beside one uncached policy-evaluation sweep (``value_iteration()`` with the successor
  cache off) of the same model on the same box.

    python tools/policy_training_probe.py [--repeat 20] [--grid 64] [--skip-grid] [--out FILE]

One JSON line per measurement.  No thresholds: the figures are recorded in profiles/policy_training.md.
Needs a GPU; there is no fallback.
"""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(call):
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = call()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop), out


def notebook_step(repeat):
    import scipy.linalg
    import torch
    import safe_learning_amd as sl
    from safe_learning_amd.benchmarks import build_specs, make_case, notebook_kernels
    case = make_case("pendulum", n_gp=130, stack=True)
    case["dynamics"]["kernels"] = notebook_kernels(case)
    _, dynamics, _, _ = build_specs(case)
    grid = sl.GridWorld(case["limits"], 41)
    pts = grid.all_points
    values = -np.einsum("ij,jk,ik->i", pts, case["P"], pts)[:, None]
    vf = sl.Triangulation(grid, values, project=True)
    policy = sl.NeuralNetwork([32, 32, 1], ["relu", "relu", "tanh"], output_scale=1.0, input_dim=2, seed=0)
    reward = sl.QuadraticFunction(-scipy.linalg.block_diag(np.eye(2), 0.1 * np.eye(1)))
    rl = sl.PolicyIteration(policy, dynamics, reward, vf, gamma=0.98)
    states = np.random.default_rng(0).uniform(-1, 1, (1000, 2))
    d_states = torch.from_numpy(states).cuda()
    for _ in range(3):
        sl.policy_improvement_step(rl, d_states, 0.01)
    torch.cuda.synchronize()
    wall = []
    for _ in range(repeat):
        start = time.perf_counter()
        sl.policy_improvement_step(rl, d_states, 0.01)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - start) * 1e3)
    # the two engine calls alone, on the device
    rl._upload(rl.policy)
    grad = torch.empty((1000, 1), dtype=torch.float64, device="cuda")
    q = torch.empty(1000, dtype=torch.float64, device="cuda")
    action_ms = [_timed(lambda: rl._ctx.action_gradient(1000, d_states, None, grad, q))[0] for _ in range(repeat)]
    ctx = policy._on_engine()
    total = sum(p.size for p in policy.parameters)
    out = torch.empty(total, dtype=torch.float64, device="cuda")
    param_ms = [_timed(lambda: ctx.policy_param_grad(1000, 2, d_states, grad, out))[0] for _ in range(repeat)]
    return dict(what="notebook step", states=1000, gp_points=130, heads=2, network=[32, 32, 1], repeat=repeat,
                step_wall_ms_median=float(np.median(wall)), step_wall_ms_min=float(np.min(wall)),
                step_wall_ms_max=float(np.max(wall)), action_gradient_ms_median=float(np.median(action_ms)),
                policy_param_grad_ms_median=float(np.median(param_ms)))


def grid_gradient(num_points):
    import scipy.linalg
    import torch
    import safe_learning_amd as sl
    from safe_learning_amd.benchmarks import build_specs, make_case
    case = make_case("cartpole", num_points=num_points, n_gp=1024)
    policy, dynamics, _, _ = build_specs(case)
    grid = sl.GridWorld(case["limits"], num_points)
    n = grid.nindex
    values = -np.random.default_rng(4).random((n, 1))
    vf = sl.Triangulation(grid, values, project=True)
    reward = sl.QuadraticFunction(-scipy.linalg.block_diag(np.eye(4), 0.1 * np.eye(1)))
    rl = sl.PolicyIteration(policy, dynamics, reward, vf, gamma=0.95)
    rl.successor_cache(0)
    rl._upload(rl.policy)
    grad = torch.empty((n, 1), dtype=torch.float64, device="cuda")
    q = torch.empty(n, dtype=torch.float64, device="cuda")
    gradient_ms, _ = _timed(lambda: rl._ctx.action_gradient(n, None, None, grad, q))
    gradient_ms2, _ = _timed(lambda: rl._ctx.action_gradient(n, None, None, grad, q))
    fv = torch.from_numpy(rl.future_values()[:, 0]).cuda()
    worst = float(((q - fv).abs() / fv.abs().clamp_min(1e-300)).max())
    sweep_ms, _ = _timed(rl.value_iteration)
    kernel = rl._ctx.last_kernel()
    sweep_ms2, _ = _timed(rl.value_iteration)
    return dict(what="action gradient on the value grid", vertices=n, gp_points=1024,
                action_gradient_ms=[gradient_ms, gradient_ms2], uncached_policy_sweep_ms=[sweep_ms, sweep_ms2],
                sweep_kernel=kernel, q_vs_future_values_max_rel=worst)


def main():
    import torch
    parser = argparse.ArgumentParser()
    parser.add_argument("--repeat", type=int, default=20)
    parser.add_argument("--grid", type=int, default=64)
    parser.add_argument("--skip-grid", action="store_true")
    parser.add_argument("--out", default=None)
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("policy_training_probe needs a GPU")
    lines = [notebook_step(args.repeat)]
    print(json.dumps(lines[-1]), flush=True)
    if not args.skip_grid:
        lines.append(grid_gradient(args.grid))
        print(json.dumps(lines[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as handle:
            for line in lines:
                handle.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
