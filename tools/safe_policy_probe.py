#!/usr/bin/env python
"""Time the safe policy update on the GPU (sl_decrease_gradient beside sl_action_gradient):

* one ``policy_improvement_step(..., lyapunov=lyap)`` at the shape of ``examples/inverted_pendulum.ipynb`` cell 17:
  1000 sampled states, a FunctionStack of two 130-point heads with the notebook's kernels (Linear + Matern32 x
  Linear), a ``[32, 32, 1]`` relu / relu / tanh ``NeuralNetwork`` policy, a Triangulation value function, the
  Lyapunov function its negation with ``L_v = |gradient|`` - wall clock per step beside the unpenalised step of
  tools/policy_training_probe.py on the same objects, and the device time of the ``sl_decrease_gradient`` call;
* one ``sl_decrease_gradient`` of 1000 states under ONE 1024-point RBF head (two outputs): device time of the call
  and the useful flops of its triangular products, ``(1 + m) n_points n^2`` (n^2 / 2 multiply-adds per column),
  against the FP64 matrix peak of the datasheet (78.6 TFLOP/s).

    python tools/safe_policy_probe.py [--repeat 20] [--out FILE]

One JSON line per measurement.  No thresholds: the figures are recorded in profiles/safe_policy_training.md.  The
call's three kernels are timed together (the library's sl_timing_* channels bracket the sweep entry points only).
Needs a GPU; there is no fallback.
"""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP64_MATRIX_PEAK = 78.6e12


def _timed(call):
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = call()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop), out


def _wall(call, repeat):
    import torch
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeat):
        start = time.perf_counter()
        call()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - start) * 1e3)
    return out


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
    lyapunov_function = -vf                                            # cell 14 of the notebook
    lyap = sl.Lyapunov(sl.GridWorld(case["limits"], 41), lyapunov_function, dynamics, case["lf"],
                       sl.AbsFunction(sl.Gradient(lyapunov_function)), case["tau"], policy)
    states = np.random.default_rng(0).uniform(-1, 1, (1000, 2))
    d_states = torch.from_numpy(states).cuda()
    plain = _wall(lambda: sl.policy_improvement_step(rl, d_states, 0.01), repeat)
    safe = _wall(lambda: sl.policy_improvement_step(rl, d_states, 0.01, lyapunov=lyap, lagrange_multiplier=1.0), repeat)
    lyap._upload_model()
    from safe_learning_amd import _evaluate
    d_actions = _evaluate.policy(policy, d_states)
    grad = torch.empty((1000, 1), dtype=torch.float64, device="cuda")
    c = torch.empty(1000, dtype=torch.float64, device="cuda")
    call_ms = [_timed(lambda: lyap._ctx.decrease_gradient(1000, d_states, d_actions, grad, c))[0] for _ in range(repeat)]
    return dict(what="safe notebook step", states=1000, gp_points=130, heads=2, network=[32, 32, 1], repeat=repeat,
                safe_step_wall_ms_median=float(np.median(safe)), safe_step_wall_ms_min=float(np.min(safe)),
                plain_step_wall_ms_median=float(np.median(plain)), plain_step_wall_ms_min=float(np.min(plain)),
                decrease_gradient_ms_median=float(np.median(call_ms)), decrease_gradient_ms_min=float(np.min(call_ms)))


def rbf_head(repeat, n_gp=1024, n_points=1000):
    import torch
    import safe_learning_amd as sl
    from safe_learning_amd.benchmarks import GP_VARIANTS, build_specs, make_case
    case = make_case("pendulum", n_gp=n_gp, **GP_VARIANTS["informed"])
    policy, dynamics, value, lv = build_specs(case)
    lyap = sl.Lyapunov(sl.GridWorld(case["limits"], 41), value, dynamics, case["lf"], lv, case["tau"], policy)
    rng = np.random.default_rng(1)
    d_states = torch.from_numpy(rng.uniform(-1, 1, (n_points, 2))).cuda()
    d_actions = torch.from_numpy(rng.uniform(-1, 1, (n_points, 1))).cuda()
    lyap._upload_model()
    grad = torch.empty((n_points, 1), dtype=torch.float64, device="cuda")
    c = torch.empty(n_points, dtype=torch.float64, device="cuda")
    for _ in range(3):
        lyap._ctx.decrease_gradient(n_points, d_states, d_actions, grad, c)
    call_ms = [_timed(lambda: lyap._ctx.decrease_gradient(n_points, d_states, d_actions, grad, c))[0]
               for _ in range(repeat)]
    flops = 2.0 * n_points * float(n_gp) ** 2                         # (1 + m) columns, n^2 flops each
    best = float(np.min(call_ms))
    return dict(what="one RBF head", states=n_points, gp_points=n_gp, repeat=repeat,
                decrease_gradient_ms_median=float(np.median(call_ms)), decrease_gradient_ms_min=best,
                triangular_product_flops=flops, tflops_of_the_whole_call=flops / (best * 1e-3) / 1e12,
                share_of_fp64_matrix_peak=flops / (best * 1e-3) / FP64_MATRIX_PEAK)


def main():
    import torch
    parser = argparse.ArgumentParser()
    parser.add_argument("--repeat", type=int, default=20)
    parser.add_argument("--out", default=None)
    parser.add_argument("--only", choices=["notebook", "rbf"], default=None,
                        help="one of the two measurements (a kernel trace of one shape)")
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("safe_policy_probe needs a GPU")
    lines = []
    for name, measure in (("notebook", notebook_step), ("rbf", rbf_head)):
        if args.only not in (None, name):
            continue
        lines.append(measure(args.repeat))
        print(json.dumps(lines[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as handle:
            for line in lines:
                handle.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
