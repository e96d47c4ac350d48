"""Closed-loop rollouts: the fused kernel (csrc/sl_rollout.hip) against the stepwise composition of
the point evaluations, and against the Lyapunov sweep of the same cells.

    python tools/rollout_probe.py [--repeats 3] [--quick] [--out profiles/rollout_roa.md]

Per shape, in ONE process, after a warm-up of both paths, alternating, device-synchronised wall clock:

* fused     ``compute_roa(grid, (dynamics, policy), horizon, tol)`` - k_rollout + k_rollout_mask;
* stepwise  ``x <- dynamics(x, policy(x))`` with the specs on device tensors through ``_evaluate.py``
            (two launches and a model upload per call, the state through memory between them), then
            the same membership test;
* sweep     one decrease-check sweep (``sl_lyap_sweep``) over the same cells: one dynamics step plus
            the check per cell - the project's own roof for this arithmetic; a rollout of H - 1 steps
            should take no more than (H - 1) x that.

The outputs must agree before a time counts: end states bit for bit for the linear shape, masks equal
for the Euler shapes (the table says which was checked).  Writes a Markdown table and the raw
repeats; ``--quick``: small shapes (a functional check of the tool itself, numbers meaningless)."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [  # name, family, make_case keywords, horizon, tol
    ("pendulum 2001x1501", "pendulum", dict(num_points=[2001, 1501], dynamics="analytic"), 500, 0.01),
    ("cart-pole 64^4", "cartpole", dict(num_points=64, dynamics="analytic"), 200, 0.1),
    ("cart-pole-linear 64^4", "cartpole", dict(num_points=64, dynamics="linear"), 200, 0.1),
]
QUICK = [
    ("pendulum 201x151", "pendulum", dict(num_points=[201, 151], dynamics="analytic"), 50, 0.01),
    ("cart-pole 12^4", "cartpole", dict(num_points=12, dynamics="analytic"), 20, 0.1),
    ("cart-pole-linear 12^4", "cartpole", dict(num_points=12, dynamics="linear"), 20, 0.1),
]


def timed(fn, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_roa.md"))
    args = ap.parse_args()
    import torch
    import safe_learning_amd as sl
    from safe_learning_amd import _evaluate, utilities
    from safe_learning_amd.benchmarks import build_lyapunov, build_specs, make_case

    rows, raw = [], []
    for name, family, kw, horizon, tol in (QUICK if args.quick else SHAPES):
        case = make_case(family, tau_scale=0.0, **kw)
        policy, dynamics, _, _ = build_specs(case)
        grid = sl.GridWorld(case["limits"], case["num_points"])
        n, steps = int(grid.nindex), horizon - 1
        ctx = _evaluate._ctx()

        def fused():
            end, _, _ = utilities._rollout(dynamics, policy, grid, steps)
            return end, utilities._membership(ctx, end, None, tol)

        start = torch.empty((n, grid.ndim), dtype=torch.float64, device=ctx.torch_device)

        def stepwise():
            x = start
            for _ in range(steps):
                x = _evaluate.dynamics(dynamics, x, _evaluate.policy(policy, x))
            x = x.contiguous()
            return x, utilities._membership(ctx, x, None, tol)

        # the start states of the stepwise loop: the grid points as the kernel generates them
        start.copy_(utilities._rollout(dynamics, policy, grid, 0)[0])
        lyap = build_lyapunov(case)

        def sweep():
            lyap._ctx.lyap_sweep(0, n, lyap._d_init, lyap._values_arg(), lyap._d_neg, lyap._d_result)

        lyap._upload_model()
        _, (end_f, roa_f) = timed(fused, torch)                    # warm-up of the three, and the outputs
        rollout_kernel = ctx.last_kernel()
        _, (end_s, roa_s) = timed(stepwise, torch)
        timed(sweep, torch)
        sweep_kernel = lyap._ctx.last_kernel()
        bit_equal = bool(torch.equal(end_f, end_s))
        masks_equal = bool(torch.equal(roa_f, roa_s))
        inside = float(roa_f.double().mean())
        finite = bool(torch.isfinite(end_f).all())
        del end_f, end_s, roa_s
        t_f, t_s, t_w = [], [], []
        for _ in range(args.repeats):
            t_f.append(timed(fused, torch)[0])
            t_s.append(timed(stepwise, torch)[0])
            t_w.append(min(timed(sweep, torch)[0] for _ in range(3)))
        entry = dict(shape=name, cells=n, horizon=horizon, tol=tol, fused_ms=t_f, stepwise_ms=t_s, sweep_ms=t_w,
                     end_states_bit_equal=bit_equal, masks_equal=masks_equal, in_roa=inside,
                     end_states_finite=finite, rollout_kernel=rollout_kernel, sweep_kernel=sweep_kernel,
                     device=torch.cuda.get_device_name())
        raw.append(entry)
        print(json.dumps(entry), flush=True)
        fmin, fmax, smin, smax, wmed = min(t_f), max(t_f), min(t_s), max(t_s), float(np.median(t_w))
        rows.append("| %s | %d | %d | %.1f - %.1f | %.1f - %.1f | %.2f | %.3f | %.1f | %.3f | %s | %s | %.3f |" % (
            name, n, horizon, fmin, fmax, smin, smax, smin / fmax, wmed, steps * wmed,
            float(np.median(t_f)) / (steps * wmed), "yes" if bit_equal else "no", "yes" if masks_equal else "no",
            inside))
        del lyap, start
        torch.cuda.empty_cache()
    text = ["# Closed-loop rollouts: fused kernel vs stepwise composition vs the sweep of the same cells", "",
            "`python tools/rollout_probe.py%s` on %s, %d repeats after a warm-up, the three alternating in one"
            % (" --quick" if args.quick else "", raw[0]["device"], args.repeats),
            "process, wall clock around a device synchronisation (ms, smallest - largest of the repeats).",
            "`stepwise / fused` = fastest stepwise over slowest fused; `sweep` = one decrease-check sweep over the same",
            "cells (median); `fused / (H-1) sweeps` = median fused time over (H - 1) x that.", "",
            "| shape | cells | H | fused ms | stepwise ms | stepwise / fused | sweep ms | (H-1) x sweep ms | "
            "fused / (H-1) sweeps | end states bit-equal | masks equal | in-ROA fraction |",
            "|---|---|---|---|---|---|---|---|---|---|---|---|"] + rows + ["", "Kernels:", ""]
    for e in raw:
        text.append("* %s: `%s`; sweep `%s`" % (e["shape"], e["rollout_kernel"], e["sweep_kernel"]))
    text += ["", "Raw repeats:", "", "```"] + [json.dumps(e) for e in raw] + ["```", ""]
    with open(args.out, "w") as f:
        f.write("\n".join(text))
    print("wrote", args.out)
    bad = [e["shape"] for e in raw if not e["masks_equal"] or ("linear" in e["shape"] and not e["end_states_bit_equal"])]
    if bad:
        raise SystemExit("outputs disagree: %s" % bad)


if __name__ == "__main__":
    main()
