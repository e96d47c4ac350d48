"""reward_rollout: the fused kernel (csrc/sl_rollout.hip, k_reward_rollout) against the stepwise
composition of the point evaluations, and against the plain rollout of the same number of steps.

    python tools/reward_rollout_probe.py [--repeats 3] [--quick] [--out profiles/reward_rollout.md]
                                         [--resources LOG]

Per shape, in ONE process, after a warm-up of all paths, alternating, device-synchronised wall clock:

* fused     ``reward_rollout(grid, (dynamics, policy), reward, discount, horizon, tol)`` - k_reward_rollout
            + k_reward_fold, one host read per launch;
* stepwise  the same call through the callable path: ``x <- dynamics(x, policy(x))`` and
            ``reward([x, policy(x)])`` with the specs on device tensors through ``_evaluate.py`` (the point
            evaluation kernels: four launches and model uploads per step, the state through memory, one
            maximum read back per step);
* rollout   ``compute_roa``'s k_rollout over the number of steps the fused path summed: the same
            closed loop without reward, reduction and chunking.

The step counts must agree and the sums must agree before a time counts: bit for bit where the model
is linear, to 1e-9 relative for the Euler shapes (the same device functions in both paths; the table
says which was checked).  ``--resources LOG``: a compiler log of ``-Rpass-analysis=kernel-resource-usage``
for sl_rollout.hip, whose k_reward_* lines are copied into the report.  ``--quick``: small shapes (a
functional check of the tool itself, numbers meaningless)."""

import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PENDULUM_REWARD = (np.diag([1.0, 2.0]), 1.2)
CARTPOLE_REWARD = (0.1 * np.eye(4), 0.1)
SHAPES = [  # name, family, make_case keywords, (Q, R), discount, horizon, tol
    ("pendulum 2001x1501", "pendulum", dict(num_points=[2001, 1501], dynamics="analytic"), PENDULUM_REWARD,
     0.98, 1000, 1e-2),
    ("cart-pole 64^4", "cartpole", dict(num_points=64, dynamics="analytic"), CARTPOLE_REWARD, 0.98, 500, 1e-2),
    ("cart-pole-linear 64^4", "cartpole", dict(num_points=64, dynamics="linear"), CARTPOLE_REWARD, 0.98, 500, 1e-2),
]
QUICK = [
    ("pendulum 201x151", "pendulum", dict(num_points=[201, 151], dynamics="analytic"), PENDULUM_REWARD,
     0.98, 100, 1e-2),
    ("cart-pole 12^4", "cartpole", dict(num_points=12, dynamics="analytic"), CARTPOLE_REWARD, 0.98, 40, 1e-2),
    ("cart-pole-linear 12^4", "cartpole", dict(num_points=12, dynamics="linear"), CARTPOLE_REWARD, 0.98, 40, 1e-2),
]


def timed(fn, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def resource_table(path):
    """The k_reward_* kernels of a -Rpass-analysis=kernel-resource-usage log as Markdown rows."""
    fields = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill",
              "VGPRs Spill", "LDS Size [bytes/block]")
    rows, current = [], None
    for line in open(path):
        m = re.search(r"remark: +Function Name: (\S+)", line)
        if m:
            current = {"name": m.group(1)} if "k_reward_" in m.group(1) else None
            if current:
                rows.append(current)
            continue
        m = re.search(r"remark: +([^:]+): (\d+)", line)
        if current is not None and m and m.group(1).strip() in fields:
            current[m.group(1).strip()] = int(m.group(2))
    out = ["| kernel (mangled) | " + " | ".join(fields) + " |", "|---|" + "---|" * len(fields)]
    for r in rows:
        out.append("| `%s` | " % r["name"] + " | ".join(str(r.get(f, "")) for f in fields) + " |")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reward_rollout.md"))
    ap.add_argument("--resources", default=None)
    args = ap.parse_args()
    import scipy.linalg
    import torch
    import safe_learning_amd as sl
    from safe_learning_amd import _evaluate, utilities
    from safe_learning_amd.benchmarks import build_specs, make_case

    rows, raw = [], []
    for name, family, kw, (q, r), discount, horizon, tol in (QUICK if args.quick else SHAPES):
        case = make_case(family, tau_scale=0.0, **kw)
        policy, dynamics, _, _ = build_specs(case)
        reward = sl.QuadraticFunction(scipy.linalg.block_diag(-q, -np.atleast_2d(r)))
        grid = sl.GridWorld(case["limits"], case["num_points"])
        n = int(grid.nindex)
        ctx = _evaluate._ctx()
        # the start states of the stepwise loop: the grid points as the kernel generates them
        start = utilities._rollout(dynamics, policy, grid, 0)[0].clone()

        def fused():
            return utilities.reward_rollout(start, (dynamics, policy), reward, discount, horizon=horizon, tol=tol,
                                            full_output=True)

        def step(x):
            return _evaluate.dynamics(dynamics, x, _evaluate.policy(policy, x))

        def reward_on_states(x):
            return _evaluate.value(reward, torch.cat([x, _evaluate.policy(policy, x)], dim=1))

        def stepwise():
            return utilities.reward_rollout(start, step, reward_on_states, discount, horizon=horizon, tol=tol,
                                            full_output=True)

        _, (sum_f, steps_f, conv_f) = timed(fused, torch)            # warm-up of the three, and the outputs
        fused_kernel = ctx.last_kernel()
        _, (sum_s, steps_s, conv_s) = timed(stepwise, torch)

        def plain():
            return utilities._rollout(dynamics, policy, start, steps_f)[0]

        timed(plain, torch)
        plain_kernel = ctx.last_kernel()
        bit_equal = bool(torch.equal(sum_f, sum_s))
        scale = torch.clamp(sum_s.abs(), min=1.0)
        worst = float(((sum_f - sum_s).abs() / scale).max())
        finite = bool(torch.isfinite(sum_f).all())
        lowest = float(sum_f.min())
        del sum_f, sum_s
        t_f, t_s, t_p = [], [], []
        for _ in range(args.repeats):
            t_f.append(timed(fused, torch)[0])
            t_s.append(timed(stepwise, torch)[0])
            t_p.append(timed(plain, torch)[0])
        launches = re.search(r"in (\d+) launches \((\d+) redone\)", fused_kernel)
        entry = dict(shape=name, cells=n, horizon=horizon, tol=tol, discount=discount, fused_ms=t_f, stepwise_ms=t_s,
                     rollout_ms=t_p, steps=steps_f, converged=conv_f, stepwise_steps=steps_s,
                     stepwise_converged=conv_s, sums_bit_equal=bit_equal, sums_worst_relative=worst,
                     sums_finite=finite, lowest_sum=lowest, launches=int(launches.group(1)) if launches else None,
                     redone=int(launches.group(2)) if launches else None, fused_kernel=fused_kernel,
                     rollout_kernel=plain_kernel, device=torch.cuda.get_device_name())
        raw.append(entry)
        print(json.dumps(entry), flush=True)
        faster = all(f < s for f, s in zip(t_f, t_s))
        rows.append("| %s | %d | %d | %d (%s) | %s / %s | %.1f - %.1f | %.1f - %.1f | %.2f | %s | %.1f - %.1f | %.2f | %s | %.2g |"
                    % (name, n, horizon, steps_f, "converged" if conv_f else "horizon", entry["launches"],
                       entry["redone"], min(t_f), max(t_f), min(t_s), max(t_s), min(t_s) / max(t_f),
                       "yes" if faster else "NO", min(t_p), max(t_p), float(np.median(t_f)) / float(np.median(t_p)),
                       "yes" if bit_equal else "no", worst))
        del start
        torch.cuda.empty_cache()
    text = ["# reward_rollout: fused kernel vs stepwise composition vs the plain rollout of the same steps", "",
            "`python tools/reward_rollout_probe.py%s` on %s, %d repeats after a warm-up, the three alternating in one"
            % (" --quick" if args.quick else "", raw[0]["device"], args.repeats),
            "process, wall clock around a device synchronisation (ms, smallest - largest of the repeats).",
            "`stepwise / fused` = fastest stepwise over slowest fused; `fused / rollout` = median fused time over the",
            "median time of `k_rollout` (compute_roa's kernel) for the steps the fused path summed: the price of reward,",
            "reduction, chunking and the launch that is run again.", "",
            "| shape | cells | horizon | steps summed | launches / redone | fused ms | stepwise ms | stepwise / fused | "
            "fused faster in every repeat | rollout ms | fused / rollout | sums bit-equal | worst relative difference |",
            "|---|---|---|---|---|---|---|---|---|---|---|---|---|"] + rows + ["", "Kernels:", ""]
    for e in raw:
        text.append("* %s: `%s`; rollout `%s`" % (e["shape"], e["fused_kernel"], e["rollout_kernel"]))
    if args.resources:
        text += ["", "Resources of the new kernels (`-Rpass-analysis=kernel-resource-usage`, gfx950):", ""]
        text += resource_table(args.resources)
    text += ["", "Raw repeats:", "", "```"] + [json.dumps(e) for e in raw] + ["```", ""]
    with open(args.out, "w") as f:
        f.write("\n".join(text))
    print("wrote", args.out)
    bad = [e["shape"] for e in raw
           if e["steps"] != e["stepwise_steps"] or e["converged"] != e["stepwise_converged"]
           or e["sums_worst_relative"] > 1e-9 or ("linear" in e["shape"] and not e["sums_bit_equal"])]
    if bad:
        raise SystemExit("outputs disagree: %s" % bad)
    slow = [e["shape"] for e in raw if not all(f < s for f, s in zip(e["fused_ms"], e["stepwise_ms"]))]
    if slow:
        raise SystemExit("the fused path was not faster than the stepwise one in every repeat: %s" % slow)


if __name__ == "__main__":
    main()
