"""compute_roa of a GP's posterior mean: the fused kernel (csrc/sl_gp_rollout.hip, k_gp_rollout) against the
callable form ``lambda x: dynamics(x, policy(x))[0]``, which steps the policy and a full posterior call through the
point evaluations.

    python tools/gp_rollout_probe.py [--repeats 3] [--quick] [--out profiles/gp_rollout_gpu.md]

Per shape, in ONE process, after a warm-up of both paths, alternating, device-synchronised wall clock:

* fused     ``compute_roa(grid points, (dynamics.to_mean_function(), policy), horizon, tol)``;
* callable  ``compute_roa(grid points, lambda x: dynamics(x, policy(x))[0], horizon, tol)`` with the specs on device
            tensors through ``_evaluate.py``: per step a policy launch and ``sl_eval_points``' posterior (the
            triangular product for a variance the step throws away).

Both start from the grid points as the kernel generates them.  The masks are compared (the two means are different
sums: cells whose end distance lies within rounding of tol may differ, their number is reported) and the end states
must agree to 1e-6 before a time counts.  The rate is (trajectories x steps x training points) per second of the
fused path - the unit of sl_gp_rollout_chunk's budget (csrc/sl_gp_rollout.h) - and the resources of the
instantiations that ran are read from the library (tools/kernel_resources.py).  ``--quick``: small shapes (a
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
sys.path.insert(0, os.path.join(ROOT, "tools"))


def shapes(quick):
    """name, case, horizon, tol"""
    from safe_learning_amd.benchmarks import GP_VARIANTS, make_case, table_case
    if quick:
        return [("pendulum 201x151, table policy, 128 points", table_case(num_points=(201, 151), n_gp=128), 20, 0.2),
                ("cart-pole 12^4, 256 points", make_case("cartpole", num_points=12, n_gp=256, tau_scale=0.0,
                                                         **GP_VARIANTS["informed"]), 5, 1.0)]
    return [("pendulum 2001x1501, table policy, 128 points (the notebooks' shape)", table_case(n_gp=128), 100, 0.2),
            ("cart-pole 64^4, 1024 points", make_case("cartpole", num_points=64, n_gp=1024, tau_scale=0.0,
                                                      **GP_VARIANTS["informed"]), 8, 1.0)]


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gp_rollout_gpu.md"))
    args = ap.parse_args()
    import torch
    import kernel_resources
    import safe_learning_amd as sl
    from safe_learning_amd import _evaluate, _hip, utilities
    from safe_learning_amd.benchmarks import build_specs
    from safe_learning_amd.functions import _gp_heads

    resources = kernel_resources.resources(_hip.LIB_PATH)
    rows, raw = [], []
    for name, case, horizon, tol in shapes(args.quick):
        policy, dynamics, _, _ = build_specs(case)
        mean = dynamics.to_mean_function()
        grid = sl.GridWorld(case["limits"], case["num_points"])
        n, steps = int(grid.nindex), horizon - 1
        points = sum(len(gp.X) for gp, _, _ in _gp_heads(dynamics)[0])
        ctx = _evaluate._ctx()
        start = utilities._rollout(mean, policy, grid, 0)[0].clone()      # the grid points as the kernel generates them

        def fused():
            return utilities._rollout(mean, policy, start, steps)[0]

        def closed_loop(x):
            return _evaluate.dynamics(dynamics, x, _evaluate.policy(policy, x))[0]

        def stepwise():
            x = start
            for _ in range(steps):
                x = closed_loop(x)
            return x.contiguous()                      # (the mean is a column slice of the posterior records)

        _, end_f = timed(fused, torch)                                    # warm-up of both, and the outputs
        kernel = ctx.last_kernel()
        _, end_s = timed(stepwise, torch)
        both = torch.isfinite(end_f).all(dim=1) & torch.isfinite(end_s).all(dim=1)
        worst = float((end_f - end_s)[both].abs().max())
        mask_f = utilities._membership(ctx, end_f, None, tol)
        mask_s = utilities._membership(ctx, end_s, None, tol)
        differ, share = int((mask_f != mask_s).sum()), float(mask_f.double().mean())
        del end_f, end_s, mask_f, mask_s
        t_f, t_s = [], []
        for _ in range(args.repeats):
            t_f.append(timed(fused, torch)[0])
            t_s.append(timed(stepwise, torch)[0])
        rate = n * steps * points / (float(np.median(t_f)) * 1e-3)
        general, d = re.search(r"general=(\d), d=(\d)", kernel).groups()
        mangled = "k_gp_rolloutILb%sELi%sELi1EEE" % (general, d)
        used = {k: v for k, v in resources.items() if mangled in k}
        entry = dict(shape=name, cells=n, steps=steps, training_points=points, fused_ms=t_f, callable_ms=t_s,
                     rate=rate, end_states_worst_difference=worst, mask_differences=differ, in_roa_share=share,
                     finite_in_both=int(both.sum()), kernel=kernel, resources=used, device=torch.cuda.get_device_name())
        raw.append(entry)
        print(json.dumps(entry), flush=True)
        rows.append("| %s | %d | %d | %d | %.1f - %.1f | %.1f - %.1f | %.3f | %.3f | %.2f | %.3g | %d | %.3g |"
                    % (name, n, steps, points, min(t_f), max(t_f), min(t_s), max(t_s), float(np.median(t_f)) / steps,
                       float(np.median(t_s)) / steps, min(t_s) / max(t_f), rate, differ, worst))
        del start
        torch.cuda.empty_cache()
    text = ["# compute_roa of a GP mean: fused kernel vs the callable form", "",
            "`python tools/gp_rollout_probe.py%s` on %s, %d repeats after a warm-up, the two alternating in one process,"
            % (" --quick" if args.quick else "", raw[0]["device"], args.repeats),
            "wall clock around a device synchronisation (ms, smallest - largest of the repeats); per step: the median.",
            "`callable / fused` = fastest callable over slowest fused.  rate = trajectories x steps x training points per",
            "second of the fused path.", "",
            "| shape | cells | steps | training points | fused ms | callable ms | fused ms per step | callable ms per step | "
            "callable / fused | rate | mask differences | worst end-state difference |",
            "|---|---|---|---|---|---|---|---|---|---|---|---|"] + rows + ["", "Kernels and their resources:", ""]
    for e in raw:
        text.append("* %s: `%s`; %s" % (e["shape"], e["kernel"], json.dumps(e["resources"])))
    text += ["", "Raw repeats:", "", "```"] + [json.dumps(e) for e in raw] + ["```", ""]
    with open(args.out, "w") as f:
        f.write("\n".join(text))
    print("wrote", args.out)
    bad = [e["shape"] for e in raw if not e["end_states_worst_difference"] <= 1e-6]
    if bad:
        raise SystemExit("end states disagree: %s" % bad)


if __name__ == "__main__":
    main()
