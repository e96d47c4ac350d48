#!/usr/bin/env python
"""Time one critic step and one actor step of ``ActorCritic`` on the GPU, split per engine call, beside PyTorch
float64 autograd on a torch restatement of the same model on the same device.

    python tools/actor_critic_probe.py [--sizes 100,1048576] [--repeat 20] [--out FILE]

The cart-pole of examples/reinforcement_learning_cartpole.ipynb (normalised, 10 Euler sub-steps), a [64, 64, 1]
relu policy and a bias-free [64, 64, 1] relu value network, at the notebook's batch (100) and at 2^20 samples.
Every size is warmed up, then timed ``repeat`` times with device events on the stream the calls go to (the
library's sl_timing_* channels belong to the sweeps); the events bracket the host's part of a call too (launches,
ctypes, the copy of the gradient to the host).  At batch 100 the calls that walk a network still take far longer
than that: one sample per lane is two wavefronts, each lane running its dot products one after another
(profiles/actor_critic.md); read the kernels' rates off the large size.  One JSON line per size.  Needs a GPU; there is no fallback.
"""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CARTPOLE = dict(pendulum_mass=0.175, cart_mass=1.732, length=0.28, rot_friction=0.001, dt=0.01)
NORMALIZATION = [[0.5, np.deg2rad(30), 2.0, 4 * np.sqrt(9.81 / 0.28)], [20.0]]
GAMMA = 0.98


def torch_cartpole(x, u):
    import torch
    p = CARTPOLE
    m, M, L, b, g = p["pendulum_mass"], p["cart_mass"], p["length"], p["rot_friction"], 9.81
    tx, tu = NORMALIZATION
    px, th, v, om = (x[:, k] * tx[k] for k in range(4))
    act = u[:, 0] * tu[0]
    dt = p["dt"] / 10
    for _ in range(10):
        s, c = torch.sin(th), torch.cos(th)
        det = L * (M + m * s * s)
        vd = (act - m * L * om * om * s - b * om * c + 0.5 * m * g * L * torch.sin(2 * th)) * L / det
        wd = (act * c - 0.5 * m * L * om * om * torch.sin(2 * th) - b * (m + M) * om / (m * L) + (m + M) * g * s) / det
        px, th, v, om = px + dt * v, th + dt * om, v + dt * vd, om + dt * wd
    return torch.stack([col / t for col, t in zip((px, th, v, om), tx)], dim=1)


def torch_net(params, x, biased, scale):
    import torch
    it = iter(params)
    for layer in range(3):
        x = x @ next(it)
        if biased and layer < 2:
            x = x + next(it)
        if layer < 2:
            x = torch.relu(x)
    return x * scale


def main():
    import torch
    import safe_learning_amd as sl
    from safe_learning_amd import _evaluate
    parser = argparse.ArgumentParser()
    parser.add_argument("--sizes", default="100,1048576")
    parser.add_argument("--repeat", type=int, default=20)
    parser.add_argument("--out", default=None)
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("actor_critic_probe needs a GPU")
    policy = sl.NeuralNetwork([64, 64, 1], ['relu', 'relu', None], output_scale=0.5, input_dim=4, seed=1)
    value = sl.NeuralNetwork([64, 64, 1], ['relu', 'relu', None], use_bias=False, input_dim=4, seed=2)
    reward = -np.diag([1.0, 1.0, 0.1, 0.1, 0.05])
    ac = sl.ActorCritic(policy, sl.CartPole(normalization=NORMALIZATION, **CARTPOLE), sl.QuadraticFunction(reward),
                        value, gamma=GAMMA)
    t_policy = [torch.from_numpy(p).cuda().requires_grad_(True) for p in policy.parameters]
    t_value = [torch.from_numpy(p).cuda().requires_grad_(True) for p in value.parameters]
    t_reward = torch.from_numpy(reward).cuda()

    def autograd(x, which):
        u = torch_net(t_policy, x, True, 0.5)
        z = torch.cat((x, u), dim=1)
        q = torch.einsum("ni,ij,nj->n", z, t_reward, z) + GAMMA * torch_net(t_value, torch_cartpole(x, u), False, 1.0)[:, 0]
        if which == "value":
            loss = (torch_net(t_value, x, False, 1.0)[:, 0] - q.detach()).abs().mean()
            return loss, torch.autograd.grad(loss, t_value)
        return q.mean(), torch.autograd.grad(q.mean(), t_policy)

    def timed(call):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        wall = time.perf_counter()
        start.record()
        out = call()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop), 1e3 * (time.perf_counter() - wall), out

    def median(call):
        runs = [timed(call)[:2] for _ in range(args.repeat)]
        return float(np.median([r[0] for r in runs])), float(np.median([r[1] for r in runs]))

    lines = []
    for n in [int(s) for s in args.sizes.split(",")]:
        x = torch.from_numpy(np.random.default_rng(n).uniform(-0.5, 0.5, (n, 4))).cuda()
        ctx = ac._ctx
        for _ in range(3):
            ac.value_gradient(x)
            ac.policy_gradient(x)
            autograd(x, "value")
            autograd(x, "policy")
        torch.cuda.synchronize()
        batch = ac._batch(x, None, None)
        dims, acts, has_bias = value._description()
        params = value._device_parameters(ctx)
        flat = torch.empty(params.numel(), dtype=torch.float64, device="cuda")
        coeff_u = batch["dq_du"] * (1.0 / n)
        line = dict(samples=n, repeat=args.repeat)
        for key, call in (
                ("value_step", lambda: ac.value_gradient(x)), ("policy_step", lambda: ac.policy_gradient(x)),
                ("policy_actions", lambda: _evaluate.policy(policy, x)),
                ("critic_batch", lambda: ac._batch(x, None, batch["actions"])),
                ("dense_param_grad", lambda: ctx.dense_param_grad(dims, acts, has_bias, 1.0, params, n, 4, x,
                                                                  batch["coeff"], flat)),
                ("policy_param_grad", lambda: policy.parameter_gradient(x, coeff_u)),
                ("autograd_value_step", lambda: autograd(x, "value")),
                ("autograd_policy_step", lambda: autograd(x, "policy"))):
            line[key + "_event_ms"], line[key + "_wall_ms"] = median(call)
        # the two sides must agree before their times are compared
        (objective, grad), (loss, t_grad) = ac.value_gradient(x), autograd(x, "value")
        loss = loss.detach()
        worst = max(float(np.abs(g - t.detach().cpu().numpy()).max()) for g, t in zip(grad, t_grad))
        scale = max(float(np.abs(g).max()) for g in grad)
        assert abs(objective - float(loss)) <= 1e-10 * abs(float(loss)) and worst <= 1e-8 * scale, (worst, scale)
        (objective, grad), (mean_q, t_grad) = ac.policy_gradient(x), autograd(x, "policy")
        mean_q = mean_q.detach()
        worst_p = max(float(np.abs(g - t.detach().cpu().numpy()).max()) for g, t in zip(grad, t_grad))
        scale_p = max(float(np.abs(g).max()) for g in grad)
        assert abs(objective - float(mean_q)) <= 1e-10 * abs(float(mean_q)) and worst_p <= 1e-8 * scale_p, (worst_p, scale_p)
        line.update(value_gradient_difference=worst, value_gradient_scale=scale, policy_gradient_difference=worst_p,
                    policy_gradient_scale=scale_p)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as handle:
            for line in lines:
                handle.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
