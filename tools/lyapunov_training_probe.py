#!/usr/bin/env python
"""Time one training gradient of a LyapunovNetwork on the GPU: sl_nn_loss + sl_nn_param_grad against
PyTorch float64 autograd of the same network on the same device - the stepwise composition the fused
kernels replace.  Both sides are bracketed by device events on the stream they run on (the library's
sl_timing_* channels belong to the sweeps; a fourth one would touch sl_common.h, whose hash ties the
recorded counter measurements of other kernels to their sources).

    python tools/lyapunov_training_probe.py [--sizes 1000,63001,4194304] [--repeat 20] [--out FILE]

A [64, 64, 64] tanh network on d = 2 at the notebook's batch (1 000), its 251^2 grid (63 001) and the
C3 grid (2048^2).  The loss is the pre-training loss mean |V(x) - target|; every size is warmed up,
then timed `repeat` times; the median and the spread are printed, one JSON line per size.  The events
bracket the host's calls too: at 1 000 points both sides are launch-bound (four launches through ctypes
here, some forty small ones under autograd) and the figures say little about the kernels; read the
kernels' rate off the two large sizes.  Needs a GPU; there is no fallback.
"""

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def autograd_gradient(kernels_of, weights, x, target):
    """mean |V(x) - target| and its gradient by autograd; kernels_of(weights) -> layer kernels."""
    import torch
    h = x
    for K in kernels_of(weights):
        h = torch.tanh(h @ K.T)
    loss = ((h * h).sum(dim=1) - target).abs().mean()
    return loss, torch.autograd.grad(loss, weights)


def main():
    import torch
    import safe_learning_amd as sl
    from safe_learning_amd import _hip
    parser = argparse.ArgumentParser()
    parser.add_argument("--sizes", default="1000,63001,4194304")
    parser.add_argument("--repeat", type=int, default=20)
    parser.add_argument("--out", default=None)
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lyapunov_training_probe needs a GPU")
    dims, eps = [64, 64, 64], 1e-6
    net = sl.LyapunovNetwork(2, dims, ["tanh"] * 3, eps=eps, seed=0)
    net.weights = [0.6 * w for w in net.weights]
    ctx = net._on_engine()
    total = sum(k.size for k in net.kernels())
    t_weights = [torch.from_numpy(w).cuda().requires_grad_(True) for w in net.weights]

    def kernels_of(ws):
        out, it, in_dim = [], iter(ws), 2
        for rows in dims:
            W = next(it)
            K = W.T @ W + eps * torch.eye(in_dim, dtype=torch.float64, device="cuda")
            if rows > in_dim:
                K = torch.cat([K, next(it)], dim=0)
            out.append(K)
            in_dim = rows
        return out

    lines = []
    for m in [int(s) for s in args.sizes.split(",")]:
        rng = np.random.default_rng(m)
        x = torch.from_numpy(rng.uniform(-1, 1, (m, 2))).cuda()
        target = 0.1 * (x * x).sum(dim=1)
        losses = torch.empty(3, dtype=torch.float64, device="cuda")
        coeff = torch.empty(m, dtype=torch.float64, device="cuda")
        grad = torch.empty(total, dtype=torch.float64, device="cuda")

        def fused():
            ctx.nn_loss(_hip.NN_LOSS_ABS, m, 2, x, None, target, None, 0., 0., 0., losses, coeff)
            ctx.nn_param_grad(m, 2, x, coeff, grad)

        for _ in range(3):
            fused()
            autograd_gradient(kernels_of, t_weights, x, target)
        torch.cuda.synchronize()

        def timed(call):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            out = call()
            stop.record()
            stop.synchronize()
            return start.elapsed_time(stop), out

        fused_ms = np.array([timed(fused)[0] for _ in range(args.repeat)])
        loss_ms = np.array([timed(lambda: ctx.nn_loss(_hip.NN_LOSS_ABS, m, 2, x, None, target, None, 0., 0., 0.,
                                                      losses, coeff))[0] for _ in range(args.repeat)])
        grad_ms = np.array([timed(lambda: ctx.nn_param_grad(m, 2, x, coeff, grad))[0] for _ in range(args.repeat)])
        auto_ms = []
        for _ in range(args.repeat):
            elapsed, (loss, grads) = timed(lambda: autograd_gradient(kernels_of, t_weights, x, target))
            auto_ms.append(elapsed)
        auto_ms = np.array(auto_ms)
        # the two must agree before their times are compared
        ref = net._weights_gradient(grad.cpu().numpy())
        worst = max(float(np.abs(g.detach().cpu().numpy() - r).max()) for g, r in zip(grads, ref))
        scale = max(float(np.abs(r).max()) for r in ref)
        assert abs(float(loss) - float(losses[0])) <= 1e-10 * abs(float(loss)) and worst <= 1e-9 * scale, (worst, scale)
        line = dict(points=m, repeat=args.repeat,
                    fused_ms_median=float(np.median(fused_ms)), fused_ms_min=float(fused_ms.min()),
                    fused_ms_max=float(fused_ms.max()), loss_ms_median=float(np.median(loss_ms)),
                    param_grad_ms_median=float(np.median(grad_ms)),
                    autograd_ms_median=float(np.median(auto_ms)), autograd_ms_min=float(auto_ms.min()),
                    autograd_ms_max=float(auto_ms.max()), max_abs_difference=worst, gradient_scale=scale)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as handle:
            for line in lines:
                handle.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
