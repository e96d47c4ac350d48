"""First timings of one GP likelihood call (``sl_gp_likelihood``): value alone, and value plus gradient, at
n = 130 / 1024 / 4096 observations.

    python tools/gp_likelihood_probe.py [--out profiles/gp_likelihood_timings.md]

Prints a markdown section (and writes it to ``--out``).  Nothing is asserted on the numbers: they are kept to
compare later work against.  Host clock around calls that end in a device synchronise; one warm-up call, then three
timed ones, all listed."""

import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import safe_learning_amd as sl                                   # noqa: E402
from safe_learning_amd import _evaluate                          # noqa: E402

SIZES = (130, 1024, 4096)
RUNS = 3


def problem(n):
    """The notebook's kernel family on inputs [x, u]: Linear + Matern32 * Linear."""
    rng = np.random.default_rng(0)
    X = rng.uniform(-1, 1, (n, 2))
    Y = np.sin(2.0 * X[:, :1]) + 0.3 * X[:, 1:] + 0.05 * rng.standard_normal((n, 1))
    kern = (sl.Linear(2, variance=[0.04, 0.01], ARD=True)
            + sl.Matern32(1, variance=0.2, lengthscales=0.9, active_dims=[0]) * sl.Linear(1, variance=0.3, active_dims=[0]))
    return X, Y, kern._factors(2)


def timed(call):
    call()
    runs = []
    for _ in range(RUNS):
        start = time.perf_counter()
        call()
        runs.append(1e3 * (time.perf_counter() - start))
    return runs


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--out", default=None)
    args = parser.parse_args()
    import torch
    ctx = _evaluate._ctx()
    lines = ["## Timings of one call", "",
             "Written by `tools/gp_likelihood_probe.py`.  Device: %s.  `Linear + Matern32 * Linear` on inputs `[x, u]`, "
             "one output column, noise variance 1e-2; one warm-up call, then %d timed calls (host clock around a call "
             "that ends in a device synchronise; allocation and the host copies included), all listed, in ms."
             % (torch.cuda.get_device_name(ctx.device), RUNS), "",
             "| n | value alone (ms) | value and gradient (ms) | best, with gradient (ms) |", "|---|---|---|---|"]
    for n in SIZES:
        X, Y, factors = problem(n)
        value = timed(lambda: ctx.gp_likelihood(X, Y, factors, 1e-2, gradient=False))
        both = timed(lambda: ctx.gp_likelihood(X, Y, factors, 1e-2, gradient=True))
        lines.append("| %d | %s | %s | %.3f |" % (n, ", ".join("%.3f" % v for v in value),
                                                  ", ".join("%.3f" % v for v in both), min(both)))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as handle:
            handle.write(text)


if __name__ == "__main__":
    main()
