"""First measurement of GP sampling on the GPU (profiles/gp_sample.md).

    python tools/gp_sample_probe.py [--sizes 1024 4096 16384] [--repeats 3] [--quick] [--no-gpu] [--out FILE.md]

Per size N - a Matern32 GP (sigma = 0.3, l = 0.5, five observations) on N points of a 2-D lattice, 10 samples -
the four stages of ``sample_gp_function`` one by one: covariance (``sl_gp_posterior_cov``), factorization
(``sl_cholesky``), samples (``sl_tri_mult``), alphas (two ``sl_tri_solve``).  Each stage is warmed up once at its
shape, then timed ``--repeats`` times with a host clock around work that ends in a device synchronise; the file
states every repeat.  Then one sample function on 10^6 points (``sl_gp_sample_eval``), and
``scipy.linalg.cholesky`` of the same matrix on the CPUs the process is granted (OMP_NUM_THREADS).  FLOP/s of the
factorization: N^3 / 3 over its time - a whole-call rate, launches and the readback of the pivot word included,
not a kernel's share of peak.

The file also lists registers, LDS and scratch of every kernel of sl_gp_sample.hip, read from the library
(tools/kernel_resources.py; needs no GPU).  ``--no-gpu``: only that table, and the file says that nothing was
timed.  ``--quick``: small sizes, a functional check of the tool (numbers meaningless)."""

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def lattice(n):
    side = int(np.ceil(np.sqrt(n)))
    axis = np.linspace(-1, 1, side)
    mesh = np.meshgrid(axis, axis, indexing="ij")
    return np.stack([m.ravel() for m in mesh], axis=1)[:n].copy()


def resources_table():
    import kernel_resources
    table = kernel_resources.resources()
    rows = sorted((name, e) for name, e in table.items() if "k_gs_" in name)
    lines = ["| kernel | SGPRs | VGPRs | AGPRs | scratch (B/lane) | LDS (B/workgroup) |", "|---|---|---|---|---|---|"]
    for name, e in rows:
        lines.append("| `%s` | %d | %d | %d | %d | %d |" % (name, e["sgpr"], e["vgpr"], e["agpr"], e["scratch"], e["lds"]))
    if not rows or any(e["scratch"] for _, e in rows):
        raise SystemExit("the kernels of sl_gp_sample.hip are missing from the library or use scratch")
    return lines


def timed(fn, torch, repeats):
    fn()                                                   # warm-up at this shape
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def measure(n, number, repeats, eval_points):
    import scipy.linalg
    import torch
    import safe_learning_amd as sl
    from safe_learning_amd import _evaluate
    from safe_learning_amd.functions import SAMPLE_JITTER
    ctx = _evaluate._ctx()
    dev = ctx.torch_device
    rng = np.random.default_rng(0)
    X = rng.uniform(-1, 1, (5, 2))
    gp = sl.GPRCached(X, 0.2 * np.sin(2 * X[:, :1]), sl.Matern32(2, variance=0.3 ** 2, lengthscales=0.5),
                      likelihood_variance=1e-4)
    points = lattice(n)
    d_points = torch.from_numpy(points).to(dev)
    d_mean = torch.empty(n, dtype=torch.float64, device=dev)
    d_cov = torch.empty((n, n), dtype=torch.float64, device=dev)
    factors = gp.kern._factors(2)

    def covariance():
        ctx.gp_posterior_cov(gp.X, gp.cholesky_inverse, gp.alpha, factors, None, d_points, SAMPLE_JITTER, d_mean, d_cov)
    times = {"covariance": timed(covariance, torch, repeats)}
    cov_host = d_cov.cpu().numpy()
    d_chol = torch.empty_like(d_cov)

    def factorization():
        d_chol.copy_(d_cov)
        if ctx.cholesky(d_chol):
            raise SystemExit("the probe's covariance did not factor")
    copy_ms = timed(lambda: d_chol.copy_(d_cov), torch, repeats)
    times["factorization (with a device copy of the matrix: %.3g ms)" % min(copy_ms)] = timed(factorization, torch, repeats)
    d_normal = torch.from_numpy(rng.standard_normal((n, number))).to(dev)
    d_values = torch.empty_like(d_normal)
    times["samples"] = timed(lambda: ctx.tri_mult(d_chol, d_normal, d_mean, d_values), torch, repeats)
    d_alpha = torch.empty_like(d_values)

    def alphas():
        d_alpha.copy_(d_values)
        ctx.tri_solve(d_chol, d_alpha, False)
        ctx.tri_solve(d_chol, d_alpha, True)
    times["alphas"] = timed(alphas, torch, repeats)
    d_x = torch.from_numpy(rng.uniform(-1, 1, (eval_points, 2))).to(dev)
    d_out = torch.empty((eval_points, 1), dtype=torch.float64, device=dev)
    d_one = d_alpha[:, :1].contiguous()
    times["one sample function on %d points" % eval_points] = timed(
        lambda: ctx.gp_sample_eval(factors, None, d_points, d_one, d_x, d_out), torch, repeats)
    cpu = []
    for _ in range(max(1, min(repeats, 2))):
        t0 = time.perf_counter()
        scipy.linalg.cholesky(cov_host, lower=True)
        cpu.append((time.perf_counter() - t0) * 1e3)
    times["scipy.linalg.cholesky on the CPU (%s threads)" % os.environ.get("OMP_NUM_THREADS", "all")] = cpu
    chol = d_chol.cpu().numpy()
    resid = float(np.max(np.abs(chol.dot(chol.T) - cov_host)) / np.max(np.abs(cov_host))) if n <= 4096 else None
    return times, resid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[1024, 4096, 16384])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--no-gpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gp_sample.md"))
    args = ap.parse_args()
    lines = ["# GP sample paths on the GPU: a first measurement", "",
             "Written by `tools/gp_sample_probe.py`.  There is no time to meet here: these are the first numbers of "
             "`sample_gp_function`'s building blocks (`sl_gp_sample.hip`), kept to compare later work against.", ""]
    if args.no_gpu:
        lines += ["**No GPU run: nothing below was timed.**  Only the kernels' resources, which the library records.", ""]
    else:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("no GPU: the probe does not time anything on a CPU (use --no-gpu for the resource table)")
        sizes = [200, 500] if args.quick else args.sizes
        eval_points = 10000 if args.quick else 10 ** 6
        lines += ["Device: %s.  Matern32 GP (sigma 0.3, l 0.5, 5 observations) on N lattice points of [-1, 1]^2, 10 "
                  "samples; every stage warmed up once, then %d timed runs (host clock around work that ends in a "
                  "device synchronise), all listed, in ms." % (torch.cuda.get_device_name(0), args.repeats), ""]
        for n in sizes:
            times, resid = measure(n, 10, args.repeats, eval_points)
            lines += ["## N = %d" % n, "", "| stage | runs (ms) | best (ms) |", "|---|---|---|"]
            for stage, runs in times.items():
                lines.append("| %s | %s | %.3f |" % (stage, ", ".join("%.3f" % r for r in runs), min(runs)))
            best = min(v for k, v in times.items() if k.startswith("factorization"))
            best = min(best)
            lines += ["", "Factorization: N^3 / 3 = %.3g FLOP over the best call = %.3g GFLOP/s (a whole-call rate)."
                      % (n ** 3 / 3.0, n ** 3 / 3.0 / (best * 1e-3) / 1e9)]
            if resid is not None:
                lines.append("max |L L^T - C| / max |C| = %.3g." % resid)
            lines.append("")
            print("\n".join(lines[-(len(times) + 8):]))
    lines += ["## Kernel resources", "", "From the library's code objects (`tools/kernel_resources.py`); every kernel "
              "is free of scratch.", ""] + resources_table() + [""]
    with open(args.out, "w") as handle:
        handle.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
