"""Host tests (no GPU) of the deciding pass in front of ``k_gp_mean_blocks`` (DESIGN.md 4.1 "Deciding
before the mean"): the constants ``sl_gp_set_head`` computes for it (``sl_gp_mean_bound.h``), the
inequality they rest on, and the decision rule itself (``sl_gp4_predecide.h``) - run by the
stand-alone program ``tests/hostsim/gp4_predecide_sim.cpp``, built with
``-fsanitize=address,undefined`` - against the oracle: no cell the rule decides may pass there,
and the decided blocks are the ones ``tools/early_block_counts.py --mean-lattice`` counts."""

import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg

import cases
import hostsim_build
from safe_learning_amd import functions as F
from safe_learning_amd._model import ModelBuilder
from safe_learning_amd.benchmarks import build_specs
from test_gpu_gp4_early import SLAB_HI, SLAB_LO, _informed, _slab_case

sys.path.insert(0, os.path.join(hostsim_build.ROOT, "tools"))

LD = np.longdouble
NORM_MARGIN, ROUND_TERMS, EPS_MULT = 1e-6, 8.0, 4096.0          # sl_gp_mean_bound.h


class _RecordingCtx(object):
    """Captures the model description and the GP upload instead of sending them to a device."""
    torch_device = None

    def model_set(self, desc):
        self.desc = desc

    def gp_set_head(self, head, X, Linv, alpha, col0, variance, lengthscales):
        assert head == 0 and col0 == 0
        self.head = (np.array(X, dtype=np.float64), np.array(Linv, dtype=np.float64), np.array(alpha, dtype=np.float64),
                     float(variance), np.array(lengthscales, dtype=np.float64))

    def gp_configure(self, nheads, beta):
        assert nheads == 1


def _describe(case):
    grid = F.GridWorld(case["limits"], case["num_points"])
    policy, dynamics, value, lv = build_specs(case)
    ctx = _RecordingCtx()
    ModelBuilder(ctx, grid).upload(policy, dynamics, value, lv, case["lf"], case["tau"])
    return grid, ctx.desc, ctx.head


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return hostsim_build.program("gp4_predecide_sim.cpp", tmp_path_factory.mktemp("gp4_predecide"),
                                 ["-g", "-O1"] + hostsim_build.SHIM_FLAGS[1:], sanitize=True)


def _run(sim, tmp_path, case, spacing, lo, hi):
    """The program on the case: ({"norm": [...], "eps": [...], "upload_ms": v, "blocks": B, "decided": D}, sure[hi - lo])."""
    _, desc, (X, Linv, alpha, variance, ls) = _describe(case)
    n, p = X.shape
    raw = bytes(desc)
    raw += b"\0" * (-len(raw) % 8)
    src, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([n, p, alpha.shape[1], variance, spacing, lo, hi, len(bytes(desc))], dtype=np.float64).tobytes())
        f.write(ls.tobytes())
        f.write(raw)
        for a in (X, Linv, alpha):
            f.write(np.ascontiguousarray(a).tobytes())
    res = subprocess.run([sim, src, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert res.returncode == 0, res.stderr
    got = {"norm": [], "eps": []}
    for line in res.stdout.splitlines():
        w = line.split()
        if w[0] in ("norm", "eps"):
            got[w[0]].append(float(w[2]))
        elif w[0] == "upload_ms":
            got["upload_ms"] = float(w[1])
        elif w[0] == "blocks":
            got["blocks"], got["decided"] = int(w[1]), int(w[3])
    return got, np.fromfile(out, dtype=np.uint8).astype(bool)


def _exact_norms(X, Linv, alpha, variance, ls):
    """(||g_j||_H^2, sum_ik |a_i| |a_k| K_ik, ||alpha'_j||_1, scaled inputs, alpha') in np.longdouble."""
    xs = (X / ls).astype(LD)
    ap = Linv.T.dot(alpha)
    a = ap.astype(LD)
    quad = np.zeros(a.shape[1], dtype=LD)
    mag = np.zeros(a.shape[1], dtype=LD)
    for i in range(len(xs)):
        k = LD(variance) * np.exp(LD(-0.5) * ((xs - xs[i]) ** 2).sum(1))
        quad += a[i] * (k[:, None] * a).sum(0)
        mag += np.abs(a[i]) * (k[:, None] * np.abs(a)).sum(0)
    return quad, mag, np.abs(a).sum(0), xs, a


def _models():
    return {"headline": _slab_case(),
            "257 points": cases.make_case("cartpole", num_points=[6, 6, 6, 64], n_gp=257, **_informed(tau_scale=0.0005)),
            "tiny lengthscale": cases.make_case("cartpole", num_points=[6, 6, 6, 64], n_gp=257,
                                                **_informed(tau_scale=0.0005, lengthscale=0.02))}


@pytest.mark.parametrize("name", ["headline", "257 points", "tiny lengthscale"])
def test_constants_bound_the_exact_norm_within_the_margin(sim, tmp_path, name):
    """norm_j of the upload against alpha'_j^T K alpha'_j in long double: never below its root, and
    above it by no more than the stated margin (1e-6 relative on the root of the value plus its
    summation allowance, 8 n eps_ld sum |a_i| |a_k| K_ik).  eps_j is the stated multiple of n 2^-53
    s^2 ||alpha'_j||_1.  The upload's cost is printed (87 ms at 1024 points in this -O1 build under the
    sanitizers, 5 ms at 257 points)."""
    case = _models()[name]
    got, _ = _run(sim, tmp_path, case, 8, 0, 64)
    _, _, (X, Linv, alpha, variance, ls) = _describe(case)
    quad, mag, l1, _, _ = _exact_norms(X, Linv, alpha, variance, ls)
    print(name, "norms", got["norm"], "upload ms", got["upload_ms"])
    n = len(X)
    exact = np.sqrt(np.maximum(quad, 0))
    upper = np.sqrt(quad + ROUND_TERMS * n * np.finfo(LD).eps * mag) * (1 + LD(NORM_MARGIN))
    norm = np.array(got["norm"], dtype=LD)
    # (alpha' of the program is summed in another order than NumPy's: 1e-12 relative covers it)
    assert (norm >= exact * (1 - LD(1e-12))).all(), (norm, exact)
    assert (norm <= upper * (1 + LD(1e-12))).all(), (norm, upper)
    assert (upper <= exact * (1 + LD(1e-5))).all()                     # the allowance itself is small
    eps = EPS_MULT * n * 2.0 ** -53 * variance * l1.astype(np.float64)
    np.testing.assert_allclose(got["eps"], eps, rtol=1e-9)


@pytest.mark.parametrize("name", ["headline", "257 points", "tiny lengthscale"])
def test_rkhs_inequality_on_random_pairs(name):
    """|g_j(z) - g_j(z_c)| <= ||g_j||_H d(z, z_c), d^2 = 2 s^2 (1 - exp(-|z - z_c|^2 / 2)) <= s^2 |z -
    z_c|^2, and the Taylor remainder the rule uses, |g_j(z) - g_j(z_c) - J_j (z - z_c)| <= (sqrt(3) / 2)
    ||g_j||_H s |z - z_c|^2, in long double on 400 random pairs: near ones (a grid step apart), far
    ones, and pairs at training points."""
    case = _models()[name]
    _, _, (X, Linv, alpha, variance, ls) = _describe(case)
    quad, _, _, xs, a = _exact_norms(X, Linv, alpha, variance, ls)
    norm = np.sqrt(quad)
    rng = np.random.default_rng(3)
    lo, hi = xs.min(0), xs.max(0)
    z = (lo + (hi - lo) * rng.random((400, xs.shape[1]))).astype(LD)
    step = np.concatenate((rng.normal(scale=0.01, size=(150, xs.shape[1])), rng.normal(scale=1.0, size=(150, xs.shape[1])),
                           rng.normal(scale=30.0, size=(100, xs.shape[1])))).astype(LD)
    z[350:] = xs[rng.integers(0, len(xs), 50)]
    z_c = z + step

    def g(pts):
        r2 = ((pts[:, None, :] - xs[None, :, :]) ** 2).sum(2)
        return (LD(variance) * np.exp(LD(-0.5) * r2)).dot(a)

    lhs = np.abs(g(z) - g(z_c))
    dist2 = (step ** 2).sum(1)
    d = np.sqrt(2 * LD(variance) * (1 - np.exp(LD(-0.5) * dist2)))
    rhs = norm[None, :] * d[:, None]
    slack = 64 * len(xs) * np.finfo(LD).eps * LD(variance) * np.abs(a).sum(0)     # rounding of the two sums
    assert (lhs <= rhs * (1 + LD(1e-12)) + slack).all(), float((lhs - rhs).max())
    assert (d <= np.sqrt(LD(variance) * dist2) * (1 + LD(1e-15))).all()
    assert (lhs > 0.01 * rhs).any()                       # the bound is not vacuous on these pairs
    diff = xs[None, :, :] - z_c[:, None, :]
    k = LD(variance) * np.exp(LD(-0.5) * (diff ** 2).sum(2))
    J = np.einsum("ci,ij,ciq->cjq", k, a, diff)           # dg/dz at z_c
    taylor = np.abs(g(z) - g(z_c) - np.einsum("cjq,cq->cj", J, -step))
    rem = (np.sqrt(LD(3)) / 2) * norm[None, :] * np.sqrt(LD(variance)) * dist2[:, None]
    assert (taylor <= rem * (1 + LD(1e-12)) + slack * (1 + np.abs(step).sum(1))[:, None]).all(), float((taylor - rem).max())
    if name != "tiny lengthscale":                        # (there g vanishes a few lengthscales off the training points)
        assert (taylor[:150] > 0.01 * rem[:150]).any()


def _oracle_final(case, lo, hi):
    from early_block_counts import cell_stages
    out = [cell_stages(case, np.arange(b, min(b + 4096, hi)))[1] for b in range(lo, hi, 4096)]
    return np.concatenate(out)


# CPU counts (this rule, the oracle): decided / all 16-cell blocks
@pytest.mark.parametrize("name,spacing,lo,hi,expect", [
    ("headline", 8, SLAB_LO, SLAB_HI, 55),
    ("headline", 4, SLAB_LO, SLAB_HI, 57),
    ("257 points", 2, 0, 6 * 6 * 6 * 64, 281),
    ("257 points", 1, 0, 6 * 6 * 6 * 64, 647),
])
def test_no_wrong_verdict_and_the_count_of_the_tool(sim, tmp_path, name, spacing, lo, hi, expect):
    """Every cell the rule decides fails in the oracle (zero wrong verdicts), both decided and open
    blocks occur, and the decided blocks are exactly those of tools/early_block_counts.py
    --mean-lattice (the rule in NumPy).  Decided blocks on the CPU: headline slab (rows of the headline
    grid 13 / 14 / 7 cells apart in the leading axes, so its references lie far apart), 640 blocks: 55
    at S = 8, 57 at S = 4, where the exact mean decides 155; 6 x 6 x 6 x 64 with 257 points, 864 blocks:
    281 at S = 2, 647 at S = 1."""
    from early_block_counts import mean_lattice_sure
    case = _models()[name]
    got, sure = _run(sim, tmp_path, case, spacing, lo, hi)
    passes = _oracle_final(case, lo, hi)
    assert not (sure & passes).any(), int((sure & passes).sum())
    blocks = sure.reshape(-1, 16).all(1)
    print(name, "S =", spacing, "decided", int(blocks.sum()), "of", len(blocks))
    assert got["blocks"] == len(blocks) and got["decided"] == int(blocks.sum())
    assert 0 < blocks.sum() < len(blocks)
    tool = mean_lattice_sure(case, np.arange(lo, hi), spacing).reshape(-1, 16).all(1)
    assert int(tool.sum()) == int(blocks.sum())
    assert np.array_equal(tool, blocks)
    if expect is not None:
        assert int(blocks.sum()) == expect
