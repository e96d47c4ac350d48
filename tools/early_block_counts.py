"""How much variance-panel work does k_gp_sweep4's early decision leave, by the granule of cells
that must be wholly decided before its panels stop?  Counted on the CPU with the oracle alone (no
GPU): random 64-cell tiles of ``benchmarks.headline_case(variant)``, the bounds the kernel uses
(``err = 0`` from below, ``beta sqrt(variance - partial |a|^2)`` from above, 256-row panels), for
granules of 64 / 32 / 16 / 1 cells.  The kernel's granule is the 16-cell block; the
64-cell row is what its predecessor counted on the device (profiles/early_stage_counts.txt), the
1-cell row the floor.

    python tools/early_block_counts.py [--variant informed|tight|survey] [--tiles 3000] [--seed 0]
                                       [--variance-floor] [--headline-tau] [--halves] [--mean-lattice S]

--variance-floor: the lower bound of a cell before panel s is the decrease at err = beta sqrt(c_s
(variance - partial |a|^2)) instead of err = 0, with c_s = sigma_n^2 sigma_min(Linv[256 s:, 256 s:])^2
= sigma_n^2 / lambda_max of the Schur complement of the first 256 s rows (the
posterior variance of all n points is at least c_s times the one of the first 256 s).  Before
panel 0 the bound stays err = 0, as in k_gp_mean_blocks.
--headline-tau: the variant's hyper-parameters on the headline's discretisation constant (the
"little skipped" line of profiles/blocks_little_skipped.txt).

--halves: the kernel decides the two 8-cell halves of a block separately and packs the low half of
one block beside the high half of another into one slot of a composite tile (DESIGN.md 4.1 "Half
blocks").  Adds the 8- and 4-cell granules to the table and prints, per panel, of all blocks: the
full slots (both halves open), the paired slots (a low-only half beside a high-only half, as many
as the rarer kind allows), the lone halves (the surplus of the other kind, a slot each), the share of
open halves whose sibling is open too, the slots over the blocks open at the 16-cell granule - and
the panel work at that packing.  (The first decision of a large launch is per block: the line
"halves from panel 1 on" keeps the 16-cell count for panel 0.)

--mean-lattice S: the blocks k_gp_predecide decides before the mean is computed, by the kernel's
rule (safe_learning_amd/csrc/sl_gp4_predecide.h, the constants of sl_gp_mean_bound.h) in NumPy: the
mean of a cell lies within (sqrt(3) / 2) norm_j s |z - z_c|^2 (and a rounding allowance) of its
first-order Taylor expansion about the nearest point of a lattice of every S-th grid index per axis
(and the last index), and a block is decided when
the lower bound of V(mean) that follows keeps every cell of it from passing.  Printed beside the
blocks the exact mean decides (stage 0 of the table above).

Panel p of a tile multiplies (p + 1) 4 chunks against its 16 row blocks, the diagonal band a
triangle: 40 / 104 / 168 / 232 (row block, chunk) products for p = 0 .. 3, 64 more per panel
after that."""
import argparse
import os
import sys

import numpy as np
import scipy.linalg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

RP = 256                                         # rows per panel of k_gp_sweep4
GRANULES = (64, 32, 16, 1)


def panel_weights(npan):
    """(row block, chunk) products of panel 0 .. npan - 1 of a tile."""
    return np.array([40 + 64 * p for p in range(npan)], dtype=float)


def floor_constants(L, noise, npan):
    """c_s = sigma_n^2 / lambda_max(L[256 s:, 256 s:] L[256 s:, 256 s:]^T) for s = 0 .. npan - 1."""
    return np.array([noise / np.linalg.svd(L[RP * s:, RP * s:], compute_uv=False)[0] ** 2 for s in range(npan)])


def cell_stages(case, idx, floor=False):
    """Per cell of ``idx``: the stage at which the bounds decide it (0 = from the mean alone, s =
    with s panels in |a|^2, npan = only the full sum does), its final mask bit, and whether its
    decrease is clear of the threshold (beyond the 1e-7 relative agreement of engine and oracle).
    floor: the variance floor c_s (variance - partial |a|^2) in the lower bound instead of 0.
    Returns (stage, final, clear, npan)."""
    import cases
    ol = cases.oracle_lyapunov(case, compute_values=False)
    grid, G = ol.discretization, ol.dynamics
    gp = G.gaussian_process
    L = gp.cholesky
    npan = (L.shape[0] + RP - 1) // RP
    x = grid.index_to_state(np.asarray(idx))
    Xn = np.hstack((x, ol.policy(x)))
    a = scipy.linalg.solve_triangular(L, gp.kern.K(gp.X, Xn), lower=True)
    mean = a.T.dot(gp.alpha) + gp._mean(Xn)
    var0 = gp.kern.Kdiag(Xn)
    thr = np.broadcast_to(ol.threshold(x, ol.tau), (len(idx), 1))[:, 0]

    def decrease(sumsq):
        err = G.beta * np.sqrt(np.maximum(var0 - sumsq, 0))[:, None] * np.ones((1, mean.shape[1]))
        return ol.v_decrease_bound(x, (mean, err))[:, 0]

    dec = decrease(np.sum(a ** 2, 0))
    final = dec < thr
    clear = np.abs(dec - thr) > 1e-7 * (np.abs(dec) + np.abs(thr)) + 1e-12
    c = floor_constants(L, case["dynamics"]["noise_variance"], npan) if floor else np.zeros(npan)
    c[0] = 0.0        # the first decision of a large launch is k_gp_mean_blocks', which keeps err = 0
    stage = np.full(len(idx), npan)
    part = np.zeros_like(var0)
    for s in range(npan):
        if s:
            part = part + np.sum(a[(s - 1) * RP:s * RP] ** 2, 0)
        sure_fail = ~(decrease(var0 - c[s] * (var0 - part)) < thr)       # err^2 = beta^2 c_s (var0 - part); c = 0: err = 0
        assert not (sure_fail & final).any()
        done = sure_fail | (decrease(part) < thr)
        stage[(stage == npan) & done] = s
    return stage, final, clear, npan


def granule_stages(stage, granule):
    """Stage at which every cell of a granule of consecutive cells is decided."""
    return stage.reshape(-1, granule).max(1)


def open_fractions(gstage, npan):
    """Fraction of granules still open before panel 0 .. npan - 1."""
    return np.array([(gstage > p).mean() for p in range(npan)])


def panel_work(gstage, npan):
    """Panel work executed, as a fraction of every panel of every granule."""
    w = panel_weights(npan)
    return float(open_fractions(gstage, npan).dot(w) / w.sum())


def half_packing(stage, npan):
    """Per panel, as fractions of all 16-cell blocks: (full slots, paired slots, lone halves, share of
    open halves whose sibling is open, slots / blocks open at the 16-cell granule), and the panel work
    with every panel packed in halves / with panel 0 on whole blocks."""
    h = granule_stages(stage, 8).reshape(-1, 2)
    rows, slots, blocks = [], [], []
    for p in range(npan):
        lo, hi = h[:, 0] > p, h[:, 1] > p
        full, lo_only, hi_only = (lo & hi).mean(), (lo & ~hi).mean(), (~lo & hi).mean()
        paired, lone = min(lo_only, hi_only), abs(lo_only - hi_only)
        open_blocks, open_halves = (lo | hi).mean(), lo.mean() + hi.mean()
        slots.append(full + paired + lone)
        blocks.append(open_blocks)
        rows.append((full, paired, lone, 2 * full / open_halves if open_halves else 1.0,
                     slots[-1] / open_blocks if open_blocks else 1.0, 0.5 * open_halves / open_blocks if open_blocks else 1.0))
    w = panel_weights(npan)
    work = float(np.dot(slots, w) / w.sum())
    work_from_1 = float((blocks[0] * w[0] + np.dot(slots[1:], w[1:])) / w.sum())
    return rows, work, work_from_1


# ---- k_gp_predecide's rule (sl_gp4_predecide.h), vectorised ---------------------------------------
NORM_MARGIN, ROUND_TERMS, EPS_MULT, SLACK = 1e-6, 8.0, 4096.0, 2.0 ** -40      # sl_gp_mean_bound.h, sl_gp4_predecide.h
HALF_SQRT3 = 0.8660254037844388


def mean_bound_constants(xs, alphap, variance):
    """(norm[dout], eps[dout]) of sl_gp_mean_bound.h from the scaled inputs xs [n][p] and alpha'
    [n][dout], in np.longdouble."""
    ld = np.longdouble
    n = len(xs)
    x = xs.astype(ld)
    a = alphap.astype(ld)
    quad = np.zeros(a.shape[1], dtype=ld)
    mag = np.zeros(a.shape[1], dtype=ld)
    for i in range(n):                                   # (row by row: n x n long doubles are 16 MB at 1024)
        k = ld(variance) * np.exp(ld(-0.5) * ((x - x[i]) ** 2).sum(1))
        quad += a[i] * (k[:, None] * a).sum(0)
        mag += np.abs(a[i]) * (k[:, None] * np.abs(a)).sum(0)
    up = np.maximum(quad, 0) + ld(ROUND_TERMS) * n * np.finfo(ld).eps * mag
    norm = (np.sqrt(up) * (1 + ld(NORM_MARGIN))).astype(np.float64)
    eps = (ld(EPS_MULT) * n * ld(2.0) ** -53 * ld(variance) * np.abs(a).sum(0) * (1 + ld(2.0) ** -40)).astype(np.float64)
    return norm, eps


def lattice_nearest(i, num, spacing):
    """Grid index of the lattice point nearest to grid index i (arrays), the lower one on a tie."""
    ia = (i // spacing) * spacing
    ib = np.minimum(ia + spacing, num - 1)
    return np.where((i - ia) > (ib - i), ib, ia)


def mean_lattice_sure(case, idx, spacing):
    """Per cell of ``idx``: does k_gp_predecide's rule at lattice spacing ``spacing`` show it to fail?"""
    import cases
    ol = cases.oracle_lyapunov(case, compute_values=False)
    grid, gp = ol.discretization, ol.dynamics.gaussian_process
    dyn = case["dynamics"]
    ls = np.asarray(dyn["lengthscales"], dtype=float)
    variance = float(dyn["variance"])
    xs = gp.X / ls
    alphap = scipy.linalg.solve_triangular(gp.cholesky, gp.alpha, lower=True, trans="T")
    norm, eps = mean_bound_constants(xs, alphap, variance)
    sdev = np.sqrt(variance) * (1 + 2.0 ** -50)
    idx = np.asarray(idx)
    num = np.asarray(grid.num_points)
    ijk = np.stack(np.unravel_index(idx, num), 1)
    near = np.stack([lattice_nearest(ijk[:, k], num[k], spacing) for k in range(len(num))], 1)
    ref = np.ravel_multi_index(tuple(near.T), num)
    uniq, inverse = np.unique(ref, return_inverse=True)

    def scaled(cells):
        x = grid.index_to_state(cells)
        return x, np.hstack((x, ol.policy(x))) / ls

    _, zc_u = scaled(uniq)
    g_u = np.empty((len(uniq), alphap.shape[1]))
    J_u = np.empty((len(uniq), alphap.shape[1], xs.shape[1]))
    for b in range(0, len(uniq), 2048):
        diff = xs[None, :, :] - zc_u[b:b + 2048][:, None, :]
        k = variance * np.exp(-0.5 * (diff ** 2).sum(2))
        g_u[b:b + 2048] = k.dot(alphap)
        J_u[b:b + 2048] = np.einsum("ci,ij,ciq->cjq", k, alphap, diff)      # d/dz k(z, z_i) = k (z_i - z)
    x, z = scaled(idx)
    z_c, g_c, J = zc_u[inverse], g_u[inverse], J_u[inverse]
    prior = gp._mean(np.hstack((x, ol.policy(x))))
    v_x = ol.lyapunov_function(x)[:, 0]
    thr = np.broadcast_to(ol.threshold(x, ol.tau), (len(idx), 1))[:, 0]
    P = np.asarray(case["P"], dtype=float)
    D = z - z_c
    dist2 = (D ** 2).sum(1) * (1 + 2.0 ** -40)
    zmax = np.maximum(1.0, np.maximum(np.abs(z).max(1), np.abs(z_c).max(1)))
    terms = J * D[:, None, :]
    mu = g_c + terms.sum(2) + prior
    absm = np.abs(g_c) + np.abs(terms).sum(2) + np.abs(prior)
    B = (((HALF_SQRT3 * norm) * sdev) * dist2[:, None] + eps * (2 * zmax + np.abs(D).sum(1))[:, None]) * (1 + 2.0 ** -40) \
        + 2.0 ** -48 * absm
    A = np.abs(mu) + B
    vc = (mu.dot(P) * mu).sum(1)
    lin = (np.abs(mu.dot(P + P.T)) * B).sum(1)
    quad = (B.dot(np.abs(P)) * B).sum(1)
    mag = (A.dot(np.abs(P)) * A).sum(1) + np.abs(v_x) + np.abs(thr)
    lower = ((vc - lin) - quad) - v_x
    return np.isfinite(mag) & (lower >= thr + SLACK * mag)


def count_mean_lattice(variant=None, tiles=1500, seed=0, spacing=8, headline_tau=False, batch=500):
    """(blocks the bound decides, blocks the exact mean decides) as fractions of the blocks of random
    headline tiles."""
    from safe_learning_amd.benchmarks import headline_case
    case = headline_case(variant=variant)
    if headline_tau:
        case["tau"] = headline_case()["tau"]
    idx = sample_tiles(case, tiles, seed)
    sure = mean_lattice_sure(case, idx, spacing)
    stages = [cell_stages(case, idx[b:b + batch * 64])[0] for b in range(0, len(idx), batch * 64)]
    stage = np.concatenate(stages)
    final_fail_at_0 = granule_stages(stage, 16) == 0
    by_bound = sure.reshape(-1, 16).all(1)
    assert not (by_bound & ~final_fail_at_0).any()       # (the bound decides nothing the exact mean leaves open)
    return float(by_bound.mean()), float(final_fail_at_0.mean())


def sample_tiles(case, tiles, seed):
    """Cell indices of ``tiles`` random 64-cell tiles of the case's grid (tile-aligned)."""
    n = int(np.prod(case["num_points"]))
    rng = np.random.default_rng(seed)
    first = rng.choice(n // 64, size=min(tiles, n // 64), replace=False) * 64
    return (first[:, None] + np.arange(64)[None, :]).reshape(-1)


def count(variant=None, tiles=3000, seed=0, batch=500, floor=False, headline_tau=False, granules=GRANULES,
          halves=False):
    """{granule: (open fractions before each panel, panel work)} over random tiles; halves: also
    half_packing() of the same cells, under the key "halves"."""
    from safe_learning_amd.benchmarks import headline_case
    case = headline_case(variant=variant)
    if headline_tau:
        case["tau"] = headline_case()["tau"]
    idx = sample_tiles(case, tiles, seed)
    stages = []
    for b in range(0, len(idx), batch * 64):             # (bounded memory: n x cells factors)
        st, _, _, npan = cell_stages(case, idx[b:b + batch * 64], floor)
        stages.append(st)
    stage = np.concatenate(stages)
    result = {g: (open_fractions(granule_stages(stage, g), npan), panel_work(granule_stages(stage, g), npan))
              for g in granules}
    if halves:
        result["halves"] = half_packing(stage, npan)
    return result, npan


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--variant", default=None)
    ap.add_argument("--tiles", type=int, default=3000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--variance-floor", action="store_true")
    ap.add_argument("--headline-tau", action="store_true")
    ap.add_argument("--halves", action="store_true")
    ap.add_argument("--mean-lattice", type=int, default=0, metavar="S")
    args = ap.parse_args()
    if args.mean_lattice:
        bound, exact = count_mean_lattice(args.variant, args.tiles, args.seed, args.mean_lattice, args.headline_tau)
        print("# headline_case(variant=%r)%s, %d random tiles, seed %d, lattice spacing %d" % (
            args.variant, " at the headline tau" if args.headline_tau else "", args.tiles, args.seed, args.mean_lattice))
        print("blocks with all 16 cells decided by the bound: %.4f | blocks the exact mean decides: %.4f" % (bound, exact))
        sys.exit(0)
    granules = (64, 32, 16, 8, 4, 1) if args.halves else GRANULES
    result, npan = count(args.variant, args.tiles, args.seed, floor=args.variance_floor, headline_tau=args.headline_tau,
                         granules=granules, halves=args.halves)
    print("# headline_case(variant=%r)%s, %d random tiles, seed %d, %d panels, lower bound: %s" % (
        args.variant, " at the headline tau" if args.headline_tau else "", args.tiles, args.seed, npan,
        "variance floor" if args.variance_floor else "err = 0"))
    print("# granule (cells) | open before panel 0 .. %d | panel work executed" % (npan - 1))
    for g in granules:
        frac, work = result[g]
        print(("%5d | %s | %.4f" if args.halves else "%5d | %s | %.3f") % (g, " / ".join("%.3f" % f for f in frac), work))
    if args.halves:
        rows, work, work_from_1 = result["halves"]
        print("# packed halves, per panel, of all blocks: full slots | paired slots | lone halves | open halves with an "
              "open sibling | slots / open blocks | halves / 2 / open blocks")
        for p, row in enumerate(rows):
            print("panel %d | %.4f | %.4f | %.4f | %.3f | %.3f | %.3f" % ((p,) + row))
        print("panel work at that packing: %.4f (16-cell blocks: %.4f); halves from panel 1 on: %.4f"
              % (work, result[16][1], work_from_1))
