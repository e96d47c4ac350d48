"""How much variance-panel work does k_gp_sweep4's early decision leave, by the granule of cells
that must be wholly decided before its panels stop?  Counted on the CPU with the oracle alone (no
GPU): random 64-cell tiles of ``benchmarks.headline_case(variant)``, the bounds the kernel uses
(``err = 0`` from below, ``beta sqrt(variance - partial |a|^2)`` from above, 256-row panels), for
granules of 64 / 32 / 16 / 1 cells.  The kernel's granule is the 16-cell block; the
64-cell row is what its predecessor counted on the device (profiles/early_stage_counts.txt), the
1-cell row the floor.

    python tools/early_block_counts.py [--variant informed|tight|survey] [--tiles 3000] [--seed 0]
                                       [--variance-floor] [--headline-tau] [--halves]

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
    args = ap.parse_args()
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
