// sl_gp4_predecide.h - the rule by which k_gp_predecide (sl_gp4_predecide.hip) decides a cell of a
// block-mode GP sweep as failing BEFORE its posterior mean is computed (DESIGN.md 4.1 "Deciding
// before the mean"), and what the launcher of k_gp_mean_blocks needs of that pass.  The rule is
// host / device code (SL_HD): tests/test_gp_mean_bound_host.py runs it on the CPU.
//
// The mean without the prior, g_j(z) = sum_i alpha'_ij k(z, z_i), lies in the RKHS of the RBF
// kernel k(z, z') = s^2 exp(-|z - z'|^2 / 2) of the scaled input z, and for every f of that space
// and every unit direction v
//     |d^2/dv^2 f(z)| = |<f, d^2/dv^2 k(z, .)>| <= ||f||_H sqrt(3 s^2) = sqrt(3) s ||f||_H
// (the norm of d^2/dv^2 k(z, .) is the root of s^2 times the fourth derivative of exp(-t^2 / 2) at 0,
// which is 3).  A lattice of reference cells c (every S-th grid index of every axis and the last
// index of the axis; a cell uses the nearest lattice index per axis, the lower one on a tie)
// carries z_c, g(z_c) and the gradient J = dg/dz (z_c) - k_gp_mean_lattice - and Taylor's theorem
// on the segment from z_c to z gives, with D = z - z_c and norm_j >= ||g_j||_H (sl_gp_mean_bound.h),
//     |g_j(z) - g_j(z_c) - J_j D| <= (sqrt(3) / 2) norm_j s |D|^2.
// (The first-order bound |g_j(z) - g_j(z_c)| <= norm_j s |D| alone decides little: the norms of a
// well-informed model are large - 7 to 46 on the headline model, whose g stays below 3.5 s - because
// they carry the fit of the noise.)  With mu_c = g(z_c) + J D + prior(x) therefore
//     |mu_j(x) - mu_c,j| <= B_j,     V(mu) >= V(mu_c) - sum_j |((P + P^T) mu_c)_j| B_j - sum_ij |P_ij| B_i B_j
// for the quadratic V(mu) = mu^T P mu.  If that lower bound minus V(x) is not below the threshold,
// the decrease of the cell is not either, whatever its variance: the engine adds sum_j L_v,j err_j
// >= 0 to fl(V(mu) - V(x)) (beta >= 0, L_v >= 0: gp4_early_ok) and a rounded sum is monotone.
//
// Rounding.  mu is the ENGINE's rounded mean fl(g^(z) + prior): B_j therefore holds, besides the
// remainder with the computed |D|^2 (rounded up by 2^-40: p + 1 roundings of 2^-53),
//   * eps_j (2 max(1, |z|_inf) + |D|_1): the allowance of sl_gp_mean_bound.h once for the engine's g^
//     at the cell, once for the lattice kernel's at the reference, and per entry of J (its terms
//     alpha'_i k_i (z_i - z_c)_q are below 0.61 s^2 |alpha'_i|: |t| exp(-t^2 / 2) <= 0.61);
//   * 2^-48 (|g_c,j| + sum_q |J_jq| |D_q| + |prior_j|) for the p + 1 additions and p products of
//     mu_c here and the engine's addition of the prior, which is computed here by the engine's
//     own code and has the engine's bits.
// The quadratic forms here and in the engine are sums of at most d^2 + d products (d <= 4): each
// differs from its exact value by less than 2^-47 sum_ij |P_ij| A_i A_j with A_j = |mu_c,j| + B_j >=
// |mu_j|.  One relative slack covers them all, and the bits of V(x) and of the threshold too:
//     lower bound - V(x) >= threshold + SLACK (sum_ij |P_ij| A_i A_j + |V(x)| + |threshold|),  SLACK = 2^-40,
// against a total of less than 2^-44 of that magnitude.  A non-finite value anywhere makes the
// comparison false: the cell stays open.
#pragma once
#include "sl_model.h"

namespace gp4p {

constexpr double SLACK = 0x1p-40;
constexpr long long MAX_LATTICE = 1ll << 24;
constexpr long long MAX_TABLE_BYTES = 64ll << 20;       // the table is to stay in the 256 MB last-level cache beside the sweep's data

struct PreConst {
    double norm[SL_D], eps[SL_D];          // sl_gp_mean_bound.h
    double sdev;                           // >= sqrt(prior variance)
    int32_t spacing, count[SL_D];          // lattice spacing S, lattice points per axis
};

// doubles per lattice point: z_c [p], g(z_c) [d], dg/dz (z_c) [d][p]
SL_HD int row_doubles(int d, int p) { return p + d + d * p; }
// lattice points of an axis of `num` grid points: indices 0, S, 2 S, ... and num - 1
SL_HD int lattice_count(int num, int S) { return (num - 1 + S - 1) / S + 1; }
// grid index of lattice index a
SL_HD int lattice_grid_index(int a, int num, int S) { return a * S < num - 1 ? a * S : num - 1; }
// nearest lattice index of grid index i (the lower one on a tie)
SL_HD int lattice_nearest(int i, int num, int S) {
    const int a = i / S, ia = a * S;
    const int ib = ia + S < num - 1 ? ia + S : num - 1;
    return (i - ia) > (ib - i) ? a + 1 : a;
}

constexpr double HALF_SQRT3 = 0.8660254037844388;      // >= sqrt(3) / 2 = 0.86602540378443864...

// Is the cell sure to fail?  z_c [p], g_c [d], J [d][p]: the reference's table row; z: the cell's
// scaled input [p]; prior: the cell's prior mean [d]; v_x, thr: V(x) and the threshold as the engine
// computes them.
SL_HD bool sure_fail(const sl_value_desc& v, int d, int p, const PreConst& k, const double* z, const double* z_c,
                     const double* g_c, const double* J, const double* prior, double v_x, double thr) {
    double D[SL_P], dist2 = 0.0, d1 = 0.0, zmax = 1.0;
#pragma unroll
    for (int q = 0; q < SL_P; ++q) {
        D[q] = 0.0;
        if (q < p) {
            D[q] = z[q] - z_c[q];
            dist2 = dist2 + D[q] * D[q];
            d1 = d1 + fabs(D[q]);
            zmax = fmax(zmax, fmax(fabs(z[q]), fabs(z_c[q])));
        }
    }
    dist2 = dist2 * (1.0 + 0x1p-40);
    double mu[SL_D], B[SL_D], A[SL_D];
#pragma unroll
    for (int j = 0; j < SL_D; ++j) {
        mu[j] = B[j] = A[j] = 0.0;
        if (j < d) {
            double lin = g_c[j], absm = fabs(g_c[j]) + fabs(prior[j]);
#pragma unroll
            for (int q = 0; q < SL_P; ++q) {
                if (q < p) {
                    const double t = J[j * p + q] * D[q];
                    lin = lin + t;
                    absm = absm + fabs(t);
                }
            }
            mu[j] = lin + prior[j];
            B[j] = (((HALF_SQRT3 * k.norm[j]) * k.sdev) * dist2 + k.eps[j] * (2.0 * zmax + d1)) * (1.0 + 0x1p-40) +
                   0x1p-48 * absm;
            A[j] = fabs(mu[j]) + B[j];
        }
    }
    double vc = 0.0, lin = 0.0, quad = 0.0, mag = 0.0;
#pragma unroll
    for (int j = 0; j < SL_D; ++j) {
        if (j < d) {
            double row = 0.0, grad = 0.0, qb = 0.0, qa = 0.0;
#pragma unroll
            for (int i = 0; i < SL_D; ++i) {
                if (i < d) {
                    row = row + mu[i] * v.matrix[i][j];
                    grad = grad + mu[i] * (v.matrix[i][j] + v.matrix[j][i]);
                    qb = qb + fabs(v.matrix[i][j]) * B[i];
                    qa = qa + fabs(v.matrix[i][j]) * A[i];
                }
            }
            vc = vc + row * mu[j];
            lin = lin + fabs(grad) * B[j];
            quad = quad + qb * B[j];
            mag = mag + qa * A[j];
        }
    }
    mag = mag + fabs(v_x) + fabs(thr);
    const double lower = ((vc - lin) - quad) - v_x;
    return mag < INFINITY && lower >= thr + SLACK * mag;
}

}  // namespace gp4p

#if defined(__HIPCC__)
#include "sl_common.h"
#include "sl_gp4_open.h"

// The open-block list of the pass (sl_gp4_open.h) lies in ctx->d_gp4_pre around the tile bytes: a head
// of gp4o::HEAD_BYTES in front of them, behind them one count per chunk of tiles and then the list
// itself, sized for every block open.  Everything follows from the address of the tile bytes and the
// number of tiles, so the context carries nothing new.
struct Gp4OpenView {
    unsigned long long* head;        // [gp4o::HEAD_LENGTH], [gp4o::HEAD_NTILES], [gp4o::HEAD_BUILT]
    unsigned* counts;                // open blocks of every chunk
    unsigned* list;                  // block numbers 4 tile + jb, ascending
};
inline Gp4OpenView sl_gp4_open_view(const unsigned char* tiles, long long ntiles) {
    unsigned char* t = const_cast<unsigned char*>(tiles);
    Gp4OpenView v;
    v.head = reinterpret_cast<unsigned long long*>(t - gp4o::HEAD_BYTES);
    v.counts = reinterpret_cast<unsigned*>(t + gp4o::tile_bytes(ntiles));
    v.list = reinterpret_cast<unsigned*>(t + gp4o::tile_bytes(ntiles) + gp4o::count_bytes(ntiles));
    return v;
}
// May the mean pass of a shard of ntiles tiles run from the list?  (block numbers and list positions are 32 bits)
inline bool sl_gp4_open_fits(long long ntiles) { return 4 * ntiles < (1ll << 31); }
// k_gp_open_count and k_gp_open_scatter over the tile bytes k_gp_predecide has just written, on the context's stream
int sl_gp4_open_build(sl_ctx* ctx, const unsigned char* tiles, long long ntiles);

struct Gp4PreLaunch {
    int workgroups;                  // one key per wavefront: 4 workgroups keys, written (not folded)
    sl_key* partials;
    unsigned long long* decided;     // device counter of decided blocks (zeroed by the sweep's launcher)
};

// May the pass run for this sweep?  (block mode holds: the caller is the launcher of k_gp_mean_blocks)
bool sl_gp4_predecide_ok(const sl_ctx* ctx, const SlDevModel& model, const SlSweepArgs& a);

// Lattice pass and deciding pass over the whole shard [a.lo, a.hi) on the context's stream; *tiles:
// one byte per 64-cell tile of the shard, bit jb = block jb is decided (its mask bits and key are
// written).  Every tile with cells below a.hi has its byte written.
template <int D>
int sl_gp4_predecide_launch_dim(sl_ctx* ctx, const SlDevModel& model, const SlSweepArgs& a, const Gp4PreLaunch& m,
                                const unsigned char** tiles);
#define SL_GP4_PRE_DECL(D_)                                                                                  \
    template <> int sl_gp4_predecide_launch_dim<D_>(sl_ctx*, const SlDevModel&, const SlSweepArgs&,          \
                                                    const Gp4PreLaunch&, const unsigned char**);
SL_GP4_PRE_DECL(1) SL_GP4_PRE_DECL(2) SL_GP4_PRE_DECL(3) SL_GP4_PRE_DECL(4)
#undef SL_GP4_PRE_DECL
#endif
