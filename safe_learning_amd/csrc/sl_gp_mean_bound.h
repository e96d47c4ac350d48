// sl_gp_mean_bound.h - constants of the Taylor bound on the posterior mean that k_gp_predecide
// (sl_gp4_predecide.hip, DESIGN.md 4.1 "Deciding before the mean") uses to decide blocks before
// k_gp_mean_blocks computes their mean.
//
// Column j of the mean without the prior is g_j(z) = sum_i alpha'_ij k(z, z_i), a function of the
// RKHS of k(z, z') = s^2 exp(-|z - z'|^2 / 2) (z the scaled input).  For any two inputs
//     |g_j(z) - g_j(z_c)| <= ||g_j||_H d(z, z_c),   ||g_j||_H^2 = alpha'_j^T K alpha'_j  (K without noise),
//     d^2 = 2 s^2 (1 - exp(-|z - z_c|^2 / 2)) <= s^2 |z - z_c|^2,
// and by the same argument on second derivatives |d^2/dv^2 g_j| <= sqrt(3) s ||g_j||_H, which is what the rule
// uses: the remainder of a first-order Taylor expansion about a reference cell (sl_gp4_predecide.h).
// Per column this header gives
//   * norm[j] >= ||g_j||_H: alpha'_j^T K alpha'_j from the uploaded (rounded) alpha' and scaled
//     inputs, accumulated in long double, plus an allowance for that accumulation and for expl
//     (ROUND_TERMS n eps_ld sum_ik |alpha'_i| |alpha'_k| K_ik: every product and sum of the double
//     sum rounds once, the kernel value a few times), the root rounded up by NORM_MARGIN;
//   * eps[j]: what the engine's own mean of a cell may differ from g_j at that cell's input,
//     eps[j] max(1, |z|_inf) with eps[j] = EPS_MULT n 2^-53 s^2 ||alpha'_j||_1 (the kernel applies
//     the factor of the cell's own scaled input z).  The MFMA sum of n products rounds to within
//     n 2^-53 s^2 ||alpha'_j||_1; the rest of the multiple covers the k_x values themselves, which
//     the sweep generates by a 16-step recurrence from one exponential per run (relative error
//     below 200 2^-53) on inputs it treats as affine while their second difference stays below
//     2e-14 max(1, |z|): over 16 cells a deviation below 128 times that per coordinate, 6e-12
//     max(1, |z|_inf) in norm for p <= 5, and an absolute error of the kernel value below 3.5e-12
//     s^2 max(1, |z|_inf) (|t| exp(-t^2 / 2) <= 0.61).  The gate below (more than 192 points)
//     makes EPS_MULT n 2^-53 at least 8.7e-11.
// false = "off" is the answer to every doubt: a non-finite entry or result, a variance that is not
// positive.  (The caller gates on the kernel family and the size of the head.)
//
// Plain C++: g++ compiles it for the tests.
#pragma once

#include <cmath>
#include <limits>
#include <vector>

namespace gpbound {

constexpr double NORM_MARGIN = 1e-6;      // norm[j] <= (1 + NORM_MARGIN) sqrt(exact + allowance)
constexpr double ROUND_TERMS = 8.0;       // roundings per term of the double sum, of n eps_ld
constexpr double EPS_MULT = 4096.0;       // eps[j] in units of n 2^-53 s^2 ||alpha'_j||_1
constexpr int MAX_COLS = 8;
constexpr int MIN_POINTS = 193;           // the heads k_gp_sweep4 serves; eps[j] relies on it (above)

// xs: scaled inputs [p][n_pad] (as uploaded), alphap: alpha' [n_pad][dout] (as uploaded).
inline bool mean_bound(const double* xs, int n, int n_pad, int p, const double* alphap, int dout, double variance,
                       double* norm, double* eps) {
    for (int j = 0; j < dout && j < MAX_COLS; ++j) norm[j] = eps[j] = 0.0;
    if (n < MIN_POINTS || p < 1 || dout < 1 || dout > MAX_COLS || !(variance > 0.0) || !(variance < INFINITY)) return false;
    for (int i = 0; i < n; ++i) {
        for (int q = 0; q < p; ++q)
            if (!(std::fabs(xs[(size_t)q * n_pad + i]) < INFINITY)) return false;
        for (int j = 0; j < dout; ++j)
            if (!(std::fabs(alphap[(size_t)i * dout + j]) < INFINITY)) return false;
    }
    const long double s2 = variance;
    std::vector<long double> quad(dout, 0.0L), mag(dout, 0.0L), l1(dout, 0.0L), row(dout), rowm(dout);
    for (int i = 0; i < n; ++i) {
        // row i of K alpha' below the diagonal (K is symmetric: those terms count twice)
        for (int j = 0; j < dout; ++j) row[j] = rowm[j] = 0.0L;
        for (int k = 0; k < i; ++k) {
            long double r2 = 0.0L;
            for (int q = 0; q < p; ++q) {
                const long double dz = (long double)xs[(size_t)q * n_pad + i] - (long double)xs[(size_t)q * n_pad + k];
                r2 += dz * dz;
            }
            const long double kik = s2 * expl(-0.5L * r2);
            for (int j = 0; j < dout; ++j) {
                const long double a = alphap[(size_t)k * dout + j];
                row[j] += kik * a;
                rowm[j] += kik * fabsl(a);
            }
        }
        for (int j = 0; j < dout; ++j) {
            const long double a = alphap[(size_t)i * dout + j];
            quad[j] += a * (2.0L * row[j] + s2 * a);
            mag[j] += fabsl(a) * (2.0L * rowm[j] + s2 * fabsl(a));
            l1[j] += fabsl(a);
        }
    }
    const long double eps_ld = std::numeric_limits<long double>::epsilon();
    for (int j = 0; j < dout; ++j) {
        const long double allowance = (long double)ROUND_TERMS * n * eps_ld * mag[j];
        const long double up = (quad[j] > 0.0L ? quad[j] : 0.0L) + allowance;
        const double nj = (double)(sqrtl(up) * (1.0L + (long double)NORM_MARGIN));
        const double ej = (double)((long double)EPS_MULT * n * 0x1p-53L * s2 * l1[j] * (1.0L + 0x1p-40L));
        if (!(nj >= 0.0) || !(nj < INFINITY) || !(ej >= 0.0) || !(ej < INFINITY)) return false;
        norm[j] = nj;
        eps[j] = ej;
    }
    return true;
}

}  // namespace gpbound
