// sl_gp_floor.h - the variance floor of k_gp_sweep4's early decision: constants c_s
// with
//     V_n(x) >= c_s V_m(x),  m = s RP,
// for every input x, V_m the posterior variance with the first m training points.  With S_m the
// Schur complement of the first m rows of K + sigma_n^2 I (the covariance of the remaining noisy
// observations given the first m),
//     c_s = sigma_n^2 / lambda_max(S_m) = sigma_n^2 lambda_min(P),  P = B^T B,  B = Linv[m:, m:],
// because the trailing block of the inverse factor is the inverse of the factor of S_m.
//
// The constant must be an UNDER-estimate, so an eigenvalue estimate alone will not do:
//   * theta ~ lambda_min(P) from inverse iteration (two triangular solves with B per step; the
//     Rayleigh quotient of P, which is never below lambda_min);
//   * t = theta (1 - 1e-3) is certified by a Cholesky factorisation of P - t I that runs through
//     (then P - t I is positive definite up to the rounding of P and of the factorisation, which
//     `round` below allows for).  P and the factorisation are in long double: lambda_min(P) lies
//     cond(K + sigma_n^2 I) below ||P||, and in double the allowance would swallow the constant of
//     a well-informed model (64 more mantissa bits where long double is the x87 format; `round`
//     follows the format's epsilon, so a host whose long double is double merely gets 0 more
//     often).  A breakdown doubles the step - 1e-3, 2e-3, 4e-3, ... - and after
//     FLOOR_RETRIES of them the constant is 0;
//   * c_s = sigma_n^2 (1 - 1e-3) (t - round): the factor absorbs the rounding of the uploaded
//     factor, sigma_n^2 = 1 / Linv[0][0]^2 - s^2 as in gp4_early_ok (k(x, x) = s^2: RBF).
// 0 means "no floor" - the lower bound err = 0 - and is the answer to every doubt: a non-finite
// entry, a noise that is not positive, a certificate that never succeeds.
//
// Plain C++: g++ compiles it for the tests.
#pragma once

#include <cmath>
#include <limits>
#include <vector>

namespace gpfloor {

constexpr int FLOOR_ITERATIONS = 300;    // inverse iteration: at most this many steps
constexpr int FLOOR_RETRIES = 8;         // certificates tried: theta (1 - 1e-3 2^j), j = 0 .. 7
constexpr double FLOOR_MARGIN = 1e-3;

// sum_j a[j] b[j], four partial sums (the compiler keeps the order of a single one)
template <typename T>
inline T dot4(const T* a, const T* b, int n) {
    T s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    int j = 0;
    for (; j + 4 <= n; j += 4) {
        s0 += a[j] * b[j];
        s1 += a[j + 1] * b[j + 1];
        s2 += a[j + 2] * b[j + 2];
        s3 += a[j + 3] * b[j + 3];
    }
    for (; j < n; ++j) s0 += a[j] * b[j];
    return (s0 + s1) + (s2 + s3);
}

// Cholesky factorisation of the lower triangle of a[k][k] in place; false on a pivot that is not
// positive (or not finite)
inline bool cholesky_runs(std::vector<long double>& a, int k) {
    for (int i = 0; i < k; ++i) {
        long double* ai = &a[(size_t)i * k];
        for (int j = 0; j < i; ++j) {
            const long double* aj = &a[(size_t)j * k];
            ai[j] = (ai[j] - dot4(ai, aj, j)) / aj[j];
        }
        const long double piv = ai[i] - dot4(ai, ai, i);
        if (!(piv > 0.0L) || !(piv < (long double)INFINITY)) return false;
        ai[i] = std::sqrt(piv);
    }
    return true;
}

// A certified lower bound of lambda_min(B^T B) for the lower-triangular B = Linv[m:, m:] of the
// row-major Linv[n][n], or 0.
inline double lambda_min_certified(const double* Linv, int n, int m) {
    const int k = n - m;
    if (k < 1) return 0.0;
    auto B = [&](int r) { return Linv + (size_t)(m + r) * n + m; };     // row r of B: entries 0 .. r
    for (int r = 0; r < k; ++r)
        if (!(B(r)[r] > 0.0)) return 0.0;
    // inverse iteration on P = B^T B: y = B^-1 (B^-T x)
    std::vector<double> x(k), y(k), w(k);
    unsigned state = 12345u;
    for (int i = 0; i < k; ++i) {
        state = state * 1664525u + 1013904223u;
        x[i] = 0.5 + (double)(state >> 8) / (double)(1u << 24);
    }
    double theta = 0.0;
    for (int it = 0; it < FLOOR_ITERATIONS; ++it) {
        double nx = std::sqrt(dot4(x.data(), x.data(), k));
        if (!(nx > 0.0) || !(nx < INFINITY)) return 0.0;
        for (int i = 0; i < k; ++i) w[i] = x[i] = x[i] / nx;
        for (int i = k - 1; i >= 0; --i) {                   // B^T z = x, z in w
            const double* bi = B(i);
            const double zi = w[i] / bi[i];
            w[i] = zi;
            for (int j = 0; j < i; ++j) w[j] -= bi[j] * zi;
        }
        for (int i = 0; i < k; ++i) {                        // B y = z
            const double* bi = B(i);
            y[i] = (w[i] - dot4(bi, y.data(), i)) / bi[i];
        }
        const double yx = dot4(y.data(), x.data(), k), yy = dot4(y.data(), y.data(), k);
        if (!(yx > 0.0) || !(yy > 0.0) || !(yy < INFINITY)) return 0.0;
        const double rq = yx / yy;                           // Rayleigh quotient of P at y
        const bool settled = it > 0 && std::fabs(rq - theta) <= 1e-7 * rq;
        theta = rq;
        x.swap(y);
        if (settled) break;
    }
    // P = B^T B (lower triangle) and ||P||_inf, which bounds lambda_max(P)
    std::vector<long double> P((size_t)k * k, 0.0L), A((size_t)k * k), row(k);
    for (int r = 0; r < k; ++r) {
        const double* br = B(r);
        for (int j = 0; j <= r; ++j) row[j] = br[j];
        for (int i = 0; i <= r; ++i) {
            const long double bri = row[i];
            long double* pi = &P[(size_t)i * k];
            for (int j = 0; j <= i; ++j) pi[j] += bri * row[j];
        }
    }
    long double pnorm = 0.0L;
    for (int i = 0; i < k; ++i) {
        long double sum = 0.0L;
        for (int j = 0; j < k; ++j) sum += std::fabs(j <= i ? P[(size_t)i * k + j] : P[(size_t)j * k + i]);
        pnorm = sum > pnorm ? sum : pnorm;
    }
    if (!(pnorm < (long double)INFINITY)) return 0.0;
    // rounding of the products of P and of the factorisation: each of the order k epsilon ||P||
    const double round = (double)(64.0L * k * std::numeric_limits<long double>::epsilon() * pnorm);
    double step = FLOOR_MARGIN;
    for (int attempt = 0; attempt < FLOOR_RETRIES; ++attempt, step *= 2.0) {
        const double t = theta * (1.0 - step);
        A = P;
        for (int i = 0; i < k; ++i) A[(size_t)i * k + i] -= t;
        if (cholesky_runs(A, k)) return t > round ? t - round : 0.0;
    }
    return 0.0;
}

// floor_c[s], s = 0 .. stages - 1, for the boundaries m = s rp of the factor h_Linv[n][n] of an RBF
// head with prior variance `variance` (stages = ceil(n / rp)).
inline void variance_floor(const double* h_Linv, int n, int rp, int stages, double variance, double* floor_c) {
    for (int s = 0; s < stages; ++s) floor_c[s] = 0.0;
    if (n < 1 || rp < 1 || !(variance > 0.0) || !(variance < INFINITY)) return;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j)
            if (!(std::fabs(h_Linv[(size_t)i * n + j]) < INFINITY)) return;
    const double noise = 1.0 / (h_Linv[0] * h_Linv[0]) - variance;
    if (!(noise > 0.0) || !(noise < INFINITY)) return;
    for (int s = 0; s < stages && s * rp < n; ++s) {
        const double c = noise * (1.0 - FLOOR_MARGIN) * lambda_min_certified(h_Linv, n, s * rp);
        floor_c[s] = (c > 0.0 && c < 1.0) ? c : 0.0;
    }
}

}  // namespace gpfloor
