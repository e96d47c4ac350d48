// sl_policy_grad.h - per-point arithmetic of the policy gradient of PolicyIteration.future_values
// (safe_learning/reinforcement_learning.py:65-114 differentiated with respect to the action), shared by
// the kernels of sl_policy_grad.hip and the host tests.
//
//   Q(x, u) = r(z) + gamma V(mu(z)),  z = [x, u]
//   dQ/du_a = [(P + P^T) z]_{d+a} + gamma sum_k c_k dmu_k/du_a
//
// with r the quadratic reward, mu the dynamics mean (a LinearSystem, or the GP posterior mean plus its
// linear prior) and c the gradient of the value Triangulation's simplex at the successor, masked where
// the table projects the successor onto its grid (functions.py:1485: tf.minimum(tf.maximum(x, lo), hi)
// passes the gradient inside the limits and on them, and gives 0 strictly outside).
//
// One rounding per operation, in the order written here (the library is built without contraction);
// where a fused operation is meant it is written fma(), as sl_kernel_eval does for the kernel value -
// the kernel values below are sl_kernel_eval's and sl_next_state_mean's, operation for operation, so
// the successor this header leads to is the one the Bellman sweeps interpolate at.
//
// The activation and kernel derivatives live here and not among the shared routines of sl_model.h:
// the sweeps' kernels never see them (their register allocation stays what it was).
//
// Plain C++ on scalars: g++ compiles it for the tests.
#pragma once

#include "sl_model.h"

// ---- activations of a NeuralNetwork policy (sl_policy_network_set: 0 none, 1 tanh, 2 relu, 3 sigmoid)
// derivative from the layer's OUTPUT, as TensorFlow's gradients take it: relu' = 1 where the output (and
// with it the pre-activation) is > 0, tanh' = 1 - h^2, sigmoid' = h (1 - h)
SL_HD double sl_pg_dact(int a, double post) {
    if (a == 1) { const double sq = post * post; return 1.0 - sq; }
    if (a == 2) return post > 0.0 ? 1.0 : 0.0;
    if (a == 3) { const double om = 1.0 - post; return post * om; }
    return 1.0;
}

// ---- reward: d(z P z^T)/dz_q = sum_i z_i (P[i][q] + P[q][i]), left to right ------------------------
SL_HD double sl_pg_quadratic_grad(const sl_value_desc& v, int n, const double* z, int q) {
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < SL_P; ++i) {
        if (i < n) {
            const double s = v.matrix[i][q] + v.matrix[q][i];
            const double t = z[i] * s;
            acc = (i == 0) ? t : (acc + t);
        }
    }
    return v.negate ? (acc * -1.0) : acc;
}

// ---- GP kernels: k(a, z) and dk/dz_q for the action columns q = d .. d + m - 1 --------------------
// RBF head of sl_gp_set_head: xa = a / lengthscales (as stored), xg = z / lengthscales.
//   k = variance exp(-r2 / 2),  dk/dz_q = k (xa_q - xg_q) inv_ls_q      - the one exponential serves both
SL_HD double sl_pg_rbf(double variance, const double* inv_ls, int p, int d, int m, const double* xa,
                       const double* xg, double* dk) {
    double r2 = 0.0;
#pragma unroll
    for (int q = 0; q < SL_P; ++q) {
        if (q < p) {
            const double dlt = xa[q] - xg[q];
            r2 = fma(dlt, dlt, r2);
        }
    }
    const double k = variance * sl_exp_nonpos(-0.5 * r2);
#pragma unroll
    for (int a = 0; a < SL_M; ++a) {
        if (a < m) {
            double dlt = 0.0, il = 0.0;
#pragma unroll
            for (int q = 0; q < SL_P; ++q)
                if (q == d + a) { dlt = xa[q] - xg[q]; il = inv_ls[q]; }
            const double t = k * dlt;
            dk[a] = t * il;
        }
    }
    return k;
}

// Sum-of-products kernel of sl_gp_set_head_kernel (unscaled inputs): the value as sl_kernel_eval
// computes it, and its derivative by the product rule over the factors of a product,
//   (v_1 .. v_F)' = sum_f v_f' prod_{g != f} v_g   carried as  dprod <- dprod v_f + prod v_f',
// summed over the products.  Factor derivatives with respect to z_q (a the training point):
//   Linear    variance_q a_q
//   RBF       k (a_q - z_q) inv_ls_q^2
//   Matern32  3 variance e^{-s} (a_q - z_q) inv_ls_q^2,  s = sqrt(3) sqrt(r2 + 1e-12)  (smooth at r = 0)
SL_HD double sl_pg_kernel(const sl_gp_kernel& ks, int p, int d, int m, const double* a, const double* z,
                          double* dk) {
    double total = 0.0, prod = 1.0;
    double dtotal[SL_M], dprod[SL_M];
#pragma unroll
    for (int c = 0; c < SL_M; ++c) { dtotal[c] = 0.0; dprod[c] = 0.0; }
    int cur = 0;
    for (int f = 0; f < ks.nfactors; ++f) {
        const sl_gp_kernel_factor& fac = ks.factor[f];
        if (fac.product != cur) {
            total += prod;
            prod = 1.0;
#pragma unroll
            for (int c = 0; c < SL_M; ++c) { dtotal[c] = dtotal[c] + dprod[c]; dprod[c] = 0.0; }
            cur = fac.product;
        }
        double v = 0.0, dv[SL_M];
#pragma unroll
        for (int c = 0; c < SL_M; ++c) dv[c] = 0.0;
        if (fac.kind == SL_KERNEL_LINEAR) {
#pragma unroll
            for (int q = 0; q < SL_P; ++q) {
                if (q < p) {
                    const double av = a[q] * fac.variance[q];
                    v = fma(av, z[q], v);
#pragma unroll
                    for (int c = 0; c < SL_M; ++c)
                        if (c < m && q == d + c) dv[c] = av;
                }
            }
        } else {
            double r2 = 0.0, w[SL_M];
#pragma unroll
            for (int c = 0; c < SL_M; ++c) w[c] = 0.0;
#pragma unroll
            for (int q = 0; q < SL_P; ++q) {
                if (q < p) {
                    const double il = fac.inv_lengthscales[q];
                    const double dlt = a[q] - z[q];
                    const double dq = dlt * il;
                    r2 = fma(dq, dq, r2);
#pragma unroll
                    for (int c = 0; c < SL_M; ++c)
                        if (c < m && q == d + c) w[c] = dq * il;        // (a_q - z_q) inv_ls_q^2
                }
            }
            if (fac.kind == SL_KERNEL_RBF) {
                v = fac.variance[0] * sl_exp_nonpos(-0.5 * r2);
#pragma unroll
                for (int c = 0; c < SL_M; ++c) if (c < m) dv[c] = v * w[c];
            } else {                                    // Matern32, euclid_dist's 1e-12
                const double r = 1.7320508075688772 * sqrt(r2 + 1e-12);
                const double e = sl_exp_nonpos(-r);
                v = fac.variance[0] * (1.0 + r) * e;
                const double g = (3.0 * fac.variance[0]) * e;
#pragma unroll
                for (int c = 0; c < SL_M; ++c) if (c < m) dv[c] = g * w[c];
            }
        }
#pragma unroll
        for (int c = 0; c < SL_M; ++c) {
            if (c < m) {
                const double t0 = dprod[c] * v, t1 = prod * dv[c];
                dprod[c] = t0 + t1;
            }
        }
        prod *= v;
    }
#pragma unroll
    for (int c = 0; c < SL_M; ++c) if (c < m) dk[c] = dtotal[c] + dprod[c];
    return total + prod;
}

// ---- one point: everything after the dynamics --------------------------------------------------------
// mean[k] = mu_k(z) and jac[k][a] = dmu_k/du_a are the caller's (sl_pg_head and sl_pg_linear_part below).  Returns Q; grad[a] = dQ/du_a.
//   c = simplex gradient of the value table at the successor (sl_tri_eval: located from the unclipped
//   point, functions.py:1461), negated with the value, masked per coordinate when the table projects
//   t_a = sum_k (c_k * jac[k][a]), left to right;  grad_a = dr_a + gamma * t_a
SL_HD double sl_pg_point(const sl_value_desc& reward, const sl_value_desc& value, double gamma, const SlTri& vt,
                         int d, int m, const double* z, const double* mean, const double (*jac)[SL_M],
                         double* grad) {
    const int p = d + m;
    double c[SL_D];
    double v = sl_tri_eval(vt, mean, 0, c);
    if (value.negate) v = v * -1.0;
#pragma unroll
    for (int k = 0; k < SL_D; ++k) {
        if (k < d) {
            double ck = value.negate ? (c[k] * -1.0) : c[k];
            if (vt.project) {
                const bool inside = mean[k] >= vt.grid.offset[k] && mean[k] <= vt.grid.upper[k];
                ck = inside ? ck : 0.0;
            }
            c[k] = ck;
        }
    }
    const double r = sl_quadratic(reward, p, z);
    const double t = gamma * v;
#pragma unroll
    for (int a = 0; a < SL_M; ++a) {
        if (a < m) {
            double q = 0.0;
#pragma unroll
            for (int qq = 0; qq < SL_P; ++qq) if (qq == d + a) q = sl_pg_quadratic_grad(reward, p, z, qq);
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < SL_D; ++k) {
                if (k < d) {
                    const double tk = c[k] * jac[k][a];
                    acc = (k == 0) ? tk : (acc + tk);
                }
            }
            const double ga = gamma * acc;
            grad[a] = q + ga;
        }
    }
    return r + t;                                                // reinforcement_learning.py:104
}

// A GP head as plain arrays (the host tests hand them in; the kernel builds one from SlGpHeadDev)
struct SlPgHead {
    int n, n_pad, dout, col0;
    double variance;
    const double* inv_ls;          // [p] (RBF head; ones for a kernel description)
    const double* xs;              // [p][n_pad]
    const double* alpha;           // [n][dout]  alpha' = Linv^T alpha
    const sl_gp_kernel* kernel;    // or null: RBF head with pre-scaled inputs
};

// mean += sum_j k_j alpha'_j (fma, ascending j: sl_next_state_mean's sum) and
// jac[k][a] += sum_j dk_j/du_a alpha'_jk (fma, ascending j) for the columns the head owns
SL_HD void sl_pg_head(const SlPgHead& hd, int p, int d, int m, const double* z, double* mean,
                      double (*jac)[SL_M]) {
    double xg[SL_P];
#pragma unroll
    for (int q = 0; q < SL_P; ++q) xg[q] = (q < p) ? z[q] * hd.inv_ls[q] : 0.0;
    for (int j = 0; j < hd.n; ++j) {
        double xa[SL_P], dk[SL_M];
#pragma unroll
        for (int q = 0; q < SL_P; ++q) xa[q] = (q < p) ? hd.xs[q * hd.n_pad + j] : 0.0;
        const double kx = hd.kernel ? sl_pg_kernel(*hd.kernel, p, d, m, xa, xg, dk)
                                    : sl_pg_rbf(hd.variance, hd.inv_ls, p, d, m, xa, xg, dk);
#pragma unroll
        for (int k = 0; k < SL_D; ++k) {
            const int dd = k - hd.col0;
            if (k < d && dd >= 0 && dd < hd.dout) {
                const double al = hd.alpha[j * hd.dout + dd];
                mean[k] = fma(kx, al, mean[k]);
#pragma unroll
                for (int a = 0; a < SL_M; ++a)
                    if (a < m) jac[k][a] = fma(dk[a], al, jac[k][a]);
            }
        }
    }
}

// after the heads: the linear part (SL_DYN_LINEAR: the dynamics; SL_DYN_GP: the prior mean)
//   mean_k <- mean_k + (z . M[k]),  jac[k][a] <- jac[k][a] + M[k][d + a]
SL_HD void sl_pg_linear_part(const sl_dynamics_desc& f, int d, int m, const double* z, double* mean,
                             double (*jac)[SL_M]) {
    double lin[SL_D];
    sl_rows_dot<SL_D, SL_P>(f.matrix, d, d + m, z, lin);
#pragma unroll
    for (int k = 0; k < SL_D; ++k) {
        if (k < d) {
            mean[k] = mean[k] + lin[k];
#pragma unroll
            for (int a = 0; a < SL_M; ++a) {
                if (a < m) {
                    double col = 0.0;
#pragma unroll
                    for (int q = 0; q < SL_P; ++q) if (q == d + a) col = f.matrix[k][q];
                    jac[k][a] = jac[k][a] + col;
                }
            }
        }
    }
}

// ---- the table look-up as (vertex, weight) pairs -----------------------------------------------------
// sl_tri_eval's own point location and weights (rectangle from the unclipped point, the unit-cell simplex
// whose smallest barycentric weight is largest, weights from the projected point when the table
// projects), written out again so that the sweeps' routine stays as it is: the interpolant is
// sum_k w[k] table[vert[k]] with w[0] = 1 - (w[1] + ... + w[d]).
SL_HD void sl_pg_tri_locate(const SlTri& t, const double* x, int64_t* vert, double* w) {
    const int d = t.grid.d;
    const double eps2 = 2.0 * 2.220446049250313e-16;
    int64_t corner = 0;
    int64_t rk[SL_D];
    double unitc[SL_D], xc[SL_D];
#pragma unroll
    for (int k = 0; k < SL_D; ++k) {
        if (k < d) {
            const int64_t r = sl_rectangle_1d(t, k, x[k]);
            rk[k] = r;
            corner += r * t.stride[k];
            double c = x[k] - t.grid.offset[k];
            const double lo = 0.0 + eps2, hi = (t.grid.upper[k] - t.grid.offset[k]) - eps2;
            c = (c < lo) ? lo : c;
            c = (c > hi) ? hi : c;
            unitc[k] = sl_fmod_pos(c, t.grid.unit_maxes[k]);
            double p = x[k];
            if (t.project) {
                p = (p > t.grid.offset[k]) ? p : t.grid.offset[k];
                p = (p < t.grid.upper[k]) ? p : t.grid.upper[k];
            }
            xc[k] = p;
        }
    }
    int best = 0;
    double best_min = -1e300;
    for (int s = 0; s < t.nsimplex; ++s) {
        double w0 = 1.0, wmin = 1e300;
        double org[SL_D];
#pragma unroll
        for (int k = 0; k < SL_D; ++k)
            if (k < d) org[k] = ((t.simplices[s][0] >> k) & 1) ? t.grid.unit_maxes[k] : 0.0;
#pragma unroll
        for (int j = 0; j < SL_D; ++j) {
            if (j < d) {
                double ww = 0.0;
#pragma unroll
                for (int k = 0; k < SL_D; ++k)
                    if (k < d) ww += (unitc[k] - org[k]) * t.hyper[s][k][j];
                w0 -= ww;
                wmin = (ww < wmin) ? ww : wmin;
            }
        }
        wmin = (w0 < wmin) ? w0 : wmin;
        if (wmin > best_min) { best_min = wmin; best = s; }
    }
    int64_t v0 = corner;
    double org[SL_D];
#pragma unroll
    for (int k = 0; k < SL_D; ++k) {
        if (k < d) {
            const int bit = (t.simplices[best][0] >> k) & 1;
            v0 += bit * t.stride[k];
            const double tt = (double)(rk[k] + bit) * t.grid.unit_maxes[k];
            org[k] = tt + t.grid.offset[k];
        }
    }
    double wsum = 0.0;
#pragma unroll
    for (int j = 0; j < SL_D; ++j) {
        if (j < d) {
            double ww = 0.0;
#pragma unroll
            for (int k = 0; k < SL_D; ++k)
                if (k < d) ww += (xc[k] - org[k]) * t.hyper[best][k][j];
            int64_t vj = corner;
#pragma unroll
            for (int k = 0; k < SL_D; ++k)
                if (k < d) vj += ((t.simplices[best][j + 1] >> k) & 1) * t.stride[k];
            vert[j + 1] = vj;
            w[j + 1] = ww;
            wsum += ww;
        }
    }
    vert[0] = v0;
    w[0] = 1.0 - wsum;
}
