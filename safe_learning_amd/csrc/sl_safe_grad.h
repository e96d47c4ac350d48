// sl_safe_grad.h - per-point arithmetic of the action derivative of the Lyapunov penalty of
// PolicyIteration.future_values (safe_learning/reinforcement_learning.py:107-112; the
// `rl.future_values(tf_states, lyapunov=lyapunov)` of examples/inverted_pendulum.ipynb cell 17), shared by the
// kernels of sl_safe_grad.hip and the host tests.
//
//   C(x, u)  = V_L(mu) - V_L(x) + sum_k L_k(mu) e_k + |L(x)|_1 (1 + L_f(x)) tau       (decrease - threshold)
//   e_k      = beta sqrt(var_h),  var_h = k(z, z) - |a|^2,  a = L^-1 k_x               (functions.py:438-456, 507-515)
//   dC/du_a  = sum_j [g_j(mu) + sum_k dL_k/dmu_j(mu) e_k] J_ja + sum_k L_k(mu) beta dvar_h/du_a / (2 sqrt(var_h))
//   dvar_h/du_a = dk(z, z)/du_a - 2 a^T b_a,  b_a = L^-1 dk_x/du_a
//
// z = [x, u], mu and J = dmu/du the dynamics mean and its action Jacobian of sl_policy_grad.h (sl_pg_head,
// sl_pg_linear_part), the kernel values and derivatives those of sl_pg_rbf / sl_pg_kernel.  The threshold sees
// x only and adds nothing to dC/du.  sqrt(var) is not clamped (the sweeps and the reference do not clamp
// either): a variance <= 0 gives NaN or inf.
//
// One rounding per operation, in the order written here (the library is built without contraction); where a
// fused operation is meant it is written fma().  Plain C++ on scalars: g++ compiles it for the tests.
#pragma once

#include "sl_policy_grad.h"

// ---- k(z, z) as sl_kernel_diag states it, and its total derivative with respect to the action columns ----
// Stationary factor: the variance, derivative 0.  Linear factor: sum_q variance_q z_q^2, derivative
// (2 variance_q) z_q.  Sums and products by the product rule of sl_pg_kernel.
SL_HD double sl_sg_kernel_diag(const sl_gp_kernel& ks, int p, int d, int m, const double* z, double* dk) {
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
        double v = fac.variance[0], dv[SL_M];
#pragma unroll
        for (int c = 0; c < SL_M; ++c) dv[c] = 0.0;
        if (fac.kind == SL_KERNEL_LINEAR) {
            v = 0.0;
#pragma unroll
            for (int q = 0; q < SL_P; ++q) {
                if (q < p) {
                    v = fma(z[q] * z[q], fac.variance[q], v);
#pragma unroll
                    for (int c = 0; c < SL_M; ++c)
                        if (c < m && q == d + c) dv[c] = (2.0 * fac.variance[q]) * z[q];
                }
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

// prior variance k(z, z) of a head and its action derivative (an RBF head of sl_gp_set_head: the variance, 0)
SL_HD double sl_sg_prior(const SlPgHead& hd, int p, int d, int m, const double* z, double* dprior) {
#pragma unroll
    for (int c = 0; c < SL_M; ++c) dprior[c] = 0.0;
    if (!hd.kernel) return hd.variance;
    return sl_sg_kernel_diag(*hd.kernel, p, d, m, z, dprior);
}

// var = k(z, z) - sum a^2 and dvar_c = dk(z, z)/du_c - 2 sum a b_c, from the two sums of the triangular product
SL_HD double sl_sg_variance(double prior, const double* dprior, double ss, const double* sab, int m, double* dvar) {
#pragma unroll
    for (int c = 0; c < SL_M; ++c) {
        if (c < m) {
            const double t = 2.0 * sab[c];
            dvar[c] = dprior[c] - t;
        }
    }
    return prior - ss;
}

// The two sums of one head at one point on scalars: a_i = sum_{j <= i} Linv[i][j] k_j and b_ci likewise from
// dk_j/du_c (fma, ascending j), ss = sum_i a_i^2, sab_c = sum_i a_i b_ci (fma, ascending i).  The kernels of
// sl_safe_grad.hip form the same products on the matrix cores, the same sums in another order.
// linv: [n][n] row-major (lower triangle read); kx, dkx: work space of n and n * SL_M doubles.
SL_HD void sl_sg_head_sums(const SlPgHead& hd, const double* linv, int p, int d, int m, const double* z, double* kx,
                           double* dkx, double* ss, double* sab) {
    double xg[SL_P];
#pragma unroll
    for (int q = 0; q < SL_P; ++q) xg[q] = (q < p) ? z[q] * hd.inv_ls[q] : 0.0;
    for (int j = 0; j < hd.n; ++j) {
        double xa[SL_P], dk[SL_M];
#pragma unroll
        for (int q = 0; q < SL_P; ++q) xa[q] = (q < p) ? hd.xs[q * hd.n_pad + j] : 0.0;
#pragma unroll
        for (int c = 0; c < SL_M; ++c) dk[c] = 0.0;
        kx[j] = hd.kernel ? sl_pg_kernel(*hd.kernel, p, d, m, xa, xg, dk)
                          : sl_pg_rbf(hd.variance, hd.inv_ls, p, d, m, xa, xg, dk);
#pragma unroll
        for (int c = 0; c < SL_M; ++c) dkx[j * SL_M + c] = dk[c];
    }
    *ss = 0.0;
#pragma unroll
    for (int c = 0; c < SL_M; ++c) sab[c] = 0.0;
    for (int i = 0; i < hd.n; ++i) {
        double a = 0.0, b[SL_M];
#pragma unroll
        for (int c = 0; c < SL_M; ++c) b[c] = 0.0;
        for (int j = 0; j <= i; ++j) {
            const double l = linv[(size_t)i * hd.n + j];
            a = fma(l, kx[j], a);
#pragma unroll
            for (int c = 0; c < SL_M; ++c) if (c < m) b[c] = fma(l, dkx[j * SL_M + c], b[c]);
        }
        *ss = fma(a, a, *ss);
#pragma unroll
        for (int c = 0; c < SL_M; ++c) if (c < m) sab[c] = fma(a, b[c], sab[c]);
    }
}

// ---- V_L, L_v and their derivatives at one state ---------------------------------------------------------
// value: V_L(s).  lv: L_v(s) as the sweeps compute it (sl_lv; |simplex gradient| for the gradient kinds over a
// table).  With `derivatives` (the successor) also
//   g[j]    = dV_L/ds_j: (P + P^T) s for a quadratic; the simplex gradient for a table, negated with the value
//             and masked per coordinate where the table projects (as sl_pg_point masks the value table's)
//   sgn[k]  = sign of the term under the abs of row k of the L_v matrix (0 at 0, TensorFlow's gradient of abs);
//             all 0 for the kinds whose derivative is 0 (a constant; gradient kinds over a table, whose simplex
//             gradient is piecewise constant)
SL_HD double sl_sg_value_lv(const SlDevModel& M, const SlTri& vt, int d, const double* s, double* lv, bool derivatives,
                            double* g, double* sgn) {
    const sl_lipschitz_desc& l = M.m.lipschitz;
    const int kind = l.lv_kind;
    const bool grad_kind = kind == SL_LIP_ABS_GRAD || kind == SL_LIP_NORM_GRAD;
    double value;
    double c[SL_D];
#pragma unroll
    for (int k = 0; k < SL_D; ++k) { c[k] = 0.0; if (derivatives) sgn[k] = 0.0; }
    if (M.m.value.kind == SL_V_QUADRATIC) {
        value = sl_quadratic(M.m.value, d, s);
        if (derivatives) {
#pragma unroll
            for (int j = 0; j < SL_D; ++j) if (j < d) g[j] = sl_pg_quadratic_grad(M.m.value, d, s, j);
        }
    } else {
        value = sl_tri_eval(vt, s, 0, c);
        if (M.m.value.negate) value = value * -1.0;
#pragma unroll
        for (int k = 0; k < SL_D; ++k) {
            if (k < d) {
                c[k] = M.m.value.negate ? (c[k] * -1.0) : c[k];
                if (derivatives) {
                    double ck = c[k];
                    if (vt.project) {
                        const bool inside = s[k] >= vt.grid.offset[k] && s[k] <= vt.grid.upper[k];
                        ck = inside ? ck : 0.0;
                    }
                    g[k] = ck;
                }
            }
        }
    }
    if (!grad_kind) {
        sl_lv(M, d, s, lv);
        if (derivatives && kind != SL_LIP_CONST) {
            double t[SL_D];
            sl_rows_dot<SL_D, SL_D>(l.lv_matrix, d, d, s, t);
#pragma unroll
            for (int k = 0; k < SL_D; ++k) if (k < d) sgn[k] = t[k] > 0.0 ? 1.0 : (t[k] < 0.0 ? -1.0 : 0.0);
        }
    } else if (kind == SL_LIP_ABS_GRAD) {
#pragma unroll
        for (int k = 0; k < SL_D; ++k) if (k < d) lv[k] = fabs(c[k]);
    } else {
        double acc = fabs(c[0]);
#pragma unroll
        for (int k = 1; k < SL_D; ++k) if (k < d) acc = acc + fabs(c[k]);
        lv[0] = acc;
    }
    return value;
}

// ---- one point: everything after the dynamics and the variances ----------------------------------------------
// x [d]; mean[k], jac[k][a] as sl_pg_point takes them; var[k], dvar[k][a]: the posterior variance of the head that
// owns output column k and its action derivative.  Writes err[k] = beta sqrt(var[k]) and grad[a] = dC/du_a.
//   s_k = sqrt(var_k), e_k = beta s_k, de_ka = (beta dvar_ka) / (2 s_k)
//   w_j = sum_k e_k sgn_k G_kj (per-column L_v)  or  (sum_k e_k) (sum_k sgn_k G_kj) (one-column L_v), left to right
//   grad_a = [sum_j (g_j + w_j) J_ja] + [sum_k L_k de_ka], both left to right
struct SlSgPoint { double constraint, decrease, threshold; };
SL_HD SlSgPoint sl_sg_point(const SlDevModel& M, const SlTri& vt, double beta, int d, int m, const double* x,
                            const double* mean, const double (*jac)[SL_M], const double* var,
                            const double (*dvar)[SL_M], double* err, double* grad) {
    const sl_lipschitz_desc& l = M.m.lipschitz;
    const bool bcast = !(l.lv_kind == SL_LIP_ABS_LINEAR || l.lv_kind == SL_LIP_ABS_GRAD) || d == 1;
    double de[SL_D][SL_M];
#pragma unroll
    for (int k = 0; k < SL_D; ++k) {
        if (k < d) {
            const double s = sqrt(var[k]);
            err[k] = beta * s;
            const double den = 2.0 * s;
#pragma unroll
            for (int a = 0; a < SL_M; ++a) {
                if (a < m) {
                    const double t = beta * dvar[k][a];
                    de[k][a] = t / den;
                }
            }
        }
    }
    double lv_x[SL_D], lv_n[SL_D], g[SL_D], sgn[SL_D];
    const double v_x = sl_sg_value_lv(M, vt, d, x, lv_x, false, nullptr, nullptr);
    const double v_n = sl_sg_value_lv(M, vt, d, mean, lv_n, true, g, sgn);
    SlSgPoint r;
    r.decrease = sl_decrease(M, d, v_x, v_n, lv_n, err);
    r.threshold = sl_threshold(M, d, lv_x, l.tau, x);
    r.constraint = r.decrease - r.threshold;
    // w_j: the derivative of L_v(mu) through the abs, times the errors
    double w[SL_D], esum = err[0];
#pragma unroll
    for (int k = 1; k < SL_D; ++k) if (k < d) esum = esum + err[k];
#pragma unroll
    for (int j = 0; j < SL_D; ++j) {
        if (j < d) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < SL_D; ++k) {
                if (k < d) {
                    const double sg = sgn[k] * l.lv_matrix[k][j];
                    const double t = bcast ? sg : (err[k] * sg);
                    acc = (k == 0) ? t : (acc + t);
                }
            }
            w[j] = bcast ? (esum * acc) : acc;
        }
    }
#pragma unroll
    for (int a = 0; a < SL_M; ++a) {
        if (a < m) {
            double chain = 0.0, spread = 0.0;
#pragma unroll
            for (int j = 0; j < SL_D; ++j) {
                if (j < d) {
                    const double cj = g[j] + w[j];
                    const double t = cj * jac[j][a];
                    chain = (j == 0) ? t : (chain + t);
                    const double lk = bcast ? lv_n[0] : lv_n[j];
                    const double u = lk * de[j][a];
                    spread = (j == 0) ? u : (spread + u);
                }
            }
            grad[a] = chain + spread;
        }
    }
    return r;
}
