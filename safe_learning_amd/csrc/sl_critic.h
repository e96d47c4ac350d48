// sl_critic.h - per-sample arithmetic of the actor-critic steps of examples/reinforcement_learning_pendulum.ipynb
// (cells 16, 31, 34, 48) and examples/reinforcement_learning_cartpole.ipynb (cell 15), shared by k_critic_batch
// (sl_critic.hip) and the host tests.  Policy and value function are NeuralNetworks, the dynamics the true
// Euler models (or a LinearSystem):
//
//   u = pi(x),  x+ = f(x, u),  z = [x, u]
//   r = z P z^T,  q = r + gamma V(x+)                         the target of the critic, the objective of the actor
//   dq/du_a = [(P + P^T) z]_{d+a} + gamma sum_k g_k dx+_k/du_a,   g = dV/dx at x+
//   delta = V(x) - q,  coefficient c = w sign(delta), sign(0) = 0  (TensorFlow's gradient of abs)
//
// One rounding per operation, in the order written here (the library is built without contraction); where a
// fused operation is meant it is written fma().  The primal sequences of the Euler dynamics are sl_pendulum and
// sl_cartpole of sl_model.h operation for operation, so x+ is the successor every other kernel computes; the
// tangent dx+/du (m = 1) is carried in forward mode through the same ten sub-steps, every derivative written
// next to the primal operation it belongs to.  The dense network's dot products are the fma chains of
// k_policy_network and k_policy_param_grad (ascending input index from 0, then the bias), so V is the value the
// point kernels return for the same network as a policy.
//
// Plain C++ on scalars: g++ compiles it for the tests.  A network is any struct with the fields of SlPolicyNet
// (nlayers, dims, act, koff, boff, scale, params): the kernels hand in that struct, the host tests their own.
#pragma once

#include "sl_policy_grad.h"

#ifndef SL_NN_MAXW
#define SL_NN_MAXW 64
#endif

// ---- Euler dynamics with their action tangent ------------------------------------------------------------
// pendulum: d th/du, d om/du through th' = th + dt om, om' = om + dt (g/l sin th + act / I - fr om)
SL_HD void sl_pendulum_du(const sl_dynamics_desc& f, const double* x, const double* u, double* nxt, double* dnx) {
    double th = x[0], om = x[1], act = u[0];
    double gth = 0.0, gom = 0.0, gact = 1.0;
    if (f.normalize) { th = th * f.tx[0]; om = om * f.tx[1]; act = act * f.tu[0]; gact = f.tu[0]; }
    const double dt = f.coef[0];
    const double gt2 = gact / f.coef[2];
    for (int it = 0; it < 10; ++it) {
        double sth, cth;
        sl_sincos(th, &sth, &cth);
        double acc = f.coef[1] * sth;
        double gs = cth * gth;                           // d sin(th)
        double gacc = f.coef[1] * gs;
        double t2 = act / f.coef[2];
        acc = acc + t2;
        gacc = gacc + gt2;
        if (f.coef[4] != 0.0) {
            double t3 = f.coef[3] * om;
            acc = acc - t3;
            double g3 = f.coef[3] * gom;
            gacc = gacc - g3;
        }
        double dth = dt * om;
        double dom = dt * acc;
        double gdth = dt * gom;
        double gdom = dt * gacc;
        th = th + dth;
        om = om + dom;
        gth = gth + gdth;
        gom = gom + gdom;
    }
    if (f.normalize) {
        th = th * f.tx_inv[0]; om = om * f.tx_inv[1];
        gth = gth * f.tx_inv[0]; gom = gom * f.tx_inv[1];
    }
    nxt[0] = th; nxt[1] = om;
    dnx[0] = gth; dnx[1] = gom;
}

// cart-pole: both accelerations are quotients n / det, (n / det)' = (n' - (n / det) det') / det
SL_HD void sl_cartpole_du(const sl_dynamics_desc& f, const double* x, const double* u, double* nxt, double* dnx) {
    double px = x[0], th = x[1], v = x[2], om = x[3], act = u[0];
    double gpx = 0.0, gth = 0.0, gv = 0.0, gom = 0.0, gact = 1.0;
    if (f.normalize) {
        px = px * f.tx[0]; th = th * f.tx[1]; v = v * f.tx[2]; om = om * f.tx[3];
        act = act * f.tu[0];
        gact = f.tu[0];
    }
    const double dt = f.coef[0], m = f.coef[1], M = f.coef[2], L = f.coef[3], b = f.coef[4];
    for (int it = 0; it < 10; ++it) {
        double s, c;
        sl_sincos(th, &s, &c);
        double gs = c * gth;                             // d sin, d cos from the primal's own s, c
        double gc = -(s * gth);
        double s2 = 2.0 * (s * c);                   // sin(2 theta)
        double gs2 = 2.0 * ((gs * c) + (s * gc));
        double om2 = om * om;
        double gom2 = 2.0 * (om * gom);
        double det = m * (s * s);
        det = M + det;
        det = L * det;
        double gdet = L * (m * (2.0 * (s * gs)));
        double t1 = (f.coef[5] * om2) * s;
        double g1 = ((f.coef[5] * gom2) * s) + ((f.coef[5] * om2) * gs);
        double t2 = (b * om) * c;
        double g2 = ((b * gom) * c) + ((b * om) * gc);
        double t3 = f.coef[6] * s2;
        double g3 = f.coef[6] * gs2;
        double vd = act - t1;
        vd = vd - t2;
        vd = vd + t3;
        vd = vd * L;
        vd = vd / det;
        double gvd = gact - g1;
        gvd = gvd - g2;
        gvd = gvd + g3;
        gvd = gvd * L;
        gvd = gvd - (vd * gdet);
        gvd = gvd / det;
        double w1 = act * c;
        double h1 = (gact * c) + (act * gc);
        double w2 = (f.coef[7] * om2) * s2;
        double h2 = ((f.coef[7] * gom2) * s2) + ((f.coef[7] * om2) * gs2);
        double w3 = (f.coef[8] * om) / f.coef[5];
        double h3 = (f.coef[8] * gom) / f.coef[5];
        double w4 = f.coef[9] * s;
        double h4 = f.coef[9] * gs;
        double wd = w1 - w2;
        wd = wd - w3;
        wd = wd + w4;
        wd = wd / det;
        double gwd = h1 - h2;
        gwd = gwd - h3;
        gwd = gwd + h4;
        gwd = gwd - (wd * gdet);
        gwd = gwd / det;
        double dpx = dt * v, dth = dt * om, dv = dt * vd, dom = dt * wd;
        double gdpx = dt * gv, gdth = dt * gom, gdv = dt * gvd, gdom = dt * gwd;
        px = px + dpx; th = th + dth; v = v + dv; om = om + dom;
        gpx = gpx + gdpx; gth = gth + gdth; gv = gv + gdv; gom = gom + gdom;
    }
    if (f.normalize) {
        px = px * f.tx_inv[0]; th = th * f.tx_inv[1]; v = v * f.tx_inv[2]; om = om * f.tx_inv[3];
        gpx = gpx * f.tx_inv[0]; gth = gth * f.tx_inv[1]; gv = gv * f.tx_inv[2]; gom = gom * f.tx_inv[3];
    }
    nxt[0] = px; nxt[1] = th; nxt[2] = v; nxt[3] = om;
    dnx[0] = gpx; dnx[1] = gth; dnx[2] = gv; dnx[3] = gom;
}

// x+ = f(z) and jac[k][a] = dx+_k/du_a for the dynamics kind DYN (a compile-time value in the kernels).
// SL_DYN_LINEAR: sl_dynamics_det's rows and the action columns of the matrix.
template <int DYN>
SL_HD void sl_critic_dynamics(const sl_dynamics_desc& f, int d, int m, const double* z, double* nxt,
                              double (*jac)[SL_M]) {
    if (DYN == SL_DYN_PENDULUM || DYN == SL_DYN_CARTPOLE) {
        double u0 = 0.0, dnx[SL_D];
#pragma unroll
        for (int q = 0; q < SL_P; ++q) if (q == d) u0 = z[q];
        if (DYN == SL_DYN_PENDULUM) sl_pendulum_du(f, z, &u0, nxt, dnx); else sl_cartpole_du(f, z, &u0, nxt, dnx);
#pragma unroll
        for (int k = 0; k < SL_D; ++k) if (k < d) jac[k][0] = dnx[k];
        return;
    }
    sl_rows_dot<SL_D, SL_P>(f.matrix, d, d + m, z, nxt);
#pragma unroll
    for (int k = 0; k < SL_D; ++k) {
        if (k < d) {
#pragma unroll
            for (int a = 0; a < SL_M; ++a) {
                if (a < m) {
                    double col = 0.0;
#pragma unroll
                    for (int q = 0; q < SL_P; ++q) if (q == d + a) col = f.matrix[k][q];
                    jac[k][a] = col;
                }
            }
        }
    }
}

// ---- dense value network (the layout and activation codes of sl_policy_network_set) -----------------------
SL_HD double sl_critic_act(int a, double x) {
    if (a == 1) return sl_tanh(x);
    if (a == 2) return x > 0.0 ? x : 0.0;
    if (a == 3) return 1.0 / (1.0 + exp(-x));
    return x;
}

// V(x) = scale h_L; h[l] = the OUTPUT of layer l (what the transposed chain needs: the activation derivatives
// are taken from the outputs, sl_pg_dact)
template <class NET>
SL_HD double sl_critic_forward(const NET& net, const double* x, double (*h)[SL_NN_MAXW]) {
    const int L = net.nlayers;
    for (int l = 0; l < L; ++l) {
        const int in = net.dims[l], out = net.dims[l + 1];
        const double* K = net.params + net.koff[l];                // [in][out]
        const double* bias = net.boff[l] >= 0 ? net.params + net.boff[l] : nullptr;
        const double* src = l == 0 ? x : h[l - 1];
        for (int o = 0; o < out; ++o) {
            double s = 0.0;
            for (int i = 0; i < in; ++i) s = fma(src[i], K[i * out + o], s);
            if (bias) s = s + bias[o];
            h[l][o] = sl_critic_act(net.act[l], s);
        }
    }
    return h[L - 1][0] * net.scale;
}

// g = dV/dx at the point of the last sl_critic_forward (h its layer outputs), by the transposed chain of
// k_policy_param_grad with coefficient 1: delta_L = scale act'(h_L), delta_{l-1} = (W_l delta_l) act'(h_{l-1})
// (fma over the outputs, ascending from 0), g = W_0 delta_0.  delta and tmp: SL_NN_MAXW doubles of the caller.
template <class NET>
SL_HD void sl_critic_input_grad(const NET& net, const double (*h)[SL_NN_MAXW], double* delta, double* tmp,
                                double* g) {
    const int L = net.nlayers;
    delta[0] = net.scale * sl_pg_dact(net.act[L - 1], h[L - 1][0]);
    for (int l = L - 1; l >= 0; --l) {
        const int in = net.dims[l], out = net.dims[l + 1];
        const double* K = net.params + net.koff[l];
        for (int i = 0; i < in; ++i) {
            double s = 0.0;
            for (int o = 0; o < out; ++o) s = fma(K[i * out + o], delta[o], s);
            tmp[i] = l > 0 ? s * sl_pg_dact(net.act[l - 1], h[l - 1][i]) : s;
        }
        if (l > 0) {
            for (int i = 0; i < in; ++i) delta[i] = tmp[i];
        } else {
            for (int i = 0; i < in; ++i) g[i] = tmp[i];
        }
    }
}

// ---- one sample --------------------------------------------------------------------------------------------
struct SlCriticSample {
    double value;              // V(x)
    double q;                  // r + gamma V(x+)
    double delta;              // V(x) - q
    double coeff;              // w sign(delta)
    double dq_du[SL_M];
};

// after the dynamics and the two network passes: v_x = V(x), v_next = V(x+), g = dV/dx at x+
//   t_a = sum_k (g_k * jac[k][a]), left to right;  dq/du_a = dr_a + gamma * t_a;  q = r + gamma * v_next
SL_HD void sl_critic_point(const sl_value_desc& reward, double gamma, int d, int m, const double* z, double v_x,
                           double v_next, const double* g, const double (*jac)[SL_M], double w,
                           SlCriticSample* out) {
    const int p = d + m;
    const double r = sl_quadratic(reward, p, z);
    const double t = gamma * v_next;
    const double q = r + t;
#pragma unroll
    for (int a = 0; a < SL_M; ++a) {
        if (a < m) {
            double dr = 0.0;
#pragma unroll
            for (int qq = 0; qq < SL_P; ++qq) if (qq == d + a) dr = sl_pg_quadratic_grad(reward, p, z, qq);
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < SL_D; ++k) {
                if (k < d) {
                    const double tk = g[k] * jac[k][a];
                    acc = (k == 0) ? tk : (acc + tk);
                }
            }
            const double ga = gamma * acc;
            out->dq_du[a] = dr + ga;
        }
    }
    const double delta = v_x - q;
    out->value = v_x;
    out->q = q;
    out->delta = delta;
    out->coeff = delta > 0.0 ? w : (delta < 0.0 ? -w : 0.0);
}
