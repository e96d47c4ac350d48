// sl_gp_rollout.h - per-trajectory arithmetic of the closed-loop rollouts of a GP's posterior MEAN
// (UncertainFunction.to_mean_function, safe_learning/functions.py:209-230, simulated by
// compute_trajectory, compute_roa and reward_rollout), shared by the kernels (sl_gp_rollout.hip) and
// the host tests.
//
// One closed-loop step is sl_rollout.h's with the mean of the GP dynamics in place of
// sl_dynamics_det:
//   u = policy(x);  z = [x, u]
//   x = prior(z) + sum_h sum_j k_h(z, x_j) alpha'_hj
// in sl_next_state_mean's operations and order (sl_common.h; sl_pg_head of sl_policy_grad.h states
// the same sum beside its derivative): the prior rows by sl_rows_dot, the heads ascending, the
// training points ascending, the squared distance by fma over the inputs ascending,
// variance * sl_exp_nonpos(-0.5 r2) for an RBF head and sl_kernel_eval for a sum-of-products
// description, acc = fma(k, alpha'[j][dd], acc), the prior added last.  This is the third statement
// of that sum: sl_next_state_mean is device code of the Bellman kernels and sl_pg_head carries the
// action derivative through the same loop, and neither can change without moving the registers of
// the kernels built on them, so the sum is restated and the host tests hold it to sl_pg_head's bits.
//
// Plain C++ on scalars on top of sl_rollout.h, sl_reward_rollout.h and sl_policy_grad.h (for the head
// view): g++ compiles it for the tests.
#pragma once

#include "sl_policy_grad.h"
#include "sl_reward_rollout.h"

// A GP head as the mean needs it: n, n_pad, dout, col0, variance, inv_ls [p], xs [p][n_pad],
// alpha' [n][dout] and the kernel description (or null: an RBF head with pre-scaled inputs).  It is
// sl_policy_grad.h's view of a head: plain arrays, nothing of the context - a kernel fills one from
// SlGpHeadDev, a host test from NumPy arrays, and any other expansion sum_j k(z, x_j) w_j (a
// GPSampleFunction's) could.
typedef SlPgHead SlGpHeadView;

// The training inputs and alpha' of a head are written between launches only (sl_gp_set_head,
// sl_gp_append_point on the same stream): read through the constant address space, their
// wavefront-uniform reads are scalar loads even in kernels that store to global memory between them
// (the rollouts' trajectories), where the compiler otherwise falls back to one vector load per read.
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(4))) double* SlGpUniformDoubles;
#define SL_GP_UNIFORM(ptr) ((SlGpUniformDoubles)(ptr))
#else
typedef const double* SlGpUniformDoubles;
#define SL_GP_UNIFORM(ptr) (ptr)
#endif

// acc[t][k] += sum_j k(z[t], x_j) alpha'_j[k - col0] for the columns the head owns, NT inputs side
// by side: one walk over the training points, each point's inputs read once for the NT chains.
template <int NT>
SL_HD void sl_gp_mean_head(const SlGpHeadView& hd, SlDims nd, const double (*z)[SL_P], double (*acc)[SL_D]) {
    const int d = nd.d, p = nd.p;
    const SlGpUniformDoubles xs = SL_GP_UNIFORM(hd.xs), alpha = SL_GP_UNIFORM(hd.alpha);
    double xg[NT][SL_P];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int q = 0; q < SL_P; ++q) xg[t][q] = (q < p) ? z[t][q] * hd.inv_ls[q] : 0.0;
    }
#pragma unroll 2
    for (int j = 0; j < hd.n; ++j) {
        double xa[SL_P];
#pragma unroll
        for (int q = 0; q < SL_P; ++q) xa[q] = (q < p) ? xs[q * hd.n_pad + j] : 0.0;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            double kx;
            if (hd.kernel) {
                kx = sl_kernel_eval(*hd.kernel, p, xa, xg[t]);
            } else {
                double r2 = 0.0;
#pragma unroll
                for (int q = 0; q < SL_P; ++q) {
                    if (q < p) {
                        const double dlt = xa[q] - xg[t][q];
                        r2 = fma(dlt, dlt, r2);
                    }
                }
                kx = hd.variance * sl_exp_nonpos(-0.5 * r2);
            }
#pragma unroll
            for (int k = 0; k < SL_D; ++k) {
                const int dd = k - hd.col0;
                if (k < d && dd >= 0 && dd < hd.dout)
                    acc[t][k] = fma(kx, alpha[j * hd.dout + dd], acc[t][k]);
            }
        }
    }
}

// The mean [d] of the GP dynamics at the NT inputs z[t] = [x, u].  heads(h) returns the view of head
// h < nheads (a functor, so that a kernel can build the view from its by-value argument inside the
// loop and a host caller can index an array); f: the dynamics description, whose matrix holds the
// rows of the linear prior.  A head without observations (n = 0) contributes nothing.
template <int NT, class Heads>
SL_HD void sl_gp_mean(const sl_dynamics_desc& f, int nheads, Heads&& heads, SlDims nd, const double (*z)[SL_P],
                      double (*nxt)[SL_D]) {
    double prior[NT][SL_D];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        sl_rows_dot<SL_D, SL_P>(f.matrix, nd.d, nd.p, z[t], prior[t]);
#pragma unroll
        for (int k = 0; k < SL_D; ++k) nxt[t][k] = 0.0;
    }
    for (int h = 0; h < nheads; ++h) {
        const SlGpHeadView hd = heads(h);
        sl_gp_mean_head<NT>(hd, nd, z, nxt);
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int k = 0; k < SL_D; ++k) if (k < nd.d) nxt[t][k] = nxt[t][k] + prior[t][k];
    }
}

// sl_rollout_advance with the GP mean as the dynamics: the NT policies first, then one walk over the
// heads for the NT chains, then the sinks in the order of sl_rollout_advance (t ascending).
template <bool TRI, int NT, class Heads, class Sink>
SL_HD void sl_gp_rollout_advance(const SlDevModel& M, SlDims n, const SlTri* tri, int nheads, Heads&& heads,
                                 const double* const* table_rows, int steps, double (*z)[SL_P], Sink&& sink) {
    for (int s = 0; s < steps; ++s) {
        double u[NT][SL_M], nxt[NT][SL_D];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            sl_rollout_policy<TRI>(M, n, tri, table_rows[t], z[t], u[t]);
            sl_append_action(n, u[t], z[t]);
        }
        sl_gp_mean<NT>(M.m.dynamics, nheads, heads, n, z, nxt);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
#pragma unroll
            for (int k = 0; k < SL_D; ++k) if (k < n.d) z[t][k] = nxt[t][k];
            sink(s, t, z[t], u[t]);
        }
    }
}

// sl_reward_rollout_advance with the GP mean as the dynamics: temp = w * r, sum = sum + temp, the
// sink with |temp| (t ascending within a step), and the dynamics step after the last reward.
template <bool TRI, int NT, class Heads, class Sink>
SL_HD void sl_gp_reward_rollout_advance(const SlDevModel& M, SlDims n, const SlTri* tri, int nheads, Heads&& heads,
                                        const double* const* table_rows, int steps, const double* weights,
                                        double (*z)[SL_P], double* sum, Sink&& sink) {
    for (int s = 0; s < steps; ++s) {
        const double w = weights[s];
        double nxt[NT][SL_D];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            double u[SL_M];
            sl_rollout_policy<TRI>(M, n, tri, table_rows[t], z[t], u);
            sl_append_action(n, u, z[t]);
            const double r = sl_quadratic(M.m.reward, n.p, z[t]);
            const double temp = w * r;
            sum[t] = sum[t] + temp;
            sink(s, t, fabs(temp));
        }
        sl_gp_mean<NT>(M.m.dynamics, nheads, heads, n, z, nxt);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
#pragma unroll
            for (int k = 0; k < SL_D; ++k) if (k < n.d) z[t][k] = nxt[t][k];
        }
    }
}

// Steps of one launch when the caller leaves the choice to the library.  A step of one trajectory
// costs one kernel value per training point of every head, so the budget that keeps a launch near a
// second is counted in (trajectory x step x training point).
// SL_GP_ROLLOUT_RATE is MEASURED (tools/gp_rollout_probe.py on one MI355X, profiles/gp_rollout.md):
// 2.75e11 per second for the interpolated-policy flavour on the notebooks' shape (2001 x 1501 cells,
// 128 points) and 4.44e11 for the closed-form flavour at d = 4 (64^4 cells, 1024 points); the budget
// is the slower of the two, rounded down.  The figure DERIVED before the kernel had run was 2e11:
// about 50 FP64 vector operations per kernel value (the exponential included) at 3.9e13 FP64
// lane-operations per second and 0.4 of the issue rate, as k_gp_small reaches (3.1e11, rounded down).
// Like sl_rollout_chunk: never below 1 step, never above 2^20.
#define SL_GP_ROLLOUT_RATE 270000000000ll
SL_HD int sl_gp_rollout_chunk(int64_t n, int steps, int64_t training_points) {
    const int64_t per_step = (n > 0 ? n : 1) * (training_points > 0 ? training_points : 1);
    int64_t c = SL_GP_ROLLOUT_RATE / per_step;
    if (c > (1ll << 20)) c = 1ll << 20;
    if (c > steps) c = steps;
    if (c < 1) c = 1;
    return (int)c;
}

// The reward form: additionally at most sl_reward_rollout_chunk's 32 steps (the launch that holds
// the stopping step is run twice) and at most SL_REWARD_CHUNK_MAX.
SL_HD int sl_gp_reward_rollout_chunk(int64_t n, int horizon, int64_t training_points) {
    int c = sl_gp_rollout_chunk(n, horizon, training_points);
    const int cap = sl_reward_rollout_chunk(n, horizon);
    if (c > cap) c = cap;
    if (c > SL_REWARD_CHUNK_MAX) c = SL_REWARD_CHUNK_MAX;
    return c;
}
