// sl_rollout.h - per-trajectory arithmetic of the closed-loop rollouts (compute_trajectory,
// compute_roa), shared by the kernels (sl_rollout.hip) and the host tests.
//
// One closed-loop step is what a Lyapunov sweep does once per cell before its decrease check:
//   u = policy(x)           closed form, per-trajectory action row, or the table of slot 1 + saturation
//   z = [x, u]
//   x = f(z)                sl_dynamics_det
// with the functions and the operation order of sl_model.h (nothing re-associated, no contraction
// beyond the fma() calls written there), so a rollout of a linear system under a saturated linear
// policy equals the oracle's repeated dynamics(x, policy(x)) bit for bit
// (safe_learning/utilities.py:519-583, examples/utilities.py:654-686).
//
// Plain C++ on scalars on top of sl_model.h, like that header: g++ compiles it for the tests.
#pragma once

#include "sl_model.h"

// policy(x) of one trajectory.  TRI: the interpolated policy (SL_POLICY_TRI, `tri` = table slot 1)
// is compiled in.  table_row: the trajectory's own action row of an SL_POLICY_TABLE model (a
// network policy evaluated for this step, sl_policy_net.hip); not read for the other kinds.
template <bool TRI>
SL_HD void sl_rollout_policy(const SlDevModel& M, SlDims n, const SlTri* tri, const double* table_row,
                             const double* x, double* u) {
    const sl_policy_desc& p = M.m.policy;
    if (p.kind == SL_POLICY_TABLE) {
#pragma unroll
        for (int a = 0; a < SL_M; ++a) if (a < n.m) u[a] = table_row[a];
        sl_saturate(p, n.m, u);
    } else if (TRI && p.kind == SL_POLICY_TRI) {
#pragma unroll
        for (int a = 0; a < SL_M; ++a) if (a < n.m) u[a] = sl_tri_eval(*tri, x, a, nullptr);
        sl_saturate(p, n.m, u);
    } else {
        sl_policy_closed_form(M, n, x, u);
    }
}

// Advances NT trajectories by `steps` closed-loop steps.  z[t]: SL_P doubles, the state in
// [0, d) on entry and on return (the action of the last step behind it); table_rows[t]: the
// table_row of trajectory t (above).  The NT chains are independent and stepped side by side (one
// dependent FP64 chain per trajectory: two of them interleave in the linear kernels).  sink(step, t, state, action) is called after every step with
// the NEW state and the action that led to it - the kernels' trajectory stores, the tests' records.
template <bool TRI, int DYN, int NT, class Sink>
SL_HD void sl_rollout_advance(const SlDevModel& M, SlDims n, const SlTri* tri,
                              const double* const* table_rows, int steps, double (*z)[SL_P], Sink&& sink) {
    for (int s = 0; s < steps; ++s) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            double u[SL_M], nxt[SL_D];
            sl_rollout_policy<TRI>(M, n, tri, table_rows[t], z[t], u);
            sl_append_action(n, u, z[t]);
            sl_dynamics_det<DYN>(M, n, z[t], nxt);
#pragma unroll
            for (int k = 0; k < SL_D; ++k) if (k < n.d) z[t][k] = nxt[k];
            sink(s, t, z[t], u);
        }
    }
}

// compute_roa's membership test (examples/utilities.py:681-682): ||x - e||_2 <= tol with the norm
// as np.linalg.norm(.., ord=2, axis=1) sums it - squares added left to right (at most 8 terms: no
// pairwise blocks), then the root; the ROOTED value is compared.  NaN is outside.
SL_HD bool sl_roa_member(int d, const double* x, const double* e, double tol, double* dist) {
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < SL_D; ++k) {
        if (k < d) {
            const double t = x[k] - e[k];
            const double q = t * t;
            acc = (k == 0) ? q : (acc + q);
        }
    }
    const double r = sqrt(acc);
    if (dist) *dist = r;
    return r <= tol;
}

// steps of one launch when the caller leaves the choice to the library: a launch over n
// trajectories stays near a second at the measured 10.5 ms per Euler cart-pole step of 128^4
// cells (2.6e10 trajectory-steps per second), and never runs more than 2^20 steps of one thread.
SL_HD int sl_rollout_chunk(int64_t n, int steps) {
    const int64_t budget = 25000000000ll;
    int64_t c = budget / (n > 0 ? n : 1);
    if (c > (1ll << 20)) c = 1ll << 20;
    if (c > steps) c = steps;
    if (c < 1) c = 1;
    return (int)c;
}
