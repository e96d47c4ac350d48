// sl_reward_rollout.h - per-trajectory arithmetic of reward_rollout (examples/utilities.py:522-545):
// the discounted return of the closed loop from every start state, shared by the kernel
// (sl_rollout.hip) and the host tests.
//
// The reference's loop, per trajectory and step t:
//   u    = policy(x);  z = [x, u]
//   temp = w[t] * reward(z)          w[t] = discount ** t, a table computed by the caller
//   sum  = sum + temp                sequential, from 0.0; the product is rounded before the sum
//   (the caller's stopping rule looks at max over ALL trajectories of |temp|)
//   x    = f(z)
// with the functions of sl_rollout.h / sl_model.h in that order, so the sums of a linear system
// under a saturated linear policy with a quadratic reward equal the oracle's bit for bit.  The
// dynamics step after the last reward is computed although nothing reads it, as in the reference
// when the horizon runs out: the state a launch leaves is the input of the next launch.
//
// Plain C++ on scalars on top of sl_rollout.h: g++ compiles it for the tests.
#pragma once

#include "sl_rollout.h"

// steps of one launch at most: the kernel keeps one maximum per step of a launch in LDS (1 KB)
#define SL_REWARD_CHUNK_MAX 128

// Advances NT trajectories by `steps` iterations of (policy, reward, accumulate, dynamics).
// z[t]: SL_P doubles, the state in [0, d) on entry and on return; sum[t]: the running return;
// weights[s]: the discount weight of the launch's step s; table_rows as in sl_rollout_advance.
// sink(step, t, |temp|) is called once for every (step, trajectory), t ascending within a step.
template <bool TRI, int DYN, int NT, class Sink>
SL_HD void sl_reward_rollout_advance(const SlDevModel& M, SlDims n, const SlTri* tri,
                                     const double* const* table_rows, int steps, const double* weights,
                                     double (*z)[SL_P], double* sum, Sink&& sink) {
    for (int s = 0; s < steps; ++s) {
        const double w = weights[s];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            double u[SL_M], nxt[SL_D];
            sl_rollout_policy<TRI>(M, n, tri, table_rows[t], z[t], u);
            sl_append_action(n, u, z[t]);
            const double r = sl_quadratic(M.m.reward, n.p, z[t]);
            const double temp = w * r;
            sum[t] = sum[t] + temp;
            sink(s, t, fabs(temp));
            sl_dynamics_det<DYN>(M, n, z[t], nxt);
#pragma unroll
            for (int k = 0; k < SL_D; ++k) if (k < n.d) z[t][k] = nxt[k];
        }
    }
}

// Offset of the stopping step within a launch of `steps` steps, or -1: the first step whose
// maximum of |temp| over all trajectories is below tol (`np.max(np.abs(temp)) < tol`; a NaN
// maximum compares false, so a NaN anywhere never stops the loop).
SL_HD int sl_reward_stop_offset(const double* step_max, int steps, double tol) {
    for (int s = 0; s < steps; ++s) if (step_max[s] < tol) return s;
    return -1;
}

// Steps of one launch when the caller leaves the choice to the library.  The stopping step T* is
// known only after the launch that contains it: the steps of that launch past T* are wasted and
// the launch is run once more, cut at T*, so a chunk of c steps costs c / 2 + c / 2 = c extra steps
// on average and 2 c at most.  The notebooks' returns converge after a few hundred steps (393 and
// 679 on the test shapes): 32 steps per launch keep the average waste below a tenth of that, and a
// launch of 32 steps over any grid worth a GPU (> 10^5 cells: milliseconds) hides the one host read
// it ends with.  sl_rollout_chunk's answer for small problems - the whole horizon - would run
// every trajectory to the horizon and then once more to T*.  Like sl_rollout_chunk, a launch also
// stays near a second at 2.6e10 trajectory-steps per second.
SL_HD int sl_reward_rollout_chunk(int64_t n, int horizon) {
    int c = sl_rollout_chunk(n, horizon);
    if (c > 32) c = 32;
    return c;
}
