// reward_rollout.cpp - TEST-ONLY host build of safe_learning_amd/csrc/sl_reward_rollout.h.
//
// The per-trajectory arithmetic of k_reward_rollout, compiled with g++ from the same header, and
// the launch loop of sl_reward_rollout around it (chunks, per-step maxima as bit patterns, the
// launch that contains the stopping step run once more from its inputs), so that
// tests/test_reward_rollout_host.py can check both against the NumPy reference
// (tests/np_reward_rollout.py over the oracle's callables) without a GPU.  The model and the policy
// table are those of rollout.cpp.  Never imported by the product package.
#include <vector>
#include "rollout.cpp"
#include "sl_reward_rollout.h"

// one "launch": steps [0, c) of n trajectories from (start, sum_in) into (state, sum); step_max[s] =
// the bit pattern of max |temp| of step s, combined as the kernel combines it
template <int NT>
static void reward_launch(const SlDevModel& M, int64_t n, const double* start, const double* sum_in, int c,
                          const double* weights, double* state, double* sum, uint64_t* step_max) {
    const SlDims nd = sl_dims<0, 0>(M);
    const int d = nd.d;
    for (int s = 0; s < c; ++s) step_max[s] = 0;
    for (int64_t base = 0; base < n; base += NT) {
        double z[NT][SL_P], acc[NT];
        int64_t row[NT];
        bool valid[NT];
        const double* table_rows[NT] = {};
        for (int t = 0; t < NT; ++t) {
            valid[t] = base + t < n;
            row[t] = valid[t] ? base + t : n - 1;
            if (start) for (int k = 0; k < d; ++k) z[t][k] = start[row[t] * d + k];
            else sl_index_to_grid_point(M.m.grid, M.gf, d, row[t], z[t]);
            acc[t] = sum_in ? sum_in[row[t]] : 0.0;
        }
        sl_reward_rollout_advance<true, 0, NT>(M, nd, &g_tri, table_rows, c, weights, z, acc,
                                               [&](int s, int t, double magnitude) {
            uint64_t bits = 0;
            if (valid[t]) std::memcpy(&bits, &magnitude, sizeof(bits));
            if (bits > step_max[s]) step_max[s] = bits;
        });
        for (int t = 0; t < NT; ++t) {
            if (!valid[t]) continue;
            for (int k = 0; k < d; ++k) state[row[t] * d + k] = z[t][k];
            sum[row[t]] = acc[t];
        }
    }
}

extern "C" {

// sl_reward_rollout on the host.  start [n][d] or null (the grid points); weights [horizon]; chunk 0:
// the library's choice; per_thread 1 or 2; sum [n], state [n][d] out; maxima [horizon] out: max
// |temp| of every step summed (the rest untouched); *launches counts the "kernel launches",
// *redone is 1 when one was repeated.
int rr_reward_rollout(const sl_model_desc* desc, int64_t n, const double* start, int horizon, const double* weights,
                      double tol, int chunk, int per_thread, double* sum, double* state, double* maxima,
                      int64_t* steps, int* converged, int* launches, int* redone) {
    SlDevModel M;
    make_model(desc, &M);
    if (M.m.policy.kind == SL_POLICY_TABLE || M.m.policy.kind == SL_POLICY_NETWORK) return -1;
    if (M.m.dynamics.kind == SL_DYN_GP || n < 1 || horizon < 1 || chunk < 0) return -2;
    if (M.m.reward.kind != SL_V_QUADRATIC) return -3;
    const int d = M.m.grid.d;
    if (chunk == 0) chunk = sl_reward_rollout_chunk(n, horizon);
    if (chunk > SL_REWARD_CHUNK_MAX) chunk = SL_REWARD_CHUNK_MAX;
    std::vector<double> other_state((size_t)n * d), other_sum((size_t)n);
    double* const state_of[2] = {state, other_state.data()};
    double* const sum_of[2] = {sum, other_sum.data()};
    auto launch = per_thread == 2 ? reward_launch<2> : reward_launch<1>;
    uint64_t bits[SL_REWARD_CHUNK_MAX];
    double h_max[SL_REWARD_CHUNK_MAX];
    int out = start == state ? 1 : 0, done = 0, stopped = 0;
    const double* src_state = start;
    const double* src_sum = nullptr;
    *launches = *redone = 0;
    while (done < horizon && !stopped) {
        const int c = horizon - done < chunk ? horizon - done : chunk;
        launch(M, n, src_state, src_sum, c, weights + done, state_of[out], sum_of[out], bits);
        ++*launches;
        std::memcpy(h_max, bits, sizeof(double) * c);
        const int stop = sl_reward_stop_offset(h_max, c, tol);
        const int used = stop >= 0 ? stop + 1 : c;
        for (int s = 0; s < used; ++s) maxima[done + s] = h_max[s];
        if (stop >= 0) {
            if (stop + 1 < c) {
                launch(M, n, src_state, src_sum, stop + 1, weights + done, state_of[out], sum_of[out], bits);
                ++*launches;
                *redone = 1;
            }
            stopped = 1;
        }
        done += used;
        src_state = state_of[out];
        src_sum = sum_of[out];
        out ^= 1;
    }
    if (src_state != state) {
        std::memcpy(state, src_state, sizeof(double) * (size_t)n * d);
        std::memcpy(sum, src_sum, sizeof(double) * (size_t)n);
    }
    *steps = done;
    *converged = stopped;
    return 0;
}

int rr_chunk(int64_t n, int horizon) { return sl_reward_rollout_chunk(n, horizon); }

}  // extern "C"
