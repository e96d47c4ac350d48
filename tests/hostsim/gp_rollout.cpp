// gp_rollout.cpp - TEST-ONLY host build of safe_learning_amd/csrc/sl_gp_rollout.h.
//
// The per-trajectory arithmetic of the mean-rollout kernels (sl_gp_rollout.hip), compiled with g++ from
// the same header, so that tests/test_gp_rollout_host.py can check it against the NumPy reference
// (tests/np_gp_rollout.py) and against sl_pg_head (tests/hostsim/policy_grad.cpp) without a GPU.  The
// reward loop restates the host code of sl_reward_rollout_mean: launches of `chunk` steps, per-step
// maxima, the stopping rule and the launch run once more, cut at the stopping step.  Never imported
// by the product package.
#include <cstring>
#include <vector>
#include "sl_gp_rollout.h"

static SlTri g_tri;            // the policy table (slot 1 of the engine)

static void make_model(const sl_model_desc* desc, SlDevModel* M) {
    std::memset(M, 0, sizeof(*M));
    M->m = *desc;
    SlGridFast& gf = M->gf;
    gf.d = desc->grid.d;
    gf.all_pow2 = 1;
    gf.nindex = 1;
    for (int k = 0; k < gf.d; ++k) {
        const int64_t n = desc->grid.num_points[k];
        gf.nindex *= n;
        gf.num32[k] = (uint32_t)n;
        if ((n & (n - 1)) == 0) { int s = 0; while ((1ll << s) < n) ++s; gf.shift[k] = s; }
        else gf.all_pow2 = 0;
    }
    M->in_dim = desc->grid.d + desc->policy.m;
    M->uncertain = 0;
}

struct Heads {
    const SlGpHeadView* heads;
    SlGpHeadView operator()(int h) const { return heads[h]; }
};

template <int NT>
static void load_starts(const SlDevModel& M, int d, int64_t n, const double* start, int64_t base, int64_t* row,
                        double (*z)[SL_P]) {
    for (int t = 0; t < NT; ++t) {
        row[t] = base + t < n ? base + t : n - 1;
        for (int q = 0; q < SL_P; ++q) z[t][q] = 0.0;
        if (start) for (int k = 0; k < d; ++k) z[t][k] = start[row[t] * d + k];
        else sl_index_to_grid_point(M.m.grid, M.gf, d, row[t], z[t]);
    }
}

template <int NT>
static void run(const SlDevModel& M, int nheads, const SlGpHeadView* heads, int64_t n, const double* start,
                int steps, double* state, double* traj, double* actions) {
    const SlDims nd = sl_dims<0, 0>(M);
    const int d = nd.d, m = nd.m;
    for (int64_t base = 0; base < n; base += NT) {
        double z[NT][SL_P];
        int64_t row[NT];
        const double* table_rows[NT] = {};
        load_starts<NT>(M, d, n, start, base, row, z);
        sl_gp_rollout_advance<true, NT>(M, nd, &g_tri, nheads, Heads{heads}, table_rows, steps, z,
                                        [&](int s, int t, const double* x, const double* u) {
            if (traj) for (int k = 0; k < d; ++k) traj[((int64_t)s * n + row[t]) * d + k] = x[k];
            if (actions) for (int a = 0; a < m; ++a) actions[((int64_t)s * n + row[t]) * m + a] = u[a];
        });
        for (int t = 0; t < NT; ++t)
            for (int k = 0; k < d; ++k) state[row[t] * d + k] = z[t][k];
    }
}

// one "launch" of the reward form: `steps` steps from (start, sum_in) into (state, sum), max |temp| per step
template <int NT>
static void reward_run(const SlDevModel& M, int nheads, const SlGpHeadView* heads, int64_t n, const double* start,
                       const double* sum_in, int steps, const double* weights, double* state, double* sum,
                       double* step_max) {
    const SlDims nd = sl_dims<0, 0>(M);
    const int d = nd.d;
    for (int s = 0; s < steps; ++s) step_max[s] = 0.0;
    for (int64_t base = 0; base < n; base += NT) {
        double z[NT][SL_P], acc[NT];
        int64_t row[NT];
        const double* table_rows[NT] = {};
        load_starts<NT>(M, d, n, start, base, row, z);
        for (int t = 0; t < NT; ++t) acc[t] = sum_in ? sum_in[row[t]] : 0.0;
        sl_gp_reward_rollout_advance<true, NT>(M, nd, &g_tri, nheads, Heads{heads}, table_rows, steps, weights, z,
                                               acc, [&](int s, int t, double magnitude) {
            if (base + t < n && !(magnitude <= step_max[s])) step_max[s] = magnitude;     // (a NaN sticks)
        });
        for (int t = 0; t < NT; ++t) {
            for (int k = 0; k < d; ++k) state[row[t] * d + k] = z[t][k];
            sum[row[t]] = acc[t];
        }
    }
}

extern "C" {

// the interpolated policy (table: [nindex][ncols])
int gr_set_tri(const sl_grid_desc* grid, int nsimplex, const int32_t* simplices, const double* hyper,
               const double* discrete_points, int project, int ncols, const double* table) {
    SlTri& t = g_tri;
    std::memset(&t, 0, sizeof(t));
    t.grid = *grid;
    t.nsimplex = nsimplex; t.project = project; t.ncols = ncols; t.set = 1;
    const int d = grid->d;
    if (d < 1 || d > SL_D) return -1;
    for (int s = 0; s < nsimplex; ++s) {
        for (int v = 0; v <= d; ++v) t.simplices[s][v] = simplices[s * (d + 1) + v];
        for (int k = 0; k < d; ++k)
            for (int j = 0; j < d; ++j) t.hyper[s][k][j] = hyper[(s * d + k) * d + j];
    }
    int64_t stride = 1, total = 0;
    for (int k = d - 1; k >= 0; --k) { t.stride[k] = stride; stride *= grid->num_points[k]; }
    for (int k = 0; k < d; ++k) { t.points_off[k] = (int32_t)total; total += grid->num_points[k]; }
    t.points = discrete_points;
    t.table = table;
    sl_tri_finish(t, discrete_points);
    return 0;
}

// the mean at n rows [x, u]: inputs [n][d + m] -> mean [n][d]; per_thread 1 or 2 rows side by side
int gr_mean(const sl_dynamics_desc* dyn, int nheads, const SlGpHeadView* heads, int d, int m, int64_t n,
            int per_thread, const double* inputs, double* mean) {
    const SlDims nd{d, m, d + m};
    const int step = per_thread == 2 ? 2 : 1;
    for (int64_t i = 0; i < n; i += step) {
        double z[2][SL_P] = {{0.0}}, nxt[2][SL_D];
        const int64_t rows[2] = {i, i + 1 < n ? i + 1 : i};
        for (int t = 0; t < 2; ++t)
            for (int q = 0; q < d + m; ++q) z[t][q] = inputs[rows[t] * (d + m) + q];
        if (step == 2) sl_gp_mean<2>(*dyn, nheads, Heads{heads}, nd, z, nxt);
        else sl_gp_mean<1>(*dyn, nheads, Heads{heads}, nd, z, nxt);
        for (int t = 0; t < step; ++t)
            for (int k = 0; k < d; ++k) mean[rows[t] * d + k] = nxt[t][k];
    }
    return 0;
}

// `steps` closed-loop steps of n trajectories; start: [n][d] or null (the grid points 0 .. n - 1);
// state [n][d]; traj null or [steps][n][d]; actions null or [steps][n][m]; per_thread 1 or 2
int gr_rollout(const sl_model_desc* desc, int nheads, const SlGpHeadView* heads, int64_t n, const double* start,
               int steps, int per_thread, double* state, double* traj, double* actions) {
    SlDevModel M;
    make_model(desc, &M);
    if (M.m.policy.kind == SL_POLICY_TABLE || M.m.policy.kind == SL_POLICY_NETWORK) return -1;
    if (M.m.dynamics.kind != SL_DYN_GP || n < 1 || steps < 0) return -2;
    if (per_thread == 2) run<2>(M, nheads, heads, n, start, steps, state, traj, actions);
    else run<1>(M, nheads, heads, n, start, steps, state, traj, actions);
    return 0;
}

// sl_reward_rollout_mean's loop with launches of `chunk` steps -> sum [n], state [n][d], *steps, *converged,
// *redone (a launch was run once more, cut at the stopping step)
int gr_reward_rollout(const sl_model_desc* desc, int nheads, const SlGpHeadView* heads, int64_t n,
                      const double* start, int horizon, const double* weights, double tol, int chunk, int per_thread,
                      double* sum, double* state, int64_t* steps, int* converged, int* redone) {
    SlDevModel M;
    make_model(desc, &M);
    if (M.m.policy.kind == SL_POLICY_TABLE || M.m.policy.kind == SL_POLICY_NETWORK) return -1;
    if (M.m.dynamics.kind != SL_DYN_GP || M.m.reward.kind != SL_V_QUADRATIC || n < 1 || horizon < 1) return -2;
    if (chunk < 1 || chunk > SL_REWARD_CHUNK_MAX) return -3;
    const int d = M.m.grid.d;
    std::vector<double> st[2] = {std::vector<double>(n * d), std::vector<double>(n * d)};
    std::vector<double> sm[2] = {std::vector<double>(n), std::vector<double>(n)};
    double h_max[SL_REWARD_CHUNK_MAX];
    const double* src_state = start;
    const double* src_sum = nullptr;
    int done = 0, out = 0;
    *converged = 0;
    *redone = 0;
    auto launch = [&](int c) {
        if (per_thread == 2)
            reward_run<2>(M, nheads, heads, n, src_state, src_sum, c, weights + done, st[out].data(), sm[out].data(), h_max);
        else
            reward_run<1>(M, nheads, heads, n, src_state, src_sum, c, weights + done, st[out].data(), sm[out].data(), h_max);
    };
    while (done < horizon && !*converged) {
        const int c = horizon - done < chunk ? horizon - done : chunk;
        launch(c);
        const int stop = sl_reward_stop_offset(h_max, c, tol);
        if (stop >= 0) {
            if (stop + 1 < c) { launch(stop + 1); *redone = 1; }
            done += stop + 1;
            *converged = 1;
        } else {
            done += c;
        }
        src_state = st[out].data();
        src_sum = sm[out].data();
        out ^= 1;
    }
    std::memcpy(state, src_state, sizeof(double) * n * d);
    std::memcpy(sum, src_sum, sizeof(double) * n);
    *steps = done;
    return 0;
}

int gr_chunk(int64_t n, int steps, int64_t points) { return sl_gp_rollout_chunk(n, steps, points); }
int gr_reward_chunk(int64_t n, int horizon, int64_t points) { return sl_gp_reward_rollout_chunk(n, horizon, points); }

}  // extern "C"
