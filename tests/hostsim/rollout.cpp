// rollout.cpp - TEST-ONLY host build of safe_learning_amd/csrc/sl_rollout.h.
//
// The per-trajectory arithmetic of the rollout kernels, compiled with g++ from the same header, so
// that tests/test_rollout_host.py can check it against the NumPy reference (tests/np_rollout.py over
// the oracle's callables) without a GPU.  Never imported by the product package.
#include <cstring>
#include "sl_rollout.h"

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

template <int NT>
static void run(const SlDevModel& M, int64_t n, const double* start, int steps, double* state, double* traj,
                double* actions) {
    const SlDims nd = sl_dims<0, 0>(M);
    const int d = nd.d, m = nd.m;
    for (int64_t base = 0; base < n; base += NT) {
        double z[NT][SL_P];
        int64_t row[NT];
        const double* table_rows[NT] = {};
        for (int t = 0; t < NT; ++t) {
            row[t] = base + t < n ? base + t : n - 1;
            if (start) for (int k = 0; k < d; ++k) z[t][k] = start[row[t] * d + k];
            else sl_index_to_grid_point(M.m.grid, M.gf, d, row[t], z[t]);
        }
        sl_rollout_advance<true, 0, NT>(M, nd, &g_tri, table_rows, steps, z,
                                        [&](int s, int t, const double* x, const double* u) {
            if (traj) for (int k = 0; k < d; ++k) traj[((int64_t)s * n + row[t]) * d + k] = x[k];
            if (actions) for (int a = 0; a < m; ++a) actions[((int64_t)s * n + row[t]) * m + a] = u[a];
        });
        for (int t = 0; t < NT; ++t)
            for (int k = 0; k < d; ++k) state[row[t] * d + k] = z[t][k];
    }
}

extern "C" {

// the interpolated policy (table: [nindex][ncols])
int ro_set_tri(const sl_grid_desc* grid, int nsimplex, const int32_t* simplices, const double* hyper,
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

// `steps` closed-loop steps of n trajectories; start: [n][d] or null (the grid points 0 .. n - 1);
// state [n][d]; traj null or [steps][n][d]; actions null or [steps][n][m]; per_thread 1 or 2
// (the linear kernels step two trajectories side by side)
int ro_rollout(const sl_model_desc* desc, int64_t n, const double* start, int steps, int per_thread,
               double* state, double* traj, double* actions) {
    SlDevModel M;
    make_model(desc, &M);
    if (M.m.policy.kind == SL_POLICY_TABLE || M.m.policy.kind == SL_POLICY_NETWORK) return -1;
    if (M.m.dynamics.kind == SL_DYN_GP || n < 1 || steps < 0) return -2;
    if (per_thread == 2) run<2>(M, n, start, steps, state, traj, actions);
    else run<1>(M, n, start, steps, state, traj, actions);
    return 0;
}

// compute_roa's membership test; dist may be null
int ro_mask(int64_t n, int d, const double* state, const double* equilibrium, double tol, uint8_t* member,
            double* dist) {
    for (int64_t i = 0; i < n; ++i) {
        double r;
        member[i] = sl_roa_member(d, state + i * d, equilibrium, tol, &r) ? 1 : 0;
        if (dist) dist[i] = r;
    }
    return 0;
}

int ro_chunk(int64_t n, int steps) { return sl_rollout_chunk(n, steps); }

}  // extern "C"
