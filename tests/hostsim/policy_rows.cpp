// policy_rows.cpp - TEST-ONLY host build of safe_learning_amd/csrc/sl_policy_rows.h.
//
// The rows of the policy-evaluation operator and their combine, compiled with g++ from the same
// header the kernels include, so that tests/test_policy_rows_host.py can check them against the
// oracle's barycentric weights and against the sweep's value lookup (sl_tri_value_fast) without a
// GPU.  Never imported by the product package.
#include <cstring>
#include "sl_policy_rows.h"

static SlTri g_tri;

template <int D>
static void rows(const SlTri& t, int64_t npts, const double* pts, int negate, int32_t* cols, double* w,
                 uint8_t* negative, double* abs_sum) {
    for (int64_t i = 0; i < npts; ++i) {
        int32_t c[D + 1];
        double wt[D + 1], s;
        bool neg;
        sl_policy_row<D>(t, pts + i * D, negate != 0, c, wt, &neg, &s);
        for (int k = 0; k <= D; ++k) {
            cols[k * npts + i] = c[k];
            w[k * npts + i] = wt[k];
        }
        negative[i] = neg ? 1 : 0;
        abs_sum[i] = s;
    }
}

template <int D>
static void values(const SlTri& t, int64_t npts, const double* pts, double* out) {
    for (int64_t i = 0; i < npts; ++i) out[i] = sl_tri_value_fast<D>(t, pts + i * D);
}

extern "C" {

// the value triangulation the calls below use (table: [nindex] values, one column)
int pr_set_tri(const sl_grid_desc* grid, int nsimplex, const int32_t* simplices, const double* hyper,
               const double* discrete_points, int project, const double* table) {
    SlTri& t = g_tri;
    std::memset(&t, 0, sizeof(t));
    t.grid = *grid;
    t.nsimplex = nsimplex; t.project = project; t.ncols = 1; t.set = 1;
    const int d = grid->d;
    if (d < 1 || d > 4) return -1;
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
    return sl_policy_rows_fit(stride) ? 0 : -2;
}

// rows [K][npts] of the successors pts [npts][d]
int pr_rows(int64_t npts, const double* pts, int negate, int32_t* cols, double* w, uint8_t* negative,
            double* abs_sum) {
    switch (g_tri.grid.d) {
        case 1: rows<1>(g_tri, npts, pts, negate, cols, w, negative, abs_sum); return 0;
        case 2: rows<2>(g_tri, npts, pts, negate, cols, w, negative, abs_sum); return 0;
        case 3: rows<3>(g_tri, npts, pts, negate, cols, w, negative, abs_sum); return 0;
        case 4: rows<4>(g_tri, npts, pts, negate, cols, w, negative, abs_sum); return 0;
    }
    return -1;
}

// the sweep's value lookup at pts (sl_tri_value_fast)
int pr_values(int64_t npts, const double* pts, double* out) {
    switch (g_tri.grid.d) {
        case 1: values<1>(g_tri, npts, pts, out); return 0;
        case 2: values<2>(g_tri, npts, pts, out); return 0;
        case 3: values<3>(g_tri, npts, pts, out); return 0;
        case 4: values<4>(g_tri, npts, pts, out); return 0;
    }
    return -1;
}

// out[i] = r[i] + gamma * sum_k w[k][i] v[cols[k][i]]  (k <= SL_ROW_MAX_K)
int pr_combine(int64_t n, int k, const int32_t* cols, const double* w, const double* r, double gamma,
               const double* v, double* out) {
    if (k < 1 || k > SL_ROW_MAX_K) return -1;
    for (int64_t i = 0; i < n; ++i) {
        double wv[SL_ROW_MAX_K], vals[SL_ROW_MAX_K];
        for (int q = 0; q < k; ++q) {
            wv[q] = w[q * n + i];
            vals[q] = v[cols[q * n + i]];
        }
        out[i] = sl_policy_row_combine(r[i], gamma, sl_policy_row_dot<SL_ROW_MAX_K>(k, wv, vals));
    }
    return 0;
}

}  // extern "C"
