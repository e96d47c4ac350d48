// policy_grad.cpp - TEST-ONLY host build of safe_learning_amd/csrc/sl_policy_grad.h.
//
// The per-point arithmetic of k_action_gradient and k_tri_pg_emit, compiled with g++ from the same header,
// so that tests/test_policy_training_host.py can compare it with the NumPy reference
// (tests/np_policy_training.py) without a GPU.  The test loads it as a shared library; built as a program
// (also with -fsanitize=address,undefined), main() runs hand-worked samples through every routine.  Never
// imported by the product package.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "sl_policy_grad.h"

static void fill_tri(SlTri& t, const sl_grid_desc* grid, int nsimplex, const int32_t* simplices, const double* hyper,
                     const double* discrete_points, int project, int ncols, const double* table) {
    std::memset(&t, 0, sizeof(t));
    t.grid = *grid;
    t.nsimplex = nsimplex; t.project = project; t.ncols = ncols; t.set = 1;
    const int d = grid->d;
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
}

extern "C" {

// dQ/du at n points: states [n][d], actions [n][m] -> grad [n][m], q [n], next [n][d]
int pg_action_gradient(const sl_grid_desc* vgrid, int nsimplex, const int32_t* simplices, const double* hyper,
                       const double* discrete_points, int project, const double* table,
                       const sl_dynamics_desc* dyn, const sl_value_desc* reward, const sl_value_desc* value,
                       double gamma, int nheads, const SlPgHead* heads, int d, int m, int64_t n,
                       const double* states, const double* actions, double* grad, double* q, double* next) {
    static SlTri t;
    fill_tri(t, vgrid, nsimplex, simplices, hyper, discrete_points, project, 1, table);
    if (dyn->kind != SL_DYN_LINEAR && dyn->kind != SL_DYN_GP) return SL_ERR_UNSUPPORTED;
    const int p = d + m;
    for (int64_t i = 0; i < n; ++i) {
        double z[SL_P] = {0.0}, mean[SL_D] = {0.0}, jac[SL_D][SL_M] = {{0.0}}, g[SL_M];
        for (int k = 0; k < d; ++k) z[k] = states[i * d + k];
        for (int a = 0; a < m; ++a) z[d + a] = actions[i * m + a];
        if (dyn->kind == SL_DYN_GP)
            for (int h = 0; h < nheads; ++h) sl_pg_head(heads[h], p, d, m, z, mean, jac);
        sl_pg_linear_part(*dyn, d, m, z, mean, jac);
        q[i] = sl_pg_point(*reward, *value, gamma, t, d, m, z, mean, jac, g);
        for (int a = 0; a < m; ++a) grad[i * m + a] = g[a];
        for (int k = 0; k < d; ++k) next[i * d + k] = mean[k];
    }
    return 0;
}

// the (vertex, weight) pairs of a table look-up: vert [n][d + 1], w [n][d + 1]
int pg_tri_locate(const sl_grid_desc* grid, int nsimplex, const int32_t* simplices, const double* hyper,
                  const double* discrete_points, int project, int64_t n, const double* points, int64_t* vert,
                  double* w) {
    static SlTri t;
    fill_tri(t, grid, nsimplex, simplices, hyper, discrete_points, project, 1, nullptr);
    const int d = grid->d;
    for (int64_t i = 0; i < n; ++i) {
        double x[SL_D] = {0.0}, wi[SL_D + 1];
        int64_t vi[SL_D + 1];
        for (int k = 0; k < d; ++k) x[k] = points[i * d + k];
        sl_pg_tri_locate(t, x, vi, wi);
        for (int k = 0; k <= d; ++k) { vert[i * (d + 1) + k] = vi[k]; w[i * (d + 1) + k] = wi[k]; }
    }
    return 0;
}

// k(a_j, z_i) and dk/dz_{d + c}: K [na][nz], dK [na][nz][m]
int pg_kernel(const sl_gp_kernel* ks, int p, int d, int m, const double* a, int na, const double* z, int nz,
              double* K, double* dK) {
    for (int j = 0; j < na; ++j)
        for (int i = 0; i < nz; ++i) {
            double aa[SL_P] = {0.0}, zz[SL_P] = {0.0}, dk[SL_M] = {0.0};
            for (int q = 0; q < p; ++q) { aa[q] = a[j * p + q]; zz[q] = z[i * p + q]; }
            K[j * nz + i] = sl_pg_kernel(*ks, p, d, m, aa, zz, dk);
            for (int c = 0; c < m; ++c) dK[(j * nz + i) * m + c] = dk[c];
        }
    return 0;
}

double pg_dact(int a, double post) { return sl_pg_dact(a, post); }

}  // extern "C"

static int expect(const char* what, double got, double want, double tol = 0.0) {
    if (got == want || (tol > 0.0 && fabs(got - want) <= tol)) return 0;
    std::printf("%s: got %.17g, expected %.17g\n", what, got, want);
    return 1;
}

int main() {
    int bad = 0;
    // activation derivatives from the output
    bad += expect("relu' on", sl_pg_dact(2, 0.5), 1.0) + expect("relu' off", sl_pg_dact(2, 0.0), 0.0) +
           expect("tanh'", sl_pg_dact(1, 0.5), 0.75) + expect("sigmoid'", sl_pg_dact(3, 0.25), 0.1875) +
           expect("linear'", sl_pg_dact(0, 3.0), 1.0);
    // 1-D table on [-1, 1] with 5 vertices, V = -x^2 at the vertices, project
    sl_grid_desc grid;
    std::memset(&grid, 0, sizeof(grid));
    grid.d = 1; grid.num_points[0] = 5; grid.offset[0] = -1.0; grid.unit_maxes[0] = 0.5; grid.upper[0] = 1.0;
    const int32_t simplices[2] = {0, 1};
    const double hyper[1] = {2.0};
    std::vector<double> pts(5), table(5);
    for (int i = 0; i < 5; ++i) { pts[i] = -1.0 + 0.5 * i; table[i] = -pts[i] * pts[i]; }
    sl_dynamics_desc dyn;
    std::memset(&dyn, 0, sizeof(dyn));
    dyn.kind = SL_DYN_LINEAR; dyn.matrix[0][0] = 1.25; dyn.matrix[0][1] = 0.5;
    sl_value_desc reward, value;
    std::memset(&reward, 0, sizeof(reward));
    std::memset(&value, 0, sizeof(value));
    reward.kind = SL_V_QUADRATIC; reward.matrix[0][0] = -1.0; reward.matrix[1][1] = -0.125; reward.matrix[0][1] = 0.25;
    value.kind = SL_V_TRI;
    // x = 0.5, u = -0.25: successor 0.5, on the vertex: the cell [0.5, 1) with slope (-1 + 0.25) / 0.5 = -1.5
    // dr/du = x (P01 + P10) + u 2 P11 = 0.125 + 0.0625 = 0.1875; dQ/du = 0.1875 + 0.5 (-1.5 * 0.5) = -0.1875
    // x = 1: successor 1.125 is outside: the mask leaves dr/du = 0.25 + 0.0625
    const double states[2] = {0.5, 1.0}, actions[2] = {-0.25, -0.25};
    double grad[2], q[2], next[2];
    bad += pg_action_gradient(&grid, 1, simplices, hyper, pts.data(), 1, table.data(), &dyn, &reward, &value, 0.5, 0,
                              nullptr, 1, 1, 2, states, actions, grad, q, next);
    bad += expect("successor", next[0], 0.5) + expect("dQ/du inside", grad[0], -0.1875) +
           expect("successor outside", next[1], 1.125) + expect("dQ/du masked", grad[1], 0.3125);
    // Q = r + gamma V: r = -0.25 + 0.25 * 0.5 * -0.25 - 0.125 / 16, V(0.5) = -0.25
    bad += expect("Q", q[0], (-0.25 - 0.03125 - 0.0078125) + 0.5 * -0.25);
    // the look-up as pairs: x = 0.75 lies midway in the cell [0.5, 1]
    int64_t vert[2];
    double w[2];
    const double point[1] = {0.75};
    bad += pg_tri_locate(&grid, 1, simplices, hyper, pts.data(), 1, 1, point, vert, w);
    bad += expect("vertex 0", (double)vert[0], 3.0) + expect("vertex 1", (double)vert[1], 4.0) +
           expect("weight 0", w[0], 0.5) + expect("weight 1", w[1], 0.5);
    // kernels: Linear(variance 2 on the action column) * RBF(state column, lengthscale 1) + Matern32(action column)
    sl_gp_kernel ks;
    std::memset(&ks, 0, sizeof(ks));
    ks.nfactors = 3;
    ks.factor[0].kind = SL_KERNEL_LINEAR; ks.factor[0].product = 0; ks.factor[0].variance[1] = 2.0;
    ks.factor[1].kind = SL_KERNEL_RBF; ks.factor[1].product = 0; ks.factor[1].variance[0] = 1.0;
    ks.factor[1].inv_lengthscales[0] = 1.0;
    ks.factor[2].kind = SL_KERNEL_MATERN32; ks.factor[2].product = 1; ks.factor[2].variance[0] = 0.5;
    ks.factor[2].inv_lengthscales[1] = 1.0;
    const double a[2] = {0.25, 0.5}, z[2] = {0.25, 0.5};
    double K, dK;
    bad += pg_kernel(&ks, 2, 1, 1, a, 1, z, 1, &K, &dK);
    // same point: linear 2 * 0.5 * 0.5 = 0.5 times rbf 1; matern at r = 1e-6: 0.5 within 1e-11, derivative 0
    bad += expect("k(x, x)", K, 1.0, 1e-11) + expect("dk/du at r = 0", dK, 1.0, 1e-11);
    // an RBF head of two training points through sl_pg_head, against its own finite difference
    const double inv_ls[2] = {2.0, 4.0}, xs[4] = {0.2, -0.6, 1.2, -0.8}, alpha[2] = {0.7, -0.3};
    const SlPgHead head{2, 2, 1, 0, 0.25, inv_ls, xs, alpha, nullptr};
    double f[3];
    double jac0 = 0.0;
    for (int s = 0; s < 3; ++s) {
        const double h = 1e-6;
        double zz[SL_P] = {0.0}, mean[SL_D] = {0.0}, jac[SL_D][SL_M] = {{0.0}};
        zz[0] = 0.1; zz[1] = 0.2 + (s - 1) * h;
        sl_pg_head(head, 2, 1, 1, zz, mean, jac);
        f[s] = mean[0];
        if (s == 1) jac0 = jac[0][0];
    }
    bad += expect("rbf head jacobian", jac0, (f[2] - f[0]) / 2e-6, 1e-9);
    std::printf(bad ? "policy_grad: %d mismatches\n" : "policy_grad: ok\n", bad);
    return bad ? 1 : 0;
}
