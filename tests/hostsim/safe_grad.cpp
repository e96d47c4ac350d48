// safe_grad.cpp - TEST-ONLY host build of safe_learning_amd/csrc/sl_safe_grad.h.
//
// The per-point arithmetic of sl_decrease_gradient (k_sg_generate / k_sg_gemm as the scalar sums of
// sl_sg_head_sums, k_sg_epilogue as written), compiled with g++ from the same header, so that
// tests/test_safe_policy_training_host.py can compare it with the NumPy reference
// (tests/np_safe_policy_training.py) without a GPU.  The test loads it as a shared library; built as a program
// (also with -fsanitize=address,undefined), main() runs hand-worked samples through every routine.  Never
// imported by the product package.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "sl_safe_grad.h"

static void fill_tri(SlTri& t, const sl_grid_desc* grid, int nsimplex, const int32_t* simplices, const double* hyper,
                     const double* discrete_points, int project, const double* table) {
    std::memset(&t, 0, sizeof(t));
    t.grid = *grid;
    t.nsimplex = nsimplex; t.project = project; t.ncols = 1; t.set = 1;
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

// dC/du, C and the record [decrease, threshold, mean, error] at n points.  vgrid == NULL: no table (quadratic V_L).
// linv[h]: the explicit inverse factor of head h, [n_h][n_h] row-major.
int sg_decrease_gradient(const sl_grid_desc* vgrid, int nsimplex, const int32_t* simplices, const double* hyper,
                         const double* discrete_points, int project, const double* table, const sl_model_desc* model,
                         double beta, int nheads, const SlPgHead* heads, const double* const* linv, int d, int m,
                         int64_t n, const double* states, const double* actions, double* grad, double* constraint,
                         double* terms) {
    static SlTri t;
    std::memset(&t, 0, sizeof(t));
    if (vgrid) fill_tri(t, vgrid, nsimplex, simplices, hyper, discrete_points, project, table);
    if (model->dynamics.kind != SL_DYN_GP || model->value.kind == SL_V_NETWORK) return SL_ERR_UNSUPPORTED;
    if (model->value.kind == SL_V_TRI && !vgrid) return SL_ERR_INVALID;
    static SlDevModel M;
    std::memset(&M, 0, sizeof(M));
    M.m = *model;
    M.in_dim = d + m;
    M.uncertain = 1;
    const int p = d + m;
    int rows = 1;
    for (int h = 0; h < nheads; ++h) rows = heads[h].n > rows ? heads[h].n : rows;
    std::vector<double> kx((size_t)rows), dkx((size_t)rows * SL_M);
    for (int64_t i = 0; i < n; ++i) {
        double z[SL_P] = {0.0}, mean[SL_D] = {0.0}, jac[SL_D][SL_M] = {{0.0}}, var[SL_D] = {0.0},
               dvar[SL_D][SL_M] = {{0.0}}, err[SL_D] = {0.0}, g[SL_M] = {0.0};
        for (int k = 0; k < d; ++k) z[k] = states[i * d + k];
        for (int a = 0; a < m; ++a) z[d + a] = actions[i * m + a];
        for (int h = 0; h < nheads; ++h) {
            const SlPgHead& hd = heads[h];
            sl_pg_head(hd, p, d, m, z, mean, jac);
            double dprior[SL_M], dv[SL_M], ss = 0.0, sab[SL_M] = {0.0};
            const double prior = sl_sg_prior(hd, p, d, m, z, dprior);
            if (hd.n > 0) sl_sg_head_sums(hd, linv[h], p, d, m, z, kx.data(), dkx.data(), &ss, sab);
            const double v = sl_sg_variance(prior, dprior, ss, sab, m, dv);
            for (int k = hd.col0; k < hd.col0 + hd.dout; ++k) {
                var[k] = v;
                for (int c = 0; c < m; ++c) dvar[k][c] = dv[c];
            }
        }
        sl_pg_linear_part(M.m.dynamics, d, m, z, mean, jac);
        const SlSgPoint r = sl_sg_point(M, t, beta, d, m, z, mean, jac, var, dvar, err, g);
        for (int a = 0; a < m; ++a) grad[i * m + a] = g[a];
        if (constraint) constraint[i] = r.constraint;
        if (terms) {
            double* o = terms + i * (2 + 2 * d);
            o[0] = r.decrease; o[1] = r.threshold;
            for (int k = 0; k < d; ++k) { o[2 + k] = mean[k]; o[2 + d + k] = err[k]; }
        }
    }
    return 0;
}

// k(z, z) and its action derivative: kzz [n], dkzz [n][m]
int sg_kernel_diag(const sl_gp_kernel* ks, int p, int d, int m, const double* z, int n, double* kzz, double* dkzz) {
    for (int i = 0; i < n; ++i) {
        double zz[SL_P] = {0.0}, dk[SL_M] = {0.0};
        for (int q = 0; q < p; ++q) zz[q] = z[i * p + q];
        kzz[i] = sl_sg_kernel_diag(*ks, p, d, m, zz, dk);
        for (int c = 0; c < m; ++c) dkzz[i * m + c] = dk[c];
    }
    return 0;
}

}  // extern "C"

static int expect(const char* what, double got, double want, double tol = 0.0) {
    if (got == want || (tol > 0.0 && fabs(got - want) <= tol)) return 0;
    std::printf("%s: got %.17g, expected %.17g\n", what, got, want);
    return 1;
}

int main() {
    int bad = 0;
    // Kdiag of Linear(variance 2 on the action column) * RBF(variance 3) + Matern32(variance 0.5): 2 u^2 3 + 0.5
    sl_gp_kernel ks;
    std::memset(&ks, 0, sizeof(ks));
    ks.nfactors = 3;
    ks.factor[0].kind = SL_KERNEL_LINEAR; ks.factor[0].product = 0; ks.factor[0].variance[1] = 2.0;
    ks.factor[1].kind = SL_KERNEL_RBF; ks.factor[1].product = 0; ks.factor[1].variance[0] = 3.0;
    ks.factor[1].inv_lengthscales[0] = 1.0;
    ks.factor[2].kind = SL_KERNEL_MATERN32; ks.factor[2].product = 1; ks.factor[2].variance[0] = 0.5;
    ks.factor[2].inv_lengthscales[1] = 1.0;
    const double z[2] = {0.25, 0.5};
    double kzz, dkzz;
    bad += sg_kernel_diag(&ks, 2, 1, 1, z, 1, &kzz, &dkzz);
    bad += expect("k(z, z)", kzz, 2.0 * 0.25 * 3.0 + 0.5) + expect("dk(z, z)/du", dkzz, 2.0 * 2.0 * 0.5 * 3.0);
    // one state, one action, an RBF head of two training points, quadratic V_L = 1.5 x^2, L_v = |0.75 mu|:
    // the derivative against a central difference of the constraint itself
    const double inv_ls[2] = {2.0, 4.0}, xs[4] = {0.2, -0.6, 1.2, -0.8}, alpha[2] = {0.7, -0.3};
    const double linv[4] = {1.9, 0.0, -0.4, 2.1};
    const SlPgHead head{2, 2, 1, 0, 0.25, inv_ls, xs, alpha, nullptr};
    const double* linvs[1] = {linv};
    sl_model_desc model;
    std::memset(&model, 0, sizeof(model));
    model.grid.d = 1;
    model.policy.m = 1;
    model.dynamics.kind = SL_DYN_GP; model.dynamics.matrix[0][0] = 0.9; model.dynamics.matrix[0][1] = 0.2;
    model.value.kind = SL_V_QUADRATIC; model.value.matrix[0][0] = 1.5;
    model.lipschitz.lv_kind = SL_LIP_ABS_LINEAR; model.lipschitz.lv_matrix[0][0] = 0.75;
    model.lipschitz.lf_kind = SL_LF_CONST; model.lipschitz.lf_const = 0.5; model.lipschitz.tau = 0.01;
    double c3[3], g3[3], terms[4];
    const double x = 0.3, h = 1e-6;
    for (int s = 0; s < 3; ++s) {
        const double u = 0.1 + (s - 1) * h;
        bad += sg_decrease_gradient(nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, &model, 2.0, 1, &head, linvs, 1, 1,
                                    1, &x, &u, &g3[s], &c3[s], terms);
    }
    bad += expect("dC/du", g3[1], (c3[2] - c3[0]) / (2.0 * h), 1e-8);
    bad += expect("C = decrease - threshold", c3[2], terms[0] - terms[1]);
    // threshold = -|0.75 x| (1 + 0.5) 0.01
    bad += expect("threshold", terms[1], -(0.75 * 0.3) * 1.5 * 0.01, 1e-17);
    std::printf(bad ? "safe_grad: %d mismatches\n" : "safe_grad: ok\n", bad);
    return bad ? 1 : 0;
}
