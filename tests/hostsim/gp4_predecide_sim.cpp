// gp4_predecide_sim.cpp - stand-alone host program that runs the deciding pass of a block-mode GP
// sweep on the CPU: gpbound::mean_bound (sl_gp_mean_bound.h, as sl_gp_set_head calls it), a lattice
// table as k_gp_mean_lattice fills it and gp4p::sure_fail (sl_gp4_predecide.h) on every cell of
// [lo, hi), with the per-cell functions of sl_model.h that k_gp_predecide calls.
//
//   gp4_predecide_sim <in> <out>
//
// <in>: doubles n, p, dout, prior variance, spacing S, lo, hi, sizeof(sl_model_desc); lengthscales
// [p]; the bytes of the sl_model_desc (padded to whole doubles); X [n][p], Linv [n][n], alpha
// [n][dout] as sl_gp_set_head takes them.
// <out>: one byte per cell of [lo, hi): 1 = sure to fail.
// Prints "norm j v" / "eps j v" per column (17 digits), "upload_ms v", "blocks B decided D" for the
// 16-cell blocks of the range.  Exit status 1 with a message on a malformed file, 2 when the bound
// is off.  (tests/test_gp_mean_bound_host.py builds it with -fsanitize=address,undefined.)
#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sl_gp4_predecide.h"
#include "sl_gp_mean_bound.h"

static bool read_doubles(std::FILE* f, double* to, size_t count) { return std::fread(to, sizeof(double), count, f) == count; }

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: gp4_predecide_sim <in> <out>\n");
        return 1;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) {
        std::fprintf(stderr, "gp4_predecide_sim: cannot open %s\n", argv[1]);
        return 1;
    }
    double head[8];
    if (!read_doubles(f, head, 8)) {
        std::fprintf(stderr, "gp4_predecide_sim: short header\n");
        std::fclose(f);
        return 1;
    }
    const int n = (int)head[0], p = (int)head[1], dout = (int)head[2], S = (int)head[4];
    const double variance = head[3];
    const long long lo = (long long)head[5], hi = (long long)head[6];
    if (n < 1 || n > 8192 || p < 1 || p > SL_P || dout < 1 || dout > SL_D || S < 1 || lo < 0 || hi < lo || (lo & 63) ||
        (size_t)head[7] != sizeof(sl_model_desc)) {
        std::fprintf(stderr, "gp4_predecide_sim: bad header\n");
        std::fclose(f);
        return 1;
    }
    std::vector<double> ls(p), descbuf((sizeof(sl_model_desc) + 7) / 8), X((size_t)n * p), Linv((size_t)n * n),
        alpha((size_t)n * dout);
    if (!read_doubles(f, ls.data(), ls.size()) || !read_doubles(f, descbuf.data(), descbuf.size()) ||
        !read_doubles(f, X.data(), X.size()) || !read_doubles(f, Linv.data(), Linv.size()) ||
        !read_doubles(f, alpha.data(), alpha.size())) {
        std::fprintf(stderr, "gp4_predecide_sim: short file\n");
        std::fclose(f);
        return 1;
    }
    std::fclose(f);
    static SlDevModel M;
    std::memset(&M, 0, sizeof(M));
    std::memcpy(&M.m, descbuf.data(), sizeof(sl_model_desc));
    const int d = M.m.grid.d;
    if (d < 1 || d > SL_D || dout != d || p != d + M.m.policy.m || M.m.value.kind != SL_V_QUADRATIC || M.m.value.negate) {
        std::fprintf(stderr, "gp4_predecide_sim: a model the pass does not serve\n");
        return 1;
    }
    M.gf.d = d;
    M.gf.all_pow2 = 1;
    M.gf.nindex = 1;
    for (int k = 0; k < d; ++k) {
        const int64_t num = M.m.grid.num_points[k];
        if (num < 1 || num > (1 << 20)) {
            std::fprintf(stderr, "gp4_predecide_sim: bad grid\n");
            return 1;
        }
        M.gf.nindex *= num;
        M.gf.num32[k] = (uint32_t)num;
        if ((num & (num - 1)) == 0) { int s = 0; while ((1ll << s) < num) ++s; M.gf.shift[k] = s; }
        else M.gf.all_pow2 = 0;
    }
    M.in_dim = p;
    M.uncertain = 1;
    const int lk = M.m.lipschitz.lv_kind;
    M.m.lipschitz.lv_cols = (lk == SL_LIP_CONST || lk == SL_LIP_NORM_LINEAR || lk == SL_LIP_NORM_GRAD) ? 1 : d;
    if (hi > M.gf.nindex) {
        std::fprintf(stderr, "gp4_predecide_sim: range beyond the grid\n");
        return 1;
    }
    const SlDims nd = sl_dims<0, 0>(M);

    // the upload's arrays (sl_gp_set_head): scaled inputs [p][n], alpha' = Linv^T alpha
    std::vector<double> xs((size_t)p * n), alphap((size_t)n * dout, 0.0), inv_ls(p);
    for (int j = 0; j < n; ++j)
        for (int q = 0; q < p; ++q) xs[(size_t)q * n + j] = X[(size_t)j * p + q] / ls[q];
    for (int i = 0; i < n; ++i)
        for (int dd = 0; dd < dout; ++dd) {
            const double ai = alpha[(size_t)i * dout + dd];
            if (ai == 0.0) continue;
            for (int j = 0; j <= i; ++j) alphap[(size_t)j * dout + dd] += Linv[(size_t)i * n + j] * ai;
        }
    for (int q = 0; q < p; ++q) inv_ls[q] = 1.0 / ls[q];
    gp4p::PreConst pc;
    std::memset(&pc, 0, sizeof(pc));
    const auto t0 = std::chrono::steady_clock::now();
    const bool ok = gpbound::mean_bound(xs.data(), n, n, p, alphap.data(), dout, variance, pc.norm, pc.eps);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (!ok) {
        std::printf("off\n");
        return 2;
    }
    for (int j = 0; j < dout; ++j) std::printf("norm %d %.17g\n", j, pc.norm[j]);
    for (int j = 0; j < dout; ++j) std::printf("eps %d %.17g\n", j, pc.eps[j]);
    std::printf("upload_ms %.3f\n", ms);
    pc.spacing = S;
    pc.sdev = std::sqrt(variance) * (1.0 + 0x1p-50);
    long long npoints = 1;
    for (int k = 0; k < d; ++k) {
        pc.count[k] = gp4p::lattice_count((int)M.m.grid.num_points[k], S);
        npoints *= pc.count[k];
    }
    if (npoints > gp4p::MAX_LATTICE) {
        std::fprintf(stderr, "gp4_predecide_sim: lattice too large\n");
        return 1;
    }

    // k_gp_mean_lattice
    const int rowlen = gp4p::row_doubles(d, p);
    std::vector<double> table((size_t)npoints * rowlen);
    for (long long at = 0; at < npoints; ++at) {
        long long r = at;
        int64_t cell = 0, stride = 1;
        for (int k = d - 1; k >= 0; --k) {
            const int a = (int)(r % pc.count[k]);
            r /= pc.count[k];
            cell += stride * gp4p::lattice_grid_index(a, (int)M.m.grid.num_points[k], S);
            stride *= M.m.grid.num_points[k];
        }
        double xg[SL_P] = {}, u[SL_M] = {}, g[SL_D] = {}, J[SL_D][SL_P] = {};
        sl_index_to_state(M.m.grid, M.gf, d, cell, xg);
        sl_policy_closed_form(M, nd, xg, u);
        sl_append_action(nd, u, xg);
        for (int q = 0; q < p; ++q) xg[q] = xg[q] * inv_ls[q];
        for (int i = 0; i < n; ++i) {
            double r2 = 0.0, dz[SL_P] = {};
            for (int q = 0; q < p; ++q) {
                dz[q] = xs[(size_t)q * n + i] - xg[q];
                r2 = fma(dz[q], dz[q], r2);
            }
            const double kx = variance * sl_exp_nonpos(-0.5 * r2);
            for (int j = 0; j < dout; ++j) {
                const double ak = kx * alphap[(size_t)i * dout + j];
                g[j] = g[j] + ak;
                for (int q = 0; q < p; ++q) J[j][q] = fma(ak, dz[q], J[j][q]);
            }
        }
        for (int q = 0; q < p; ++q) table[(size_t)at * rowlen + q] = xg[q];
        for (int j = 0; j < d; ++j) {
            table[(size_t)at * rowlen + p + j] = g[j];
            for (int q = 0; q < p; ++q) table[(size_t)at * rowlen + p + d + j * p + q] = J[j][q];
        }
    }

    // k_gp_predecide
    std::vector<unsigned char> sure((size_t)(hi - lo), 0);
    for (long long idx = lo; idx < hi; ++idx) {
        double x[SL_P] = {}, u[SL_M] = {}, prior[SL_D] = {}, z[SL_P] = {}, lv_x[SL_D] = {};
        sl_index_to_state(M.m.grid, M.gf, d, idx, x);
        sl_policy_closed_form(M, nd, x, u);
        sl_append_action(nd, u, x);
        sl_rows_dot<SL_D, SL_P>(M.m.dynamics.matrix, d, p, x, prior);
        for (int q = 0; q < p; ++q) z[q] = x[q] * inv_ls[q];
        sl_lv(M, d, x, lv_x);
        const double v_x = sl_quadratic(M.m.value, d, x);
        const double thr = sl_threshold(M, d, lv_x, M.m.lipschitz.tau, x);
        int64_t ijk[SL_D];
        sl_unravel(M.m.grid, M.gf, d, idx, ijk);
        long long at = 0;
        for (int k = 0; k < d; ++k)
            at = at * pc.count[k] + gp4p::lattice_nearest((int)ijk[k], (int)M.m.grid.num_points[k], S);
        const double* row = &table[(size_t)at * rowlen];
        double z_c[SL_P] = {}, g_c[SL_D] = {};
        for (int q = 0; q < p; ++q) z_c[q] = row[q];
        for (int j = 0; j < d; ++j) g_c[j] = row[p + j];
        sure[(size_t)(idx - lo)] = gp4p::sure_fail(M.m.value, d, p, pc, z, z_c, g_c, row + p + d, prior, v_x, thr) ? 1 : 0;
    }
    long long blocks = 0, decided = 0;
    for (long long b = lo; b < hi; b += 16, ++blocks) {
        bool all = true;
        for (long long idx = b; idx < b + 16 && idx < hi; ++idx) all = all && sure[(size_t)(idx - lo)];
        decided += all ? 1 : 0;
    }
    std::printf("blocks %lld decided %lld\n", blocks, decided);
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!out || std::fwrite(sure.data(), 1, sure.size(), out) != sure.size()) {
        std::fprintf(stderr, "gp4_predecide_sim: cannot write %s\n", argv[2]);
        if (out) std::fclose(out);
        return 1;
    }
    std::fclose(out);
    return 0;
}
