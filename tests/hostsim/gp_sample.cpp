// gp_sample.cpp - TEST-ONLY host run of the blocked factorization of safe_learning_amd/csrc/sl_gp_sample.h.
//
// A stand-alone program (run under the address and undefined-behaviour sanitizers where the toolchain has them):
//     gp_sample IN OUT
// IN:  int64 N, int64 k, then A [N][N] and B [N][k] as doubles.
// OUT: double info, L [N][N], L^-1 B [N][k], L^-T B [N][k], L B [N][k].
// The blocks, the diagonal-block routine, the panel rows and the right-hand-side columns are the header's; the
// products between blocks, which the device runs on the matrix cores, are plain loops over ascending k here.
// tests/test_gp_sample_host.py compares the result with the NumPy restatement (tests/np_gp_sample.py).  Never
// imported by the product package.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "sl_gp_sample.h"

static int host_cholesky(int64_t N, std::vector<double>& A) {
    const int nblk = sl_gs_blocks(N);
    std::vector<double> block((size_t)SL_GS_NB * SL_GS_LD);
    for (int64_t i = 0; i < N; ++i)
        for (int64_t j = i + 1; j < N; ++j) A[i * N + j] = 0.0;
    for (int kb = 0; kb < nblk; ++kb) {
        const int nb = sl_gs_block_rows(N, kb);
        const int64_t r0 = (int64_t)kb * SL_GS_NB;
        for (int i = 0; i < nb; ++i)
            for (int j = 0; j <= i; ++j) block[i * SL_GS_LD + j] = A[(r0 + i) * N + r0 + j];
        const int fail = sl_gs_diag_factor(block.data(), nb, 0, 1, [] {});
        for (int i = 0; i < nb; ++i)                          // (a failed block is written back too: what is left
            for (int j = 0; j <= i; ++j) A[(r0 + i) * N + r0 + j] = block[i * SL_GS_LD + j];   // of it is looked at)
        if (fail) return (int)(r0 + fail);
        const int64_t r1 = r0 + nb;
        for (int64_t i = r1; i < N; ++i) sl_gs_panel_row(&A[i * N + r0], &A[r0 * N + r0], N, nb);
        for (int64_t i = r1; i < N; ++i)
            for (int64_t j = r1; j <= i; ++j) {
                double s = 0.0;
                for (int k = 0; k < nb; ++k) s = s + A[i * N + r0 + k] * A[j * N + r0 + k];
                A[i * N + j] = A[i * N + j] - s;
            }
    }
    return 0;
}

static void host_solve(int64_t N, int64_t k, const std::vector<double>& L, std::vector<double>& B, int transpose) {
    const int nblk = sl_gs_blocks(N);
    for (int step = 0; step < nblk; ++step) {
        const int kb = transpose ? nblk - 1 - step : step;
        const int nb = sl_gs_block_rows(N, kb);
        const int64_t r0 = (int64_t)kb * SL_GS_NB;
        for (int64_t c = 0; c < k; ++c) sl_gs_solve_col(&B[r0 * k + c], (int)k, &L[r0 * N + r0], N, nb, transpose);
        const int64_t lo = transpose ? 0 : r0 + nb, hi = transpose ? r0 : N;
        for (int64_t i = lo; i < hi; ++i)
            for (int64_t c = 0; c < k; ++c) {
                double s = 0.0;
                for (int kk = 0; kk < nb; ++kk)
                    s = s + (transpose ? L[(r0 + kk) * N + i] : L[i * N + r0 + kk]) * B[(r0 + kk) * k + c];
                B[i * k + c] = B[i * k + c] - s;
            }
    }
}

static void host_mult(int64_t N, int64_t k, const std::vector<double>& L, const std::vector<double>& Z,
                      std::vector<double>& out) {
    for (int64_t i = 0; i < N; ++i)
        for (int64_t c = 0; c < k; ++c) {
            double s = 0.0;
            for (int64_t kk = 0; kk <= i; ++kk) s = s + L[i * N + kk] * Z[kk * k + c];
            out[i * k + c] = s;
        }
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 3;
    int64_t shape[2];
    if (std::fread(shape, sizeof(int64_t), 2, in) != 2) return 4;
    const int64_t N = shape[0], k = shape[1];
    if (N < 1 || k < 1 || N > 4096 || k > 1024) return 5;
    std::vector<double> A((size_t)(N * N)), B((size_t)(N * k));
    if (std::fread(A.data(), sizeof(double), A.size(), in) != A.size()) return 6;
    if (std::fread(B.data(), sizeof(double), B.size(), in) != B.size()) return 7;
    std::fclose(in);
    const double info = host_cholesky(N, A);
    std::vector<double> fwd(B), bwd(B), prod(B.size(), 0.0);
    if (info == 0.0) {
        host_solve(N, k, A, fwd, 0);
        host_solve(N, k, A, bwd, 1);
        host_mult(N, k, A, B, prod);
    }
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 8;
    std::fwrite(&info, sizeof(double), 1, out);
    std::fwrite(A.data(), sizeof(double), A.size(), out);
    std::fwrite(fwd.data(), sizeof(double), fwd.size(), out);
    std::fwrite(bwd.data(), sizeof(double), bwd.size(), out);
    std::fwrite(prod.data(), sizeof(double), prod.size(), out);
    std::fclose(out);
    return 0;
}
