// sl_gp_sample.hip - sample paths of a Gaussian process on a discretization (sample_gp_function,
// safe_learning/functions.py:1586-1662): the full posterior covariance, a blocked FP64 Cholesky factorization,
// blocked triangular solves and products, and the evaluation of a sample function.  The sequential pieces and
// the block arithmetic: sl_gp_sample.h.
//
//   sl_gp_posterior_cov  k_gs_kxz (K(X, Z)) -> k_gs_linv (a = L^-1 K(X, Z)) -> k_gs_mean -> k_gs_cov
//                        (K(Z, Z) - a^T a + jitter I: lower tiles, mirrored)
//   sl_cholesky          per block column: k_gs_diag (one workgroup, the block in LDS) -> k_gs_panel (the block
//                        rows below it, one row per lane, by substitution) -> k_gs_trail (every lower tile of
//                        the rest minus panel x panel^T)
//   sl_tri_solve         per block: k_gs_solve_diag (one right-hand side per lane) -> k_gs_solve_update
//   sl_tri_mult          k_gs_tri_mult
//   sl_gp_sample_eval    k_gs_eval (D and Alpha streamed through LDS, ascending j)
//
// Every product between blocks is a 64 x 64 tile of a four-wavefront workgroup on v_mfma_f64_16x16x4_f64:
// wavefront w owns the rows 16 w .. 16 w + 15 (four accumulator tiles), operands straight from global memory
// (A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15]; register r of a lane: row (lane >> 4) + 4 r,
// column lane & 15).  Rows and columns past the matrix enter as zeros and are not stored.
//
// No atomics: one owner per entry, sums in a fixed order - the same input gives the same bits at every call.
// A pivot that is not > 0 is written (an ordinary store) to a device word that every later kernel of the call
// reads first; those return at once, and the host reads the word when the call ends.
#include "sl_common.h"
#include "sl_gp_sample.h"
#include "sl_gp_strip.h"

// head of the context's scratch area: the pivot word, the kernel description, the prior row
#define SL_GS_INFO_OFF 0
#define SL_GS_KERNEL_OFF 64
#define SL_GS_PRIOR_OFF (SL_GS_KERNEL_OFF + ((sizeof(sl_gp_kernel) + 63) / 64) * 64)
#define SL_GS_HEAD_BYTES (SL_GS_PRIOR_OFF + 64)
static_assert(SL_MAX_INPUT_DIM * sizeof(double) <= 64, "the prior row has 64 bytes");
static_assert(SL_GS_MAX_N == SL_GP_SAMPLE_MAX_N && SL_GS_MAX_K == SL_GP_SAMPLE_MAX_K &&
              SL_GS_MAX_TRAIN == SL_GP_SAMPLE_MAX_TRAIN, "the limits of sl_hip.h are those of sl_gp_sample.h");

// ---- sl_cholesky ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SL_BLOCK) void k_gs_zero_upper(int64_t N, double* __restrict__ A, int64_t ld) {
    for (int64_t idx = (int64_t)blockIdx.x * SL_BLOCK + threadIdx.x; idx < N * N; idx += (int64_t)gridDim.x * SL_BLOCK) {
        const int64_t row = idx / N, col = idx - row * N;
        if (col > row) A[row * ld + col] = 0.0;
    }
}

__global__ __launch_bounds__(SL_GS_THREADS) void k_gs_diag(int64_t N, double* __restrict__ A, int64_t ld, int kb,
                                                           int32_t* __restrict__ info) {
    __shared__ double a[SL_GS_NB * SL_GS_LD];
    if (*info != 0) return;
    const int tid = threadIdx.x, nb = sl_gs_block_rows(N, kb);
    const int64_t r0 = (int64_t)kb * SL_GS_NB;
    for (int t = tid; t < nb * nb; t += SL_GS_THREADS) {
        const int i = t / nb, j = t - i * nb;
        if (j <= i) a[i * SL_GS_LD + j] = A[(r0 + i) * ld + r0 + j];
    }
    __syncthreads();
    const int fail = sl_gs_diag_factor(a, nb, tid, SL_GS_THREADS, [] { __syncthreads(); });
    if (fail) {
        if (tid == 0) *info = (int32_t)(r0 + fail);
        return;
    }
    for (int t = tid; t < nb * nb; t += SL_GS_THREADS) {
        const int i = t / nb, j = t - i * nb;
        A[(r0 + i) * ld + r0 + j] = j <= i ? a[i * SL_GS_LD + j] : 0.0;
    }
}

// blockIdx.x: block row kb + 1 + blockIdx.x; lane = row of the tile
__global__ __launch_bounds__(SL_GS_NB) void k_gs_panel(int64_t N, double* A, int64_t ld, int kb, const int32_t* info) {
    __shared__ double x[SL_GS_NB * SL_GS_LD];
    if (*info != 0) return;
    const int tid = threadIdx.x, bi = kb + 1 + blockIdx.x, rows = sl_gs_block_rows(N, bi);
    const int64_t r0 = (int64_t)bi * SL_GS_NB, c0 = (int64_t)kb * SL_GS_NB;
    for (int t = tid; t < rows * SL_GS_NB; t += SL_GS_NB) {
        const int i = t / SL_GS_NB, j = t % SL_GS_NB;
        x[i * SL_GS_LD + j] = A[(r0 + i) * ld + c0 + j];
    }
    __syncthreads();
    if (tid < rows) sl_gs_panel_row(x + tid * SL_GS_LD, A + c0 * ld + c0, ld, SL_GS_NB);
    __syncthreads();
    for (int t = tid; t < rows * SL_GS_NB; t += SL_GS_NB) {
        const int i = t / SL_GS_NB, j = t % SL_GS_NB;
        A[(r0 + i) * ld + c0 + j] = x[i * SL_GS_LD + j];
    }
}

// tile (kb + 1 + blockIdx.y, kb + 1 + blockIdx.x) of the lower triangle -= panel_i panel_j^T
__global__ __launch_bounds__(SL_GS_THREADS) void k_gs_trail(int64_t N, double* A, int64_t ld, int kb,
                                                            const int32_t* info) {
    if (*info != 0 || blockIdx.x > blockIdx.y) return;
    const int lane = threadIdx.x & 63, l15 = lane & 15, lk = lane >> 4, wave = threadIdx.x >> 6;
    const int64_t c0 = (int64_t)kb * SL_GS_NB;
    const int64_t i0 = (int64_t)(kb + 1 + blockIdx.y) * SL_GS_NB + 16 * wave, j0 = (int64_t)(kb + 1 + blockIdx.x) * SL_GS_NB;
    GS_ZERO_ACC(acc);
    gs_strip(SL_GS_NB,
             [&](int r, int k) { return i0 + r < N ? A[(i0 + r) * ld + c0 + k] : 0.0; },
             [&](int k, int c) { return j0 + c < N ? A[(j0 + c) * ld + c0 + k] : 0.0; }, acc);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t row = i0 + lk + 4 * r, col = j0 + 16 * t + l15;
            if (row < N && col <= row) A[row * ld + col] = A[row * ld + col] - acc[t][r];
        }
    }
}

extern "C" int sl_cholesky(sl_ctx* ctx, int64_t N, double* d_A, int64_t ld, int32_t* h_info) {
    if (!ctx) return sl_fail(nullptr, SL_ERR_INVALID, "sl_cholesky: null context");
    if (h_info) *h_info = 0;
    if (N < 1 || !d_A || ld < N)
        return sl_fail(ctx, SL_ERR_INVALID, "sl_cholesky: N = %lld, ld = %lld, matrix %p", (long long)N, (long long)ld,
                       (void*)d_A);
    if (N > SL_GS_MAX_N)
        return sl_fail(ctx, SL_ERR_UNSUPPORTED, "sl_cholesky: N = %lld (at most %d)", (long long)N, SL_GS_MAX_N);
    SL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    SL_HIP_CHECK(ctx, sl_grow(ctx, &ctx->d_scratch, &ctx->scratch_bytes, SL_GS_HEAD_BYTES, (size_t)1 << 20));
    int32_t* info = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(ctx->d_scratch) + SL_GS_INFO_OFF);
    SL_HIP_CHECK(ctx, hipMemsetAsync(info, 0, sizeof(int32_t), ctx->stream));
    hipLaunchKernelGGL(k_gs_zero_upper, dim3(sl_grid_blocks(N * N)), dim3(SL_BLOCK), 0, ctx->stream, N, d_A, ld);
    SL_HIP_CHECK(ctx, hipGetLastError());
    const int nblk = sl_gs_blocks(N);
    for (int kb = 0; kb < nblk; ++kb) {
        hipLaunchKernelGGL(k_gs_diag, dim3(1), dim3(SL_GS_THREADS), 0, ctx->stream, N, d_A, ld, kb, info);
        SL_HIP_CHECK(ctx, hipGetLastError());
        const int below = nblk - kb - 1;
        if (!below) break;
        hipLaunchKernelGGL(k_gs_panel, dim3(below), dim3(SL_GS_NB), 0, ctx->stream, N, d_A, ld, kb, info);
        SL_HIP_CHECK(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_gs_trail, dim3(below, below), dim3(SL_GS_THREADS), 0, ctx->stream, N, d_A, ld, kb, info);
        SL_HIP_CHECK(ctx, hipGetLastError());
    }
    int32_t failed = 0;
    SL_HIP_CHECK(ctx, hipMemcpyAsync(&failed, info, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    SL_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (h_info) *h_info = failed;
    if (failed)
        return sl_fail(ctx, SL_ERR_INVALID, "sl_cholesky: pivot %d of %lld is not positive; the matrix is not positive "
                       "definite", (int)failed, (long long)N);
    return SL_OK;
}

// ---- sl_tri_solve --------------------------------------------------------------------------------------------
// blockIdx.x: 64 right-hand sides, one per lane
__global__ __launch_bounds__(SL_GS_NB) void k_gs_solve_diag(int64_t N, int64_t k, const double* __restrict__ L, int64_t ld,
                                                           double* __restrict__ B, int kb, int transpose) {
    __shared__ double xs[SL_GS_NB * SL_GS_NB];
    const int tid = threadIdx.x, nb = sl_gs_block_rows(N, kb);
    const int64_t r0 = (int64_t)kb * SL_GS_NB, col = (int64_t)blockIdx.x * SL_GS_NB + tid;
    for (int i = 0; i < nb; ++i) xs[i * SL_GS_NB + tid] = col < k ? B[(r0 + i) * k + col] : 0.0;
    sl_gs_solve_col(xs + tid, SL_GS_NB, L + r0 * ld + r0, ld, nb, transpose);
    if (col < k)
        for (int i = 0; i < nb; ++i) B[(r0 + i) * k + col] = xs[i * SL_GS_NB + tid];
}

// blockIdx.x: 64 right-hand sides; blockIdx.y: the block row that loses  L_(i, kb) X_kb  (transpose = 0: the rows
// below kb) or  L_(kb, i)^T X_kb  (the rows above)
__global__ __launch_bounds__(SL_GS_THREADS) void k_gs_solve_update(int64_t N, int64_t k, const double* __restrict__ L,
                                                                  int64_t ld, double* B, int kb, int transpose) {
    const int lane = threadIdx.x & 63, l15 = lane & 15, lk = lane >> 4, wave = threadIdx.x >> 6;
    const int bi = transpose ? (int)blockIdx.y : kb + 1 + (int)blockIdx.y;
    const int nbk = sl_gs_block_rows(N, kb);
    const int64_t c0 = (int64_t)kb * SL_GS_NB, i0 = (int64_t)bi * SL_GS_NB + 16 * wave, j0 = (int64_t)blockIdx.x * SL_GS_NB;
    GS_ZERO_ACC(acc);
    auto rhs = [&](int kk, int c) { return kk < nbk && j0 + c < k ? B[(c0 + kk) * k + j0 + c] : 0.0; };
    if (transpose)
        gs_strip(nbk, [&](int r, int kk) { return kk < nbk && i0 + r < N ? L[(c0 + kk) * ld + i0 + r] : 0.0; }, rhs, acc);
    else
        gs_strip(nbk, [&](int r, int kk) { return kk < nbk && i0 + r < N ? L[(i0 + r) * ld + c0 + kk] : 0.0; }, rhs, acc);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t row = i0 + lk + 4 * r, col = j0 + 16 * t + l15;
            if (row < N && col < k) B[row * k + col] = B[row * k + col] - acc[t][r];
        }
    }
}

static int gs_shape(sl_ctx* ctx, const char* who, int64_t N, int64_t k, int64_t ld, const void* a, const void* b) {
    if (N < 1 || k < 1 || ld < N || !a || !b)
        return sl_fail(ctx, SL_ERR_INVALID, "%s: N = %lld, k = %lld, ld = %lld, buffers %p %p", who, (long long)N,
                       (long long)k, (long long)ld, a, b);
    if (N > SL_GS_MAX_N || k > SL_GS_MAX_K)
        return sl_fail(ctx, SL_ERR_UNSUPPORTED, "%s: N = %lld (at most %d), k = %lld (at most %d)", who, (long long)N,
                       SL_GS_MAX_N, (long long)k, SL_GS_MAX_K);
    return SL_OK;
}

extern "C" int sl_tri_solve(sl_ctx* ctx, int64_t N, int64_t k, const double* d_L, int64_t ld, int transpose,
                            double* d_B) {
    if (!ctx) return sl_fail(nullptr, SL_ERR_INVALID, "sl_tri_solve: null context");
    if (const int rc = gs_shape(ctx, "sl_tri_solve", N, k, ld, d_L, d_B)) return rc;
    SL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const int nblk = sl_gs_blocks(N);
    const unsigned kblocks = (unsigned)((k + SL_GS_NB - 1) / SL_GS_NB);
    transpose = transpose ? 1 : 0;
    for (int step = 0; step < nblk; ++step) {
        const int kb = transpose ? nblk - 1 - step : step;
        hipLaunchKernelGGL(k_gs_solve_diag, dim3(kblocks), dim3(SL_GS_NB), 0, ctx->stream, N, k, d_L, ld, d_B, kb, transpose);
        SL_HIP_CHECK(ctx, hipGetLastError());
        const int others = transpose ? kb : nblk - kb - 1;
        if (!others) continue;
        hipLaunchKernelGGL(k_gs_solve_update, dim3(kblocks, others), dim3(SL_GS_THREADS), 0, ctx->stream, N, k, d_L, ld,
                           d_B, kb, transpose);
        SL_HIP_CHECK(ctx, hipGetLastError());
    }
    return SL_OK;
}

// ---- sl_tri_mult ---------------------------------------------------------------------------------------------
// blockIdx.x: 64 columns, blockIdx.y: block row.  out = mean + L Zn, the sum over ascending k up to the diagonal.
__global__ __launch_bounds__(SL_GS_THREADS) void k_gs_tri_mult(int64_t N, int64_t k, const double* __restrict__ L,
                                                              int64_t ld, const double* __restrict__ Zn,
                                                              const double* __restrict__ mean,
                                                              double* __restrict__ out) {
    const int lane = threadIdx.x & 63, l15 = lane & 15, lk = lane >> 4, wave = threadIdx.x >> 6;
    const int64_t i0 = (int64_t)blockIdx.y * SL_GS_NB + 16 * wave, j0 = (int64_t)blockIdx.x * SL_GS_NB;
    const int64_t last = (int64_t)(blockIdx.y + 1) * SL_GS_NB;
    const int kend = (int)(last < N ? last : N);
    GS_ZERO_ACC(acc);
    gs_strip(kend,
             [&](int r, int kk) { return i0 + r < N && kk <= i0 + r ? L[(i0 + r) * ld + kk] : 0.0; },
             [&](int kk, int c) { return kk < N && j0 + c < k ? Zn[(int64_t)kk * k + j0 + c] : 0.0; }, acc);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t row = i0 + lk + 4 * r, col = j0 + 16 * t + l15;
            if (row < N && col < k) out[row * k + col] = mean ? mean[row] + acc[t][r] : acc[t][r];
        }
    }
}

extern "C" int sl_tri_mult(sl_ctx* ctx, int64_t N, int64_t k, const double* d_L, int64_t ld, const double* d_Zn,
                           const double* d_mean, double* d_out) {
    if (!ctx) return sl_fail(nullptr, SL_ERR_INVALID, "sl_tri_mult: null context");
    if (const int rc = gs_shape(ctx, "sl_tri_mult", N, k, ld, d_L, d_Zn)) return rc;
    if (!d_out || d_out == d_Zn) return sl_fail(ctx, SL_ERR_INVALID, "sl_tri_mult: the output must be a buffer of its own");
    SL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_gs_tri_mult, dim3((unsigned)((k + SL_GS_NB - 1) / SL_GS_NB), sl_gs_blocks(N)), dim3(SL_GS_THREADS), 0,
                       ctx->stream, N, k, d_L, ld, d_Zn, d_mean, d_out);
    SL_HIP_CHECK(ctx, hipGetLastError());
    return SL_OK;
}

// ---- sl_gp_posterior_cov -------------------------------------------------------------------------------------
__device__ __forceinline__ void gs_point(const double* __restrict__ P, int p, int64_t i, double* x) {
#pragma unroll
    for (int q = 0; q < SL_P; ++q) x[q] = q < p ? P[i * p + q] : 0.0;
}

// out[j][i] = k(X_j, Z_i)
__global__ __launch_bounds__(SL_BLOCK) void k_gs_kxz(const sl_gp_kernel* __restrict__ kern, int p, int n,
                                                    const double* __restrict__ X, int64_t N, const double* __restrict__ Z,
                                                    double* __restrict__ out) {
    for (int64_t idx = (int64_t)blockIdx.x * SL_BLOCK + threadIdx.x; idx < (int64_t)n * N; idx += (int64_t)gridDim.x * SL_BLOCK) {
        const int64_t j = idx / N, i = idx - j * N;
        double a[SL_P], b[SL_P];
        gs_point(X, p, j, a);
        gs_point(Z, p, i, b);
        out[idx] = sl_kernel_eval(*kern, p, a, b);
    }
}

// a = Linv K(X, Z): blockIdx.x: 64 points, blockIdx.y: block row of Linv (lower triangular: k up to the diagonal)
__global__ __launch_bounds__(SL_GS_THREADS) void k_gs_linv(int n, const double* __restrict__ Linv, int64_t N,
                                                          const double* __restrict__ Kxz, double* __restrict__ out) {
    const int lane = threadIdx.x & 63, l15 = lane & 15, lk = lane >> 4, wave = threadIdx.x >> 6;
    const int64_t i0 = (int64_t)blockIdx.y * SL_GS_NB + 16 * wave, j0 = (int64_t)blockIdx.x * SL_GS_NB;
    const int64_t last = (int64_t)(blockIdx.y + 1) * SL_GS_NB;
    const int kend = (int)(last < n ? last : n);
    GS_ZERO_ACC(acc);
    gs_strip(kend,
             [&](int r, int kk) { return i0 + r < n && kk <= i0 + r ? Linv[(i0 + r) * n + kk] : 0.0; },
             [&](int kk, int c) { return kk < n && j0 + c < N ? Kxz[(int64_t)kk * N + j0 + c] : 0.0; }, acc);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t row = i0 + lk + 4 * r, col = j0 + 16 * t + l15;
            if (row < n && col < N) out[row * N + col] = acc[t][r];
        }
    }
}

// mean_i = sum_j a_ji alpha_j (ascending j) + Z_i . prior
__global__ __launch_bounds__(SL_BLOCK) void k_gs_mean(int n, const double* __restrict__ a, const double* __restrict__ alpha,
                                                     int p, const double* __restrict__ Z, const double* __restrict__ prior,
                                                     int64_t N, double* __restrict__ mean) {
    for (int64_t i = (int64_t)blockIdx.x * SL_BLOCK + threadIdx.x; i < N; i += (int64_t)gridDim.x * SL_BLOCK) {
        double s = 0.0, m = 0.0;
        for (int j = 0; j < n; ++j) s = fma(a[(int64_t)j * N + i], alpha[j], s);
        if (prior) {
#pragma unroll
            for (int q = 0; q < SL_P; ++q) if (q < p) m = fma(Z[i * p + q], prior[q], m);
        }
        mean[i] = s + m;
    }
}

// tile (blockIdx.y, blockIdx.x) of the lower triangle: K(Z, Z) - a^T a (+ jitter on the diagonal), stored at
// (i, j) and at (j, i)
__global__ __launch_bounds__(SL_GS_THREADS) void k_gs_cov(const sl_gp_kernel* __restrict__ kern, int p, int n,
                                                         const double* __restrict__ a, int64_t N,
                                                         const double* __restrict__ Z, double jitter,
                                                         double* __restrict__ cov, int64_t ld) {
    if (blockIdx.x > blockIdx.y) return;
    const int lane = threadIdx.x & 63, l15 = lane & 15, lk = lane >> 4, wave = threadIdx.x >> 6;
    const int64_t i0 = (int64_t)blockIdx.y * SL_GS_NB + 16 * wave, j0 = (int64_t)blockIdx.x * SL_GS_NB;
    GS_ZERO_ACC(acc);
    gs_strip(n,
             [&](int r, int kk) { return kk < n && i0 + r < N ? a[(int64_t)kk * N + i0 + r] : 0.0; },
             [&](int kk, int c) { return kk < n && j0 + c < N ? a[(int64_t)kk * N + j0 + c] : 0.0; }, acc);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int64_t col = j0 + 16 * t + l15;
        double zc[SL_P];
        gs_point(Z, p, col < N ? col : N - 1, zc);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t row = i0 + lk + 4 * r;
            if (row < N && col <= row) {
                double zr[SL_P];
                gs_point(Z, p, row, zr);
                double v = sl_kernel_eval(*kern, p, zr, zc) - acc[t][r];
                if (row == col) v = v + jitter;
                cov[row * ld + col] = v;
                cov[col * ld + row] = v;
            }
        }
    }
}

static int gs_kernel_check(sl_ctx* ctx, const char* who, const sl_gp_kernel* h_kernel, int p) {
    if (!h_kernel) return sl_fail(ctx, SL_ERR_INVALID, "%s: no kernel description", who);
    if (p < 1 || p > SL_MAX_INPUT_DIM)
        return sl_fail(ctx, SL_ERR_UNSUPPORTED, "%s: input dimension %d (1 .. %d)", who, p, SL_MAX_INPUT_DIM);
    if (h_kernel->nfactors < 1 || h_kernel->nfactors > SL_KERNEL_MAX_FACTORS)
        return sl_fail(ctx, SL_ERR_INVALID, "%s: kernel with %d leaf factors (1 .. %d)", who, h_kernel->nfactors,
                       SL_KERNEL_MAX_FACTORS);
    for (int f = 0; f < h_kernel->nfactors; ++f) {
        const int kind = h_kernel->factor[f].kind;
        if (kind != SL_KERNEL_RBF && kind != SL_KERNEL_MATERN32 && kind != SL_KERNEL_LINEAR)
            return sl_fail(ctx, SL_ERR_INVALID, "%s: leaf %d has kind %d", who, f, kind);
    }
    return SL_OK;
}

// the kernel description and the prior row (zeros for none) into the head of the scratch area, which has `need`
// bytes afterwards
static int gs_upload_head(sl_ctx* ctx, const sl_gp_kernel* h_kernel, const double* h_prior, int p, size_t need) {
    SL_HIP_CHECK(ctx, sl_grow(ctx, &ctx->d_scratch, &ctx->scratch_bytes, need, (size_t)1 << 20));
    char* base = reinterpret_cast<char*>(ctx->d_scratch);
    double prior[SL_MAX_INPUT_DIM] = {};
    for (int q = 0; q < p && h_prior; ++q) prior[q] = h_prior[q];
    SL_HIP_CHECK(ctx, hipMemcpyAsync(base + SL_GS_KERNEL_OFF, h_kernel, sizeof(sl_gp_kernel), hipMemcpyHostToDevice, ctx->stream));
    SL_HIP_CHECK(ctx, hipMemcpyAsync(base + SL_GS_PRIOR_OFF, prior, sizeof(prior), hipMemcpyHostToDevice, ctx->stream));
    SL_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));         // (the host copies may go away now)
    return SL_OK;
}

extern "C" int sl_gp_posterior_cov(sl_ctx* ctx, int n, int p, const double* h_X, const double* h_Linv,
                                   const double* h_alpha, const sl_gp_kernel* h_kernel, const double* h_prior,
                                   int64_t N, const double* d_Z, double jitter, double* d_mean, double* d_cov,
                                   int64_t ld) {
    const char* who = "sl_gp_posterior_cov";
    if (!ctx) return sl_fail(nullptr, SL_ERR_INVALID, "%s: null context", who);
    if (const int rc = gs_kernel_check(ctx, who, h_kernel, p)) return rc;
    if (n < 0 || N < 1 || ld < N || !d_Z || !d_mean || !d_cov || (n > 0 && (!h_X || !h_Linv || !h_alpha)))
        return sl_fail(ctx, SL_ERR_INVALID, "%s: n = %d, N = %lld, ld = %lld or a missing buffer", who, n, (long long)N,
                       (long long)ld);
    if (N > SL_GS_MAX_N || n > SL_GS_MAX_TRAIN)
        return sl_fail(ctx, SL_ERR_UNSUPPORTED, "%s: N = %lld (at most %d), n = %d observations (at most %d)", who,
                       (long long)N, SL_GS_MAX_N, n, SL_GS_MAX_TRAIN);
    SL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    // scratch: [head] [X n p] [Linv n n] [alpha n] [K(X, Z) n N] [a n N]
    const size_t nn = (size_t)n, nx = (nn * p + 7) & ~(size_t)7, nl = nn * nn, na = (nn + 7) & ~(size_t)7, nk = nn * (size_t)N;
    const size_t need = SL_GS_HEAD_BYTES + sizeof(double) * (nx + nl + na + 2 * nk);
    if (const int rc = gs_upload_head(ctx, h_kernel, h_prior, p, need)) return rc;
    char* base = reinterpret_cast<char*>(ctx->d_scratch);
    const sl_gp_kernel* kern = reinterpret_cast<const sl_gp_kernel*>(base + SL_GS_KERNEL_OFF);
    const double* prior = h_prior ? reinterpret_cast<const double*>(base + SL_GS_PRIOR_OFF) : nullptr;
    double* dX = reinterpret_cast<double*>(base + SL_GS_HEAD_BYTES);
    double* dLinv = dX + nx;
    double* dalpha = dLinv + nl;
    double* kxz = dalpha + na;
    double* a = kxz + nk;
    if (n > 0) {
        SL_HIP_CHECK(ctx, hipMemcpyAsync(dX, h_X, sizeof(double) * nn * p, hipMemcpyHostToDevice, ctx->stream));
        SL_HIP_CHECK(ctx, hipMemcpyAsync(dLinv, h_Linv, sizeof(double) * nl, hipMemcpyHostToDevice, ctx->stream));
        SL_HIP_CHECK(ctx, hipMemcpyAsync(dalpha, h_alpha, sizeof(double) * nn, hipMemcpyHostToDevice, ctx->stream));
        SL_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        hipLaunchKernelGGL(k_gs_kxz, dim3(sl_grid_blocks((int64_t)n * N)), dim3(SL_BLOCK), 0, ctx->stream, kern, p, n, dX, N,
                           d_Z, kxz);
        SL_HIP_CHECK(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_gs_linv, dim3(sl_gs_blocks(N), sl_gs_blocks(n)), dim3(SL_GS_THREADS), 0, ctx->stream, n, dLinv,
                           N, kxz, a);
        SL_HIP_CHECK(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(k_gs_mean, dim3(sl_grid_blocks(N)), dim3(SL_BLOCK), 0, ctx->stream, n, a, dalpha, p, d_Z, prior, N,
                       d_mean);
    SL_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_gs_cov, dim3(sl_gs_blocks(N), sl_gs_blocks(N)), dim3(SL_GS_THREADS), 0, ctx->stream, kern, p, n, a, N,
                       d_Z, jitter, d_cov, ld);
    SL_HIP_CHECK(ctx, hipGetLastError());
    return SL_OK;
}

// ---- sl_gp_sample_eval ---------------------------------------------------------------------------------------
#define SL_GS_EVAL_COLS 8
// blockIdx.x: 256 points (one per thread), blockIdx.y: 8 columns of Alpha.  out = points . prior + sum_j
// k(point, D_j) Alpha_j, j ascending whatever M and the launch shape are.
__global__ __launch_bounds__(SL_BLOCK) void k_gs_eval(const sl_gp_kernel* __restrict__ kern, const double* __restrict__ prior,
                                                     int p, int64_t N, const double* __restrict__ D, int64_t k,
                                                     const double* __restrict__ Alpha, int64_t M,
                                                     const double* __restrict__ points, double* __restrict__ out) {
    __shared__ double dl[SL_GS_NB * SL_P], al[SL_GS_NB * SL_GS_EVAL_COLS];
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * SL_BLOCK + tid, c0 = (int64_t)blockIdx.y * SL_GS_EVAL_COLS;
    double x[SL_P], acc[SL_GS_EVAL_COLS];
    gs_point(points, p, i < M ? i : M - 1, x);
#pragma unroll
    for (int c = 0; c < SL_GS_EVAL_COLS; ++c) acc[c] = 0.0;
    for (int64_t j0 = 0; j0 < N; j0 += SL_GS_NB) {
        __syncthreads();
        for (int t = tid; t < SL_GS_NB * SL_P; t += SL_BLOCK) {
            const int jj = t / SL_P, q = t % SL_P;
            dl[t] = (q < p && j0 + jj < N) ? D[(j0 + jj) * p + q] : 0.0;
        }
        for (int t = tid; t < SL_GS_NB * SL_GS_EVAL_COLS; t += SL_BLOCK) {
            const int jj = t / SL_GS_EVAL_COLS, c = t % SL_GS_EVAL_COLS;
            al[t] = (c0 + c < k && j0 + jj < N) ? Alpha[(j0 + jj) * k + c0 + c] : 0.0;
        }
        __syncthreads();
        const int cnt = (int)(N - j0 < SL_GS_NB ? N - j0 : SL_GS_NB);
        for (int jj = 0; jj < cnt; ++jj) {
            double b[SL_P];
#pragma unroll
            for (int q = 0; q < SL_P; ++q) b[q] = dl[jj * SL_P + q];
            const double kv = sl_kernel_eval(*kern, p, x, b);
#pragma unroll
            for (int c = 0; c < SL_GS_EVAL_COLS; ++c) acc[c] = fma(kv, al[jj * SL_GS_EVAL_COLS + c], acc[c]);
        }
    }
    double m = 0.0;
    if (prior) {
#pragma unroll
        for (int q = 0; q < SL_P; ++q) if (q < p) m = fma(x[q], prior[q], m);
    }
    if (i < M) {
#pragma unroll
        for (int c = 0; c < SL_GS_EVAL_COLS; ++c)
            if (c0 + c < k) out[i * k + c0 + c] = m + acc[c];
    }
}

extern "C" int sl_gp_sample_eval(sl_ctx* ctx, const sl_gp_kernel* h_kernel, const double* h_prior, int p, int64_t N,
                                 const double* d_D, int64_t k, const double* d_Alpha, int64_t M, const double* d_points,
                                 double* d_out) {
    const char* who = "sl_gp_sample_eval";
    if (!ctx) return sl_fail(nullptr, SL_ERR_INVALID, "%s: null context", who);
    if (const int rc = gs_kernel_check(ctx, who, h_kernel, p)) return rc;
    if (N < 1 || k < 1 || M < 0 || !d_D || !d_Alpha || (M > 0 && (!d_points || !d_out)))
        return sl_fail(ctx, SL_ERR_INVALID, "%s: N = %lld, k = %lld, M = %lld or a missing buffer", who, (long long)N,
                       (long long)k, (long long)M);
    if (N > SL_GS_MAX_N || k > SL_GS_MAX_K || M > ((int64_t)1 << 31) - SL_BLOCK)
        return sl_fail(ctx, SL_ERR_UNSUPPORTED, "%s: N = %lld (at most %d), k = %lld (at most %d), M = %lld (below 2^31)",
                       who, (long long)N, SL_GS_MAX_N, (long long)k, SL_GS_MAX_K, (long long)M);
    if (M == 0) return SL_OK;
    SL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (const int rc = gs_upload_head(ctx, h_kernel, h_prior, p, SL_GS_HEAD_BYTES)) return rc;
    const char* base = reinterpret_cast<const char*>(ctx->d_scratch);
    const sl_gp_kernel* kern = reinterpret_cast<const sl_gp_kernel*>(base + SL_GS_KERNEL_OFF);
    const double* prior = h_prior ? reinterpret_cast<const double*>(base + SL_GS_PRIOR_OFF) : nullptr;
    const dim3 grid((unsigned)((M + SL_BLOCK - 1) / SL_BLOCK), (unsigned)((k + SL_GS_EVAL_COLS - 1) / SL_GS_EVAL_COLS));
    hipLaunchKernelGGL(k_gs_eval, grid, dim3(SL_BLOCK), 0, ctx->stream, kern, prior, p, N, d_D, k, d_Alpha, M, d_points, d_out);
    SL_HIP_CHECK(ctx, hipGetLastError());
    return SL_OK;
}
