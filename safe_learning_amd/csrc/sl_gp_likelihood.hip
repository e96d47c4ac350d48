// sl_gp_likelihood.hip - log marginal likelihood of GP regression and its gradient with respect to the kernel's
// hyper-parameters and the noise variance (gpflow 0.4.0 GPR.build_likelihood; GPRCached.optimize).  With
// R = Y - m(X) [n][D], K = k(X, X) + sigma_n^2 I = L L^T, B = K^-1 R and W = B B^T - D K^-1:
//
//   lml = -1/2 sum(R o B) - D sum_i log L_ii - n D / 2 log 2 pi,    d lml / d theta = 1/2 sum_ij W_ij dK_ij / d theta
//
//   sl_gp_likelihood   sl_gp_posterior_cov with no observations (K on the device) -> sl_cholesky -> two
//                      sl_tri_solve (B) -> k_lml_identity + sl_tri_solve per chunk of at most SL_GS_MAX_K columns
//                      (L^-1) -> k_lml_kinv (K^-1 = L^-T L^-1 on the matrix cores, lower tiles) -> k_lml_grad
//                      (one workgroup per lower 64 x 64 tile: one partial per slot) -> k_lml_reduce (the tiles in
//                      ascending order; sum log L_ii and sum(R o B))
//
// The per-element arithmetic, the slots and the thread-to-entry map: sl_gp_likelihood.h.  No atomics: a
// workgroup's partial is the butterfly sum of its wavefronts' lanes, then the four wavefronts in ascending order;
// the tiles are added in ascending order by one thread per slot - the same input gives the same bits at every call.
#include "sl_common.h"
#include "sl_gp_sample.h"
#include "sl_gp_strip.h"
#include "sl_gp_likelihood.h"

static_assert(SL_LML_TILE == SL_GS_NB && SL_LML_THREADS == SL_GS_THREADS, "the tiles are those of sl_gp_sample.hip");

// E [n][kc] = the columns c0 .. c0 + kc of the identity
__global__ __launch_bounds__(SL_BLOCK) void k_lml_identity(int64_t n, int64_t kc, int64_t c0, double* __restrict__ E) {
    for (int64_t idx = (int64_t)blockIdx.x * SL_BLOCK + threadIdx.x; idx < n * kc; idx += (int64_t)gridDim.x * SL_BLOCK) {
        const int64_t row = idx / kc, c = idx - row * kc;
        E[idx] = row == c0 + c ? 1.0 : 0.0;
    }
}

// tile (blockIdx.y, blockIdx.x) of the lower triangle of K^-1 = Linv^T Linv, the sum over ascending k
__global__ __launch_bounds__(SL_GS_THREADS) void k_lml_kinv(int64_t n, const double* __restrict__ Linv,
                                                           double* __restrict__ kinv) {
    if (blockIdx.x > blockIdx.y) return;
    const int lane = threadIdx.x & 63, l15 = lane & 15, lk = lane >> 4, wave = threadIdx.x >> 6;
    const int64_t i0 = (int64_t)blockIdx.y * SL_GS_NB + 16 * wave, j0 = (int64_t)blockIdx.x * SL_GS_NB;
    GS_ZERO_ACC(acc);
    gs_strip((int)n,
             [&](int r, int kk) { return kk < n && i0 + r < n ? Linv[(int64_t)kk * n + i0 + r] : 0.0; },
             [&](int kk, int c) { return kk < n && j0 + c < n ? Linv[(int64_t)kk * n + j0 + c] : 0.0; }, acc);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t row = i0 + lk + 4 * r, col = j0 + 16 * t + l15;
            if (row < n && col <= row) kinv[row * n + col] = acc[t][r];
        }
    }
}

// tile (blockIdx.y, blockIdx.x) of the lower triangle: partial[tile][s], s < nslots + 1
__global__ __launch_bounds__(SL_LML_THREADS) void k_lml_grad(const sl_gp_kernel* __restrict__ kern,
                                                            const sl_lml_slots* __restrict__ slots, int64_t n, int p,
                                                            int dout, const double* __restrict__ X,
                                                            const double* __restrict__ B, const double* __restrict__ kinv,
                                                            double* __restrict__ partial) {
    __shared__ sl_gp_kernel ks;
    __shared__ sl_lml_slots sl;
    __shared__ double red[SL_LML_THREADS / 64][SL_LML_MAX_ACC];
    if (blockIdx.x > blockIdx.y) return;
    const int tid = threadIdx.x;
    {
        static_assert(sizeof(sl_gp_kernel) % 4 == 0 && sizeof(sl_lml_slots) % 4 == 0, "copied word by word");
        const uint32_t* s = reinterpret_cast<const uint32_t*>(kern);
        uint32_t* d = reinterpret_cast<uint32_t*>(&ks);
        for (int i = tid; i < (int)(sizeof(sl_gp_kernel) / 4); i += SL_LML_THREADS) d[i] = s[i];
        s = reinterpret_cast<const uint32_t*>(slots);
        d = reinterpret_cast<uint32_t*>(&sl);
        for (int i = tid; i < (int)(sizeof(sl_lml_slots) / 4); i += SL_LML_THREADS) d[i] = s[i];
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6, nslots = sl.nslots, nacc = nslots + 1;
    if (lane < nacc) red[wave][lane] = 0.0;                  // (lane 0 alone adds to it: one wavefront, in order)
    for (int e = 0; e < SL_LML_TILE / 4; ++e) {
        const int64_t row = sl_lml_visit_row(n, (int)blockIdx.y, wave, e);
        if (row < 0) continue;                               // (the same for the whole wavefront)
        sl_lml_entry ent;
        const double coeff = sl_lml_lane(ks, n, p, dout, X, B, kinv, row, (int)blockIdx.x, lane, ent);
        auto add = [&](int s, double v) {                     // (s and the branch to here: the same for every lane)
            for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
            if (lane == 0) red[wave][s] = red[wave][s] + v;
        };
        sl_lml_walk(ks, p, ent, [&](int s, double term) { add(s, coeff * term); });
        add(nslots, (int64_t)blockIdx.x * SL_LML_TILE + lane == row ? coeff : 0.0);
    }
    __syncthreads();
    if (tid < nacc) {
        double v = red[0][tid];
        for (int w = 1; w < SL_LML_THREADS / 64; ++w) v = v + red[w][tid];
        partial[(int64_t)sl_lml_tile_index((int)blockIdx.y, (int)blockIdx.x) * nacc + tid] = v;
    }
}

// One workgroup.  out[2 + s] = the tiles' partials of accumulator s in ascending tile order (thread s);
// out[0] = sum_i log L_ii, out[1] = sum(R o B): thread t adds the terms t, t + 256, ... in ascending order, thread
// 0 adds the 256 sums in ascending order.  L, R or partial may be null (the stage test, the value alone).
__global__ __launch_bounds__(SL_BLOCK) void k_lml_reduce(int64_t n, int dout, const double* __restrict__ L,
                                                        const double* __restrict__ R, const double* __restrict__ B,
                                                        int ntiles, int nacc, const double* __restrict__ partial,
                                                        double* __restrict__ out) {
    __shared__ double sums[2][SL_BLOCK];
    const int tid = threadIdx.x;
    if (partial && tid < nacc) {
        double v = 0.0;
        for (int t = 0; t < ntiles; ++t) v = v + partial[(int64_t)t * nacc + tid];
        out[2 + tid] = v;
    }
    double logs = 0.0, fit = 0.0;
    if (L)
        for (int64_t i = tid; i < n; i += SL_BLOCK) logs = logs + log(L[i * n + i]);
    if (R)
        for (int64_t i = tid; i < n * dout; i += SL_BLOCK) fit = fit + R[i] * B[i];
    sums[0][tid] = logs;
    sums[1][tid] = fit;
    __syncthreads();
    if (tid < 2) {
        double v = 0.0;
        for (int t = 0; t < SL_BLOCK; ++t) v = v + sums[tid][t];
        out[tid] = v;
    }
}

// the device buffers of one call, freed when it ends
struct LmlBuffers {
    double* base = nullptr;
    ~LmlBuffers() { if (base) (void)hipFree(base); }
};

static int lml_check(sl_ctx* ctx, const char* who, int n, int p, int dout, const sl_gp_kernel* h_kernel,
                     sl_lml_slots* slots) {
    if (!h_kernel) return sl_fail(ctx, SL_ERR_INVALID, "%s: no kernel description", who);
    if (n < 0 || dout < 1) return sl_fail(ctx, SL_ERR_INVALID, "%s: n = %d, %d output columns", who, n, dout);
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
    if (n > SL_GS_MAX_TRAIN)
        return sl_fail(ctx, SL_ERR_UNSUPPORTED, "%s: n = %d observations (at most %d)", who, n, SL_GS_MAX_TRAIN);
    const int nslots = sl_lml_compile_slots(*h_kernel, p, slots);
    if (nslots > SL_LML_MAX_SLOTS)
        return sl_fail(ctx, SL_ERR_UNSUPPORTED, "%s: %d hyper-parameter entries that are not zero (at most %d)", who,
                       nslots, SL_LML_MAX_SLOTS);
    return SL_OK;
}

static void lml_zero(double* h_grad_variance, double* h_grad_inv_ls, double* h_grad_noise) {
    for (int i = 0; i < SL_KERNEL_MAX_FACTORS * SL_MAX_INPUT_DIM; ++i) {
        if (h_grad_variance) h_grad_variance[i] = 0.0;
        if (h_grad_inv_ls) h_grad_inv_ls[i] = 0.0;
    }
    if (h_grad_noise) *h_grad_noise = 0.0;
}

// the accumulators of k_lml_reduce into the [nfactors][8] tables of the caller
static void lml_scatter(const sl_lml_slots& slots, const double* acc, double* h_grad_variance, double* h_grad_inv_ls,
                        double* h_grad_noise) {
    lml_zero(h_grad_variance, h_grad_inv_ls, h_grad_noise);
    for (int s = 0; s < slots.nslots; ++s) {
        const sl_lml_slot& sl = slots.slot[s];
        double* table = sl.what == SL_LML_INV_LS ? h_grad_inv_ls : h_grad_variance;
        if (table) table[sl.factor * SL_MAX_INPUT_DIM + sl.q] = acc[s];
    }
    if (h_grad_noise) *h_grad_noise = acc[slots.nslots];
}

// k_lml_grad over every lower tile, k_lml_reduce: d_out [2 + nslots + 1]
static int lml_grad_launch(sl_ctx* ctx, const sl_gp_kernel* d_kern, const sl_lml_slots* d_slots, int nacc, int n, int p,
                           int dout, const double* dX, const double* dL, const double* dR, const double* dB,
                           const double* dKinv, double* d_partial, double* d_out) {
    const int nb = sl_gs_blocks(n);
    hipLaunchKernelGGL(k_lml_grad, dim3(nb, nb), dim3(SL_LML_THREADS), 0, ctx->stream, d_kern, d_slots, (int64_t)n, p, dout,
                       dX, dB, dKinv, d_partial);
    SL_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_lml_reduce, dim3(1), dim3(SL_BLOCK), 0, ctx->stream, (int64_t)n, dout, dL, dR, dB,
                       sl_lml_tiles(n), nacc, d_partial, d_out);
    SL_HIP_CHECK(ctx, hipGetLastError());
    return SL_OK;
}

static size_t lml_round(size_t doubles) { return (doubles + 7) & ~(size_t)7; }

extern "C" int sl_gp_likelihood(sl_ctx* ctx, int n, int p, int dout, const double* h_X, const double* h_R,
                                const sl_gp_kernel* h_kernel, double noise_variance, double* h_lml,
                                double* h_grad_variance, double* h_grad_inv_ls, double* h_grad_noise, int32_t* h_info) {
    const char* who = "sl_gp_likelihood";
    if (!ctx) return sl_fail(nullptr, SL_ERR_INVALID, "%s: null context", who);
    if (h_info) *h_info = 0;
    sl_lml_slots slots;
    if (const int rc = lml_check(ctx, who, n, p, dout, h_kernel, &slots)) return rc;
    if (!h_lml || (n > 0 && (!h_X || !h_R))) return sl_fail(ctx, SL_ERR_INVALID, "%s: a missing buffer", who);
    if (dout > SL_GS_MAX_K)
        return sl_fail(ctx, SL_ERR_UNSUPPORTED, "%s: %d output columns (at most %d)", who, dout, SL_GS_MAX_K);
    const bool want_grad = h_grad_variance || h_grad_inv_ls || h_grad_noise;
    if (n == 0) {
        *h_lml = 0.0;
        lml_zero(h_grad_variance, h_grad_inv_ls, h_grad_noise);
        return SL_OK;
    }
    SL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    // one allocation: [kernel] [slots] [out] [X n p] [R n D] [B n D] [mean n] [K -> L n n], and for the gradient
    // [partial tiles x accumulators] [Linv n n] [K^-1 n n; before it the chunk of identity columns n x kc]
    const size_t nn = (size_t)n, nacc = (size_t)slots.nslots + 1, ntiles = (size_t)sl_lml_tiles(n);
    const size_t o_kern = 0, o_slots = o_kern + lml_round((sizeof(sl_gp_kernel) + 7) / 8);
    const size_t o_out = o_slots + lml_round((sizeof(sl_lml_slots) + 7) / 8), o_X = o_out + lml_round(2 + SL_LML_MAX_ACC);
    const size_t o_R = o_X + lml_round(nn * p), o_B = o_R + lml_round(nn * dout), o_mean = o_B + lml_round(nn * dout);
    const size_t o_K = o_mean + lml_round(nn), o_partial = o_K + lml_round(nn * nn);
    const size_t o_Linv = o_partial + lml_round(ntiles * nacc), o_Kinv = o_Linv + lml_round(nn * nn);
    const size_t total = want_grad ? o_Kinv + lml_round(nn * nn) : o_partial;
    LmlBuffers buf;
    SL_HIP_CHECK(ctx, hipMalloc(&buf.base, sizeof(double) * total));
    double* base = buf.base;
    double *d_out = base + o_out, *dX = base + o_X, *dR = base + o_R, *dB = base + o_B, *dK = base + o_K;
    SL_HIP_CHECK(ctx, hipMemcpyAsync(base + o_kern, h_kernel, sizeof(sl_gp_kernel), hipMemcpyHostToDevice, ctx->stream));
    SL_HIP_CHECK(ctx, hipMemcpyAsync(base + o_slots, &slots, sizeof(slots), hipMemcpyHostToDevice, ctx->stream));
    SL_HIP_CHECK(ctx, hipMemcpyAsync(dX, h_X, sizeof(double) * nn * p, hipMemcpyHostToDevice, ctx->stream));
    SL_HIP_CHECK(ctx, hipMemcpyAsync(dR, h_R, sizeof(double) * nn * dout, hipMemcpyHostToDevice, ctx->stream));
    SL_HIP_CHECK(ctx, hipMemcpyAsync(dB, h_R, sizeof(double) * nn * dout, hipMemcpyHostToDevice, ctx->stream));
    SL_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    // K = k(X, X) + sigma_n^2 I: the prior covariance at X with the noise as its jitter
    if (const int rc = sl_gp_posterior_cov(ctx, 0, p, nullptr, nullptr, nullptr, h_kernel, nullptr, n, dX, noise_variance,
                                           base + o_mean, dK, n))
        return rc;
    if (const int rc = sl_cholesky(ctx, n, dK, n, h_info)) {
        SL_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        return rc;
    }
    // B = L^-T L^-1 R
    if (const int rc = sl_tri_solve(ctx, n, dout, dK, n, 0, dB)) return rc;
    if (const int rc = sl_tri_solve(ctx, n, dout, dK, n, 1, dB)) return rc;
    if (!want_grad) {
        hipLaunchKernelGGL(k_lml_reduce, dim3(1), dim3(SL_BLOCK), 0, ctx->stream, (int64_t)n, dout, dK, dR, dB, 0, 0,
                           (const double*)nullptr, d_out);
        SL_HIP_CHECK(ctx, hipGetLastError());
    } else {
        double *dLinv = base + o_Linv, *dKinv = base + o_Kinv, *dE = dKinv;
        for (int64_t c0 = 0; c0 < n; c0 += SL_GS_MAX_K) {
            const int64_t kc = n - c0 < SL_GS_MAX_K ? n - c0 : SL_GS_MAX_K;
            hipLaunchKernelGGL(k_lml_identity, dim3(sl_grid_blocks(n * kc)), dim3(SL_BLOCK), 0, ctx->stream, (int64_t)n, kc,
                               c0, dE);
            SL_HIP_CHECK(ctx, hipGetLastError());
            if (const int rc = sl_tri_solve(ctx, n, kc, dK, n, 0, dE)) return rc;
            SL_HIP_CHECK(ctx, hipMemcpy2DAsync(dLinv + c0, sizeof(double) * nn, dE, sizeof(double) * kc, sizeof(double) * kc,
                                               nn, hipMemcpyDeviceToDevice, ctx->stream));
        }
        const int nb = sl_gs_blocks(n);
        hipLaunchKernelGGL(k_lml_kinv, dim3(nb, nb), dim3(SL_GS_THREADS), 0, ctx->stream, (int64_t)n, dLinv, dKinv);
        SL_HIP_CHECK(ctx, hipGetLastError());
        if (const int rc = lml_grad_launch(ctx, reinterpret_cast<const sl_gp_kernel*>(base + o_kern),
                                           reinterpret_cast<const sl_lml_slots*>(base + o_slots), (int)nacc, n, p, dout, dX,
                                           dK, dR, dB, dKinv, base + o_partial, d_out))
            return rc;
    }
    double h_out[2 + SL_LML_MAX_ACC] = {};
    SL_HIP_CHECK(ctx, hipMemcpyAsync(h_out, d_out, sizeof(double) * (2 + (want_grad ? nacc : 0)), hipMemcpyDeviceToHost,
                                     ctx->stream));
    SL_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    *h_lml = -0.5 * h_out[1] - (double)dout * h_out[0] - 0.5 * (double)n * (double)dout * 1.8378770664093453;
    if (want_grad) lml_scatter(slots, h_out + 2, h_grad_variance, h_grad_inv_ls, h_grad_noise);
    return SL_OK;
}

// k_lml_grad and k_lml_reduce alone, on a B [n][dout] and a K^-1 [n][n] (its lower triangle is read) from the host
extern "C" int sl_debug_gp_lml_grad(sl_ctx* ctx, int n, int p, int dout, const double* h_X, const double* h_B,
                                    const double* h_Kinv, const sl_gp_kernel* h_kernel, double* h_grad_variance,
                                    double* h_grad_inv_ls, double* h_grad_noise) {
    const char* who = "sl_debug_gp_lml_grad";
    if (!ctx) return sl_fail(nullptr, SL_ERR_INVALID, "%s: null context", who);
    sl_lml_slots slots;
    if (const int rc = lml_check(ctx, who, n, p, dout, h_kernel, &slots)) return rc;
    if (n < 1 || !h_X || !h_B || !h_Kinv) return sl_fail(ctx, SL_ERR_INVALID, "%s: n = %d or a missing buffer", who, n);
    SL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)n, nacc = (size_t)slots.nslots + 1, ntiles = (size_t)sl_lml_tiles(n);
    const size_t o_kern = 0, o_slots = o_kern + lml_round((sizeof(sl_gp_kernel) + 7) / 8);
    const size_t o_out = o_slots + lml_round((sizeof(sl_lml_slots) + 7) / 8), o_X = o_out + lml_round(2 + SL_LML_MAX_ACC);
    const size_t o_B = o_X + lml_round(nn * p), o_partial = o_B + lml_round(nn * dout);
    const size_t o_Kinv = o_partial + lml_round(ntiles * nacc), total = o_Kinv + lml_round(nn * nn);
    LmlBuffers buf;
    SL_HIP_CHECK(ctx, hipMalloc(&buf.base, sizeof(double) * total));
    double* base = buf.base;
    SL_HIP_CHECK(ctx, hipMemcpyAsync(base + o_kern, h_kernel, sizeof(sl_gp_kernel), hipMemcpyHostToDevice, ctx->stream));
    SL_HIP_CHECK(ctx, hipMemcpyAsync(base + o_slots, &slots, sizeof(slots), hipMemcpyHostToDevice, ctx->stream));
    SL_HIP_CHECK(ctx, hipMemcpyAsync(base + o_X, h_X, sizeof(double) * nn * p, hipMemcpyHostToDevice, ctx->stream));
    SL_HIP_CHECK(ctx, hipMemcpyAsync(base + o_B, h_B, sizeof(double) * nn * dout, hipMemcpyHostToDevice, ctx->stream));
    SL_HIP_CHECK(ctx, hipMemcpyAsync(base + o_Kinv, h_Kinv, sizeof(double) * nn * nn, hipMemcpyHostToDevice, ctx->stream));
    SL_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (const int rc = lml_grad_launch(ctx, reinterpret_cast<const sl_gp_kernel*>(base + o_kern),
                                       reinterpret_cast<const sl_lml_slots*>(base + o_slots), (int)nacc, n, p, dout,
                                       base + o_X, nullptr, nullptr, base + o_B, base + o_Kinv, base + o_partial,
                                       base + o_out))
        return rc;
    double h_out[2 + SL_LML_MAX_ACC] = {};
    SL_HIP_CHECK(ctx, hipMemcpyAsync(h_out, base + o_out, sizeof(double) * (2 + nacc), hipMemcpyDeviceToHost, ctx->stream));
    SL_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    lml_scatter(slots, h_out + 2, h_grad_variance, h_grad_inv_ls, h_grad_noise);
    return SL_OK;
}
