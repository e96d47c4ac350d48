// sl_safe_grad.hip - action derivative of the Lyapunov penalty of PolicyIteration.future_values
// (safe_learning/reinforcement_learning.py:107-112, examples/inverted_pendulum.ipynb cell 17): sl_decrease_gradient.
// Per-point arithmetic: sl_safe_grad.h.
//
// The expensive part is L^-1 [k_x | dk_x/du_1 .. dk_x/du_m] per point and GP head: a lower-triangular FP64
// product with (1 + m) columns per point, on v_mfma_f64_16x16x4_f64 with the A fragments the head already
// holds (mpack of sl_gp.hip: [row block I][slab pair S2][lane][2], A[i = lane & 15][k = lane >> 4]).  Per batch
// of 16-point tiles and per head:
//
//   k_sg_generate   (tile, 64-row chunk): k_x and the m derivative columns of the tile's points in B-fragment
//                   order ([column set][slab pair][lane][2], B[k = lane >> 4][point = lane & 15]) into the
//                   context's scratch
//   k_sg_gemm       a four-wavefront workgroup per tile; wavefront w owns the row blocks w, w + 4, ..: (1 + m)
//                   accumulator tiles, squared and multiplied in registers into sum a^2 and sum a b_c; the
//                   partial sums cross LDS once per tile and are added in wavefront order
//   k_sg_epilogue   one thread per point: mean and Jacobian (sl_pg_head, ascending training point: the
//                   successor of sl_action_gradient bit for bit), variances, V_L, L_v, C and dC/du
//
// No atomics; a point's results depend on that point alone (its column of the product), so they do not
// depend on the tile it falls into or on the batch: the same bits at every call and for every split of a call.
#include "sl_grad_host.h"
#include "sl_safe_grad.h"

typedef double sl_sg4 __attribute__((ext_vector_type(4)));
typedef double sl_sg2 __attribute__((ext_vector_type(2)));

#define SL_SG_WAVES 4
#define SL_SG_SCRATCH_TILES ((size_t)64 << 20)       // B fragments of one batch of tiles: at most 64 MiB

// u = policy(x) at every point (the actions are explicit from here on)
__global__ __launch_bounds__(SL_BLOCK) void k_sg_actions(const SlDevModel M, SlAux aux_in, int64_t n,
                                                        const double* __restrict__ points,
                                                        double* __restrict__ actions) {
    __shared__ SlTriLds<true> lds;
    const SlAux aux = sl_stage_aux<true>(lds, aux_in);
    const SlDims nd = sl_dims<0, 0>(M);
    for (int64_t idx = (int64_t)blockIdx.x * SL_BLOCK + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * SL_BLOCK) {
        double x[SL_P], u[SL_M];
        sl_cell_state(M, nd.d, idx, points, x);
        sl_policy_any<true>(M, nd, aux.tri, idx, x, u);
#pragma unroll
        for (int c = 0; c < SL_M; ++c) if (c < nd.m) actions[idx * nd.m + c] = u[c];
    }
}

// z = [x, u] of point idx (a point past n: the last point; its columns are zeroed by the caller)
__device__ __forceinline__ void sg_point_input(const SlDevModel& M, SlDims nd, int64_t idx,
                                               const double* __restrict__ points,
                                               const double* __restrict__ actions, double* z) {
#pragma unroll
    for (int q = 0; q < SL_P; ++q) z[q] = 0.0;
    sl_cell_state(M, nd.d, idx, points, z);
    double u[SL_M];
#pragma unroll
    for (int c = 0; c < SL_M; ++c) u[c] = c < nd.m ? actions[idx * nd.m + c] : 0.0;
    sl_append_action(nd, u, z);
}

// blockIdx.x: 64-row chunk, blockIdx.y: tile of the batch.  Wavefront w writes the slabs w, w + 4, w + 8, w + 12
// of the chunk: lane (lk, lcol) = training point 4 s + lk, point lcol of the tile.
__global__ __launch_bounds__(64 * SL_SG_WAVES) void k_sg_generate(const SlDevModel M, const SlGpHeadDev hd, int64_t n,
                                                                  int64_t first, const double* __restrict__ points,
                                                                  const double* __restrict__ actions,
                                                                  double* __restrict__ bfrag) {
    const SlDims nd = sl_dims<0, 0>(M);
    const int d = nd.d, m = nd.m, p = nd.p;
    const int lane = threadIdx.x & 63, lcol = lane & 15, lk = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ch = blockIdx.x;
    const int64_t tile = blockIdx.y;
    int64_t idx = first + tile * 16 + lcol;
    const bool valid = idx < n;
    idx = valid ? idx : n - 1;
    double z[SL_P], xg[SL_P];
    sg_point_input(M, nd, idx, points, actions, z);
#pragma unroll
    for (int q = 0; q < SL_P; ++q) xg[q] = (q < p) ? z[q] * hd.inv_ls[q] : 0.0;
    double* __restrict__ out = bfrag + (size_t)tile * (1 + m) * hd.nslab2 * 128;
    for (int k = 0; k < 4; ++k) {
        const int s = wave + k * SL_SG_WAVES;
        const int j = 64 * ch + 4 * s + lk;
        double kx = 0.0, dk[SL_M];
#pragma unroll
        for (int c = 0; c < SL_M; ++c) dk[c] = 0.0;
        if (valid && j < hd.n) {
            double xa[SL_P];
#pragma unroll
            for (int q = 0; q < SL_P; ++q) xa[q] = (q < p) ? hd.xs[q * hd.n_pad + j] : 0.0;
            kx = hd.kernel ? sl_pg_kernel(*hd.kernel, p, d, m, xa, xg, dk)
                           : sl_pg_rbf(hd.variance, hd.inv_ls, p, d, m, xa, xg, dk);
        }
        const size_t at = (((size_t)(8 * ch + (s >> 1))) * 64 + lane) * 2 + (s & 1);
        out[at] = kx;
#pragma unroll
        for (int c = 0; c < SL_M; ++c)
            if (c < m) out[(size_t)(c + 1) * hd.nslab2 * 128 + at] = dk[c];
    }
}

// One workgroup per tile of the batch.  ss [points of the batch], sab [points of the batch][SL_M].
__global__ __launch_bounds__(64 * SL_SG_WAVES) void k_sg_gemm(const SlGpHeadDev hd, int m, int64_t n, int64_t first,
                                                              const double* __restrict__ bfrag,
                                                              double* __restrict__ ss_out,
                                                              double* __restrict__ sab_out) {
    __shared__ double part[SL_SG_WAVES][16][1 + SL_M];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t tile = blockIdx.x;
    const int nslab2 = hd.nslab2;
    const double* __restrict__ bt = bfrag + (size_t)tile * (1 + m) * nslab2 * 128;
    const double* __restrict__ mpack = hd.mpack;
    const int nrb = (hd.n + 15) >> 4;                       // row blocks that hold training points
    double ss = 0.0, sab[SL_M];
#pragma unroll
    for (int c = 0; c < SL_M; ++c) sab[c] = 0.0;
    for (int I = wave; I < nrb; I += SL_SG_WAVES) {
        sl_sg4 acc[1 + SL_M];
#pragma unroll
        for (int c = 0; c <= SL_M; ++c) acc[c] = (sl_sg4){0.0, 0.0, 0.0, 0.0};
        int cnt = 2 * I + 2;                                // slab pairs on or below the diagonal
        cnt = cnt < nslab2 ? cnt : nslab2;
        for (int s2 = 0; s2 < cnt; ++s2) {
            const sl_sg2 a = *reinterpret_cast<const sl_sg2*>(mpack + ((size_t)I * nslab2 + s2) * 128 + lane * 2);
#pragma unroll
            for (int c = 0; c <= SL_M; ++c) {
                if (c <= m) {
                    const sl_sg2 b = *reinterpret_cast<const sl_sg2*>(bt + ((size_t)c * nslab2 + s2) * 128 + lane * 2);
                    acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, b.x, acc[c], 0, 0, 0);
                    acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, b.y, acc[c], 0, 0, 0);
                }
            }
        }
        // register r of lane (lcol, lk): row 16 I + lk + 4 r of column lcol
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            ss = fma(acc[0][r], acc[0][r], ss);
#pragma unroll
            for (int c = 0; c < SL_M; ++c) if (c < m) sab[c] = fma(acc[0][r], acc[c + 1][r], sab[c]);
        }
    }
    // the four lane groups of a column, then the wavefronts in order
    ss += __shfl_xor(ss, 16, 64);
    ss += __shfl_xor(ss, 32, 64);
#pragma unroll
    for (int c = 0; c < SL_M; ++c) {
        sab[c] += __shfl_xor(sab[c], 16, 64);
        sab[c] += __shfl_xor(sab[c], 32, 64);
    }
    if (lane < 16) {
        part[wave][lane][0] = ss;
#pragma unroll
        for (int c = 0; c < SL_M; ++c) part[wave][lane][1 + c] = sab[c];
    }
    __syncthreads();
    if (threadIdx.x < 16) {
        const int64_t local = tile * 16 + threadIdx.x;
        if (first + local < n) {
            double t = part[0][threadIdx.x][0];
            for (int w = 1; w < SL_SG_WAVES; ++w) t = t + part[w][threadIdx.x][0];
            ss_out[local] = t;
#pragma unroll
            for (int c = 0; c < SL_M; ++c) {
                double u = part[0][threadIdx.x][1 + c];
                for (int w = 1; w < SL_SG_WAVES; ++w) u = u + part[w][threadIdx.x][1 + c];
                sab_out[local * SL_M + c] = u;
            }
        }
    }
}

struct SlSafeGradArgs {
    int64_t n, first, count;   // points of the call, first point and number of points of the batch
    const double* points;      // [n][d] or null: the grid points of the model
    const double* actions;     // [n][m]
    const double* ss;          // [heads][count]
    const double* sab;         // [heads][count][SL_M]
    double* grad;              // [n][m]
    double* constraint;        // [n] or null
    double* terms;             // [n][2 + 2 d] or null
};

__global__ __launch_bounds__(SL_BLOCK) void k_sg_epilogue(const SlDevModel M, const SlGpDev gp, SlAux aux_in,
                                                         SlSafeGradArgs a) {
    __shared__ SlTriLds<true> lds;
    const SlAux aux = sl_stage_aux<true>(lds, aux_in);
    const SlDims nd = sl_dims<0, 0>(M);
    const int d = nd.d, m = nd.m, p = nd.p;
    const SlTri& vt = aux.tri[0];
    for (int64_t local = (int64_t)blockIdx.x * SL_BLOCK + threadIdx.x; local < a.count;
         local += (int64_t)gridDim.x * SL_BLOCK) {
        const int64_t idx = a.first + local;
        double z[SL_P];
        sg_point_input(M, nd, idx, a.points, a.actions, z);
        double mean[SL_D], jac[SL_D][SL_M], var[SL_D], dvar[SL_D][SL_M];
#pragma unroll
        for (int k = 0; k < SL_D; ++k) {
            mean[k] = 0.0;
            var[k] = 0.0;
#pragma unroll
            for (int c = 0; c < SL_M; ++c) { jac[k][c] = 0.0; dvar[k][c] = 0.0; }
        }
        for (int h = 0; h < gp.nheads; ++h) {
            const SlGpHeadDev& hd = gp.head[h];
            const SlPgHead head{hd.n, hd.n_pad, hd.dout, hd.col0, hd.variance, hd.inv_ls, hd.xs, hd.alpha, hd.kernel};
            sl_pg_head(head, p, d, m, z, mean, jac);
            double dprior[SL_M], dv[SL_M], sab[SL_M];
            const double prior = sl_sg_prior(head, p, d, m, z, dprior);
#pragma unroll
            for (int c = 0; c < SL_M; ++c) sab[c] = a.sab[((int64_t)h * a.count + local) * SL_M + c];
            const double v = sl_sg_variance(prior, dprior, a.ss[(int64_t)h * a.count + local], sab, m, dv);
#pragma unroll
            for (int k = 0; k < SL_D; ++k) {
                const int dd = k - hd.col0;
                if (k < d && dd >= 0 && dd < hd.dout) {
                    var[k] = v;
#pragma unroll
                    for (int c = 0; c < SL_M; ++c) dvar[k][c] = dv[c];
                }
            }
        }
        sl_pg_linear_part(M.m.dynamics, d, m, z, mean, jac);
        double err[SL_D], g[SL_M];
        const SlSgPoint r = sl_sg_point(M, vt, gp.beta, d, m, z, mean, jac, var, dvar, err, g);
#pragma unroll
        for (int c = 0; c < SL_M; ++c) if (c < m) a.grad[idx * m + c] = g[c];
        if (a.constraint) a.constraint[idx] = r.constraint;
        if (a.terms) {
            double* o = a.terms + idx * (2 + 2 * d);
            o[0] = r.decrease;
            o[1] = r.threshold;
#pragma unroll
            for (int k = 0; k < SL_D; ++k) if (k < d) { o[2 + k] = mean[k]; o[2 + d + k] = err[k]; }
        }
    }
}

extern "C" int sl_decrease_gradient(sl_ctx* ctx, int64_t n, const double* d_points, const double* d_actions,
                                    double* d_grad, double* d_constraint, double* d_terms) {
    const char* who = "sl_decrease_gradient";
    if (const int rc = sl_point_grad_arguments(ctx, who, n, d_grad)) return rc;
    const sl_model_desc& md = ctx->h_model.m;
    const int dk = md.dynamics.kind;
    if (dk == SL_DYN_PENDULUM || dk == SL_DYN_CARTPOLE)
        return sl_fail(ctx, SL_ERR_UNSUPPORTED, "sl_decrease_gradient: Euler dynamics (kind %d); the gradient of the "
                       "Lyapunov penalty is implemented for SL_DYN_GP", dk);
    if (dk == SL_DYN_POLYNOMIAL)
        return sl_fail(ctx, SL_ERR_UNSUPPORTED, "sl_decrease_gradient: polynomial dynamics (SL_DYN_POLYNOMIAL) have no "
                       "action tangent in the engine yet; the gradient of the Lyapunov penalty is implemented for GP "
                       "dynamics");
    if (dk != SL_DYN_GP)
        return sl_fail(ctx, SL_ERR_UNSUPPORTED, "sl_decrease_gradient: linear dynamics (kind %d) carry no error bound; "
                       "the gradient of the Lyapunov penalty is implemented for SL_DYN_GP", dk);
    if (md.value.kind == SL_V_NETWORK)
        return sl_fail(ctx, SL_ERR_UNSUPPORTED, "sl_decrease_gradient: a network Lyapunov function (SL_V_NETWORK) is "
                       "not differentiated; use a quadratic form or a table");
    if (md.value.kind == SL_V_POLYNOMIAL)
        return sl_fail(ctx, SL_ERR_UNSUPPORTED, "sl_decrease_gradient: a polynomial Lyapunov function "
                       "(SL_V_POLYNOMIAL) is not differentiated: the derivative of |grad V| needs second "
                       "derivatives; use a quadratic form or a table");
    const int d = md.grid.d, m = md.policy.m, p = ctx->h_model.in_dim;
    if (md.value.kind == SL_V_TRI && (!ctx->h_tri[0].set || ctx->h_tri[0].grid.d != d))
        return sl_fail(ctx, SL_ERR_INVALID, "sl_decrease_gradient: the Lyapunov table must be slot 0, on %d dimensions", d);
    if (const int rc = sl_point_grad_gp_heads(ctx, who)) return rc;
    int covered = 0;
    size_t rows_max = 0;
    for (int h = 0; h < ctx->h_gp.nheads; ++h) {
        const SlGpHeadHost& hh = ctx->gp_heads[h];
        if (hh.p != p)
            return sl_fail(ctx, SL_ERR_INVALID, "sl_decrease_gradient: GP head %d has input dim %d, model has %d", h,
                           hh.p, p);
        if (hh.n_pad % 64 != 0)
            return sl_fail(ctx, SL_ERR_INVALID, "sl_decrease_gradient: GP head %d padded to %d rows", h, hh.n_pad);
        covered += hh.dout;
        rows_max = (size_t)hh.n_pad > rows_max ? (size_t)hh.n_pad : rows_max;
    }
    if (covered != d)
        return sl_fail(ctx, SL_ERR_INVALID, "sl_decrease_gradient: GP heads cover %d outputs, state dimension is %d",
                       covered, d);
    if (const int rc = sl_point_grad_on_grid(ctx, who, n, d_points)) return rc;
    if (n == 0) return SL_OK;
    SL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    // a network policy: one action per point first, as everywhere else
    SlPolicyTableScope network_policy(ctx, 0, d_actions ? 0 : n, d_points);
    if (const int rc = sl_point_grad_policy(ctx, who, d_points, d_actions, network_policy)) return rc;
    // scratch: [actions n m (policy only)] [B fragments of a batch] [ss heads x batch] [sab heads x batch x SL_M]
    const int64_t ntiles = (n + 15) / 16;
    const size_t tile_doubles = (size_t)16 * (1 + m) * rows_max;
    int64_t batch_tiles = (int64_t)(SL_SG_SCRATCH_TILES / (tile_doubles * sizeof(double)));
    batch_tiles = batch_tiles < 1 ? 1 : batch_tiles;
    batch_tiles = batch_tiles > ntiles ? ntiles : batch_tiles;
    batch_tiles = batch_tiles > 32768 ? 32768 : batch_tiles;            // (blockIdx.y of k_sg_generate)
    const size_t batch_points = (size_t)batch_tiles * 16;
    const size_t nheads = (size_t)ctx->h_gp.nheads;
    const size_t act_doubles = d_actions ? 0 : (((size_t)n * m + 1) & ~(size_t)1);
    const size_t need = sizeof(double) * (act_doubles + tile_doubles * batch_tiles + nheads * batch_points * (1 + SL_M));
    SL_HIP_CHECK(ctx, sl_grow(ctx, &ctx->d_scratch, &ctx->scratch_bytes, need, (size_t)1 << 20));
    double* scratch = reinterpret_cast<double*>(ctx->d_scratch);
    double* bfrag = scratch + act_doubles;
    double* ss = bfrag + tile_doubles * batch_tiles;
    double* sab = ss + nheads * batch_points;
    const SlAux aux{ctx->d_tri, ctx->d_net};
    const SlDevModel& M = ctx->h_model;
    if (!d_actions) {
        hipLaunchKernelGGL(k_sg_actions, dim3(sl_grid_blocks(n)), dim3(SL_BLOCK), 0, ctx->stream, M, aux, n, d_points,
                           scratch);
        SL_HIP_CHECK(ctx, hipGetLastError());
        d_actions = scratch;
    }
    for (int64_t t0 = 0; t0 < ntiles; t0 += batch_tiles) {
        const int64_t tiles = ntiles - t0 < batch_tiles ? ntiles - t0 : batch_tiles;
        const int64_t first = t0 * 16;
        const int64_t count = n - first < tiles * 16 ? n - first : tiles * 16;
        for (int h = 0; h < ctx->h_gp.nheads; ++h) {
            const SlGpHeadDev& hd = ctx->h_gp.head[h];
            hipLaunchKernelGGL(k_sg_generate, dim3((unsigned)(hd.n_pad / 64), (unsigned)tiles), dim3(64 * SL_SG_WAVES), 0,
                               ctx->stream, M, hd, n, first, d_points, d_actions, bfrag);
            SL_HIP_CHECK(ctx, hipGetLastError());
            hipLaunchKernelGGL(k_sg_gemm, dim3((unsigned)tiles), dim3(64 * SL_SG_WAVES), 0, ctx->stream, hd, m, n, first,
                               bfrag, ss + (size_t)h * count, sab + (size_t)h * count * SL_M);
            SL_HIP_CHECK(ctx, hipGetLastError());
        }
        const SlSafeGradArgs a{n, first, count, d_points, d_actions, ss, sab, d_grad, d_constraint, d_terms};
        hipLaunchKernelGGL(k_sg_epilogue, dim3(sl_grid_blocks(count)), dim3(SL_BLOCK), 0, ctx->stream, M, ctx->h_gp, aux,
                           a);
        SL_HIP_CHECK(ctx, hipGetLastError());
    }
    return SL_OK;
}
