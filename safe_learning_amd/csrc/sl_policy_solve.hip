// sl_policy_solve.hip - exact evaluation of a fixed policy: V = r + gamma P V.
//
// sl_policy_operator writes the rows of P and r (sl_policy_rows.h) for the vertices of the value
// grid: policy, dynamics mean and point location exactly as the policy-evaluation sweep
// (sl_bellman_sweep, n_actions = 0) computes them.  sl_value_solve solves (I - gamma P) V = r for
// any such ELL operator by restarted GMRES(m) with classical Gram-Schmidt applied twice, safeguarded
// by Jacobi steps (the value-iteration sweep itself), or by Jacobi alone.
//
// Every reduction has a fixed order: per-block partials in a fixed grid (a function of n only),
// then one workgroup adds them up.  No floating-point atomics: two calls give the same bits.  The
// host reads one small status record per restart cycle.
#include "sl_common.h"
#include "sl_policy_rows.h"

#define SL_GM_MAXM   32          // largest restart length
#define SL_GM_CHUNK  16          // basis vectors per pass of the fused multi-dot / update kernels
#define SL_RED_MAXB  1024        // blocks of the reduction kernels (fixed per n)

// ---- fixed-order block reductions (SL_BLOCK = 4 wavefronts of 64) ----------------------------
__device__ __forceinline__ double sl_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double sl_wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

static inline int sl_red_blocks(int64_t n) {
    int64_t b = (n + SL_BLOCK - 1) / SL_BLOCK;
    return (int)(b < 1 ? 1 : (b > SL_RED_MAXB ? SL_RED_MAXB : b));
}

// =============================================================================================
// operator rows
// =============================================================================================
// One thread per vertex of [lo, hi): policy, next-state mean, reward, located successor.
// part[block * 2 + 0]: rows with a negative weight, part[block * 2 + 1]: max sum |w|.
template <int D>
__global__ __launch_bounds__(SL_BLOCK) void k_policy_operator_rows(
    const SlDevModel M, const SlGpDev gp, SlAux aux, int64_t lo, int64_t hi,
    int32_t* __restrict__ cols, double* __restrict__ w, double* __restrict__ r,
    double* __restrict__ part) {
    __shared__ SlTri vt_lds;
    __shared__ double red[2][SL_BLOCK / 64];
    sl_stage_tri(&vt_lds, &aux.tri[0]);
    const SlTri& vt = vt_lds;
    const SlDims nd = sl_dims<0, 0>(M);
    const int64_t n = hi - lo;
    const bool negate = M.m.value.negate != 0;
    double nneg = 0.0, amax = 0.0;
    for (int64_t idx = lo + (int64_t)blockIdx.x * SL_BLOCK + threadIdx.x; idx < hi;
         idx += (int64_t)gridDim.x * SL_BLOCK) {
        double x[SL_P], u[SL_M], nxt[SL_D];
        sl_index_to_state(M.m.grid, M.gf, nd.d, idx, x);
        sl_policy_any<true>(M, nd, aux.tri, idx, x, u);
        sl_append_action(nd, u, x);
        sl_next_state_mean(M, gp, nd, x, nxt);
        const int64_t i = idx - lo;
        r[i] = sl_quadratic(M.m.reward, nd.p, x);
        int32_t c[D + 1];
        double wt[D + 1], s;
        bool neg;
        sl_policy_row<D>(vt, nxt, negate, c, wt, &neg, &s);
#pragma unroll
        for (int k = 0; k <= D; ++k) {
            cols[k * n + i] = c[k];
            w[k * n + i] = wt[k];
        }
        nneg += neg ? 1.0 : 0.0;
        amax = fmax(amax, s);
    }
    nneg = sl_wave_sum(nneg);
    amax = sl_wave_max(amax);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][wave] = nneg; red[1][wave] = amax; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0;
        for (int q = 0; q < SL_BLOCK / 64; ++q) { a += red[0][q]; b = fmax(b, red[1][q]); }
        part[blockIdx.x * 2 + 0] = a;
        part[blockIdx.x * 2 + 1] = b;
    }
}

// one workgroup: the partials of nblk blocks in block order (sum of column 0, max of column 1)
__global__ __launch_bounds__(SL_BLOCK) void k_policy_operator_stats(const double* __restrict__ part, int nblk,
                                                                    double gamma, double* __restrict__ stats) {
    __shared__ double red[2][SL_BLOCK];
    double a = 0.0, b = 0.0;
    for (int q = threadIdx.x; q < nblk; q += SL_BLOCK) { a += part[q * 2]; b = fmax(b, part[q * 2 + 1]); }
    red[0][threadIdx.x] = a;
    red[1][threadIdx.x] = b;
    __syncthreads();
    for (int s = SL_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            red[0][threadIdx.x] += red[0][threadIdx.x + s];
            red[1][threadIdx.x] = fmax(red[1][threadIdx.x], red[1][threadIdx.x + s]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        stats[0] = red[0][0];
        stats[1] = gamma * red[1][0];
    }
}

extern "C" int sl_policy_operator(sl_ctx* ctx, int64_t lo, int64_t hi, int32_t* d_cols, double* d_w,
                                  double* d_r, double* d_stats) {
    if (!ctx) return sl_fail(nullptr, SL_ERR_INVALID, "sl_policy_operator: NULL context");
    if (!ctx->model_set) return sl_fail(ctx, SL_ERR_INVALID, "sl_policy_operator: call sl_model_set first");
    if (!ctx->h_tri[0].set)
        return sl_fail(ctx, SL_ERR_INVALID, "sl_policy_operator: value table (sl_tri_set slot 0) not set");
    const SlDevModel& M = ctx->h_model;
    if (M.m.value.kind != SL_V_TRI)
        return sl_fail(ctx, SL_ERR_INVALID, "sl_policy_operator: the value function must be a Triangulation");
    if (M.m.reward.kind != SL_V_QUADRATIC)
        return sl_fail(ctx, SL_ERR_INVALID, "sl_policy_operator: reward must be a QuadraticFunction");
    const int d = M.m.grid.d;
    if (ctx->h_tri[0].grid.d != d)
        return sl_fail(ctx, SL_ERR_INVALID, "sl_policy_operator: value grid / model grid mismatch");
    for (int k = 0; k < d; ++k)
        if (ctx->h_tri[0].grid.num_points[k] != M.m.grid.num_points[k])
            return sl_fail(ctx, SL_ERR_INVALID, "sl_policy_operator: value grid / model grid mismatch");
    if (d < 1 || d > 4)
        return sl_fail(ctx, SL_ERR_UNSUPPORTED, "sl_policy_operator: %d-dimensional grid (1 to 4)", d);
    if (!sl_policy_rows_fit(M.gf.nindex))
        return sl_fail(ctx, SL_ERR_UNSUPPORTED, "sl_policy_operator: %lld vertices do not fit int32 "
                                                "column indices", (long long)M.gf.nindex);
    if (lo < 0 || hi < lo || hi > M.gf.nindex || !d_cols || !d_w || !d_r || !d_stats)
        return sl_fail(ctx, SL_ERR_INVALID, "sl_policy_operator: bad range or NULL output");
    if (M.m.policy.kind == SL_POLICY_TRI && !ctx->h_tri[1].set)
        return sl_fail(ctx, SL_ERR_INVALID, "sl_policy_operator: policy table not set");
    if (M.m.dynamics.kind == SL_DYN_GP && ctx->h_gp.nheads < 1)
        return sl_fail(ctx, SL_ERR_INVALID, "sl_policy_operator: GP dynamics without heads");
    SL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    SL_HIP_CHECK(ctx, hipMemsetAsync(d_stats, 0, 2 * sizeof(double), ctx->stream));
    if (hi == lo) return SL_OK;
    // a network policy: one action per vertex first, as the sweeps do
    SlPolicyTableScope network_policy(ctx, lo, hi, nullptr);
    if (network_policy.rc) return network_policy.rc;
    const int nblk = sl_grid_blocks(hi - lo);
    SL_HIP_CHECK(ctx, sl_grow(ctx, &ctx->d_scratch, &ctx->scratch_bytes, sizeof(double) * 2 * (size_t)nblk));
    double* part = reinterpret_cast<double*>(ctx->d_scratch);
    SlAux aux{ctx->d_tri, ctx->d_net};
    const int rc = sl_with_dim<1, 2, 3, 4>(d, [&](auto dt) {
        hipLaunchKernelGGL(k_policy_operator_rows<dt>, dim3(nblk), dim3(SL_BLOCK), 0, ctx->stream, ctx->h_model,
                           ctx->h_gp, aux, lo, hi, d_cols, d_w, d_r, part);
        SL_HIP_CHECK(ctx, hipGetLastError());
        return SL_OK;
    });
    if (rc) return rc;
    hipLaunchKernelGGL(k_policy_operator_stats, dim3(1), dim3(SL_BLOCK), 0, ctx->stream, part, nblk,
                       M.m.gamma, d_stats);
    SL_HIP_CHECK(ctx, hipGetLastError());
    sl_note_kernel(ctx, false, "k_policy_operator_rows<d=%d>", d);
    return SL_OK;
}

// =============================================================================================
// the solver
// =============================================================================================
// Device-side state of one solve: the Hessenberg matrix (rotated into R as the cycle goes), the
// Givens rotations, the right-hand side g of the small least-squares problem, and the status the
// host reads once per cycle.
struct SlSolveState {
    double H[SL_GM_MAXM + 1][SL_GM_MAXM];
    double cs[SL_GM_MAXM], sn[SL_GM_MAXM], g[SL_GM_MAXM + 1], y[SL_GM_MAXM];
    double h[SL_GM_MAXM + 1];    // coefficients of the current Gram-Schmidt pass
    double inv_norm;             // 1 / norm of the vector the scale kernel normalises
    double target;               // 2-norm below which the residual estimate ends a cycle
    int32_t steps, stop;         // Arnoldi steps done in this cycle; 1: skip the rest of the cycle
    // status record (host): of the iterate whose residual the last k_solve_status reduced
    double res_inf, res_2;
    // k_solve_prep: max |r|, max sum |w|, entries that are not finite / columns out of range
    double r_inf, w_abs, bad, pad_;
};

// max |r|, max_i sum_k |w_ik|, and a count of non-finite r / w / v entries and of columns
// outside [0, n) - checked before any gather reads x[cols]
__global__ __launch_bounds__(SL_BLOCK) void k_solve_prep(int64_t n, int k, const int32_t* __restrict__ cols,
                                                         const double* __restrict__ w,
                                                         const double* __restrict__ r,
                                                         const double* __restrict__ v,
                                                         double* __restrict__ part) {
    __shared__ double red[3][SL_BLOCK / 64];
    double rmax = 0.0, wmax = 0.0, bad = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * SL_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * SL_BLOCK) {
        const double ri = r[i], vi = v[i];
        bad += (isfinite(ri) && isfinite(vi)) ? 0.0 : 1.0;
        rmax = fmax(rmax, fabs(ri));
        double s = 0.0;
        for (int q = 0; q < k; ++q) {
            const double wq = w[q * n + i];
            const int32_t c = cols[q * n + i];
            bad += (isfinite(wq) && c >= 0 && (int64_t)c < n) ? 0.0 : 1.0;
            s += fabs(wq);
        }
        wmax = fmax(wmax, s);
    }
    rmax = sl_wave_max(rmax);
    wmax = sl_wave_max(wmax);
    bad = sl_wave_sum(bad);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][wave] = rmax; red[1][wave] = wmax; red[2][wave] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0, c = 0.0;
        for (int q = 0; q < SL_BLOCK / 64; ++q) { a = fmax(a, red[0][q]); b = fmax(b, red[1][q]); c += red[2][q]; }
        part[blockIdx.x * 3 + 0] = a;
        part[blockIdx.x * 3 + 1] = b;
        part[blockIdx.x * 3 + 2] = c;
    }
}

__global__ __launch_bounds__(SL_BLOCK) void k_solve_prep_reduce(const double* __restrict__ part, int nblk,
                                                                SlSolveState* st) {
    __shared__ double red[3][SL_BLOCK];
    double a = 0.0, b = 0.0, c = 0.0;
    for (int q = threadIdx.x; q < nblk; q += SL_BLOCK) {
        a = fmax(a, part[q * 3]);
        b = fmax(b, part[q * 3 + 1]);
        c += part[q * 3 + 2];
    }
    red[0][threadIdx.x] = a; red[1][threadIdx.x] = b; red[2][threadIdx.x] = c;
    __syncthreads();
    for (int s = SL_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            red[0][threadIdx.x] = fmax(red[0][threadIdx.x], red[0][threadIdx.x + s]);
            red[1][threadIdx.x] = fmax(red[1][threadIdx.x], red[1][threadIdx.x + s]);
            red[2][threadIdx.x] += red[2][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { st->r_inf = red[0][0]; st->w_abs = red[1][0]; st->bad = red[2][0]; }
}

// y = MODE 0: x - gamma P x (the GMRES operator), 1: r + gamma P x (a Jacobi step; the partials
// get max |y - x|, the residual of x), 2: r + gamma P x - x (the residual; partials: max |y|,
// sum y^2).  `stop`: a skipped Arnoldi step (st->stop set) does nothing.
template <int MODE, int KMAX>
__global__ __launch_bounds__(SL_BLOCK) void k_value_matvec(int64_t n, int k, const int32_t* __restrict__ cols,
                                                           const double* __restrict__ w,
                                                           const double* __restrict__ r, double gamma,
                                                           const double* __restrict__ x, double* __restrict__ y,
                                                           double* __restrict__ part, const SlSolveState* st) {
    if (st && st->stop) return;
    __shared__ double red[2][SL_BLOCK / 64];
    double rmax = 0.0, rsum = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * SL_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * SL_BLOCK) {
        double wv[KMAX], vals[KMAX];
#pragma unroll
        for (int q = 0; q < KMAX; ++q) {
            if (q < k) {
                wv[q] = w[q * n + i];
                vals[q] = x[cols[q * n + i]];
            } else {
                wv[q] = 0.0;
                vals[q] = 0.0;
            }
        }
        const double pv = sl_policy_row_dot<KMAX>(k, wv, vals);
        const double xi = x[i];
        if (MODE == 0) {
            const double t = gamma * pv;
            y[i] = xi - t;
        } else {
            const double t = sl_policy_row_combine(r[i], gamma, pv);
            const double res = t - xi;
            y[i] = MODE == 1 ? t : res;
            // a non-finite entry (a diverging iterate: inf - inf = NaN) counts as an infinite
            // residual - fmax would drop a NaN
            const double ares = isfinite(res) ? fabs(res) : INFINITY;
            rmax = fmax(rmax, ares);
            if (MODE == 2) rsum = fma(ares, ares, rsum);
        }
    }
    if (MODE == 0 || !part) return;
    rmax = sl_wave_max(rmax);
    rsum = sl_wave_sum(rsum);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][wave] = rmax; red[1][wave] = rsum; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0;
        for (int q = 0; q < SL_BLOCK / 64; ++q) { a = fmax(a, red[0][q]); b += red[1][q]; }
        part[blockIdx.x * 2 + 0] = a;
        part[blockIdx.x * 2 + 1] = b;
    }
}

// status of the iterate whose residual the last MODE 1 / 2 matvec reduced: res_inf, res_2; with
// `start` the GMRES cycle begins from that residual (beta = res_2, V_0 = residual / beta)
__global__ __launch_bounds__(SL_BLOCK) void k_solve_status(const double* __restrict__ part, int nblk,
                                                           SlSolveState* st, int start, double tol_abs) {
    __shared__ double red[2][SL_BLOCK];
    double a = 0.0, b = 0.0;
    for (int q = threadIdx.x; q < nblk; q += SL_BLOCK) { a = fmax(a, part[q * 2]); b += part[q * 2 + 1]; }
    red[0][threadIdx.x] = a;
    red[1][threadIdx.x] = b;
    __syncthreads();
    for (int s = SL_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            red[0][threadIdx.x] = fmax(red[0][threadIdx.x], red[0][threadIdx.x + s]);
            red[1][threadIdx.x] += red[1][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double rinf = red[0][0], r2 = sqrt(red[1][0]);
    st->res_inf = rinf;
    st->res_2 = r2;
    if (!start) return;
    for (int i = 0; i <= SL_GM_MAXM; ++i) {
        st->g[i] = 0.0;
        for (int j = 0; j < SL_GM_MAXM; ++j) if (i < SL_GM_MAXM + 1) st->H[i][j] = 0.0;
    }
    st->g[0] = r2;
    st->steps = 0;
    st->stop = (r2 > 0.0 && rinf > tol_abs && isfinite(r2)) ? 0 : 1;
    st->inv_norm = r2 > 0.0 ? 1.0 / r2 : 0.0;
    // the estimate |g_j| bounds the 2-norm of the residual; ||.||_inf <= ||.||_2 ends the cycle
    // early once the 2-norm is below the inf-norm target
    st->target = tol_abs;
}

// v *= st->inv_norm
__global__ __launch_bounds__(SL_BLOCK) void k_gm_scale(int64_t n, double* __restrict__ v, const SlSolveState* st) {
    if (st->stop) return;
    const double s = st->inv_norm;
    for (int64_t i = (int64_t)blockIdx.x * SL_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * SL_BLOCK)
        v[i] = v[i] * s;
}

// fused multi-dot: part[block][q] = sum over the block's rows of V_{q0 + q}[i] * w[i], q < nv
// (one pass over w and up to SL_GM_CHUNK basis vectors)
__global__ __launch_bounds__(SL_BLOCK) void k_gm_dots(int64_t n, const double* __restrict__ V, int q0, int nv,
                                                      const double* __restrict__ wv, double* __restrict__ part,
                                                      const SlSolveState* st) {
    if (st->stop) return;
    __shared__ double red[SL_GM_CHUNK][SL_BLOCK / 64];
    double acc[SL_GM_CHUNK];
#pragma unroll
    for (int q = 0; q < SL_GM_CHUNK; ++q) acc[q] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * SL_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * SL_BLOCK) {
        const double wi = wv[i];
#pragma unroll
        for (int q = 0; q < SL_GM_CHUNK; ++q)
            if (q < nv) acc[q] = fma(V[(int64_t)(q0 + q) * n + i], wi, acc[q]);
    }
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < SL_GM_CHUNK; ++q) {
        if (q < nv) {
            const double s = sl_wave_sum(acc[q]);
            if ((threadIdx.x & 63) == 0) red[q][wave] = s;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < nv) {
        double s = 0.0;
        for (int q = 0; q < SL_BLOCK / 64; ++q) s += red[threadIdx.x][q];
        part[(int64_t)blockIdx.x * (SL_GM_MAXM + 1) + q0 + threadIdx.x] = s;
    }
}

// one workgroup: h[q] = sum of the dot partials in block order, H[q][j] += h[q], q < nv
__global__ __launch_bounds__(SL_BLOCK) void k_gm_dots_reduce(const double* __restrict__ part, int nblk, int nv,
                                                             int j, SlSolveState* st) {
    if (st->stop) return;
    __shared__ double red[SL_BLOCK];
    for (int q = 0; q < nv; ++q) {
        double a = 0.0;
        for (int b = threadIdx.x; b < nblk; b += SL_BLOCK) a += part[(int64_t)b * (SL_GM_MAXM + 1) + q];
        red[threadIdx.x] = a;
        __syncthreads();
        for (int s = SL_BLOCK / 2; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            st->h[q] = red[0];
            st->H[q][j] += red[0];
        }
        __syncthreads();
    }
}

// out = in + sign * sum_{q < nv} coef[q] V_{q0 + q} (coef: st->h, or st->y at the end of a cycle);
// with `part` the partials of sum out^2 (the norm after the second Gram-Schmidt pass)
__global__ __launch_bounds__(SL_BLOCK) void k_gm_update(int64_t n, const double* __restrict__ V, int q0, int nv,
                                                        int use_y, double sign, const double* in,
                                                        double* out, double* __restrict__ part,
                                                        const SlSolveState* st, int gated) {
    if (gated && st->stop) return;
    __shared__ double red[SL_BLOCK / 64];
    const double* coef = use_y ? st->y : st->h;
    // the solution update takes the basis vectors of the steps done only: the later slots hold
    // whatever an earlier cycle (or nothing) left there
    if (use_y) nv = st->steps - q0 < nv ? st->steps - q0 : nv;
    double c[SL_GM_CHUNK];
#pragma unroll
    for (int q = 0; q < SL_GM_CHUNK; ++q) c[q] = q < nv ? coef[q0 + q] : 0.0;
    double sum = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * SL_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * SL_BLOCK) {
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < SL_GM_CHUNK; ++q)
            if (q < nv) s = fma(c[q], V[(int64_t)(q0 + q) * n + i], s);
        const double o = sign > 0.0 ? in[i] + s : in[i] - s;
        out[i] = o;
        sum = fma(o, o, sum);
    }
    if (!part) return;
    sum = sl_wave_sum(sum);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0;
        for (int q = 0; q < SL_BLOCK / 64; ++q) a += red[q];
        part[blockIdx.x] = a;
    }
}

// one workgroup, after Arnoldi step j: H[j+1][j] = ||w||, the rotations so far applied to column j,
// a new rotation for it, g updated; |g[j+1]| is the 2-norm of the GMRES residual.  The cycle stops
// when that is below the target or the Krylov space is exhausted.
__global__ __launch_bounds__(SL_BLOCK) void k_gm_hessenberg(const double* __restrict__ part, int nblk, int j,
                                                            SlSolveState* st) {
    if (st->stop) return;
    __shared__ double red[SL_BLOCK];
    double a = 0.0;
    for (int b = threadIdx.x; b < nblk; b += SL_BLOCK) a += part[b];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int s = SL_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double hn = sqrt(red[0]);
    for (int i = 0; i < j; ++i) {
        const double h0 = st->H[i][j], h1 = st->H[i + 1][j];
        st->H[i][j] = st->cs[i] * h0 + st->sn[i] * h1;
        st->H[i + 1][j] = -st->sn[i] * h0 + st->cs[i] * h1;
    }
    const double hjj = st->H[j][j];
    const double rr = hypot(hjj, hn);
    const double c = rr > 0.0 ? hjj / rr : 1.0, s = rr > 0.0 ? hn / rr : 0.0;
    st->cs[j] = c;
    st->sn[j] = s;
    st->H[j][j] = rr;
    st->H[j + 1][j] = 0.0;
    const double gj = st->g[j];
    st->g[j] = c * gj;
    st->g[j + 1] = -s * gj;
    st->steps = j + 1;
    // breakdown: the next basis vector would be 0 (the solution lies in the space already)
    const bool breakdown = !(hn > 1e-300) || !(rr > 0.0);
    st->inv_norm = breakdown ? 0.0 : 1.0 / hn;
    if (breakdown || fabs(st->g[j + 1]) <= st->target) st->stop = 1;
}

// one workgroup: y = R^-1 g over the steps done (back substitution)
__global__ void k_gm_solve_small(SlSolveState* st) {
    if (threadIdx.x != 0) return;
    const int m = st->steps;
    for (int i = m - 1; i >= 0; --i) {
        double s = st->g[i];
        for (int q = i + 1; q < m; ++q) s -= st->H[i][q] * st->y[q];
        st->y[i] = st->H[i][i] != 0.0 ? s / st->H[i][i] : 0.0;
    }
    for (int i = m; i < SL_GM_MAXM; ++i) st->y[i] = 0.0;
}

namespace {

struct Solver {
    sl_ctx* ctx;
    int64_t n;
    int k, nblk;
    const int32_t* cols;
    const double* w;
    const double* r;
    double gamma;
    double* V;          // [m + 1][n] Krylov basis (V_0 also holds the residual of the current iterate)
    double* part;       // [nblk][SL_GM_MAXM + 1]
    double* normp;      // [nblk]
    SlSolveState* st;   // device
    SlSolveState h;     // host copy of the status

    template <int MODE>
    void matvec(const double* x, double* y, double* p, const SlSolveState* gate) {
        // compiled for rows of at most 2, 3, 4, 5, 8 and SL_ROW_MAX_K entries: the smallest that holds k
        const int bucket = k <= 2 ? 2 : (k <= 5 ? k : (k <= 8 ? 8 : SL_ROW_MAX_K));
        sl_with_dim<2, 3, 4, 5, 8, SL_ROW_MAX_K>(bucket, [&](auto kmax) {
            hipLaunchKernelGGL((k_value_matvec<MODE, kmax>), dim3(nblk), dim3(SL_BLOCK), 0, ctx->stream, n, k, cols,
                               w, r, gamma, x, y, p, gate);
            return SL_OK;
        });
    }
    // residual of x into V_0 and the status record (start: a GMRES cycle begins from it)
    int residual(const double* x, bool start, double tol_abs) {
        matvec<2>(x, V, part, nullptr);
        hipLaunchKernelGGL(k_solve_status, dim3(1), dim3(SL_BLOCK), 0, ctx->stream, part, nblk, st,
                           start ? 1 : 0, tol_abs);
        return read();
    }
    int read() {
        SL_HIP_CHECK(ctx, hipGetLastError());
        SL_HIP_CHECK(ctx, hipMemcpyAsync(&h, st, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
        SL_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        return SL_OK;
    }
    // Jacobi steps from a (a and b ping-pong); *last: the buffer holding the newest iterate
    void jacobi(double* a, double* b, int steps, double** last, double** before) {
        double* in = a;
        double* out = b;
        for (int s = 0; s < steps; ++s) {
            matvec<1>(in, out, part, nullptr);
            double* t = in; in = out; out = t;
        }
        *last = in;
        *before = out;
    }
    // one GMRES cycle of at most m steps from the residual in V_0 (st prepared by k_solve_status):
    // x_new = x + V y
    void gmres_cycle(const double* x, double* x_new, int m) {
        hipLaunchKernelGGL(k_gm_scale, dim3(nblk), dim3(SL_BLOCK), 0, ctx->stream, n, V, st);
        for (int j = 0; j < m; ++j) {
            double* wv = V + (int64_t)(j + 1) * n;
            matvec<0>(V + (int64_t)j * n, wv, nullptr, st);
            for (int pass = 0; pass < 2; ++pass) {          // classical Gram-Schmidt, twice
                for (int q0 = 0; q0 <= j; q0 += SL_GM_CHUNK) {
                    const int nv = (j + 1 - q0) < SL_GM_CHUNK ? (j + 1 - q0) : SL_GM_CHUNK;
                    hipLaunchKernelGGL(k_gm_dots, dim3(nblk), dim3(SL_BLOCK), 0, ctx->stream, n, V, q0, nv,
                                       (const double*)wv, part, (const SlSolveState*)st);
                }
                hipLaunchKernelGGL(k_gm_dots_reduce, dim3(1), dim3(SL_BLOCK), 0, ctx->stream, part, nblk,
                                   j + 1, j, st);
                for (int q0 = 0; q0 <= j; q0 += SL_GM_CHUNK) {
                    const int nv = (j + 1 - q0) < SL_GM_CHUNK ? (j + 1 - q0) : SL_GM_CHUNK;
                    const bool last = q0 + SL_GM_CHUNK > j;
                    hipLaunchKernelGGL(k_gm_update, dim3(nblk), dim3(SL_BLOCK), 0, ctx->stream, n,
                                       (const double*)V, q0, nv, 0, -1.0, (const double*)wv, wv,
                                       (pass == 1 && last) ? normp : nullptr, (const SlSolveState*)st, 1);
                }
            }
            hipLaunchKernelGGL(k_gm_hessenberg, dim3(1), dim3(SL_BLOCK), 0, ctx->stream, normp, nblk, j, st);
            hipLaunchKernelGGL(k_gm_scale, dim3(nblk), dim3(SL_BLOCK), 0, ctx->stream, n, wv, st);
        }
        hipLaunchKernelGGL(k_gm_solve_small, dim3(1), dim3(64), 0, ctx->stream, st);
        for (int q0 = 0; q0 < m; q0 += SL_GM_CHUNK) {
            const int nv = (m - q0) < SL_GM_CHUNK ? (m - q0) : SL_GM_CHUNK;
            hipLaunchKernelGGL(k_gm_update, dim3(nblk), dim3(SL_BLOCK), 0, ctx->stream, n, (const double*)V,
                               q0, nv, 1, 1.0, q0 == 0 ? x : (const double*)x_new, x_new, (double*)nullptr,
                               (const SlSolveState*)st, 0);
        }
    }
};

}  // namespace

extern "C" int sl_value_solve(sl_ctx* ctx, int64_t n, int k, const int32_t* d_cols, const double* d_w,
                              const double* d_r, double gamma, double* d_v, double tol, int64_t max_matvecs,
                              int restart, int method, sl_value_solve_stats* out) {
    if (!ctx) return sl_fail(nullptr, SL_ERR_INVALID, "sl_value_solve: NULL context");
    if (!out) return sl_fail(ctx, SL_ERR_INVALID, "sl_value_solve: NULL stats");
    memset(out, 0, sizeof(*out));
    if (n < 1 || !sl_policy_rows_fit(n))
        return sl_fail(ctx, SL_ERR_INVALID, "sl_value_solve: n = %lld (1 to 2^31 - 1 rows)", (long long)n);
    if (k < 1 || k > SL_ROW_MAX_K)
        return sl_fail(ctx, SL_ERR_INVALID, "sl_value_solve: k = %d entries per row (1 to %d)", k, SL_ROW_MAX_K);
    if (!(gamma >= 0.0 && gamma < 1.0))
        return sl_fail(ctx, SL_ERR_INVALID, "sl_value_solve: gamma = %g outside [0, 1)", gamma);
    if (!(tol >= 0.0) || !isfinite(tol))
        return sl_fail(ctx, SL_ERR_INVALID, "sl_value_solve: tol = %g", tol);
    if (restart < 1 || restart > SL_GM_MAXM)
        return sl_fail(ctx, SL_ERR_INVALID, "sl_value_solve: restart = %d (1 to %d)", restart, SL_GM_MAXM);
    if (method != SL_SOLVE_GMRES && method != SL_SOLVE_JACOBI)
        return sl_fail(ctx, SL_ERR_INVALID, "sl_value_solve: unknown method %d", method);
    if (max_matvecs < 1)
        return sl_fail(ctx, SL_ERR_INVALID, "sl_value_solve: max_matvecs = %lld", (long long)max_matvecs);
    if (!d_cols || !d_w || !d_r || !d_v) return sl_fail(ctx, SL_ERR_INVALID, "sl_value_solve: NULL array");
    SL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const int m = restart;
    const int64_t nbasis = method == SL_SOLVE_GMRES ? m + 1 : 1;
    Solver S;
    S.ctx = ctx;
    S.n = n;
    S.k = k;
    S.nblk = sl_red_blocks(n);
    S.cols = d_cols;
    S.w = d_w;
    S.r = d_r;
    S.gamma = gamma;
    // workspace (the context's scratch buffer, kept between calls): basis, a second iterate,
    // partials, state
    const size_t vec = sizeof(double) * (size_t)n;
    const size_t part_bytes = sizeof(double) * (size_t)S.nblk * (SL_GM_MAXM + 1);
    const size_t norm_bytes = sizeof(double) * (size_t)S.nblk;
    const size_t need = vec * (size_t)(nbasis + 1) + part_bytes + norm_bytes + sizeof(SlSolveState);
    if (sl_grow(ctx, &ctx->d_scratch, &ctx->scratch_bytes, need) != hipSuccess) {
        (void)hipGetLastError();
        return sl_fail(ctx, SL_ERR_NOMEM, "sl_value_solve: %zu bytes of workspace", need);
    }
    char* base = reinterpret_cast<char*>(ctx->d_scratch);
    S.V = reinterpret_cast<double*>(base);
    double* other = reinterpret_cast<double*>(base + vec * nbasis);
    S.part = reinterpret_cast<double*>(base + vec * (nbasis + 1));
    S.normp = reinterpret_cast<double*>(base + vec * (nbasis + 1) + part_bytes);
    S.st = reinterpret_cast<SlSolveState*>(base + vec * (nbasis + 1) + part_bytes + norm_bytes);
    SL_HIP_CHECK(ctx, hipMemsetAsync(S.st, 0, sizeof(SlSolveState), ctx->stream));

    // inputs: finite, columns in range (before any gather), max |r|, kappa
    hipLaunchKernelGGL(k_solve_prep, dim3(S.nblk), dim3(SL_BLOCK), 0, ctx->stream, n, k, d_cols, d_w, d_r,
                       (const double*)d_v, S.part);
    hipLaunchKernelGGL(k_solve_prep_reduce, dim3(1), dim3(SL_BLOCK), 0, ctx->stream, S.part, S.nblk, S.st);
    int rc = S.read();
    if (rc) return rc;
    if (S.h.bad != 0.0)
        return sl_fail(ctx, SL_ERR_INVALID, "sl_value_solve: %.0f non-finite entries or columns outside "
                                            "[0, %lld)", S.h.bad, (long long)n);
    const double kappa = gamma * S.h.w_abs;
    out->kappa = kappa;
    out->bound = INFINITY;
    sl_note_kernel(ctx, false, "%s", method == SL_SOLVE_GMRES ? "k_value_matvec + GMRES(m)" : "k_value_matvec (Jacobi)");
    if (S.h.r_inf == 0.0) {          // r = 0: the solution is 0
        SL_HIP_CHECK(ctx, hipMemsetAsync(d_v, 0, vec, ctx->stream));
        SL_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        out->converged = 1;
        out->bound = 0.0;
        return SL_OK;
    }
    const double tol_abs = tol * S.h.r_inf;
    double* cur = d_v;
    int64_t mv = 0;
    if (method == SL_SOLVE_GMRES) {
        rc = S.residual(cur, true, tol_abs);
        if (rc) return rc;
        mv = 1;
        double res = S.h.res_inf;
        while (!(res <= tol_abs) && isfinite(res) && mv < max_matvecs) {
            const int64_t left = max_matvecs - mv;
            double* alt = cur == d_v ? other : d_v;
            const int steps = (int)(left - 1 < m ? left - 1 : m);   // + 1: the new iterate's residual
            if (steps < 1) break;
            S.gmres_cycle(cur, alt, steps);
            rc = S.read();
            if (rc) return rc;
            const int done = S.h.steps;
            ++out->cycles;
            out->iterations += done;
            mv += done;
            // the new iterate's residual; V_0 then starts the next cycle from it
            rc = S.residual(alt, true, tol_abs);
            if (rc) return rc;
            mv += 1;
            const double res_new = S.h.res_inf;
            if (!isfinite(res_new) && !(kappa < 1.0)) break;     // diverged: keep cur, not converged
            const bool better = res_new < res;
            // what `done` Jacobi steps would have guaranteed (kappa < 1 only)
            const bool safeguard = kappa < 1.0 && !(res_new <= pow(kappa, done) * res);
            if (!safeguard || res_new <= tol_abs) {
                cur = alt;
                res = res_new;
                continue;
            }
            // m Jacobi steps from the better of the two iterates, then its residual
            double* from = better ? alt : cur;
            double* spare = better ? cur : alt;
            const int64_t left2 = max_matvecs - mv;
            const int js = (int)(left2 - 1 < m ? left2 - 1 : m);
            if (js < 1) {                         // out of matvecs: the better iterate
                cur = from;
                res = better ? res_new : res;
                break;
            }
            double* last;
            double* before;
            S.jacobi(from, spare, js, &last, &before);
            ++out->jacobi_cycles;
            out->iterations += js;
            mv += js;
            cur = last;
            rc = S.residual(cur, true, tol_abs);
            if (rc) return rc;
            mv += 1;
            res = S.h.res_inf;
        }
        out->residual_inf = res;
    } else {
        // Jacobi: each step also reduces the residual of its input; per cycle the host reads the
        // last one.  It keeps that input when it converged, diverged or the matvecs are used up
        // (its residual is then known exactly, with no extra matvec), the newest iterate otherwise.
        double res = INFINITY;
        double* spare = other;
        while (mv < max_matvecs) {
            const int64_t left = max_matvecs - mv;
            const int js = (int)(left < m ? left : m);
            double* last;
            double* before;
            S.jacobi(cur, spare, js, &last, &before);
            hipLaunchKernelGGL(k_solve_status, dim3(1), dim3(SL_BLOCK), 0, ctx->stream, S.part, S.nblk, S.st,
                               0, tol_abs);
            rc = S.read();
            if (rc) return rc;
            ++out->cycles;
            out->iterations += js;
            mv += js;
            res = S.h.res_inf;           // the residual of `before`
            if (res <= tol_abs || !isfinite(res) || mv >= max_matvecs) {
                cur = before;
                break;
            }
            cur = last;
            spare = before;
        }
        out->residual_inf = res;
    }
    if (cur != d_v) SL_HIP_CHECK(ctx, hipMemcpyAsync(d_v, cur, vec, hipMemcpyDeviceToDevice, ctx->stream));
    SL_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    out->matvecs = mv;
    out->converged = out->residual_inf <= tol_abs ? 1 : 0;
    out->bound = kappa < 1.0 ? out->residual_inf / (1.0 - kappa) : INFINITY;
    return SL_OK;
}
