// sl_poly_value.hip - the kernels of a polynomial Lyapunov function (SL_V_POLYNOMIAL, csrc/sl_poly_value.h)
// for gfx950: V on the grid, the decrease check under deterministic dynamics, and the check over the
// posterior records of the GP sweep.
//
// The "general" instantiations of k_values / k_det_sweep / k_check_records take a non-quadratic V for an
// interpolated table at compile time; the kind goes round them (sl_sweep_any, sl_values) to the kernels
// below, which take the context's term table as an argument.  One cell (or explicit point) per thread, the
// launch geometry, the ballot, the fail-key partials and the per-cell records of sl_kernels.hip.  The table
// reads are wavefront-uniform scalar loads; the per-cell work is the chain of unfused FP64 multiplications
// of the terms.
#include "sl_common.h"

// V(x), L_v(x), V(next) (and L_v(next) under uncertain dynamics) of one cell: sl_cell_check for the kind
__device__ __forceinline__ SlCellCheck sl_poly_cell_check(const SlDevModel& M, const SlPolyValue& table, int d,
                                                          const double* x, const double* next_mean,
                                                          const double* err) {
    SlCellCheck r;
    double lv_x[SL_D], lv_n[SL_D];
    const int negate = M.m.value.negate;
    sl_polyv_lv(M, table, d, x, lv_x);
    r.v_x = sl_polyv_value(table, d, negate, x);
    if (M.uncertain) sl_polyv_lv(M, table, d, next_mean, lv_n);
    const double v_next = sl_polyv_value(table, d, negate, next_mean);
    r.decrease = sl_decrease(M, d, r.v_x, v_next, lv_n, err);
    r.threshold = sl_threshold(M, d, lv_x, M.m.lipschitz.tau, x);
    r.negative = r.decrease < r.threshold;
    return r;
}

// =============================================================================================
// values: V(x_i)                                             (lyapunov.py:305-322)
// =============================================================================================
template <int DT>
__global__ __launch_bounds__(SL_BLOCK) void k_poly_values(const SlDevModel M_arg, const SlPolyValue* __restrict__ table,
                                                          int64_t lo, int64_t hi, double* __restrict__ values) {
    const SlDevModel& M = M_arg;
    const int d = DT > 0 ? DT : M.m.grid.d;
    for (int64_t idx = lo + (int64_t)blockIdx.x * SL_BLOCK + threadIdx.x; idx < hi;
         idx += (int64_t)gridDim.x * SL_BLOCK) {
        double x[SL_P];
        sl_index_to_grid_point(M.m.grid, M.gf, d, idx, x);
        values[idx - lo] = sl_polyv_value(*table, d, M.m.value.negate, x);
    }
}

int sl_poly_values_launch(sl_ctx* ctx, int64_t lo, int64_t hi, double* d_values) {
    const SlDevModel& M = ctx->h_model;
    const int blocks = sl_grid_blocks(hi - lo);
    const int variant = sl_dim_variant_of(M);
    return sl_with_dim<2, 4, 0>(variant, [&](auto d) {
        hipLaunchKernelGGL((k_poly_values<d>), dim3(blocks), dim3(SL_BLOCK), 0, ctx->stream, M, ctx->d_polyv, lo, hi,
                           d_values);
        SL_HIP_CHECK(ctx, hipGetLastError());
        sl_note_kernel(ctx, false, "k_poly_values<d=%d>", (int)d);
        return SL_OK;
    });
}

// =============================================================================================
// deterministic-dynamics decrease check                    (lyapunov.py:436-441, 524-535)
// =============================================================================================
// What k_det_sweep's walk over [lo, hi) does, with the polynomial V: every policy kind (the interpolated
// one from LDS), every deterministic dynamics kind (read from the model).
template <int DT, int MT>
__global__ __launch_bounds__(SL_BLOCK) void k_poly_sweep(
    const SlDevModel M_arg, SlAux aux_arg, const SlPolyValue* __restrict__ table, int64_t lo, int64_t hi,
    const uint64_t* __restrict__ init_bits, const double* __restrict__ values, uint64_t* __restrict__ neg_bits,
    sl_key* __restrict__ partials, double* __restrict__ dbg, const double* __restrict__ points) {
    __shared__ uint64_t sv[SL_BLOCK / 64];
    __shared__ int64_t si[SL_BLOCK / 64];
    // Only an interpolated policy reads a table descriptor: the launcher gives the kernel the
    // sizeof(SlTriLds<true>) bytes of dynamic LDS for the two descriptors then and none otherwise, so the 38 KB
    // do not bound the occupancy of the other policies' launches (the branch is uniform over the launch).
    extern __shared__ __align__(16) unsigned char poly_tri_lds[];
    const SlDevModel& M = M_arg;
    SlAux aux = aux_arg;
    if (M.m.policy.kind == SL_POLICY_TRI)
        aux = sl_stage_aux<true>(*reinterpret_cast<SlTriLds<true>*>(poly_tri_lds), aux_arg);
    const SlDims n = sl_dims<DT, MT>(M);
    const int d = n.d;
    const int lane = threadIdx.x & 63;
    uint64_t best_v = ~0ull;
    int64_t best_i = INT64_MAX;
    for (int64_t base = lo + (int64_t)blockIdx.x * SL_BLOCK; base < hi;
         base += (int64_t)gridDim.x * SL_BLOCK) {
        const int64_t idx = base + threadIdx.x;
        const bool valid = idx < hi;
        bool negative = false;
        double v_x = 0.0;
        const int64_t wbase = base + (threadIdx.x & ~63);        // first cell of this wavefront
        const uint64_t init = (init_bits && wbase < hi) ? init_bits[(wbase - lo) >> 6] : 0ull;
        if (valid) {
            double x[SL_P], u[SL_M], nxt[SL_D], err[SL_D];
            sl_cell_state(M, d, idx, points, x);
            sl_policy_any<true>(M, n, aux.tri, idx, x, u);
            sl_append_action(n, u, x);
            sl_dynamics_det<0>(M, n, x, nxt);
            SlCellCheck c = sl_poly_cell_check(M, *table, d, x, nxt, err);
            negative = c.negative;
            v_x = values ? values[idx - lo] : c.v_x;       // ordering key: lyapunov.py:512
            if (dbg) {
                double* o = dbg + (idx - lo) * (2 + 2 * d);
                o[0] = c.decrease; o[1] = c.threshold;
#pragma unroll
                for (int k = 0; k < SL_D; ++k) if (k < d) { o[2 + k] = nxt[k]; o[2 + d + k] = 0.0; }
            }
        }
        const uint64_t word = __ballot(negative);
        if (wbase < hi) {
            const int64_t widx = (wbase - lo) >> 6;
            if (lane == 0) neg_bits[widx] = word;
            const bool ok = negative || ((init >> lane) & 1ull);
            if (valid && !ok) sl_key_min(best_v, best_i, sl_vbits(v_x), idx);
        }
    }
    sl_block_reduce_key<true>(best_v, best_i, sv, si);
    if (threadIdx.x == 0) { partials[blockIdx.x].vbits = best_v; partials[blockIdx.x].index = best_i; }
}

int sl_poly_sweep_launch(sl_ctx* ctx, const SlSweepArgs& a, int* blocks) {
    const SlDevModel& M = ctx->h_model;
    *blocks = sl_grid_blocks(a.hi - a.lo);
    const int variant = sl_dim_variant_of(M);
    return sl_with_dim<2, 4, 0>(variant, [&](auto d) {
        constexpr int MT = d != 0 ? 1 : 0;
        const size_t lds = M.m.policy.kind == SL_POLICY_TRI ? sizeof(SlTriLds<true>) : 0;
        hipLaunchKernelGGL((k_poly_sweep<d, MT>), dim3(*blocks), dim3(SL_BLOCK), lds, ctx->stream, M,
                           SlAux{ctx->d_tri, ctx->d_net}, ctx->d_polyv, a.lo, a.hi, a.init_bits, a.values, a.neg_bits,
                           ctx->d_partials, a.dbg, a.points);
        SL_HIP_CHECK(ctx, hipGetLastError());
        sl_note_kernel(ctx, false, "k_poly_sweep<d=%d, m=%d, dynamics=%d>%s", (int)d, MT, M.m.dynamics.kind,
                       lds ? " (interpolated policy from LDS)" : "");
        return SL_OK;
    });
}

// =============================================================================================
// GP dynamics: the check over the records of the posterior pass
// =============================================================================================
// records: [decrease, threshold, mean[d], err[d]] per cell of [lo, hi) from the posterior-only pass;
// what k_check_records does for a table V (dimensions read from the model: the posterior pass is the
// work of such a sweep, not this)
__global__ __launch_bounds__(SL_BLOCK) void k_poly_check(
    const SlDevModel M_arg, const SlPolyValue* __restrict__ table, int64_t lo, int64_t hi,
    const uint64_t* __restrict__ init_bits, const double* __restrict__ values, const double* __restrict__ records,
    uint64_t* __restrict__ neg_bits, sl_key* __restrict__ partials, double* __restrict__ dbg,
    const double* __restrict__ points) {
    __shared__ uint64_t sv[SL_BLOCK / 64];
    __shared__ int64_t si[SL_BLOCK / 64];
    const SlDevModel& M = M_arg;
    const int d = M.m.grid.d;
    const int lane = threadIdx.x & 63;
    uint64_t best_v = ~0ull;
    int64_t best_i = INT64_MAX;
    for (int64_t base = lo + (int64_t)blockIdx.x * SL_BLOCK; base < hi;
         base += (int64_t)gridDim.x * SL_BLOCK) {
        const int64_t idx = base + threadIdx.x;
        const bool valid = idx < hi;
        const int64_t wbase = base + (threadIdx.x & ~63);        // first cell of this wavefront
        const uint64_t init = (init_bits && wbase < hi) ? init_bits[(wbase - lo) >> 6] : 0ull;
        bool negative = false;
        double v_x = 0.0;
        if (valid) {
            double x[SL_P], mean[SL_D], err[SL_D];
            const double* rec = records + (idx - lo) * (2 + 2 * d);
#pragma unroll
            for (int k = 0; k < SL_D; ++k) if (k < d) { mean[k] = rec[2 + k]; err[k] = rec[2 + d + k]; }
            sl_cell_state(M, d, idx, points, x);
            SlCellCheck c = sl_poly_cell_check(M, *table, d, x, mean, err);
            negative = c.negative;
            v_x = values ? values[idx - lo] : c.v_x;       // ordering key: lyapunov.py:512
            if (dbg) {
                double* o = dbg + (idx - lo) * (2 + 2 * d);
                o[0] = c.decrease; o[1] = c.threshold;
#pragma unroll
                for (int k = 0; k < SL_D; ++k) if (k < d) { o[2 + k] = mean[k]; o[2 + d + k] = err[k]; }
            }
        }
        const uint64_t word = __ballot(negative);
        if (wbase < hi) {
            if (lane == 0) neg_bits[(wbase - lo) >> 6] = word;
            const bool ok = negative || ((init >> lane) & 1ull);
            if (valid && !ok) sl_key_min(best_v, best_i, sl_vbits(v_x), idx);
        }
    }
    sl_block_reduce_key<true>(best_v, best_i, sv, si);
    if (threadIdx.x == 0) { partials[blockIdx.x].vbits = best_v; partials[blockIdx.x].index = best_i; }
}

int sl_poly_check_launch(sl_ctx* ctx, const SlSweepArgs& a, const double* d_records, int* blocks) {
    *blocks = sl_grid_blocks(a.hi - a.lo);
    hipLaunchKernelGGL(k_poly_check, dim3(*blocks), dim3(SL_BLOCK), 0, ctx->stream, ctx->h_model, ctx->d_polyv, a.lo,
                       a.hi, a.init_bits, a.values, d_records, a.neg_bits, ctx->d_partials, a.dbg, a.points);
    SL_HIP_CHECK(ctx, hipGetLastError());
    sl_note_kernel(ctx, true, "k_poly_check");
    return SL_OK;
}
