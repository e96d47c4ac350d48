// sl_nn.hip - Lyapunov check and value pass for a LyapunovNetwork value function
// (examples/utilities.py:85-104; config C3 of BASELINE.json).
//
// Both kernels run the network on the FP64 matrix cores (see nn_mfma_eval).  The posterior (mean,
// error) of GP dynamics comes from a first pass of k_gp_sweep that only emits its per-cell
// records; deterministic dynamics are evaluated here.  Below them: the training step of
// examples/lyapunov_function_learning.ipynb (k_nn_loss, k_nn_param_grad).
#include "sl_grad_host.h"
#include "sl_nn_train.h"

__device__ __forceinline__ void nn_lv_from_grad(int kind, int d, const double* g, double* lv) {
    if (kind == SL_LIP_ABS_GRAD) {
#pragma unroll
        for (int k = 0; k < SL_D; ++k) if (k < d) lv[k] = fabs(g[k]);
    } else {
        double acc = fabs(g[0]);
#pragma unroll
        for (int k = 1; k < SL_D; ++k) if (k < d) acc = acc + fabs(g[k]);
        lv[0] = acc;
    }
}

// A wavefront owns 16 cells at a time.  A layer is the FP64 MFMA GEMM  H_out[out x 16 cells] =
// W[out x in] . H_in[in x 16 cells] on v_mfma_f64_16x16x4_f64: A fragments (lane (i, k) =
// W[16 fb + i][4 s + k]) come from a zero-padded row-major copy of the layer kernels in LDS, and
// the accumulator layout of the instruction - lane (n, g) holds feature 16 fb + 4 r + g of cell n
// in register r - is exactly the B-fragment layout of slab 4 fb + r of the next layer, so the
// activations of all layers stay in registers and the layers chain without any data movement.
// The input gradient is the transposed chain (A fragments W[4 s + k][16 ib + i] from the same LDS
// copy), V = sum of squares folded over the four lane groups with two shuffles.
typedef double sl_nd4 __attribute__((ext_vector_type(4)));
#define SL_NNM_WAVES 8

__device__ __forceinline__ double nd4_get(const sl_nd4& v, int r) {
    return r == 0 ? v.x : (r == 1 ? v.y : (r == 2 ? v.z : v.w));
}

// z: the input of this lane's cell (lane & 15), identical in the four lane groups.  Returns V in
// every lane; grad[k] (k < d) in every lane when want_grad.
template <int NL>
__device__ __forceinline__ double nn_mfma_eval(const SlNet& net, const double* __restrict__ wl,
                                               int lane, const double* z, int d, bool want_grad,
                                               double* grad) {
    const int li = lane & 15, lg = lane >> 4;
    // input as B fragments: slab s holds feature 4 s + lg
    double xin[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        double v = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (4 * s + q < SL_D) v = (lg == q && 4 * s + q < d) ? z[4 * s + q] : v;
        xin[s] = v;
    }
    sl_nd4 h[NL][4];
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        const int nslab = net.nslab[l], nfb = net.nfb[l], stride = net.wstride[l], a = net.act[l];
        const double* __restrict__ W = wl + net.woff[l] + li * stride + lg;
        sl_nd4 acc[4];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) acc[fb] = (sl_nd4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            if (l == 0 && s >= 2) break;
            if (s < nslab) {
                const double b = (l == 0) ? xin[s & 1] : nd4_get(h[l > 0 ? l - 1 : 0][s >> 2], s & 3);
#pragma unroll
                for (int fb = 0; fb < 4; ++fb)
                    if (fb < nfb)
                        acc[fb] = __builtin_amdgcn_mfma_f64_16x16x4f64(W[16 * fb * stride + 4 * s], b,
                                                                       acc[fb], 0, 0, 0);
            }
        }
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            h[l][fb].x = sl_act(a, acc[fb].x);
            h[l][fb].y = sl_act(a, acc[fb].y);
            h[l][fb].z = sl_act(a, acc[fb].z);
            h[l][fb].w = sl_act(a, acc[fb].w);
        }
    }
    double value = 0.0;
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) {
        value = fma(h[NL - 1][fb].x, h[NL - 1][fb].x, value);
        value = fma(h[NL - 1][fb].y, h[NL - 1][fb].y, value);
        value = fma(h[NL - 1][fb].z, h[NL - 1][fb].z, value);
        value = fma(h[NL - 1][fb].w, h[NL - 1][fb].w, value);
    }
    value += __shfl_xor(value, 16, 64);
    value += __shfl_xor(value, 32, 64);
    if (!want_grad) return value;
    // backward: t = dV/d(pre-activation) of the current layer, in B-fragment layout
    sl_nd4 t[4];
    {
        const int a = net.act[NL - 1];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            const sl_nd4 hh = h[NL - 1][fb];
            t[fb].x = 2.0 * hh.x * sl_dact(a, hh.x > 0.0 ? 1.0 : -1.0, hh.x);
            t[fb].y = 2.0 * hh.y * sl_dact(a, hh.y > 0.0 ? 1.0 : -1.0, hh.y);
            t[fb].z = 2.0 * hh.z * sl_dact(a, hh.z > 0.0 ? 1.0 : -1.0, hh.z);
            t[fb].w = 2.0 * hh.w * sl_dact(a, hh.w > 0.0 ? 1.0 : -1.0, hh.w);
        }
    }
#pragma unroll
    for (int l = NL - 1; l >= 0; --l) {
        const int nfb = net.nfb[l], nib = net.nib[l], stride = net.wstride[l];
        const double* __restrict__ W = wl + net.woff[l] + lg * stride + li;
        sl_nd4 acc[4];
#pragma unroll
        for (int ib = 0; ib < 4; ++ib) acc[ib] = (sl_nd4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            if ((s >> 2) < nfb) {
                const double b = nd4_get(t[s >> 2], s & 3);
#pragma unroll
                for (int ib = 0; ib < 4; ++ib)
                    if (ib < nib && (l > 0 || ib == 0))
                        acc[ib] = __builtin_amdgcn_mfma_f64_16x16x4f64(W[4 * s * stride + 16 * ib], b,
                                                                       acc[ib], 0, 0, 0);
            }
        }
        if (l > 0) {
            const int a = net.act[l - 1];
#pragma unroll
            for (int ib = 0; ib < 4; ++ib) {
                const sl_nd4 hh = h[l > 0 ? l - 1 : 0][ib];
                t[ib].x = acc[ib].x * sl_dact(a, hh.x > 0.0 ? 1.0 : -1.0, hh.x);
                t[ib].y = acc[ib].y * sl_dact(a, hh.y > 0.0 ? 1.0 : -1.0, hh.y);
                t[ib].z = acc[ib].z * sl_dact(a, hh.z > 0.0 ? 1.0 : -1.0, hh.z);
                t[ib].w = acc[ib].w * sl_dact(a, hh.w > 0.0 ? 1.0 : -1.0, hh.w);
            }
        } else {
            // input feature k = 4 r + g sits in register r of lane group g
#pragma unroll
            for (int k = 0; k < SL_D; ++k)
                if (k < d) grad[k] = __shfl(nd4_get(acc[0], k >> 2), li + 16 * (k & 3), 64);
        }
    }
    return value;
}

__device__ __forceinline__ void nn_stage_weights(const SlNet& net, double* wl) {
    for (int k = threadIdx.x; k < net.wtotal; k += blockDim.x) wl[k] = net.wpad[k];
    __syncthreads();
}

template <int NL>
__global__ __launch_bounds__(64 * SL_NNM_WAVES) void k_nn_values_mfma(const SlDevModel M, SlAux aux,
                                                                      int64_t lo, int64_t hi,
                                                                      double* __restrict__ values) {
    extern __shared__ __attribute__((aligned(16))) double wl[];
    const SlNet& net = *aux.net;
    nn_stage_weights(net, wl);
    const int d = M.m.grid.d, lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t step = (int64_t)gridDim.x * SL_NNM_WAVES * 16;
    for (int64_t base = lo + ((int64_t)blockIdx.x * SL_NNM_WAVES + wave) * 16; base < hi; base += step) {
        int64_t idx = base + (lane & 15);
        const bool valid = idx < hi;
        idx = valid ? idx : hi - 1;
        double x[SL_P];
        sl_index_to_grid_point(M.m.grid, M.gf, d, idx, x);
        double v = nn_mfma_eval<NL>(net, wl, lane, x, d, false, nullptr);
        if (M.m.value.negate) v = v * -1.0;
        if (valid && lane < 16) values[idx - lo] = v;
    }
}

template <int NL, int DT, int MT>
__global__ __launch_bounds__(64 * SL_NNM_WAVES) void k_nn_check_mfma(
    const SlDevModel M, SlAux aux, int64_t lo, int64_t hi, const uint64_t* __restrict__ init_bits,
    const double* __restrict__ values, const double* __restrict__ records,
    uint64_t* __restrict__ neg_bits, sl_key* __restrict__ partials, double* __restrict__ dbg,
    const double* __restrict__ points) {
    extern __shared__ __attribute__((aligned(16))) double wl[];
    __shared__ uint64_t red_v[SL_NNM_WAVES];
    __shared__ int64_t red_i[SL_NNM_WAVES];
    const SlNet& net = *aux.net;
    nn_stage_weights(net, wl);
    const SlDims n = sl_dims<DT, MT>(M);
    const int d = n.d, lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lvk = M.m.lipschitz.lv_kind;
    const bool grad_lv = lvk == SL_LIP_ABS_GRAD || lvk == SL_LIP_NORM_GRAD;
    uint64_t best_v = ~0ull;
    int64_t best_i = INT64_MAX;
    // a wavefront owns one 64-cell word of the mask: four tiles of 16 cells
    const int64_t step = (int64_t)gridDim.x * SL_NNM_WAVES * 64;
    for (int64_t wbase = lo + ((int64_t)blockIdx.x * SL_NNM_WAVES + wave) * 64; wbase < hi; wbase += step) {
        uint64_t word = 0ull;
        const int64_t widx = (wbase - lo) >> 6;
        const uint64_t init = init_bits ? init_bits[widx] : 0ull;
        for (int tile = 0; tile < 4; ++tile) {
            const int64_t base = wbase + 16 * tile;
            if (base >= hi) break;
            int64_t idx = base + (lane & 15);
            const bool valid = idx < hi;
            idx = valid ? idx : hi - 1;
            double x[SL_P], u[SL_M], nxt[SL_D], err[SL_D], lv_x[SL_D], lv_n[SL_D], g[SL_D];
            sl_cell_state(M, d, idx, points, x);
            if (records) {
                const double* r = records + (idx - lo) * (2 + 2 * d);
#pragma unroll
                for (int k = 0; k < SL_D; ++k) if (k < d) { nxt[k] = r[2 + k]; err[k] = r[2 + d + k]; }
            } else {
                sl_policy_any<true>(M, n, aux.tri, idx, x, u);
                sl_append_action(n, u, x);
                sl_dynamics_det<0>(M, n, x, nxt);
            }
            double v_x = nn_mfma_eval<NL>(net, wl, lane, x, d, grad_lv, g);
            if (grad_lv) nn_lv_from_grad(lvk, d, g, lv_x); else sl_lv(M, d, x, lv_x);
            const bool grad_n = grad_lv && M.uncertain;
            double v_n = nn_mfma_eval<NL>(net, wl, lane, nxt, d, grad_n, g);
            if (M.uncertain) { if (grad_lv) nn_lv_from_grad(lvk, d, g, lv_n); else sl_lv(M, d, nxt, lv_n); }
            if (M.m.value.negate) { v_x = v_x * -1.0; v_n = v_n * -1.0; }
            const double decrease = sl_decrease(M, d, v_x, v_n, lv_n, err);
            const double threshold = sl_threshold(M, d, lv_x, M.m.lipschitz.tau, x);
            const bool negative = valid && (decrease < threshold);
            if (valid && dbg && lane < 16) {
                double* o = dbg + (idx - lo) * (2 + 2 * d);
                o[0] = decrease; o[1] = threshold;
#pragma unroll
                for (int k = 0; k < SL_D; ++k)
                    if (k < d) { o[2 + k] = nxt[k]; o[2 + d + k] = M.uncertain ? err[k] : 0.0; }
            }
            const uint64_t bits = __ballot(negative) & 0xffffull;
            word |= bits << (16 * tile);
            const bool ok = negative || ((init >> (16 * tile + (lane & 15))) & 1ull);
            if (valid && !ok && lane < 16) {
                const double key_v = values ? values[idx - lo] : v_x;
                sl_key_min(best_v, best_i, sl_vbits(key_v), idx);
            }
        }
        if (lane == 0) neg_bits[widx] = word;
    }
    sl_block_reduce_key<true>(best_v, best_i, red_v, red_i);
    if (threadIdx.x == 0) { partials[blockIdx.x].vbits = best_v; partials[blockIdx.x].index = best_i; }
}

// The kernels are compiled per layer count (1 .. 4: sl_with_dim over h_net.nlayers).
// (the weights of every layer sit in dynamic LDS)
static size_t nn_weight_bytes(const sl_ctx* ctx) { return sizeof(double) * (size_t)ctx->h_net.wtotal; }

int sl_nn_values_launch(sl_ctx* ctx, int64_t lo, int64_t hi, double* d_values) {
    int64_t blocks = (hi - lo + 16 * SL_NNM_WAVES - 1) / (16 * SL_NNM_WAVES);
    const int64_t cap = (int64_t)ctx->num_cu * (ctx->h_net.wtotal * 8 > 75 * 1024 ? 1 : 2);
    if (blocks > cap) blocks = cap;
    SlAux aux{ctx->d_tri, ctx->d_net};
    return sl_with_dim<1, 2, 3, 4>(ctx->h_net.nlayers, [&](auto nl) {
        SL_HIP_CHECK(ctx, sl_launch_lds(k_nn_values_mfma<nl>, dim3((unsigned)blocks), dim3(64 * SL_NNM_WAVES),
                                        nn_weight_bytes(ctx), ctx->stream, ctx->h_model, aux, lo, hi, d_values));
        return SL_OK;
    });
}

// d_records: the GP posterior records of the sweep's first pass, or null (deterministic dynamics)
int sl_nn_check_launch(sl_ctx* ctx, const SlSweepArgs& a, const double* d_records, int* nblocks) {
    int64_t blocks = (a.hi - a.lo + 64 * SL_NNM_WAVES - 1) / (64 * SL_NNM_WAVES);
    int64_t cap = (int64_t)ctx->num_cu * (ctx->h_net.wtotal * 8 > 75 * 1024 ? 1 : 2);
    if (cap > SL_MAX_GRID) cap = SL_MAX_GRID;
    if (blocks > cap) blocks = cap;
    *nblocks = (int)blocks;
    SlAux aux{ctx->d_tri, ctx->d_net};
    const int variant = sl_dim_variant_of(ctx->h_model);
    const int rc = sl_with_dim<2, 4, 0>(variant, [&](auto d) {
        constexpr int D = d;
        return sl_with_dim<1, 2, 3, 4>(ctx->h_net.nlayers, [&](auto nl) {
            SL_HIP_CHECK(ctx, sl_launch_lds(k_nn_check_mfma<nl, D, D != 0 ? 1 : 0>, dim3((unsigned)blocks),
                                            dim3(64 * SL_NNM_WAVES), nn_weight_bytes(ctx), ctx->stream, ctx->h_model,
                                            aux, a.lo, a.hi, a.init_bits, a.values, d_records, a.neg_bits,
                                            ctx->d_partials, a.dbg, a.points));
            return SL_OK;
        });
    });
    if (rc) return rc;
    sl_note_kernel(ctx, d_records != nullptr, "k_nn_check_mfma<layers=%d, d=%d>", ctx->h_net.nlayers,
                   variant);
    return SL_OK;
}

// ---- training: sum_m c_m dV(p_m)/dK_l and the notebook's losses (sl_nn_param_grad, sl_nn_loss) ----
//
// G_l = sum_m c_m t_l(p_m) h_{l-1}(p_m)^T with t_l = dV/d(pre-activation of layer l), the quantity
// the backward chain of nn_mfma_eval carries, and h_{l-1} the layer's input (h_0 = p): per layer
// one more FP64 MFMA GEMM, [out x cells] . [cells x in], whose reduction dimension is the cells.
//
// A workgroup of four wavefronts owns 64 points at a time.  Every wavefront runs the forward and
// the transposed chain of its 16 points as nn_mfma_eval does (point on the lane, feature in the
// register).  The outer product needs the point along the MFMA's k, so at every layer of the way
// back the workgroup's c t_l and then its h_{l-1} cross one [64 points][64 features] staging tile
// in LDS behind the weights: c t_l is written and wavefront w takes the A fragments of ITS 16 output
// rows (16 fb = 16 w) into registers, the tile is overwritten with h_{l-1} and read back as B
// fragments.  The 16 accumulator tiles of a [64 x 64] layer are thereby shared out over the four
// wavefronts (4 tiles = 16 registers per lane and layer, kept for the whole grid-stride loop)
// instead of standing 4 x 16 tiles beside each wavefront's activations, and one staging tile
// (33 KB) rather than two keeps the largest network (four layers of 64: 108 KB of weights) inside
// the 160 KB of a CU.  No atomics: a workgroup writes its G to its own slice of the context's
// scratch buffer and sl_sum_slices adds the slices in ascending order.
// (The two chains are written out again here and not shared with nn_mfma_eval as helpers: with helpers
// the register allocation of the sweeps' kernels changes - k_nn_values_mfma<2..4> go from 121 - 125
// VGPRs without scratch to 256 with it; profiles/lyapunov_training.md.)
#define SL_NNG_WAVES 4
#define SL_NNG_CELLS (16 * SL_NNG_WAVES)
#define SL_NNG_STRIDE (SL_NN_MAXW + 2)          // staging row of one point (+2: LDS bank spread)

template <int NL>
__global__ __launch_bounds__(64 * SL_NNG_WAVES) void k_nn_param_grad(SlAux aux, int64_t m, int d,
                                                                     const double* __restrict__ points,
                                                                     const double* __restrict__ coeff,
                                                                     double* __restrict__ partials, int total) {
    extern __shared__ __attribute__((aligned(16))) double wl[];
    const SlNet& net = *aux.net;
    nn_stage_weights(net, wl);
    double* __restrict__ stage = wl + net.wtotal;
    const int lane = threadIdx.x & 63, li = lane & 15, lg = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double* __restrict__ my_row = stage + (16 * wave + li) * SL_NNG_STRIDE + lg;   // this lane's point
    const double* __restrict__ frag = stage + lg * SL_NNG_STRIDE + li;             // point 4 s + lg, feature li
    sl_nd4 gacc[NL][4];
#pragma unroll
    for (int l = 0; l < NL; ++l)
#pragma unroll
        for (int ib = 0; ib < 4; ++ib) gacc[l][ib] = (sl_nd4){0.0, 0.0, 0.0, 0.0};
    const int64_t step = (int64_t)gridDim.x * SL_NNG_CELLS;
    // (the trip count is the same for the four wavefronts: the barriers below are uniform)
    for (int64_t base = (int64_t)blockIdx.x * SL_NNG_CELLS; base < m; base += step) {
        int64_t idx = base + 16 * wave + li;
        const bool valid = idx < m;
        idx = valid ? idx : m - 1;
        // a point past m: a real point's activations with coefficient 0 - it adds exactly nothing
        const double c = valid ? coeff[idx] : 0.0;
        double z[SL_D];
#pragma unroll
        for (int k = 0; k < SL_D; ++k) z[k] = k < d ? points[idx * d + k] : 0.0;
        // forward, as nn_mfma_eval: input as B fragments, slab s holds feature 4 s + lg
        double xin[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            double v = 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (4 * s + q < SL_D) v = (lg == q && 4 * s + q < d) ? z[4 * s + q] : v;
            xin[s] = v;
        }
        sl_nd4 h[NL][4];
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            const int nslab = net.nslab[l], nfb = net.nfb[l], stride = net.wstride[l], a = net.act[l];
            const double* __restrict__ W = wl + net.woff[l] + li * stride + lg;
            sl_nd4 acc[4];
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) acc[fb] = (sl_nd4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                if (l == 0 && s >= 2) break;
                if (s < nslab) {
                    const double b = (l == 0) ? xin[s & 1] : nd4_get(h[l > 0 ? l - 1 : 0][s >> 2], s & 3);
#pragma unroll
                    for (int fb = 0; fb < 4; ++fb)
                        if (fb < nfb)
                            acc[fb] = __builtin_amdgcn_mfma_f64_16x16x4f64(W[16 * fb * stride + 4 * s], b,
                                                                           acc[fb], 0, 0, 0);
                }
            }
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) {
                h[l][fb].x = sl_act(a, acc[fb].x);
                h[l][fb].y = sl_act(a, acc[fb].y);
                h[l][fb].z = sl_act(a, acc[fb].z);
                h[l][fb].w = sl_act(a, acc[fb].w);
            }
        }
        // backward: t = dV/d(pre-activation) of layer l, feature 16 fb + 4 r + lg in register r
        sl_nd4 t[4];
        {
            const int a = net.act[NL - 1];
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) {
                const sl_nd4 hh = h[NL - 1][fb];
                t[fb].x = 2.0 * hh.x * sl_dact(a, hh.x > 0.0 ? 1.0 : -1.0, hh.x);
                t[fb].y = 2.0 * hh.y * sl_dact(a, hh.y > 0.0 ? 1.0 : -1.0, hh.y);
                t[fb].z = 2.0 * hh.z * sl_dact(a, hh.z > 0.0 ? 1.0 : -1.0, hh.z);
                t[fb].w = 2.0 * hh.w * sl_dact(a, hh.w > 0.0 ? 1.0 : -1.0, hh.w);
            }
        }
#pragma unroll
        for (int l = NL - 1; l >= 0; --l) {
            const int nfb = net.nfb[l], nib = net.nib[l], stride = net.wstride[l];
            const bool mine = wave < nfb;                  // this wavefront owns output rows 16 wave ..
            // c t_l of the 64 points -> A fragments of this wavefront's rows
            __syncthreads();                               // (the tile's last readers are through)
#pragma unroll
            for (int fb = 0; fb < 4; ++fb)
                if (fb < nfb) {
                    my_row[16 * fb + 0] = c * t[fb].x;
                    my_row[16 * fb + 4] = c * t[fb].y;
                    my_row[16 * fb + 8] = c * t[fb].z;
                    my_row[16 * fb + 12] = c * t[fb].w;
                }
            __syncthreads();
            double af[16];
#pragma unroll
            for (int s = 0; s < 16; ++s) af[s] = mine ? frag[4 * s * SL_NNG_STRIDE + 16 * wave] : 0.0;
            __syncthreads();
            // h_{l-1} of the 64 points (the input, zero-padded to one block of 16, below layer 0)
#pragma unroll
            for (int ib = 0; ib < 4; ++ib)
                if (ib < nib && (l > 0 || ib == 0)) {
                    // (xin[s] is input feature 4 s + lg: the layout of a block's registers 0 and 1)
                    const sl_nd4 hh = l > 0 ? h[l > 0 ? l - 1 : 0][ib] : (sl_nd4){xin[0], xin[1], 0.0, 0.0};
                    my_row[16 * ib + 0] = hh.x;
                    my_row[16 * ib + 4] = hh.y;
                    my_row[16 * ib + 8] = hh.z;
                    my_row[16 * ib + 12] = hh.w;
                }
            __syncthreads();
            if (mine) {
#pragma unroll
                for (int s = 0; s < 16; ++s)
#pragma unroll
                    for (int ib = 0; ib < 4; ++ib)
                        if (ib < nib && (l > 0 || ib == 0))
                            gacc[l][ib] = __builtin_amdgcn_mfma_f64_16x16x4f64(
                                af[s], frag[4 * s * SL_NNG_STRIDE + 16 * ib], gacc[l][ib], 0, 0, 0);
            }
            if (l > 0) {
                // t_{l-1} = (K_l^T t_l) * act'(layer l - 1), as nn_mfma_eval
                const double* __restrict__ W = wl + net.woff[l] + lg * stride + li;
                sl_nd4 acc[4];
#pragma unroll
                for (int ib = 0; ib < 4; ++ib) acc[ib] = (sl_nd4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int s = 0; s < 16; ++s) {
                    if ((s >> 2) < nfb) {
                        const double b = nd4_get(t[s >> 2], s & 3);
#pragma unroll
                        for (int ib = 0; ib < 4; ++ib)
                            if (ib < nib)
                                acc[ib] = __builtin_amdgcn_mfma_f64_16x16x4f64(W[4 * s * stride + 16 * ib], b,
                                                                               acc[ib], 0, 0, 0);
                    }
                }
                const int a = net.act[l > 0 ? l - 1 : 0];
#pragma unroll
                for (int ib = 0; ib < 4; ++ib) {
                    const sl_nd4 hh = h[l > 0 ? l - 1 : 0][ib];
                    t[ib].x = acc[ib].x * sl_dact(a, hh.x > 0.0 ? 1.0 : -1.0, hh.x);
                    t[ib].y = acc[ib].y * sl_dact(a, hh.y > 0.0 ? 1.0 : -1.0, hh.y);
                    t[ib].z = acc[ib].z * sl_dact(a, hh.z > 0.0 ? 1.0 : -1.0, hh.z);
                    t[ib].w = acc[ib].w * sl_dact(a, hh.w > 0.0 ? 1.0 : -1.0, hh.w);
                }
            }
        }
    }
    // accumulator tile (wave, ib) of layer l: register r of lane (li, lg) = G_l[16 wave + 4 r + lg][16 ib + li]
    double* __restrict__ out = partials + (size_t)blockIdx.x * total;
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        const int in = net.dims[l], rows = net.dims[l + 1];
#pragma unroll
        for (int ib = 0; ib < 4; ++ib) {
            const int col = 16 * ib + li;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * wave + 4 * r + lg;
                if (row < rows && col < in) out[net.koff[l] + row * in + col] = nd4_get(gacc[l][ib], r);
            }
        }
    }
}

// The losses: V(x) (and V(x+)) of 16 samples per wavefront on the matrix cores, the per-sample terms
// of sl_nn_train.h on lanes 0..15, the coefficients and the point list [x; x+] written in place, the
// three sums per workgroup to the scratch area (lane sums -> LDS -> thread 0, ascending).
struct SlNnLossArgs {
    int kind, d;
    int64_t m;
    const double* states;
    const double* next;
    const double* labels;          // ROA: labels; ABS: targets
    const double* weights;
    double safe_level, lagrange, eps;
    double* coeff;
    double* points;
    double* partials;              // [gridDim.x][3]
};

template <int NL>
__global__ __launch_bounds__(64 * SL_NNM_WAVES) void k_nn_loss(SlAux aux, SlNnLossArgs a) {
    extern __shared__ __attribute__((aligned(16))) double wl[];
    __shared__ double red[16 * SL_NNM_WAVES][3];
    const SlNet& net = *aux.net;
    nn_stage_weights(net, wl);
    const int d = a.d, lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool roa = a.kind == SL_NN_LOSS_ROA;
    const double batch = (double)a.m;
    double sum[3] = {0.0, 0.0, 0.0};
    const int64_t step = (int64_t)gridDim.x * SL_NNM_WAVES * 16;
    for (int64_t base = ((int64_t)blockIdx.x * SL_NNM_WAVES + wave) * 16; base < a.m; base += step) {
        int64_t idx = base + (lane & 15);
        const bool valid = idx < a.m;
        idx = valid ? idx : a.m - 1;
        double x[SL_D], xn[SL_D];
#pragma unroll
        for (int k = 0; k < SL_D; ++k) if (k < d) x[k] = a.states[idx * d + k];
        const double v = nn_mfma_eval<NL>(net, wl, lane, x, d, false, nullptr);
        double v_next = 0.0;
        if (roa) {
#pragma unroll
            for (int k = 0; k < SL_D; ++k) if (k < d) xn[k] = a.next[idx * d + k];
            v_next = nn_mfma_eval<NL>(net, wl, lane, xn, d, false, nullptr);
        }
        if (valid && lane < 16) {
            const SlNnLossSample s = roa ? sl_nn_loss_roa(v, v_next, a.labels[idx], a.weights[idx], a.safe_level,
                                                          a.lagrange, a.eps, batch)
                                         : sl_nn_loss_abs(v, a.labels[idx], batch);
            a.coeff[idx] = s.coeff_x;
            if (roa) a.coeff[a.m + idx] = s.coeff_next;
            if (a.points) {
#pragma unroll
                for (int k = 0; k < SL_D; ++k)
                    if (k < d) {
                        a.points[idx * d + k] = x[k];
                        if (roa) a.points[(a.m + idx) * d + k] = xn[k];
                    }
            }
            sum[0] = sum[0] + s.objective;
            sum[1] = sum[1] + s.classifier;
            sum[2] = sum[2] + s.decrease;
        }
    }
    if (lane < 16) {
        red[16 * wave + lane][0] = sum[0];
        red[16 * wave + lane][1] = sum[1];
        red[16 * wave + lane][2] = sum[2];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double s = 0.0;
        for (int k = 0; k < 16 * SL_NNM_WAVES; ++k) s = s + red[k][threadIdx.x];
        a.partials[3 * blockIdx.x + threadIdx.x] = s;
    }
}

// losses[j] = (partials[0][j] + partials[1][j] + ...) / m
__global__ void k_nn_loss_finish(const double* __restrict__ partials, int nblocks, int64_t m,
                                 double* __restrict__ losses) {
    if (threadIdx.x >= 3) return;
    double s = 0.0;
    for (int b = 0; b < nblocks; ++b) s = s + partials[3 * b + threadIdx.x];
    losses[threadIdx.x] = s / (double)m;
}

// The two calls keep their per-workgroup slices in the context's scratch buffer (d_scratch, shared with
// sl_eval_points, whose use of it ends on the stream before theirs begins), between two guard zones of
// SL_NN_GUARD_WORDS words, written in front of the kernels of every call: one in the first words of the
// allocation and one directly behind the last double the kernels of that call own (not at the end of the
// allocation, which grows in steps of 1 MiB: a slice written a little past its area must hit it).  Word
// 0 of the front zone holds the number of doubles between the two, the other words a fixed pattern.
// sl_debug_nn_train_scratch reads them back.
#define SL_NN_GUARD_WORDS 8
#define SL_NN_GUARD_PATTERN 0x7ff8a5a55a5aa5a5ull

__global__ void k_nn_guards(uint64_t* __restrict__ front, uint64_t doubles) {
    uint64_t* __restrict__ back = front + SL_NN_GUARD_WORDS + doubles;
    if (threadIdx.x == 0) front[0] = doubles;
    else if (threadIdx.x < SL_NN_GUARD_WORDS) front[threadIdx.x] = SL_NN_GUARD_PATTERN;
    else if (threadIdx.x < 2 * SL_NN_GUARD_WORDS) back[threadIdx.x - SL_NN_GUARD_WORDS] = SL_NN_GUARD_PATTERN;
}

static int nn_train_scratch(sl_ctx* ctx, size_t doubles, double** out) {
    const size_t need = sizeof(double) * (doubles + 2 * SL_NN_GUARD_WORDS);
    SL_HIP_CHECK(ctx, sl_grow(ctx, &ctx->d_scratch, &ctx->scratch_bytes, need, (size_t)1 << 20));
    uint64_t* words = reinterpret_cast<uint64_t*>(ctx->d_scratch);
    hipLaunchKernelGGL(k_nn_guards, dim3(1), dim3(64), 0, ctx->stream, words, (uint64_t)doubles);
    SL_HIP_CHECK(ctx, hipGetLastError());
    *out = reinterpret_cast<double*>(words + SL_NN_GUARD_WORDS);
    return SL_OK;
}

extern "C" int sl_debug_nn_train_scratch(sl_ctx* ctx, int64_t* h_bytes, int* h_guards_intact) {
    if (!ctx || !h_bytes || !h_guards_intact)
        return sl_fail(ctx, SL_ERR_INVALID, "sl_debug_nn_train_scratch: NULL argument");
    *h_bytes = 0;
    *h_guards_intact = 0;
    const size_t capacity = ctx->scratch_bytes / sizeof(uint64_t);
    if (capacity < 2 * SL_NN_GUARD_WORDS) return SL_OK;
    SL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    SL_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    uint64_t guard[2][SL_NN_GUARD_WORDS];
    const uint64_t* words = reinterpret_cast<const uint64_t*>(ctx->d_scratch);
    SL_HIP_CHECK(ctx, hipMemcpy(guard[0], words, sizeof(guard[0]), hipMemcpyDeviceToHost));
    const uint64_t doubles = guard[0][0];
    // (a count that does not fit the allocation: the front zone was overwritten, or no call has run yet)
    if (doubles > capacity - 2 * SL_NN_GUARD_WORDS) return SL_OK;
    SL_HIP_CHECK(ctx, hipMemcpy(guard[1], words + SL_NN_GUARD_WORDS + doubles, sizeof(guard[1]),
                                hipMemcpyDeviceToHost));
    *h_bytes = (int64_t)(sizeof(double) * doubles);
    *h_guards_intact = 1;
    for (int k = 1; k < SL_NN_GUARD_WORDS; ++k)
        if (guard[0][k] != SL_NN_GUARD_PATTERN) *h_guards_intact = 0;
    for (int k = 0; k < SL_NN_GUARD_WORDS; ++k)
        if (guard[1][k] != SL_NN_GUARD_PATTERN) *h_guards_intact = 0;
    return SL_OK;
}

static int nn_train_check(sl_ctx* ctx, const char* who, int64_t m, int d) {
    if (!ctx) return sl_fail(nullptr, SL_ERR_INVALID, "%s: NULL context", who);
    if (!ctx->h_net.set) return sl_fail(ctx, SL_ERR_INVALID, "%s: network not set (sl_network_set)", who);
    if (m <= 0) return sl_fail(ctx, SL_ERR_INVALID, "%s: m = %lld points", who, (long long)m);
    if (d != ctx->h_net.dims[0])
        return sl_fail(ctx, SL_ERR_INVALID, "%s: points of %d columns, the network takes %d inputs", who, d,
                       ctx->h_net.dims[0]);
    // (sl_network_set takes inputs up to SL_NN_MAXW wide and these calls run without sl_model_set, where
    // the sweeps meet this limit: the kernels hold a point in SL_D registers)
    if (d < 1 || d > SL_MAX_STATE_DIM)
        return sl_fail(ctx, SL_ERR_INVALID, "%s: state dimension %d outside [1,%d]", who, d, SL_MAX_STATE_DIM);
    return SL_OK;
}

static int64_t nn_blocks_per_cu(size_t lds) { return lds > 75 * 1024 ? 1 : 2; }

extern "C" int sl_nn_param_grad(sl_ctx* ctx, int64_t m, int d, const double* d_points, const double* d_coeff,
                                double* d_grad_kernels) {
    if (const int rc = nn_train_check(ctx, "sl_nn_param_grad", m, d)) return rc;
    if (!d_points || !d_coeff || !d_grad_kernels)
        return sl_fail(ctx, SL_ERR_INVALID, "sl_nn_param_grad: NULL argument");
    SL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const SlNet& n = ctx->h_net;
    const int total = n.koff[n.nlayers - 1] + n.dims[n.nlayers - 1] * n.dims[n.nlayers];
    const size_t lds = nn_weight_bytes(ctx) + sizeof(double) * SL_NNG_CELLS * SL_NNG_STRIDE;
    int64_t blocks = (m + SL_NNG_CELLS - 1) / SL_NNG_CELLS;
    const int64_t cap = (int64_t)ctx->num_cu * nn_blocks_per_cu(lds);
    if (blocks > cap) blocks = cap;
    double* partials = nullptr;
    if (const int rc = nn_train_scratch(ctx, (size_t)blocks * total, &partials)) return rc;
    SlAux aux{ctx->d_tri, ctx->d_net};
    const int rc = sl_with_dim<1, 2, 3, 4>(n.nlayers, [&](auto nl) {
        SL_HIP_CHECK(ctx, sl_launch_lds(k_nn_param_grad<nl>, dim3((unsigned)blocks), dim3(64 * SL_NNG_WAVES), lds,
                                        ctx->stream, aux, m, d, d_points, d_coeff, partials, total));
        return SL_OK;
    });
    if (rc) return rc;
    return sl_sum_slices(ctx, partials, (int)blocks, total, d_grad_kernels);
}

extern "C" int sl_nn_loss(sl_ctx* ctx, int kind, int64_t m, int d, const double* d_states, const double* d_next,
                          const double* d_labels_or_targets, const double* d_class_weights, double safe_level,
                          double lagrange, double eps, double* d_losses, double* d_coeff, double* d_points) {
    if (const int rc = nn_train_check(ctx, "sl_nn_loss", m, d)) return rc;
    if (kind != SL_NN_LOSS_ABS && kind != SL_NN_LOSS_ROA)
        return sl_fail(ctx, SL_ERR_INVALID, "sl_nn_loss: unknown loss kind %d", kind);
    if (!d_states || !d_labels_or_targets || !d_losses || !d_coeff)
        return sl_fail(ctx, SL_ERR_INVALID, "sl_nn_loss: NULL argument");
    if (kind == SL_NN_LOSS_ROA && (!d_next || !d_class_weights))
        return sl_fail(ctx, SL_ERR_INVALID, "sl_nn_loss: SL_NN_LOSS_ROA needs the successors and the class weights");
    SL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    int64_t blocks = (m + 16 * SL_NNM_WAVES - 1) / (16 * SL_NNM_WAVES);
    const int64_t cap = (int64_t)ctx->num_cu * nn_blocks_per_cu(nn_weight_bytes(ctx));
    if (blocks > cap) blocks = cap;
    double* partials = nullptr;
    if (const int rc = nn_train_scratch(ctx, (size_t)blocks * 3, &partials)) return rc;
    SlAux aux{ctx->d_tri, ctx->d_net};
    const SlNnLossArgs a{kind, d, m, d_states, d_next, d_labels_or_targets, d_class_weights, safe_level, lagrange,
                         eps, d_coeff, d_points, partials};
    const int rc = sl_with_dim<1, 2, 3, 4>(ctx->h_net.nlayers, [&](auto nl) {
        SL_HIP_CHECK(ctx, sl_launch_lds(k_nn_loss<nl>, dim3((unsigned)blocks), dim3(64 * SL_NNM_WAVES),
                                        nn_weight_bytes(ctx), ctx->stream, aux, a));
        return SL_OK;
    });
    if (rc) return rc;
    hipLaunchKernelGGL(k_nn_loss_finish, dim3(1), dim3(64), 0, ctx->stream, partials, (int)blocks, m, d_losses);
    SL_HIP_CHECK(ctx, hipGetLastError());
    return SL_OK;
}
