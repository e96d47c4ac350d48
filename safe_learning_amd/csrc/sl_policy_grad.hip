// sl_policy_grad.hip - policy gradients of PolicyIteration.future_values
// (safe_learning/reinforcement_learning.py:65-114; the `optimizer.minimize(-reduce(rl.future_values(states)),
// var_list=rl.policy.parameters)` of examples/inverted_pendulum.ipynb cells 9/12 and of
// safe_learning/tests/test_rl.py:29-77), with the chain rule cut at the action:
//
//   sl_action_gradient     dQ/du at every point (per-point arithmetic: sl_policy_grad.h)
//   sl_policy_param_grad   sum_i sum_o coeff[i][o] d pi_o(p_i)/d theta for a NeuralNetwork policy
//   sl_tri_param_grad      the same sum for the vertex table of a Triangulation policy
//
// Nothing here uses floating-point atomics: two calls with the same inputs return the same bits.
#include "sl_grad_host.h"
#include "sl_policy_grad.h"

// =============================================================================================
// dQ/du: one thread per point, grid stride
// =============================================================================================
// Both table descriptors are staged in the workgroup's LDS (the look-ups walk every unit-cell simplex).
// The GP heads' inputs and alpha' are read from global memory as sl_next_state_mean reads them, one
// training point at a time with wavefront-uniform addresses (scalar loads, one fetch per wavefront and
// point) and not staged through LDS in chunks: the resource summary (profiles/policy_training.md) shows
// the kernel limited by registers - the generic table walk of sl_tri_eval beside the model in scalar
// registers takes the whole budget of a 256-thread workgroup, one wavefront per SIMD, without scratch
// in the fixed-dimension instantiations - so LDS for a chunk would buy no second workgroup, and per
// training point the exponential and the product rule outweigh the p + dout scalar loads.
struct SlActionGradArgs {
    int64_t n;
    const double* points;      // [n][d] or null: the grid points of the model
    const double* actions;     // [n][m] or null: policy(x)
    double* grad;              // [n][m]
    double* q;                 // [n] or null
    double* next;              // [n][d] or null
};

template <int DT, int MT>
__global__ __launch_bounds__(SL_BLOCK) void k_action_gradient(const SlDevModel M, const SlGpDev gp, SlAux aux_in,
                                                             SlActionGradArgs a) {
    __shared__ SlTriLds<true> lds;
    const SlAux aux = sl_stage_aux<true>(lds, aux_in);
    const SlDims nd = sl_dims<DT, MT>(M);
    const int d = nd.d, m = nd.m, p = nd.p;
    const SlTri& vt = aux.tri[0];
    for (int64_t idx = (int64_t)blockIdx.x * SL_BLOCK + threadIdx.x; idx < a.n;
         idx += (int64_t)gridDim.x * SL_BLOCK) {
        double z[SL_P], u[SL_M];
#pragma unroll
        for (int q = 0; q < SL_P; ++q) z[q] = 0.0;
        sl_cell_state(M, d, idx, a.points, z);
        if (a.actions) {
#pragma unroll
            for (int c = 0; c < SL_M; ++c) if (c < m) u[c] = a.actions[idx * m + c];
        } else {
            sl_policy_any<true>(M, nd, aux.tri, idx, z, u);
        }
        sl_append_action(nd, u, z);
        double mean[SL_D], jac[SL_D][SL_M];
#pragma unroll
        for (int k = 0; k < SL_D; ++k) {
            mean[k] = 0.0;
#pragma unroll
            for (int c = 0; c < SL_M; ++c) jac[k][c] = 0.0;
        }
        if (M.m.dynamics.kind == SL_DYN_GP) {
            for (int h = 0; h < gp.nheads; ++h) {
                const SlGpHeadDev& hd = gp.head[h];
                const SlPgHead head{hd.n, hd.n_pad, hd.dout, hd.col0, hd.variance, hd.inv_ls, hd.xs, hd.alpha,
                                    hd.kernel};
                sl_pg_head(head, p, d, m, z, mean, jac);
            }
        }
        sl_pg_linear_part(M.m.dynamics, d, m, z, mean, jac);
        double g[SL_M];
        const double qv = sl_pg_point(M.m.reward, M.m.value, M.m.gamma, vt, d, m, z, mean, jac, g);
#pragma unroll
        for (int c = 0; c < SL_M; ++c) if (c < m) a.grad[idx * m + c] = g[c];
        if (a.q) a.q[idx] = qv;
        if (a.next) {
#pragma unroll
            for (int k = 0; k < SL_D; ++k) if (k < d) a.next[idx * d + k] = mean[k];
        }
    }
}

extern "C" int sl_action_gradient(sl_ctx* ctx, int64_t n, const double* d_points, const double* d_actions,
                                  double* d_grad, double* d_q, double* d_next) {
    const char* who = "sl_action_gradient";
    if (const int rc = sl_point_grad_arguments(ctx, who, n, d_grad)) return rc;
    const sl_model_desc& md = ctx->h_model.m;
    if (md.dynamics.kind == SL_DYN_POLYNOMIAL)
        return sl_fail(ctx, SL_ERR_UNSUPPORTED, "sl_action_gradient: polynomial dynamics (SL_DYN_POLYNOMIAL) have no "
                       "action tangent in the engine yet; the action gradient is implemented for linear and GP "
                       "dynamics");
    if (md.dynamics.kind != SL_DYN_LINEAR && md.dynamics.kind != SL_DYN_GP)
        return sl_fail(ctx, SL_ERR_UNSUPPORTED, "sl_action_gradient: dynamics kind %d; the action gradient is "
                       "implemented for SL_DYN_LINEAR and SL_DYN_GP", md.dynamics.kind);
    if (md.value.kind != SL_V_TRI || !ctx->h_tri[0].set)
        return sl_fail(ctx, SL_ERR_INVALID, "sl_action_gradient: the value function must be the table of slot 0");
    if (md.reward.kind != SL_V_QUADRATIC)
        return sl_fail(ctx, SL_ERR_INVALID, "sl_action_gradient: the reward must be a quadratic form on [x, u]");
    if (ctx->h_tri[0].grid.d != md.grid.d)
        return sl_fail(ctx, SL_ERR_INVALID, "sl_action_gradient: value table of %d dimensions, states of %d",
                       ctx->h_tri[0].grid.d, md.grid.d);
    if (const int rc = sl_point_grad_gp_heads(ctx, who)) return rc;
    if (const int rc = sl_point_grad_on_grid(ctx, who, n, d_points)) return rc;
    if (n == 0) return SL_OK;
    SL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    // a network policy: one action per point first, as everywhere else
    SlPolicyTableScope network_policy(ctx, 0, d_actions ? 0 : n, d_points);
    if (const int rc = sl_point_grad_policy(ctx, who, d_points, d_actions, network_policy)) return rc;
    int64_t blocks = (n + SL_BLOCK - 1) / SL_BLOCK;
    const int64_t cap = 2 * (int64_t)ctx->num_cu;
    if (blocks > cap) blocks = cap;
    const SlAux aux{ctx->d_tri, ctx->d_net};
    const SlActionGradArgs a{n, d_points, d_actions, d_grad, d_q, d_next};
    // (state, action) dimensions fixed at compile time for the grids the sweeps are compiled for, one
    // generic instantiation for the rest
    return sl_with_dim<1, 2, 3, 4, 0>(sl_dim_variant_of(ctx->h_model), [&](auto dim) {
        constexpr int D = dim;
        hipLaunchKernelGGL((k_action_gradient<D, D != 0 ? 1 : 0>), dim3((unsigned)blocks), dim3(SL_BLOCK), 0,
                           ctx->stream, ctx->h_model, ctx->h_gp, aux, a);
        SL_HIP_CHECK(ctx, hipGetLastError());
        return SL_OK;
    });
}

// =============================================================================================
// NeuralNetwork policy: sum_i sum_o coeff[i][o] d pi_o(p_i)/d theta
// =============================================================================================
// pi = scale h_L, h_l = act_l(h_{l-1} W_l + b_l) (functions.py:1702-1729).  With delta_l = d(sum_o
// coeff_o pi_o)/d(pre-activation of layer l) the gradient of W_l ([in][out]) is the outer product
// h_{l-1} delta_l^T summed over the points and the gradient of b_l the column sums of delta_l.
//
// A workgroup of four wavefronts owns 256 points at a time, the point on the lane: every thread runs
// the forward chain and the transposed chain of its point (the weights read with wavefront-uniform
// addresses, the activations in per-lane arrays, as k_policy_network).  The outer products need the
// point along the MFMA's k: at every layer of the way back the workgroup's four 64-point groups cross
// two [64 points][64 features] staging tiles in LDS in turn - h_{l-1} and delta_l - and the FOUR
// wavefronts share the [in x out] product of each group out among themselves as k_nn_param_grad does:
// wavefront w owns the input rows 16 w .. 16 w + 15 (A fragments from the h tile), the output blocks of
// 16 come as B fragments from the delta tile, v_mfma_f64_16x16x4_f64 with the points as the reduction
// dimension.  The accumulator tiles (4 per layer and wavefront) stay in registers for the whole
// grid-stride loop.  Bias gradients: thread o < out adds column o of the delta tile, points ascending.
// A point past n enters with coefficient 0.  No atomics: a workgroup writes its sums to its own slice of
// the context's scratch and sl_sum_slices adds the slices in ascending order.
#define SL_PPG_WAVES 4
#define SL_PPG_POINTS (64 * SL_PPG_WAVES)
#define SL_PPG_STRIDE (SL_NN_MAXW + 2)          // staging row of one point (+2: LDS bank spread)
#define SL_PPG_TILE (64 * SL_PPG_STRIDE)

typedef double sl_pg4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ double pg_act(int a, double x) {
    if (a == 1) return sl_tanh(x);
    if (a == 2) return x > 0.0 ? x : 0.0;
    if (a == 3) return 1.0 / (1.0 + exp(-x));
    return x;
}

template <int NL>
__global__ __launch_bounds__(SL_PPG_POINTS) void k_policy_param_grad(const SlPolicyNet net, int64_t n, int d,
                                                                     const double* __restrict__ points,
                                                                     const double* __restrict__ coeff,
                                                                     double* __restrict__ partials, int total) {
    extern __shared__ __attribute__((aligned(16))) double tiles[];
    double* __restrict__ tile_h = tiles;                       // [64][SL_PPG_STRIDE]: h_{l-1} of a 64-point group
    double* __restrict__ tile_d = tiles + SL_PPG_TILE;         // [64][SL_PPG_STRIDE]: delta_l of the same group
    const int lane = threadIdx.x & 63, li = lane & 15, lg = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m = net.dims[NL];
    sl_pg4 gacc[NL][4];
    double bacc[NL];
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        bacc[l] = 0.0;
#pragma unroll
        for (int ob = 0; ob < 4; ++ob) gacc[l][ob] = (sl_pg4){0.0, 0.0, 0.0, 0.0};
    }
    const int64_t step = (int64_t)gridDim.x * SL_PPG_POINTS;
    // (the trip count is the same for every thread of the workgroup: the barriers below are uniform)
    for (int64_t base = (int64_t)blockIdx.x * SL_PPG_POINTS; base < n; base += step) {
        int64_t idx = base + threadIdx.x;
        const bool valid = idx < n;
        idx = valid ? idx : n - 1;
        // forward: h[l] = input of layer l, h[NL] = the last layer's output
        double h[NL + 1][SL_NN_MAXW], delta[SL_NN_MAXW], dprev[SL_NN_MAXW];
        for (int k = 0; k < d; ++k) h[0][k] = points[idx * d + k];
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            const int in = net.dims[l], out = net.dims[l + 1];
            const double* K = net.params + net.koff[l];            // [in][out]
            const double* bias = net.boff[l] >= 0 ? net.params + net.boff[l] : nullptr;
            for (int o = 0; o < out; ++o) {
                double s = 0.0;
                for (int i = 0; i < in; ++i) s = fma(h[l][i], K[i * out + o], s);
                if (bias) s = s + bias[o];
                h[l + 1][o] = pg_act(net.act[l], s);
            }
        }
        // delta_L[o] = (coeff[i][o] * scale) * act'(h_L[o]); a point past n: coefficient 0
        for (int o = 0; o < m; ++o) {
            const double c = valid ? coeff[idx * m + o] : 0.0;
            const double cs = c * net.scale;
            delta[o] = cs * sl_pg_dact(net.act[NL - 1], h[NL][o]);
        }
#pragma unroll
        for (int l = NL - 1; l >= 0; --l) {
            const int in = net.dims[l], out = net.dims[l + 1];
            const int in_pad = (in + 15) & ~15, out_pad = (out + 15) & ~15;
            const int nob = out_pad >> 4;
            const bool mine = 16 * wave < in;                  // this wavefront owns input rows 16 wave ..
            for (int sub = 0; sub < SL_PPG_WAVES; ++sub) {
                __syncthreads();                               // (the tiles' last readers are through)
                if (wave == sub) {
                    double* __restrict__ row_h = tile_h + lane * SL_PPG_STRIDE;
                    double* __restrict__ row_d = tile_d + lane * SL_PPG_STRIDE;
                    for (int i = 0; i < in_pad; ++i) row_h[i] = i < in ? h[l][i] : 0.0;
                    for (int o = 0; o < out_pad; ++o) row_d[o] = o < out ? delta[o] : 0.0;
                }
                __syncthreads();
                if (mine) {
                    const double* __restrict__ fa = tile_h + lg * SL_PPG_STRIDE + 16 * wave + li;
                    const double* __restrict__ fb = tile_d + lg * SL_PPG_STRIDE + li;
#pragma unroll
                    for (int s = 0; s < 16; ++s) {
                        const double af = fa[4 * s * SL_PPG_STRIDE];   // point 4 s + lg, input row 16 wave + li
#pragma unroll
                        for (int ob = 0; ob < 4; ++ob)
                            if (ob < nob)
                                gacc[l][ob] = __builtin_amdgcn_mfma_f64_16x16x4f64(
                                    af, fb[4 * s * SL_PPG_STRIDE + 16 * ob], gacc[l][ob], 0, 0, 0);
                    }
                }
                if ((int)threadIdx.x < out && net.boff[l] >= 0) {
                    double s = bacc[l];
                    for (int q = 0; q < 64; ++q) s = s + tile_d[q * SL_PPG_STRIDE + threadIdx.x];
                    bacc[l] = s;
                }
            }
            if (l > 0) {
                // delta_{l-1} = (W_l delta_l) * act'(layer l - 1)
                const double* K = net.params + net.koff[l];
                const int a_prev = net.act[l > 0 ? l - 1 : 0];
                for (int i = 0; i < in; ++i) {
                    double s = 0.0;
                    for (int o = 0; o < out; ++o) s = fma(K[i * out + o], delta[o], s);
                    dprev[i] = s * sl_pg_dact(a_prev, h[l][i]);
                }
                for (int i = 0; i < in; ++i) delta[i] = dprev[i];
            }
        }
    }
    // accumulator tile (wave, ob) of layer l: register r of lane (li, lg) = G_l[16 wave + 4 r + lg][16 ob + li]
    double* __restrict__ out_slice = partials + (size_t)blockIdx.x * total;
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        const int in = net.dims[l], out = net.dims[l + 1];
#pragma unroll
        for (int ob = 0; ob < 4; ++ob) {
            const int col = 16 * ob + li;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * wave + 4 * r + lg;
                if (row < in && col < out) out_slice[net.koff[l] + row * out + col] = gacc[l][ob][r];
            }
        }
        if ((int)threadIdx.x < out && net.boff[l] >= 0) out_slice[net.boff[l] + threadIdx.x] = bacc[l];
    }
}

// out[e] = partials[0][e] + partials[1][e] + ... in that order: the same bits at every call
__global__ __launch_bounds__(SL_BLOCK) void k_sum_slices(const double* __restrict__ partials, int nblocks, int total,
                                                         double* __restrict__ out) {
    const int e = blockIdx.x * SL_BLOCK + threadIdx.x;
    if (e >= total) return;
    double s = 0.0;
    for (int b = 0; b < nblocks; ++b) s = s + partials[(size_t)b * total + e];
    out[e] = s;
}

int sl_sum_slices(sl_ctx* ctx, const double* partials, int nblocks, int total, double* out) {
    hipLaunchKernelGGL(k_sum_slices, dim3((total + SL_BLOCK - 1) / SL_BLOCK), dim3(SL_BLOCK), 0, ctx->stream, partials,
                       nblocks, total, out);
    SL_HIP_CHECK(ctx, hipGetLastError());
    return SL_OK;
}

// k_policy_param_grad on a checked network description, then the slices in order (sl_policy_param_grad: the
// context's policy network; sl_dense_param_grad, sl_critic.hip: a description built from its arguments)
int sl_param_grad_launch(sl_ctx* ctx, const SlPolicyNet& net, int64_t n, int d, const double* d_points,
                         const double* d_coeff, double* d_grad) {
    SL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const int L = net.nlayers;
    int total = net.koff[L - 1] + net.dims[L - 1] * net.dims[L];
    if (net.boff[L - 1] >= 0) total = net.boff[L - 1] + net.dims[L];
    const size_t lds = sizeof(double) * 2 * SL_PPG_TILE;
    int64_t blocks = (n + SL_PPG_POINTS - 1) / SL_PPG_POINTS;
    const int64_t cap = 2 * (int64_t)ctx->num_cu;
    if (blocks > cap) blocks = cap;
    SL_HIP_CHECK(ctx, sl_grow(ctx, &ctx->d_scratch, &ctx->scratch_bytes, sizeof(double) * (size_t)blocks * total,
                              (size_t)1 << 20));
    double* partials = reinterpret_cast<double*>(ctx->d_scratch);
    const int rc = sl_with_dim<1, 2, 3, 4>(L, [&](auto nl) {
        SL_HIP_CHECK(ctx, sl_launch_lds(k_policy_param_grad<nl>, dim3((unsigned)blocks), dim3(SL_PPG_POINTS), lds,
                                        ctx->stream, net, n, d, d_points, d_coeff, partials, total));
        return SL_OK;
    });
    if (rc) return rc;
    return sl_sum_slices(ctx, partials, (int)blocks, total, d_grad);
}

extern "C" int sl_policy_param_grad(sl_ctx* ctx, int64_t n, int d, const double* d_points, const double* d_coeff,
                                    double* d_grad) {
    if (!ctx) return sl_fail(nullptr, SL_ERR_INVALID, "sl_policy_param_grad: NULL context");
    const SlPolicyNet& net = ctx->pnet;
    if (!net.set) return sl_fail(ctx, SL_ERR_INVALID, "sl_policy_param_grad: network policy not set "
                                                      "(sl_policy_network_set)");
    if (n <= 0) return sl_fail(ctx, SL_ERR_INVALID, "sl_policy_param_grad: n = %lld points", (long long)n);
    if (d != net.dims[0])
        return sl_fail(ctx, SL_ERR_INVALID, "sl_policy_param_grad: points of %d columns, the network takes %d "
                       "inputs", d, net.dims[0]);
    if (d < 1 || d > SL_MAX_STATE_DIM)
        return sl_fail(ctx, SL_ERR_INVALID, "sl_policy_param_grad: input width %d outside [1,%d]", d,
                       SL_MAX_STATE_DIM);
    if (!d_points || !d_coeff || !d_grad) return sl_fail(ctx, SL_ERR_INVALID, "sl_policy_param_grad: NULL argument");
    return sl_param_grad_launch(ctx, net, n, d, d_points, d_coeff, d_grad);
}

// =============================================================================================
// Triangulation policy: grad[v][:] = sum over (i, k) with simplex_k(p_i) = v of coeff[i][:] w_ik
// =============================================================================================
// (vertex, position) pairs are emitted per point, ordered by vertex with sl_sort_pairs (stable: ties in
// position order, i.e. ascending point and corner), and the first pair of every run adds its run in
// that order.
__global__ __launch_bounds__(SL_BLOCK) void k_tri_pg_emit(const SlTri* __restrict__ tri, int64_t n,
                                                         const double* __restrict__ points,
                                                         uint64_t* __restrict__ keys, int64_t* __restrict__ vals,
                                                         double* __restrict__ weights) {
    __shared__ SlTri t;
    sl_stage_tri(&t, tri);
    const int d = t.grid.d, k1 = d + 1;
    for (int64_t idx = (int64_t)blockIdx.x * SL_BLOCK + threadIdx.x; idx < n;
         idx += (int64_t)gridDim.x * SL_BLOCK) {
        double x[SL_D], w[SL_D + 1];
        int64_t vert[SL_D + 1];
#pragma unroll
        for (int k = 0; k < SL_D; ++k) x[k] = k < d ? points[idx * d + k] : 0.0;
        sl_pg_tri_locate(t, x, vert, w);
#pragma unroll
        for (int k = 0; k <= SL_D; ++k) {
            if (k < k1) {
                keys[idx * k1 + k] = (uint64_t)vert[k];
                vals[idx * k1 + k] = idx * k1 + k;
                weights[idx * k1 + k] = w[k];
            }
        }
    }
}

__global__ __launch_bounds__(SL_BLOCK) void k_tri_pg_sum(int64_t npairs, int k1, int cols, int64_t nindex,
                                                        const uint64_t* __restrict__ keys,
                                                        const int64_t* __restrict__ vals,
                                                        const double* __restrict__ weights,
                                                        const double* __restrict__ coeff, double* __restrict__ grad) {
    for (int64_t q = (int64_t)blockIdx.x * SL_BLOCK + threadIdx.x; q < npairs;
         q += (int64_t)gridDim.x * SL_BLOCK) {
        const uint64_t v = keys[q];
        if (q > 0 && keys[q - 1] == v) continue;               // not the first pair of its run
        if (v >= (uint64_t)nindex) continue;
        for (int c = 0; c < cols; ++c) {
            double s = 0.0;
            for (int64_t r = q; r < npairs && keys[r] == v; ++r) {
                const int64_t pos = vals[r];
                const double t = coeff[(pos / k1) * cols + c] * weights[pos];
                s = s + t;
            }
            grad[(int64_t)v * cols + c] = s;
        }
    }
}

extern "C" int sl_tri_param_grad(sl_ctx* ctx, int slot, int64_t n, const double* d_points, const double* d_coeff,
                                 double* d_grad) {
    if (!ctx) return sl_fail(nullptr, SL_ERR_INVALID, "sl_tri_param_grad: NULL context");
    if (slot < 0 || slot > 1 || !ctx->h_tri[slot].set)
        return sl_fail(ctx, SL_ERR_INVALID, "sl_tri_param_grad: table slot %d not set (sl_tri_set)", slot);
    if (n <= 0 || !d_points || !d_coeff || !d_grad)
        return sl_fail(ctx, SL_ERR_INVALID, "sl_tri_param_grad: bad argument");
    const SlTri& t = ctx->h_tri[slot];
    const int k1 = t.grid.d + 1, cols = t.ncols;
    int64_t nindex = 1;
    for (int k = 0; k < t.grid.d; ++k) nindex *= t.grid.num_points[k];
    const int64_t npairs = n * k1;
    if (npairs > 0x7fffffffll)
        return sl_fail(ctx, SL_ERR_UNSUPPORTED, "sl_tri_param_grad: %lld (point, corner) pairs, at most 2^31 - 1",
                       (long long)npairs);
    SL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    // keys, keys_tmp, vals, vals_tmp, weights: npairs words each, then the counters of the sort
    const size_t need = sizeof(uint64_t) * 5 * (size_t)npairs + sizeof(uint32_t) * SL_SORT_COUNT_WORDS;
    SL_HIP_CHECK(ctx, sl_grow(ctx, &ctx->d_scratch, &ctx->scratch_bytes, need, (size_t)1 << 20));
    uint64_t* keys = reinterpret_cast<uint64_t*>(ctx->d_scratch);
    uint64_t* keys_tmp = keys + npairs;
    int64_t* vals = reinterpret_cast<int64_t*>(keys_tmp + npairs);
    int64_t* vals_tmp = vals + npairs;
    double* weights = reinterpret_cast<double*>(vals_tmp + npairs);
    uint32_t* counts = reinterpret_cast<uint32_t*>(weights + npairs);
    SL_HIP_CHECK(ctx, hipMemsetAsync(d_grad, 0, sizeof(double) * (size_t)nindex * cols, ctx->stream));
    hipLaunchKernelGGL(k_tri_pg_emit, dim3(sl_grid_blocks(n)), dim3(SL_BLOCK), 0, ctx->stream, ctx->d_tri + slot, n,
                       d_points, keys, vals, weights);
    SL_HIP_CHECK(ctx, hipGetLastError());
    if (const int rc = sl_sort_pairs(ctx, npairs, keys, vals, keys_tmp, vals_tmp, counts)) return rc;
    hipLaunchKernelGGL(k_tri_pg_sum, dim3(sl_grid_blocks(npairs)), dim3(SL_BLOCK), 0, ctx->stream, npairs, k1, cols,
                       nindex, keys, vals, weights, d_coeff, d_grad);
    SL_HIP_CHECK(ctx, hipGetLastError());
    return SL_OK;
}
