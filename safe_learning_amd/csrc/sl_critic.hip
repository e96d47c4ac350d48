// sl_critic.hip - the actor-critic steps of examples/reinforcement_learning_pendulum.ipynb (cells 16, 31, 34, 48)
// and examples/reinforcement_learning_cartpole.ipynb (cell 15) with a NeuralNetwork as the value function:
//
//   target = stop_gradient(r(x, u) + gamma V(f(x, u))),  u = pi(x)
//   value objective  = reduce |V(x) - target|              -> var_list = value_function.parameters
//   policy objective = reduce (r(x, u) + gamma V(f(x, u)))   -> var_list = policy.parameters
//
//   sl_critic_batch       per sample x+, V(x), q = r + gamma V(x+), dq/du and the TD coefficient w sign(V(x) - q),
//                         and the two sums the objectives are made of (per-sample arithmetic: sl_critic.h)
//   sl_dense_param_grad   sum_i sum_o coeff[i][o] d net_o(p_i)/d theta for a dense network given in the call
//
// The context has one network slot and it belongs to the policy (sl_policy_network_set), so both calls take
// the value network in their arguments: the layer description on the host, the parameters as one device
// pointer packed as sl_policy_network_set packs its own (W_0, b_0, W_1, b_1, ..; W_l [in][out] row-major).
// Nothing here uses floating-point atomics: two calls with the same inputs return the same bits.
#include "sl_grad_host.h"
#include "sl_critic.h"

// the description of a dense network from the arguments of an entry point (`who`, for the message)
static int sl_dense_describe(sl_ctx* ctx, const char* who, int nlayers, const int32_t* h_dims,
                             const int32_t* h_activations, const int32_t* h_has_bias, double output_scale,
                             const double* d_params, SlPolicyNet* out) {
    if (!h_dims || !h_activations || !d_params) return sl_fail(ctx, SL_ERR_INVALID, "%s: NULL argument", who);
    if (nlayers < 1 || nlayers > SL_MAX_NN_LAYERS)
        return sl_fail(ctx, SL_ERR_INVALID, "%s: %d layers (max %d)", who, nlayers, SL_MAX_NN_LAYERS);
    SlPolicyNet n;
    memset(&n, 0, sizeof(n));
    n.nlayers = nlayers;
    n.scale = output_scale;
    for (int l = 0; l <= nlayers; ++l) {
        if (h_dims[l] < 1 || h_dims[l] > SL_NN_MAXW)
            return sl_fail(ctx, SL_ERR_INVALID, "%s: width %d outside [1,%d]", who, h_dims[l], SL_NN_MAXW);
        n.dims[l] = h_dims[l];
    }
    int32_t off = 0;
    for (int l = 0; l < nlayers; ++l) {
        if (h_activations[l] < 0 || h_activations[l] > 3)
            return sl_fail(ctx, SL_ERR_INVALID, "%s: activation code %d", who, h_activations[l]);
        n.act[l] = h_activations[l];
        n.koff[l] = off;
        off += h_dims[l] * h_dims[l + 1];
        n.boff[l] = -1;
        if (h_has_bias && h_has_bias[l]) {
            n.boff[l] = off;
            off += h_dims[l + 1];
        }
    }
    n.params = d_params;
    n.set = 1;
    *out = n;
    return SL_OK;
}

// =============================================================================================
// one sample per lane, grid stride
// =============================================================================================
// Every thread runs the dynamics with their tangent, the value network at x and at x+ and the transposed chain
// at x+ for its sample: the weights are read with wavefront-uniform addresses (scalar loads), the layer outputs
// live in per-lane arrays (private memory: profiles/actor_critic.md has what the compiler made of it).  The two
// sums: every lane adds its samples in ascending order, the wavefront and then the workgroup add their lanes
// in a fixed order, and the workgroup writes its pair to its own slot of context scratch for sl_sum_slices.
struct SlCriticModel {
    sl_dynamics_desc dynamics;
    sl_value_desc reward;
    double gamma;
    int32_t d, m;
};

struct SlCriticArgs {
    int64_t n;
    const double* states;      // [n][d]
    const double* actions;     // [n][m]
    double w;                  // 1/n ('mean') or 1 ('sum')
    double* next;              // [n][d] or null
    double* value;             // [n]
    double* q;                 // [n]
    double* dq_du;             // [n][m] or null
    double* coeff;             // [n] or null
    double* partials;          // [blocks][2]
};

template <int DYN, int DT>
__global__ __launch_bounds__(SL_BLOCK) void k_critic_batch(const SlCriticModel M, const SlPolicyNet net,
                                                          SlCriticArgs a) {
    __shared__ double red[2][SL_BLOCK / 64];
    const int d = DT > 0 ? DT : M.d, m = DT > 0 ? 1 : M.m;
    double sum_abs = 0.0, sum_q = 0.0;
    for (int64_t idx = (int64_t)blockIdx.x * SL_BLOCK + threadIdx.x; idx < a.n;
         idx += (int64_t)gridDim.x * SL_BLOCK) {
        double z[SL_P], nxt[SL_D], jac[SL_D][SL_M], g[SL_D];
        double h[SL_MAX_NN_LAYERS][SL_NN_MAXW], delta[SL_NN_MAXW], tmp[SL_NN_MAXW];
#pragma unroll
        for (int q = 0; q < SL_P; ++q) z[q] = 0.0;
#pragma unroll
        for (int k = 0; k < SL_D; ++k) if (k < d) z[k] = a.states[idx * d + k];
#pragma unroll
        for (int q = 0; q < SL_P; ++q) {
#pragma unroll
            for (int c = 0; c < SL_M; ++c) if (c < m && q == d + c) z[q] = a.actions[idx * m + c];
        }
        sl_critic_dynamics<DYN>(M.dynamics, d, m, z, nxt, jac);
        const double v_x = sl_critic_forward(net, z, h);
        const double v_next = sl_critic_forward(net, nxt, h);
        sl_critic_input_grad(net, h, delta, tmp, g);
        SlCriticSample s;
        sl_critic_point(M.reward, M.gamma, d, m, z, v_x, v_next, g, jac, a.w, &s);
        a.value[idx] = s.value;
        a.q[idx] = s.q;
        if (a.next) {
#pragma unroll
            for (int k = 0; k < SL_D; ++k) if (k < d) a.next[idx * d + k] = nxt[k];
        }
        if (a.dq_du) {
#pragma unroll
            for (int c = 0; c < SL_M; ++c) if (c < m) a.dq_du[idx * m + c] = s.dq_du[c];
        }
        if (a.coeff) a.coeff[idx] = s.coeff;
        sum_abs = sum_abs + fabs(s.delta);
        sum_q = sum_q + s.q;
    }
    for (int off = 32; off >= 1; off >>= 1) {
        sum_abs = sum_abs + __shfl_xor(sum_abs, off, 64);
        sum_q = sum_q + __shfl_xor(sum_q, off, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][wave] = sum_abs; red[1][wave] = sum_q; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < SL_BLOCK / 64; ++w) { sum_abs = sum_abs + red[0][w]; sum_q = sum_q + red[1][w]; }
        a.partials[2 * blockIdx.x] = sum_abs;
        a.partials[2 * blockIdx.x + 1] = sum_q;
    }
}

extern "C" int sl_critic_batch(sl_ctx* ctx, int nlayers, const int32_t* h_dims, const int32_t* h_activations,
                               const int32_t* h_has_bias, double output_scale, const double* d_params, int64_t n,
                               const double* d_states, const double* d_actions, int reduction, double* d_next,
                               double* d_value, double* d_q, double* d_dq_du, double* d_coeff, double* d_sums) {
    const char* who = "sl_critic_batch";
    if (!ctx) return sl_fail(nullptr, SL_ERR_INVALID, "%s: NULL context", who);
    if (!ctx->model_set) return sl_fail(ctx, SL_ERR_INVALID, "%s: call sl_model_set first", who);
    if (n <= 0) return sl_fail(ctx, SL_ERR_INVALID, "%s: n = %lld samples", who, (long long)n);
    if (!d_states || !d_actions || !d_value || !d_q || !d_sums)
        return sl_fail(ctx, SL_ERR_INVALID, "%s: NULL argument", who);
    if (reduction != SL_REDUCE_MEAN && reduction != SL_REDUCE_SUM)
        return sl_fail(ctx, SL_ERR_INVALID, "%s: reduction %d (SL_REDUCE_MEAN or SL_REDUCE_SUM)", who, reduction);
    SlPolicyNet net;
    if (const int rc = sl_dense_describe(ctx, who, nlayers, h_dims, h_activations, h_has_bias, output_scale, d_params,
                                         &net))
        return rc;
    const sl_model_desc& md = ctx->h_model.m;
    const int d = md.grid.d, m = md.policy.m, kind = md.dynamics.kind;
    if (net.dims[nlayers] != 1)
        return sl_fail(ctx, SL_ERR_INVALID, "%s: a value network has one output, this one %d", who, net.dims[nlayers]);
    if (net.dims[0] != d)
        return sl_fail(ctx, SL_ERR_INVALID, "%s: the value network takes %d inputs, the model's states have %d", who,
                       net.dims[0], d);
    if (kind == SL_DYN_GP)
        return sl_fail(ctx, SL_ERR_UNSUPPORTED, "%s: GP dynamics are not implemented here; sl_action_gradient serves "
                       "GP models with a value table", who);
    if (kind == SL_DYN_POLYNOMIAL)
        return sl_fail(ctx, SL_ERR_UNSUPPORTED, "%s: polynomial dynamics (SL_DYN_POLYNOMIAL) have no action tangent "
                       "in the engine yet", who);
    if (kind != SL_DYN_LINEAR && kind != SL_DYN_PENDULUM && kind != SL_DYN_CARTPOLE)
        return sl_fail(ctx, SL_ERR_UNSUPPORTED, "%s: dynamics kind %d", who, kind);
    // (sl_model_set has checked the Euler models' dimensions: (2, 1) and (4, 1))
    if (d < 1 || d > SL_MAX_STATE_DIM || m < 1 || m > SL_MAX_ACTION_DIM)
        return sl_fail(ctx, SL_ERR_INVALID, "%s: %d states and %d actions", who, d, m);
    if (md.reward.kind != SL_V_QUADRATIC)
        return sl_fail(ctx, SL_ERR_INVALID, "%s: the reward must be a quadratic form on [x, u]", who);
    SL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    int64_t blocks = (n + SL_BLOCK - 1) / SL_BLOCK;
    const int64_t cap = 2 * (int64_t)ctx->num_cu;
    if (blocks > cap) blocks = cap;
    SL_HIP_CHECK(ctx, sl_grow(ctx, &ctx->d_scratch, &ctx->scratch_bytes, sizeof(double) * 2 * (size_t)blocks,
                              (size_t)1 << 20));
    double* partials = reinterpret_cast<double*>(ctx->d_scratch);
    SlCriticModel M;
    M.dynamics = md.dynamics;
    M.reward = md.reward;
    M.gamma = md.gamma;
    M.d = d;
    M.m = m;
    const double w = reduction == SL_REDUCE_MEAN ? 1.0 / (double)n : 1.0;
    const SlCriticArgs a{n, d_states, d_actions, w, d_next, d_value, d_q, d_dq_du, d_coeff, partials};
    // the dynamics kind is a compile-time value; the Euler models fix the dimensions with it, a LinearSystem
    // has the (4, 1) instantiation and the generic one
    const int rc = sl_with_dim<SL_DYN_PENDULUM, SL_DYN_CARTPOLE, SL_DYN_LINEAR>(kind, [&](auto dyn) {
        constexpr int DYN = dyn;
        auto launch = [&](auto dim) {
            constexpr int D = dim;
            hipLaunchKernelGGL((k_critic_batch<DYN, D>), dim3((unsigned)blocks), dim3(SL_BLOCK), 0, ctx->stream, M,
                               net, a);
            SL_HIP_CHECK(ctx, hipGetLastError());
            return SL_OK;
        };
        if constexpr (DYN == SL_DYN_PENDULUM) return launch(std::integral_constant<int, 2>());
        else if constexpr (DYN == SL_DYN_CARTPOLE) return launch(std::integral_constant<int, 4>());
        else return sl_with_dim<4, 0>(m == 1 ? d : 0, launch);
    });
    if (rc) return rc;
    return sl_sum_slices(ctx, partials, (int)blocks, 2, d_sums);
}

extern "C" int sl_dense_param_grad(sl_ctx* ctx, int nlayers, const int32_t* h_dims, const int32_t* h_activations,
                                   const int32_t* h_has_bias, double output_scale, const double* d_params, int64_t n,
                                   int d, const double* d_points, const double* d_coeff, double* d_out) {
    const char* who = "sl_dense_param_grad";
    if (!ctx) return sl_fail(nullptr, SL_ERR_INVALID, "%s: NULL context", who);
    if (n <= 0) return sl_fail(ctx, SL_ERR_INVALID, "%s: n = %lld points", who, (long long)n);
    if (!d_points || !d_coeff || !d_out) return sl_fail(ctx, SL_ERR_INVALID, "%s: NULL argument", who);
    SlPolicyNet net;
    if (const int rc = sl_dense_describe(ctx, who, nlayers, h_dims, h_activations, h_has_bias, output_scale, d_params,
                                         &net))
        return rc;
    if (d != net.dims[0])
        return sl_fail(ctx, SL_ERR_INVALID, "%s: points of %d columns, the network takes %d inputs", who, d,
                       net.dims[0]);
    if (d < 1 || d > SL_MAX_STATE_DIM)
        return sl_fail(ctx, SL_ERR_INVALID, "%s: input width %d outside [1,%d]", who, d, SL_MAX_STATE_DIM);
    return sl_param_grad_launch(ctx, net, n, d, d_points, d_coeff, d_out);
}
