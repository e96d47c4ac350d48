// sl_grad_host.h - host code the gradient entry points share.  Host only: the kernels share nothing through it.
// (Not in sl_common.h: the counter measurements under profiles/ are tied to the bytes of that file.)
#pragma once

#include "sl_common.h"

// out[e] = partials[0][e] + partials[1][e] + .. + partials[nblocks - 1][e], e < total, added in that order on
// ctx->stream (k_sum_slices, sl_policy_grad.hip): what makes the parameter gradients the same bits at every call
int sl_sum_slices(sl_ctx* ctx, const double* partials, int nblocks, int total, double* out);

// k_policy_param_grad (sl_policy_grad.hip) for a network description the caller has checked (widths, layer count,
// d = net.dims[0] <= SL_MAX_STATE_DIM, n >= 1, non-null pointers), then sl_sum_slices into d_grad
int sl_param_grad_launch(sl_ctx* ctx, const SlPolicyNet& net, int64_t n, int d, const double* d_points,
                         const double* d_coeff, double* d_grad);

// The checks sl_action_gradient and sl_decrease_gradient have in common (`who`: the entry point, for the
// message), in the order both call them, each with its own checks in between.
static inline int sl_point_grad_arguments(sl_ctx* ctx, const char* who, int64_t n, const double* d_grad) {
    if (!ctx) return sl_fail(nullptr, SL_ERR_INVALID, "%s: NULL context", who);
    if (!ctx->model_set) return sl_fail(ctx, SL_ERR_INVALID, "%s: call sl_model_set first", who);
    if (n < 0 || !d_grad) return sl_fail(ctx, SL_ERR_INVALID, "%s: bad argument", who);
    return SL_OK;
}
static inline int sl_point_grad_gp_heads(sl_ctx* ctx, const char* who) {
    if (ctx->h_model.m.dynamics.kind == SL_DYN_GP && ctx->h_gp.nheads < 1)
        return sl_fail(ctx, SL_ERR_INVALID, "%s: GP dynamics without heads (sl_gp_configure)", who);
    return SL_OK;
}
static inline int sl_point_grad_on_grid(sl_ctx* ctx, const char* who, int64_t n, const double* d_points) {
    if (!d_points && n > ctx->h_model.gf.nindex)
        return sl_fail(ctx, SL_ERR_INVALID, "%s: %lld points on a grid of %lld", who, (long long)n,
                       (long long)ctx->h_model.gf.nindex);
    return SL_OK;
}
// ... and behind the entry point's own SlPolicyTableScope: can the kernels evaluate the policy at the points?
static inline int sl_point_grad_policy(sl_ctx* ctx, const char* who, const double* d_points, const double* d_actions,
                                       const SlPolicyTableScope& network_policy) {
    if (network_policy.rc) return network_policy.rc;
    if (d_actions) return SL_OK;
    const int kind = ctx->h_model.m.policy.kind;
    if (kind == SL_POLICY_TRI && !ctx->h_tri[1].set)
        return sl_fail(ctx, SL_ERR_INVALID, "%s: policy table not set", who);
    if (kind == SL_POLICY_TABLE && d_points && !network_policy.swapped)
        return sl_fail(ctx, SL_ERR_UNSUPPORTED, "%s: a per-vertex policy table cannot be "
                                                "evaluated at arbitrary points", who);
    return SL_OK;
}
