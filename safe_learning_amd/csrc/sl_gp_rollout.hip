// sl_gp_rollout.hip - closed-loop rollouts of the posterior MEAN of GP dynamics: what
// compute_trajectory, compute_roa and reward_rollout run for a GPMeanFunction
// (UncertainFunction.to_mean_function, safe_learning/functions.py:209-230).
//
// Stepped through the point evaluations, x -> mean f(x, policy(x)) is a policy launch and a full
// posterior call per step - the triangular product L^-1 k_x, O(n^2) per point, for a variance the step
// throws away.  The mean alone is prior(z) + sum_j k(z, x_j) alpha'_j, O(n p) per point: here one
// thread owns a trajectory, its state stays in registers between the steps as in k_rollout, and every
// step walks the training points of every head once (sl_gp_rollout.h: sl_next_state_mean's operations
// in its order).  The training inputs and alpha' are the same for every lane: they are read with
// wavefront-uniform addresses, one training point at a time, as k_bellman reads them, and through the
// constant address space so that they stay scalar loads beside the trajectory stores
// (SL_GP_UNIFORM, sl_gp_rollout.h); the exponential per (training point, trajectory, step) is the cost, and the dout <= d
// multiply-adds beside it are too few for the matrix cores.
//
// The contracts of sl_rollout_mean and sl_reward_rollout_mean are sl_rollout's and sl_reward_rollout's
// (sl_rollout.hip) with SL_DYN_GP as the one dynamics kind; the launch loop, the slab of per-step
// maxima, the fold and the launch run once more at the stopping step are restated from there, because
// that file's kernels must keep their registers and its host code is static beside them.
// Deterministic: no atomics on global memory, a maximum has no order.
#include "sl_common.h"
#include "sl_gp_rollout.h"

namespace {

struct GpRolloutArgs {
    int64_t lo, hi;
    const double* start;       // [hi - lo][d], or null: the grid points lo .. hi - 1
    int steps;
    double* state;             // [hi - lo][d] out
    double* traj;              // null or [steps][hi - lo][d]
    double* actions;           // null or [steps][hi - lo][m]
};

struct GpRewardArgs {
    int64_t lo, hi;
    const double* start;       // [hi - lo][d], or null: the grid points lo .. hi - 1
    const double* sum_in;      // [hi - lo] partial sums, or null: 0.0
    int steps;                 // <= SL_REWARD_CHUNK_MAX
    const double* weights;     // [steps] discount weights of this launch's steps
    double* state;             // [hi - lo][d] out
    double* sum;               // [hi - lo] out
    unsigned long long* slab;  // [gridDim.x][SL_REWARD_CHUNK_MAX] out: bit patterns of max |temp| per step
    int* h_workgroups;         // host: the launcher leaves gridDim.x here (the rows of the slab)
};

// the view of head h, built from the kernel's by-value head table inside the loop over the heads
struct GpHeads {
    const SlGpDev& gp;
    __device__ __forceinline__ SlGpHeadView operator()(int h) const {
        const SlGpHeadDev& hd = gp.head[h];
        return SlGpHeadView{hd.n, hd.n_pad, hd.dout, hd.col0, hd.variance, hd.inv_ls, hd.xs, hd.alpha, hd.kernel};
    }
};

// trajectories per thread.  A step is one long dependent chain per trajectory (the exponential).  The
// closed-form flavours need few registers, so several wavefronts per SIMD interleave their chains: one
// trajectory per thread.  The table flavour's look-up takes the registers of a whole SIMD (one wavefront
// each, and a bound of two workgroups spills): there two trajectories per thread interleave instead.
template <bool GENERAL>
struct GpPerThread { static constexpr int value = GENERAL ? 2 : 1; };

// mean of the GP dynamics at explicit [x, u] rows: one thread per row, grid stride
template <int DT, int MT>
__global__ __launch_bounds__(SL_BLOCK) void k_gp_mean_points(const SlDevModel M, const SlGpDev gp, int64_t n,
                                                            const double* __restrict__ inputs,
                                                            double* __restrict__ mean) {
    const SlDims nd = sl_dims<DT, MT>(M);
    for (int64_t idx = (int64_t)blockIdx.x * SL_BLOCK + threadIdx.x; idx < n;
         idx += (int64_t)gridDim.x * SL_BLOCK) {
        double z[1][SL_P], nxt[1][SL_D];
#pragma unroll
        for (int q = 0; q < SL_P; ++q) z[0][q] = (q < nd.p) ? inputs[idx * nd.p + q] : 0.0;
        sl_gp_mean<1>(M.m.dynamics, gp.nheads, GpHeads{gp}, nd, z, nxt);
#pragma unroll
        for (int k = 0; k < SL_D; ++k) if (k < nd.d) mean[idx * nd.d + k] = nxt[0][k];
    }
}

// k_rollout with the GP mean as the dynamics.  GENERAL: the interpolated policy of table slot 1, its
// descriptor staged in LDS.
template <bool GENERAL, int DT, int MT>
__global__ __launch_bounds__(SL_BLOCK) void k_gp_rollout(const SlDevModel M, const SlGpDev gp, SlAux aux_arg,
                                                        const GpRolloutArgs a) {
    __shared__ SlTriLds<GENERAL> tri_lds;
    const SlAux aux = sl_stage_aux<GENERAL>(tri_lds, aux_arg);
    constexpr int NT = GpPerThread<GENERAL>::value;
    const SlDims n = sl_dims<DT, MT>(M);
    const int64_t count = a.hi - a.lo;
    // a per-trajectory action table (a network policy's actions of this step) is indexed by the
    // absolute trajectory number
    const double* table = M.m.policy.kind == SL_POLICY_TABLE ? M.m.policy.d_table : nullptr;
    for (int64_t base = (int64_t)blockIdx.x * (NT * SL_BLOCK); base < count;
         base += (int64_t)gridDim.x * (NT * SL_BLOCK)) {
        double z[NT][SL_P];
        int64_t row[NT];
        bool valid[NT];
        const double* table_rows[NT];
        // no branches on `valid`: lanes past the end simulate the last trajectory and store nothing
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int64_t raw = base + (int64_t)t * SL_BLOCK + threadIdx.x;
            valid[t] = raw < count;
            row[t] = valid[t] ? raw : count - 1;
#pragma unroll
            for (int q = 0; q < SL_P; ++q) z[t][q] = 0.0;
            if (a.start) {
#pragma unroll
                for (int k = 0; k < SL_D; ++k) if (k < n.d) z[t][k] = a.start[row[t] * n.d + k];
            } else {
                sl_index_to_grid_point(M.m.grid, M.gf, n.d, a.lo + row[t], z[t]);
            }
            table_rows[t] = table ? table + (a.lo + row[t]) * n.m : nullptr;
        }
        sl_gp_rollout_advance<GENERAL, NT>(
            M, n, aux.tri + 1, gp.nheads, GpHeads{gp}, table_rows, a.steps, z,
            [&](int s, int t, const double* x, const double* u) {
                if (!valid[t]) return;
                if (a.traj) {
                    double* o = a.traj + ((int64_t)s * count + row[t]) * n.d;
#pragma unroll
                    for (int k = 0; k < SL_D; ++k) if (k < n.d) o[k] = x[k];
                }
                if (a.actions) {
                    double* o = a.actions + ((int64_t)s * count + row[t]) * n.m;
#pragma unroll
                    for (int q = 0; q < SL_M; ++q) if (q < n.m) o[q] = u[q];
                }
            });
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (valid[t]) {
#pragma unroll
                for (int k = 0; k < SL_D; ++k) if (k < n.d) a.state[row[t] * n.d + k] = z[t][k];
            }
        }
    }
}

// max over the wavefront of the bit patterns of non-negative doubles (they order like unsigned
// integers; every NaN pattern lies above infinity's, so a NaN anywhere comes out as a NaN)
__device__ __forceinline__ unsigned long long gp_wave_max_bits(unsigned long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

// k_reward_rollout with the GP mean as the dynamics: state, action and running sum in registers for
// the a.steps steps of the launch; step_max[s] collects max |temp| of step s over the wavefronts and
// the grid-stride passes of this workgroup (LDS atomics of lane 0) and leaves it once, as plain
// stores into the slab.
template <bool GENERAL, int DT, int MT>
__global__ __launch_bounds__(SL_BLOCK) void k_gp_reward_rollout(const SlDevModel M, const SlGpDev gp, SlAux aux_arg,
                                                               const GpRewardArgs a) {
    __shared__ SlTriLds<GENERAL> tri_lds;
    __shared__ unsigned long long step_max[SL_REWARD_CHUNK_MAX];
    for (int s = threadIdx.x; s < SL_REWARD_CHUNK_MAX; s += SL_BLOCK) step_max[s] = 0ull;
    const SlAux aux = sl_stage_aux<GENERAL>(tri_lds, aux_arg);
    __syncthreads();
    constexpr int NT = GpPerThread<GENERAL>::value;
    const SlDims n = sl_dims<DT, MT>(M);
    const int64_t count = a.hi - a.lo;
    const double* table = M.m.policy.kind == SL_POLICY_TABLE ? M.m.policy.d_table : nullptr;
    // (the loop bound depends on the workgroup alone: every lane is there for the shuffles)
    for (int64_t base = (int64_t)blockIdx.x * (NT * SL_BLOCK); base < count;
         base += (int64_t)gridDim.x * (NT * SL_BLOCK)) {
        double z[NT][SL_P], acc[NT];
        int64_t row[NT];
        bool valid[NT];
        const double* table_rows[NT];
        // lanes past the end simulate the last trajectory, contribute 0 to the maxima and store nothing
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int64_t raw = base + (int64_t)t * SL_BLOCK + threadIdx.x;
            valid[t] = raw < count;
            row[t] = valid[t] ? raw : count - 1;
#pragma unroll
            for (int q = 0; q < SL_P; ++q) z[t][q] = 0.0;
            if (a.start) {
#pragma unroll
                for (int k = 0; k < SL_D; ++k) if (k < n.d) z[t][k] = a.start[row[t] * n.d + k];
            } else {
                sl_index_to_grid_point(M.m.grid, M.gf, n.d, a.lo + row[t], z[t]);
            }
            acc[t] = a.sum_in ? a.sum_in[row[t]] : 0.0;
            table_rows[t] = table ? table + (a.lo + row[t]) * n.m : nullptr;
        }
        unsigned long long mine = 0ull;
        sl_gp_reward_rollout_advance<GENERAL, NT>(
            M, n, aux.tri + 1, gp.nheads, GpHeads{gp}, table_rows, a.steps, a.weights, z, acc,
            [&](int s, int t, double magnitude) {
                const unsigned long long bits =
                    valid[t] ? (unsigned long long)__double_as_longlong(magnitude) : 0ull;
                mine = (t == 0 || bits > mine) ? bits : mine;
                if (t == NT - 1) {
                    const unsigned long long top = gp_wave_max_bits(mine);
                    if ((threadIdx.x & 63) == 0) atomicMax(&step_max[s], top);
                }
            });
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (valid[t]) {
#pragma unroll
                for (int k = 0; k < SL_D; ++k) if (k < n.d) a.state[row[t] * n.d + k] = z[t][k];
                a.sum[row[t]] = acc[t];
            }
        }
    }
    __syncthreads();
    for (int s = threadIdx.x; s < a.steps; s += SL_BLOCK)
        a.slab[(int64_t)blockIdx.x * SL_REWARD_CHUNK_MAX + s] = step_max[s];
}

// workgroup s: out[s] = max over the slab's workgroups of step s
__global__ __launch_bounds__(SL_BLOCK) void k_gp_reward_fold(const unsigned long long* __restrict__ slab,
                                                             int workgroups, unsigned long long* __restrict__ out) {
    __shared__ unsigned long long part[SL_BLOCK / 64];
    unsigned long long v = 0ull;
    for (int b = threadIdx.x; b < workgroups; b += SL_BLOCK) {
        const unsigned long long o = slab[(int64_t)b * SL_REWARD_CHUNK_MAX + blockIdx.x];
        v = o > v ? o : v;
    }
    v = gp_wave_max_bits(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < SL_BLOCK / 64; ++w) v = part[w] > v ? part[w] : v;
        out[blockIdx.x] = v;
    }
}

template <bool G, int D, int MM>
void launch_variant(sl_ctx* ctx, const GpRolloutArgs& a) {
    constexpr int NT = GpPerThread<G>::value;
    const int blocks = sl_grid_blocks((a.hi - a.lo + NT - 1) / NT);
    hipLaunchKernelGGL((k_gp_rollout<G, D, MM>), dim3(blocks), dim3(SL_BLOCK), 0, ctx->stream, ctx->h_model,
                       ctx->h_gp, SlAux{ctx->d_tri, ctx->d_net}, a);
}

template <bool G, int D, int MM>
void launch_variant(sl_ctx* ctx, const GpRewardArgs& a) {
    constexpr int NT = GpPerThread<G>::value;
    const int blocks = sl_grid_blocks((a.hi - a.lo + NT - 1) / NT);
    *a.h_workgroups = blocks;
    hipLaunchKernelGGL((k_gp_reward_rollout<G, D, MM>), dim3(blocks), dim3(SL_BLOCK), 0, ctx->stream, ctx->h_model,
                       ctx->h_gp, SlAux{ctx->d_tri, ctx->d_net}, a);
}

// one launch of a.steps steps under the model the context holds right now: the closed-form (and
// per-trajectory table) policies for (d, 1), d = 1 .. 4 and, generic, for the other dimensions; the
// interpolated policy for (2, 1) (check_model refuses it elsewhere: its generic flavour with the
// mean beside the table walk does not fit the registers without scratch)
template <class Args>
int launch_any(sl_ctx* ctx, const Args& a) {
    const SlDevModel& M = ctx->h_model;
    if (M.m.policy.kind == SL_POLICY_TRI) {
        launch_variant<true, 2, 1>(ctx, a);
    } else {
        sl_with_dim<1, 2, 3, 4, 0>(sl_dim_variant_of(M), [&](auto dt) {
            launch_variant<false, dt, dt != 0 ? 1 : 0>(ctx, a);
            return SL_OK;
        });
    }
    SL_HIP_CHECK(ctx, hipGetLastError());
    return SL_OK;
}

// what both entry points check before anything runs (`who`: the entry point; `like`: the
// deterministic entry point a model without GP dynamics belongs to)
int check_model(sl_ctx* ctx, const char* who, const char* like, int64_t lo, int64_t hi, const double* d_start,
                int steps) {
    if (!d_start && hi > ctx->h_model.gf.nindex)
        return sl_fail(ctx, SL_ERR_INVALID, "%s: trajectories [%lld, %lld) past the grid's %lld cells", who,
                       (long long)lo, (long long)hi, (long long)ctx->h_model.gf.nindex);
    if (ctx->h_model.m.dynamics.kind != SL_DYN_GP)
        return sl_fail(ctx, SL_ERR_UNSUPPORTED, "%s: dynamics kind %d; the mean rollouts simulate SL_DYN_GP only "
                                                "(deterministic dynamics: %s)", who, ctx->h_model.m.dynamics.kind, like);
    if (ctx->h_gp.nheads < 1)
        return sl_fail(ctx, SL_ERR_INVALID, "%s: GP dynamics without heads (sl_gp_configure)", who);
    const int policy = ctx->h_model.m.policy.kind;
    if (policy == SL_POLICY_TRI && !ctx->h_tri[1].set)
        return sl_fail(ctx, SL_ERR_INVALID, "%s: policy table (sl_tri_set slot 1) not set", who);
    if (policy == SL_POLICY_TRI && sl_dim_variant_of(ctx->h_model) != 2)
        return sl_fail(ctx, SL_ERR_UNSUPPORTED, "%s: the interpolated policy is compiled for 2 states and 1 action, "
                                                "the model has %d and %d", who, ctx->h_model.m.grid.d,
                       ctx->h_model.m.policy.m);
    if (policy == SL_POLICY_TABLE && steps > 1)
        return sl_fail(ctx, SL_ERR_INVALID, "%s: a per-vertex policy table is defined at the vertices only (one "
                                            "step); use the interpolated table (SL_POLICY_TRI)", who);
    return SL_OK;
}

int64_t training_points(const sl_ctx* ctx) {
    int64_t total = 0;
    for (int h = 0; h < ctx->h_gp.nheads; ++h) total += ctx->h_gp.head[h].n;
    return total;
}

// The launches of one sl_reward_rollout_mean call: a kernel launch, the fold of its slab and the one
// host read of the folded maxima.
struct GpRewardRun {
    sl_ctx* ctx;
    int64_t lo, hi;
    const double* weights;         // [horizon] on the device
    unsigned long long* slab;      // [SL_MAX_GRID][SL_REWARD_CHUNK_MAX]
    unsigned long long* folded;    // [SL_REWARD_CHUNK_MAX]
    int launches;

    // steps [done, done + c) from (start, sum_in) into (state, sum); h_max: the maxima of the c
    // steps read back (one synchronisation), or null: nobody needs them (a launch run again)
    int run(const double* start, const double* sum_in, int done, int c, double* state, double* sum, double* h_max) {
        int workgroups = 0;
        const int rc = launch_any(ctx, GpRewardArgs{lo, hi, start, sum_in, c, weights + done, state, sum, slab,
                                                    &workgroups});
        if (rc) return rc;
        ++launches;
        if (!h_max) return SL_OK;
        hipLaunchKernelGGL(k_gp_reward_fold, dim3(c), dim3(SL_BLOCK), 0, ctx->stream, slab, workgroups, folded);
        SL_HIP_CHECK(ctx, hipGetLastError());
        static_assert(sizeof(double) == sizeof(unsigned long long), "the maxima travel as bit patterns");
        SL_HIP_CHECK(ctx, hipMemcpyAsync(h_max, folded, sizeof(double) * c, hipMemcpyDeviceToHost, ctx->stream));
        SL_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        return SL_OK;
    }
};

}  // namespace

extern "C" int sl_gp_mean_points(sl_ctx* ctx, int64_t n, const double* d_inputs, double* d_mean) {
    if (!ctx) return sl_fail(nullptr, SL_ERR_INVALID, "sl_gp_mean_points: NULL context");
    if (!ctx->model_set) return sl_fail(ctx, SL_ERR_INVALID, "sl_gp_mean_points: call sl_model_set first");
    if (n < 0 || (n > 0 && (!d_inputs || !d_mean)))
        return sl_fail(ctx, SL_ERR_INVALID, "sl_gp_mean_points: negative count or NULL buffer");
    if (ctx->h_model.m.dynamics.kind != SL_DYN_GP)
        return sl_fail(ctx, SL_ERR_UNSUPPORTED, "sl_gp_mean_points: dynamics kind %d; the model's dynamics must be GP "
                                                "dynamics (SL_DYN_GP)", ctx->h_model.m.dynamics.kind);
    if (ctx->h_gp.nheads < 1)
        return sl_fail(ctx, SL_ERR_INVALID, "sl_gp_mean_points: GP dynamics without heads (sl_gp_configure)");
    if (n == 0) return SL_OK;
    SL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const int blocks = sl_grid_blocks(n);
    const int rc = sl_with_dim<1, 2, 3, 4, 0>(sl_dim_variant_of(ctx->h_model), [&](auto dim) {
        constexpr int D = dim;
        hipLaunchKernelGGL((k_gp_mean_points<D, D != 0 ? 1 : 0>), dim3(blocks), dim3(SL_BLOCK), 0, ctx->stream,
                           ctx->h_model, ctx->h_gp, n, d_inputs, d_mean);
        SL_HIP_CHECK(ctx, hipGetLastError());
        return SL_OK;
    });
    if (rc) return rc;
    sl_note_kernel(ctx, false, "k_gp_mean_points<d=%d>, %lld training points", sl_dim_variant_of(ctx->h_model),
                   (long long)training_points(ctx));
    return SL_OK;
}

extern "C" int sl_rollout_mean(sl_ctx* ctx, int64_t lo, int64_t hi, const double* d_start, int steps,
                               int steps_per_launch, double* d_state, double* d_traj, double* d_actions) {
    const char* who = "sl_rollout_mean";
    if (!ctx) return sl_fail(nullptr, SL_ERR_INVALID, "%s: NULL context", who);
    if (!ctx->model_set) return sl_fail(ctx, SL_ERR_INVALID, "%s: call sl_model_set first", who);
    const int d = ctx->h_model.m.grid.d, m = ctx->h_model.m.policy.m;
    const int policy = ctx->h_model.m.policy.kind;
    if (lo < 0 || hi < lo || steps < 0 || steps_per_launch < 0 || !d_state)
        return sl_fail(ctx, SL_ERR_INVALID, "%s: bad range, negative step count or NULL state buffer", who);
    if (const int rc = check_model(ctx, who, "sl_rollout", lo, hi, d_start, steps)) return rc;
    if (hi == lo) return SL_OK;
    SL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const int64_t n = hi - lo;
    ctx->last_kernel[0] = 0;
    if (policy == SL_POLICY_NETWORK) {
        // the network's actions of a step become a per-trajectory table (k_policy_network), then one
        // single-step launch reads it: the states pass through d_state between the two
        if (d_start != d_state) {
            const int rc = launch_any(ctx, GpRolloutArgs{lo, hi, d_start, 0, d_state, nullptr, nullptr});
            if (rc) return rc;
        }
        for (int s = 0; s < steps; ++s) {
            SlPolicyTableScope network_policy(ctx, lo, hi, d_state - lo * d);   // (indexed by trajectory number)
            if (network_policy.rc) return network_policy.rc;
            const int rc = launch_any(ctx, GpRolloutArgs{lo, hi, d_state, 1, d_state,
                                                         d_traj ? d_traj + (int64_t)s * n * d : nullptr,
                                                         d_actions ? d_actions + (int64_t)s * n * m : nullptr});
            if (rc) return rc;
        }
        sl_note_kernel(ctx, false, "k_policy_network + k_gp_rollout, %d single steps", steps);
        return SL_OK;
    }
    const int chunk = steps_per_launch > 0 ? steps_per_launch : sl_gp_rollout_chunk(n, steps, training_points(ctx));
    const double* src = d_start;
    int done = 0, launches = 0;
    do {
        const int c = steps - done < chunk ? steps - done : chunk;
        const int rc = launch_any(ctx, GpRolloutArgs{lo, hi, src, c, d_state,
                                                     d_traj ? d_traj + (int64_t)done * n * d : nullptr,
                                                     d_actions ? d_actions + (int64_t)done * n * m : nullptr});
        if (rc) return rc;
        src = d_state;
        done += c;
        ++launches;
    } while (done < steps);
    sl_note_kernel(ctx, false, "k_gp_rollout<general=%d, d=%d>, %lld training points, %d steps in %d launches",
                   (int)(policy == SL_POLICY_TRI), d, (long long)training_points(ctx), steps, launches);
    return SL_OK;
}

extern "C" int sl_reward_rollout_mean(sl_ctx* ctx, int64_t lo, int64_t hi, const double* d_start, int horizon,
                                      const double* d_weights, double tol, int steps_per_launch, double* d_sum,
                                      double* d_state, int64_t* h_steps, int* h_converged) {
    const char* who = "sl_reward_rollout_mean";
    if (!ctx) return sl_fail(nullptr, SL_ERR_INVALID, "%s: NULL context", who);
    if (!ctx->model_set) return sl_fail(ctx, SL_ERR_INVALID, "%s: call sl_model_set first", who);
    const int d = ctx->h_model.m.grid.d;
    const int policy = ctx->h_model.m.policy.kind;
    if (lo < 0 || hi < lo || horizon < 1 || steps_per_launch < 0 || !d_weights || !d_sum || !d_state)
        return sl_fail(ctx, SL_ERR_INVALID, "%s: bad range, horizon < 1, negative steps per launch or NULL weights, "
                                            "sum or state buffer", who);
    if (const int rc = check_model(ctx, who, "sl_reward_rollout", lo, hi, d_start, horizon)) return rc;
    if (ctx->h_model.m.reward.kind != SL_V_QUADRATIC)
        return sl_fail(ctx, SL_ERR_INVALID, "%s: the model's reward is not a quadratic function on [x, u] "
                                            "(reward.kind %d)", who, ctx->h_model.m.reward.kind);
    if (h_steps) *h_steps = 0;
    if (h_converged) *h_converged = 0;
    if (hi == lo) return SL_OK;
    SL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const int64_t n = hi - lo;
    ctx->last_kernel[0] = 0;
    // scratch: the second (state, sum) pair, the slab and the folded maxima
    const size_t pair_doubles = (size_t)n * (d + 1);
    const size_t slab_words = (size_t)SL_MAX_GRID * SL_REWARD_CHUNK_MAX;
    SL_HIP_CHECK(ctx, sl_grow(ctx, &ctx->d_scratch, &ctx->scratch_bytes,
                              sizeof(double) * (pair_doubles + slab_words + SL_REWARD_CHUNK_MAX)));
    double* const other_state = reinterpret_cast<double*>(ctx->d_scratch);
    double* const other_sum = other_state + (size_t)n * d;
    unsigned long long* const slab = reinterpret_cast<unsigned long long*>(other_sum + n);
    GpRewardRun r{ctx, lo, hi, d_weights, slab, slab + slab_words, 0};
    double h_max[SL_REWARD_CHUNK_MAX];
    int done = 0, converged = 0;
    if (policy == SL_POLICY_NETWORK) {
        // the network's actions of a step become a per-trajectory table (k_policy_network), then one
        // single-step launch in place: a launch of one step never has steps past the stopping step
        if (d_start != d_state) {
            const int rc = launch_any(ctx, GpRolloutArgs{lo, hi, d_start, 0, d_state, nullptr, nullptr});
            if (rc) return rc;
        }
        while (done < horizon && !converged) {
            SlPolicyTableScope network_policy(ctx, lo, hi, d_state - lo * d);   // (indexed by trajectory number)
            if (network_policy.rc) return network_policy.rc;
            const int rc = r.run(d_state, done ? d_sum : nullptr, done, 1, d_state, d_sum, h_max);
            if (rc) return rc;
            converged = sl_reward_stop_offset(h_max, 1, tol) == 0;
            ++done;
        }
        sl_note_kernel(ctx, false, "k_policy_network + k_gp_reward_rollout, %d single steps", done);
    } else {
        int chunk = steps_per_launch > 0 ? steps_per_launch
                                         : sl_gp_reward_rollout_chunk(n, horizon, training_points(ctx));
        if (chunk > SL_REWARD_CHUNK_MAX) chunk = SL_REWARD_CHUNK_MAX;
        // launch k reads what launch k - 1 wrote and writes the other pair; the first one reads d_start
        // and may write d_state unless that is d_start itself
        double* const state[2] = {d_state, other_state};
        double* const sum[2] = {d_sum, other_sum};
        int out = d_start == d_state ? 1 : 0, redone = 0;
        const double* src_state = d_start;
        const double* src_sum = nullptr;
        while (done < horizon && !converged) {
            const int c = horizon - done < chunk ? horizon - done : chunk;
            int rc = r.run(src_state, src_sum, done, c, state[out], sum[out], h_max);
            if (rc) return rc;
            const int stop = sl_reward_stop_offset(h_max, c, tol);
            if (stop >= 0) {
                // the sums hold terms past the stopping step unless it is the launch's last: once more,
                // from the same inputs, cut there
                if (stop + 1 < c) {
                    rc = r.run(src_state, src_sum, done, stop + 1, state[out], sum[out], nullptr);
                    if (rc) return rc;
                    redone = 1;
                }
                done += stop + 1;
                converged = 1;
            } else {
                done += c;
            }
            src_state = state[out];
            src_sum = sum[out];
            out ^= 1;
        }
        if (src_state != d_state) {
            SL_HIP_CHECK(ctx, hipMemcpyAsync(d_state, src_state, sizeof(double) * (size_t)n * d,
                                             hipMemcpyDeviceToDevice, ctx->stream));
            SL_HIP_CHECK(ctx, hipMemcpyAsync(d_sum, src_sum, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice,
                                             ctx->stream));
        }
        sl_note_kernel(ctx, false, "k_gp_reward_rollout<general=%d, d=%d>, %lld training points, %d steps in %d "
                                   "launches (%d redone)", (int)(policy == SL_POLICY_TRI), d,
                       (long long)training_points(ctx), done, r.launches, redone);
    }
    if (h_steps) *h_steps = done;
    if (h_converged) *h_converged = converged;
    return SL_OK;
}
