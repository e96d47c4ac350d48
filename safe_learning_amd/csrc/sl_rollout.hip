// sl_rollout.hip - closed-loop rollouts: compute_trajectory (safe_learning/utilities.py:519-583)
// and the simulation behind compute_roa (examples/utilities.py:654-686) for every trajectory of a
// grid or a point list at once.
//
// A Lyapunov sweep evaluates x -> f(x, policy(x)) once per cell; a rollout applies it H - 1 times
// to the same cell.  Composed from the point evaluations (sl_eval_points: policy, then dynamics)
// every step is two launches and d + m + (d + m) + (2 + 2 d) doubles of traffic per trajectory;
// here one thread owns a trajectory and its state stays in registers between the steps
// (sl_rollout.h: the same device functions, in the same order, as the sweeps).  What leaves the
// registers is the end state and, on request, the state and action of every step, written
// step-major so that the 64 rows a wavefront stores per step are one contiguous block.
//
// reward_rollout (examples/utilities.py:522-545) adds a reward and a running sum to the same
// registers (sl_reward_rollout.h) and the reference's GLOBAL stopping rule: the loop ends after the
// first step whose max over all trajectories of |discount^t reward| is below tol.  Every step of a
// launch therefore leaves one maximum: reduced inside the wavefront, combined across the
// wavefronts and the grid-stride passes of a workgroup in LDS, stored once per workgroup and step
// into a [workgroups][steps] slab that k_reward_fold folds - no global atomics, and a maximum has
// no order, so the result is deterministic.  The host reads the folded maxima once per launch; when
// the stopping step lies inside the launch, the launch is run once more from its own inputs (state
// and partial sums ping-pong between two buffer pairs) with the step count cut there, because a
// sequential floating-point sum cannot be undone by subtraction.
#include "sl_common.h"
#include "sl_reward_rollout.h"

namespace {

struct RolloutArgs {
    int64_t lo, hi;
    const double* start;       // [hi - lo][d], or null: the grid points lo .. hi - 1
    int steps;
    double* state;             // [hi - lo][d] out
    double* traj;              // null or [steps][hi - lo][d]
    double* actions;           // null or [steps][hi - lo][m]
};

// trajectories per thread: the linear step is one short chain of dependent FP64 operations, two of
// them interleave (k_det_sweep's CPT = 2); the Euler steps have no registers to spare for that
template <bool GENERAL, int DT, int DYN>
struct PerThread { static constexpr int value = (!GENERAL && DT > 0 && DYN == SL_DYN_LINEAR) ? 2 : 1; };

struct RewardArgs {
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

// The model constants of a closed-loop step outnumber the scalar registers; each one is held in a
// VGPR of its own - the same value in all lanes, opaque to the optimiser - and is then a plain
// vector operand (k_det_sweep's sl_constants_to_vgprs, without the constants of the decrease
// check that a rollout does not have).
template <int DT, int MT, int DYN>
__device__ __forceinline__ void rollout_constants_to_vgprs(SlDevModel& L) {
#define SL_TO_VGPR(x) asm volatile("" : "+v"(x))
    if (DYN != SL_DYN_LINEAR) {
        // (the polynomial kind reads no coef[]: its terms come from the context's table)
        if (DYN != SL_DYN_POLYNOMIAL) {
#pragma unroll
            for (int q = 0; q < 16; ++q) SL_TO_VGPR(L.m.dynamics.coef[q]);
        }
#pragma unroll
        for (int k = 0; k < DT; ++k) { SL_TO_VGPR(L.m.dynamics.tx[k]); SL_TO_VGPR(L.m.dynamics.tx_inv[k]); }
#pragma unroll
        for (int a = 0; a < MT; ++a) SL_TO_VGPR(L.m.dynamics.tu[a]);
    } else {
#pragma unroll
        for (int k = 0; k < DT; ++k) {
#pragma unroll
            for (int q = 0; q < DT + MT; ++q) SL_TO_VGPR(L.m.dynamics.matrix[k][q]);
        }
    }
#pragma unroll
    for (int a = 0; a < MT; ++a) {
#pragma unroll
        for (int k = 0; k < DT; ++k) SL_TO_VGPR(L.m.policy.matrix[a][k]);
        SL_TO_VGPR(L.m.policy.lower[a]);
        SL_TO_VGPR(L.m.policy.upper[a]);
    }
#undef SL_TO_VGPR
}

// One thread per trajectory (NT of them where they interleave), grid stride over [lo, hi).
// GENERAL: the interpolated policy of table slot 1, its descriptor staged in LDS.
template <bool GENERAL, int DT, int MT, int DYN>
__global__ __launch_bounds__(SL_BLOCK, GENERAL ? 2 : 1) void k_rollout(const SlDevModel M_arg, SlAux aux_arg,
                                                                       const RolloutArgs a) {
    __shared__ SlTriLds<GENERAL> tri_lds;
    const SlAux aux = sl_stage_aux<GENERAL>(tri_lds, aux_arg);
    SlDevModel M = M_arg;
    if (!GENERAL && DT > 0 && DYN != 0) rollout_constants_to_vgprs<DT, MT, DYN>(M);
    constexpr int NT = PerThread<GENERAL, DT, DYN>::value;
    const SlDims n = sl_dims<DT, MT>(M);
    const int64_t count = a.hi - a.lo;
    // a per-trajectory action table (a network policy's actions of this step) is indexed like the
    // sweeps index theirs: by the absolute trajectory number
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
            if (a.start) {
#pragma unroll
                for (int k = 0; k < SL_D; ++k) if (k < n.d) z[t][k] = a.start[row[t] * n.d + k];
            } else {
                sl_index_to_grid_point(M.m.grid, M.gf, n.d, a.lo + row[t], z[t]);
            }
            table_rows[t] = table ? table + (a.lo + row[t]) * n.m : nullptr;
        }
        sl_rollout_advance<GENERAL, DYN, NT>(
            M, n, aux.tri + 1, table_rows, a.steps, z,
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

// max over the wavefront of the bit patterns of non-negative doubles: they order like unsigned
// integers, and every NaN pattern lies above infinity's, so a NaN anywhere comes out as a NaN
__device__ __forceinline__ unsigned long long wave_max_bits(unsigned long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

// k_rollout with a reward: one thread per trajectory (NT where they interleave), state, action and
// running sum in registers for the a.steps steps of the launch.  step_max[s] collects max |temp| of
// step s over the wavefronts and the grid-stride passes of this workgroup (LDS atomics of lane 0,
// at most four contenders); it leaves the workgroup once, as plain stores into the slab.
// (One workgroup per CU is all the bound asks for: the generic table variant then keeps in the 512
// registers of a lone wavefront per SIMD what k_rollout's bound of two makes it spill.)
template <bool GENERAL, int DT, int MT, int DYN>
__global__ __launch_bounds__(SL_BLOCK, 1) void k_reward_rollout(const SlDevModel M_arg, SlAux aux_arg,
                                                                              const RewardArgs a) {
    __shared__ SlTriLds<GENERAL> tri_lds;
    __shared__ unsigned long long step_max[SL_REWARD_CHUNK_MAX];
    for (int s = threadIdx.x; s < SL_REWARD_CHUNK_MAX; s += SL_BLOCK) step_max[s] = 0ull;
    const SlAux aux = sl_stage_aux<GENERAL>(tri_lds, aux_arg);
    __syncthreads();
    SlDevModel M = M_arg;
    if (!GENERAL && DT > 0 && DYN != 0) {
        rollout_constants_to_vgprs<DT, MT, DYN>(M);
#pragma unroll
        for (int i = 0; i < DT + MT; ++i) {
#pragma unroll
            for (int j = 0; j < DT + MT; ++j) asm volatile("" : "+v"(M.m.reward.matrix[i][j]));
        }
    }
    constexpr int NT = PerThread<GENERAL, DT, DYN>::value;
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
        sl_reward_rollout_advance<GENERAL, DYN, NT>(
            M, n, aux.tri + 1, table_rows, a.steps, a.weights, z, acc, [&](int s, int t, double magnitude) {
                const unsigned long long bits =
                    valid[t] ? (unsigned long long)__double_as_longlong(magnitude) : 0ull;
                mine = (t == 0 || bits > mine) ? bits : mine;
                if (t == NT - 1) {
                    const unsigned long long top = wave_max_bits(mine);
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
__global__ __launch_bounds__(SL_BLOCK) void k_reward_fold(const unsigned long long* __restrict__ slab, int workgroups,
                                                          unsigned long long* __restrict__ out) {
    __shared__ unsigned long long part[SL_BLOCK / 64];
    unsigned long long v = 0ull;
    for (int b = threadIdx.x; b < workgroups; b += SL_BLOCK) {
        const unsigned long long o = slab[(int64_t)b * SL_REWARD_CHUNK_MAX + blockIdx.x];
        v = o > v ? o : v;
    }
    v = wave_max_bits(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < SL_BLOCK / 64; ++w) v = part[w] > v ? part[w] : v;
        out[blockIdx.x] = v;
    }
}

struct Equilibrium { double e[SL_D]; };

// end states -> bit mask (one ballot per wavefront, like the sweeps' neg_bits) and its population
__global__ __launch_bounds__(SL_BLOCK) void k_rollout_mask(int64_t n, int d, const double* __restrict__ state,
                                                           const Equilibrium eq, double tol,
                                                           uint64_t* __restrict__ bits,
                                                           unsigned long long* __restrict__ count) {
    unsigned long long inside = 0;
    for (int64_t base = (int64_t)blockIdx.x * SL_BLOCK; base < n; base += (int64_t)gridDim.x * SL_BLOCK) {
        const int64_t idx = base + threadIdx.x;
        bool member = false;
        if (idx < n) {
            double x[SL_D];
#pragma unroll
            for (int k = 0; k < SL_D; ++k) if (k < d) x[k] = state[idx * d + k];
            member = sl_roa_member(d, x, eq.e, tol, nullptr);
        }
        const uint64_t word = __ballot(member);
        const int64_t wbase = base + (threadIdx.x & ~63);
        if ((threadIdx.x & 63) == 0 && wbase < n) {
            bits[wbase >> 6] = word;
            inside += (unsigned long long)__popcll(word);
        }
    }
    if (count && inside) atomicAdd(count, inside);
}

template <bool G, int D, int MM, int DYN>
void launch_variant(sl_ctx* ctx, const RolloutArgs& a) {
    constexpr int NT = PerThread<G, D, DYN>::value;
    const int blocks = sl_grid_blocks((a.hi - a.lo + NT - 1) / NT);
    hipLaunchKernelGGL((k_rollout<G, D, MM, DYN>), dim3(blocks), dim3(SL_BLOCK), 0, ctx->stream, ctx->h_model,
                       SlAux{ctx->d_tri, ctx->d_net}, a);
}

template <bool G, int D, int MM, int DYN>
void launch_variant(sl_ctx* ctx, const RewardArgs& a) {
    constexpr int NT = PerThread<G, D, DYN>::value;
    const int blocks = sl_grid_blocks((a.hi - a.lo + NT - 1) / NT);
    *a.h_workgroups = blocks;
    hipLaunchKernelGGL((k_reward_rollout<G, D, MM, DYN>), dim3(blocks), dim3(SL_BLOCK), 0, ctx->stream, ctx->h_model,
                       SlAux{ctx->d_tri, ctx->d_net}, a);
}

// one launch of a.steps steps under the model the context holds right now: k_rollout for
// RolloutArgs, k_reward_rollout for RewardArgs, the same instantiation of either
template <class Args>
int launch_any(sl_ctx* ctx, const Args& a) {
    const SlDevModel& M = ctx->h_model;
    const int d = M.m.grid.d, m = M.m.policy.m, dyn = M.m.dynamics.kind;
    const bool general = M.m.policy.kind == SL_POLICY_TRI;
    if (general) {
        if (d == 2 && m == 1) launch_variant<true, 2, 1, 0>(ctx, a);
        else launch_variant<true, 0, 0, 0>(ctx, a);
    } else if (dyn == SL_DYN_PENDULUM) {              // (sl_model_set: d = 2, m = 1)
        launch_variant<false, 2, 1, SL_DYN_PENDULUM>(ctx, a);
    } else if (dyn == SL_DYN_CARTPOLE) {              // (d = 4, m = 1)
        launch_variant<false, 4, 1, SL_DYN_CARTPOLE>(ctx, a);
    } else if (dyn == SL_DYN_LINEAR && m == 1 && d >= 1 && d <= 4) {
        sl_with_dim<1, 2, 3, 4>(d, [&](auto dt) {
            launch_variant<false, dt, 1, SL_DYN_LINEAR>(ctx, a);
            return SL_OK;
        });
    } else if (dyn == SL_DYN_POLYNOMIAL && m == 1 && d >= 1 && d <= 4) {
        sl_with_dim<1, 2, 3, 4>(d, [&](auto dt) {
            launch_variant<false, dt, 1, SL_DYN_POLYNOMIAL>(ctx, a);
            return SL_OK;
        });
    } else {
        launch_variant<false, 0, 0, 0>(ctx, a);
    }
    SL_HIP_CHECK(ctx, hipGetLastError());
    return SL_OK;
}
int launch(sl_ctx* ctx, const RolloutArgs& a) { return launch_any(ctx, a); }
int launch(sl_ctx* ctx, const RewardArgs& a) { return launch_any(ctx, a); }

}  // namespace

extern "C" int sl_rollout(sl_ctx* ctx, int64_t lo, int64_t hi, const double* d_start, int steps,
                          int steps_per_launch, double* d_state, double* d_traj, double* d_actions) {
    if (!ctx) return sl_fail(nullptr, SL_ERR_INVALID, "sl_rollout: NULL context");
    if (!ctx->model_set) return sl_fail(ctx, SL_ERR_INVALID, "sl_rollout: call sl_model_set first");
    const int d = ctx->h_model.m.grid.d, m = ctx->h_model.m.policy.m;
    const int policy = ctx->h_model.m.policy.kind;
    if (lo < 0 || hi < lo || steps < 0 || steps_per_launch < 0 || !d_state)
        return sl_fail(ctx, SL_ERR_INVALID, "sl_rollout: bad range, negative step count or NULL state buffer");
    if (!d_start && hi > ctx->h_model.gf.nindex)
        return sl_fail(ctx, SL_ERR_INVALID, "sl_rollout: trajectories [%lld, %lld) past the grid's %lld cells",
                       (long long)lo, (long long)hi, (long long)ctx->h_model.gf.nindex);
    if (ctx->h_model.m.dynamics.kind == SL_DYN_GP)
        return sl_fail(ctx, SL_ERR_UNSUPPORTED, "sl_rollout: GP dynamics are not simulated inside the kernel "
                                                "(step the posterior mean through sl_eval_points)");
    if (policy == SL_POLICY_TRI && !ctx->h_tri[1].set)
        return sl_fail(ctx, SL_ERR_INVALID, "sl_rollout: policy table (sl_tri_set slot 1) not set");
    if (policy == SL_POLICY_TABLE && steps > 1)
        return sl_fail(ctx, SL_ERR_INVALID, "sl_rollout: a per-vertex policy table is defined at the vertices "
                                            "only (one step); use the interpolated table (SL_POLICY_TRI)");
    if (hi == lo) return SL_OK;
    SL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const int64_t n = hi - lo;
    ctx->last_kernel[0] = 0;
    if (policy == SL_POLICY_NETWORK) {
        // the network's actions of a step become a per-trajectory table (k_policy_network), then one
        // single-step launch reads it: the states pass through d_state between the two
        if (d_start != d_state) {
            const int rc = launch(ctx, {lo, hi, d_start, 0, d_state, nullptr, nullptr});
            if (rc) return rc;
        }
        for (int s = 0; s < steps; ++s) {
            SlPolicyTableScope network_policy(ctx, lo, hi, d_state - lo * d);   // (indexed by trajectory number)
            if (network_policy.rc) return network_policy.rc;
            const int rc = launch(ctx, {lo, hi, d_state, 1, d_state, d_traj ? d_traj + (int64_t)s * n * d : nullptr,
                                        d_actions ? d_actions + (int64_t)s * n * m : nullptr});
            if (rc) return rc;
        }
        sl_note_kernel(ctx, false, "k_policy_network + k_rollout, %d single steps", steps);
        return SL_OK;
    }
    const int chunk = steps_per_launch > 0 ? steps_per_launch : sl_rollout_chunk(n, steps);
    const double* src = d_start;
    int done = 0, launches = 0;
    do {
        const int c = steps - done < chunk ? steps - done : chunk;
        const int rc = launch(ctx, {lo, hi, src, c, d_state, d_traj ? d_traj + (int64_t)done * n * d : nullptr,
                                    d_actions ? d_actions + (int64_t)done * n * m : nullptr});
        if (rc) return rc;
        src = d_state;
        done += c;
        ++launches;
    } while (done < steps);
    sl_note_kernel(ctx, false, "k_rollout<general=%d, d=%d, dynamics=%d>, %d steps in %d launches",
                   (int)(policy == SL_POLICY_TRI), d, ctx->h_model.m.dynamics.kind, steps, launches);
    return SL_OK;
}

extern "C" int sl_rollout_mask(sl_ctx* ctx, int64_t n, int d, const double* d_state,
                               const double* h_equilibrium, double tol, uint64_t* d_bits, int64_t* d_count) {
    if (!ctx) return sl_fail(nullptr, SL_ERR_INVALID, "sl_rollout_mask: NULL context");
    if (n < 0 || d < 1 || d > SL_MAX_STATE_DIM || (n > 0 && (!d_state || !d_bits)))
        return sl_fail(ctx, SL_ERR_INVALID, "sl_rollout_mask: bad argument (n >= 0, 1 <= d <= %d, buffers)",
                       SL_MAX_STATE_DIM);
    SL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (d_count) SL_HIP_CHECK(ctx, hipMemsetAsync(d_count, 0, sizeof(int64_t), ctx->stream));
    if (n == 0) return SL_OK;
    Equilibrium eq;
    for (int k = 0; k < SL_D; ++k) eq.e[k] = (h_equilibrium && k < d) ? h_equilibrium[k] : 0.0;
    hipLaunchKernelGGL(k_rollout_mask, dim3(sl_grid_blocks(n)), dim3(SL_BLOCK), 0, ctx->stream, n, d, d_state, eq,
                       tol, d_bits, reinterpret_cast<unsigned long long*>(d_count));
    SL_HIP_CHECK(ctx, hipGetLastError());
    return SL_OK;
}

namespace {

// The launches of one sl_reward_rollout call: a kernel launch, the fold of its slab and the one
// host read of the folded maxima.
struct RewardRun {
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
        const int rc = launch(ctx, RewardArgs{lo, hi, start, sum_in, c, weights + done, state, sum, slab, &workgroups});
        if (rc) return rc;
        ++launches;
        if (!h_max) return SL_OK;
        hipLaunchKernelGGL(k_reward_fold, dim3(c), dim3(SL_BLOCK), 0, ctx->stream, slab, workgroups, folded);
        SL_HIP_CHECK(ctx, hipGetLastError());
        static_assert(sizeof(double) == sizeof(unsigned long long), "the maxima travel as bit patterns");
        SL_HIP_CHECK(ctx, hipMemcpyAsync(h_max, folded, sizeof(double) * c, hipMemcpyDeviceToHost, ctx->stream));
        SL_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        return SL_OK;
    }
};

}  // namespace

extern "C" int sl_reward_rollout(sl_ctx* ctx, int64_t lo, int64_t hi, const double* d_start, int horizon,
                                 const double* d_weights, double tol, int steps_per_launch, double* d_sum,
                                 double* d_state, int64_t* h_steps, int* h_converged) {
    if (!ctx) return sl_fail(nullptr, SL_ERR_INVALID, "sl_reward_rollout: NULL context");
    if (!ctx->model_set) return sl_fail(ctx, SL_ERR_INVALID, "sl_reward_rollout: call sl_model_set first");
    const int d = ctx->h_model.m.grid.d;
    const int policy = ctx->h_model.m.policy.kind;
    if (lo < 0 || hi < lo || horizon < 1 || steps_per_launch < 0 || !d_weights || !d_sum || !d_state)
        return sl_fail(ctx, SL_ERR_INVALID, "sl_reward_rollout: bad range, horizon < 1, negative steps per launch "
                                            "or NULL weights, sum or state buffer");
    if (!d_start && hi > ctx->h_model.gf.nindex)
        return sl_fail(ctx, SL_ERR_INVALID, "sl_reward_rollout: trajectories [%lld, %lld) past the grid's %lld cells",
                       (long long)lo, (long long)hi, (long long)ctx->h_model.gf.nindex);
    if (ctx->h_model.m.dynamics.kind == SL_DYN_GP)
        return sl_fail(ctx, SL_ERR_UNSUPPORTED, "sl_reward_rollout: GP dynamics are not simulated inside the kernel "
                                                "(step the posterior mean through sl_eval_points)");
    if (ctx->h_model.m.reward.kind != SL_V_QUADRATIC)
        return sl_fail(ctx, SL_ERR_INVALID, "sl_reward_rollout: the model's reward is not a quadratic function on "
                                            "[x, u] (reward.kind %d)", ctx->h_model.m.reward.kind);
    if (policy == SL_POLICY_TRI && !ctx->h_tri[1].set)
        return sl_fail(ctx, SL_ERR_INVALID, "sl_reward_rollout: policy table (sl_tri_set slot 1) not set");
    if (policy == SL_POLICY_TABLE && horizon > 1)
        return sl_fail(ctx, SL_ERR_INVALID, "sl_reward_rollout: a per-vertex policy table is defined at the vertices "
                                            "only (one step); use the interpolated table (SL_POLICY_TRI)");
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
    RewardRun r{ctx, lo, hi, d_weights, slab, slab + slab_words, 0};
    double h_max[SL_REWARD_CHUNK_MAX];
    int done = 0, converged = 0;
    if (policy == SL_POLICY_NETWORK) {
        // the network's actions of a step become a per-trajectory table (k_policy_network), then one
        // single-step launch in place: a launch of one step never has steps past the stopping step
        if (d_start != d_state) {
            const int rc = launch(ctx, RolloutArgs{lo, hi, d_start, 0, d_state, nullptr, nullptr});
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
        sl_note_kernel(ctx, false, "k_policy_network + k_reward_rollout, %d single steps", done);
    } else {
        int chunk = steps_per_launch > 0 ? steps_per_launch : sl_reward_rollout_chunk(n, horizon);
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
        sl_note_kernel(ctx, false, "k_reward_rollout<general=%d, d=%d, dynamics=%d>, %d steps in %d launches (%d redone)",
                       (int)(policy == SL_POLICY_TRI), d, ctx->h_model.m.dynamics.kind, done, r.launches, redone);
    }
    if (h_steps) *h_steps = done;
    if (h_converged) *h_converged = converged;
    return SL_OK;
}
