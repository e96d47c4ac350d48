// sl_gp4_predecide.hip - k_gp_mean_lattice and k_gp_predecide: the blocks of a segmented block-mode
// GP sweep that a Taylor bound of the posterior mean already decides as failing, found in a
// streaming pass in front of k_gp_mean_blocks (sl_gp4_mean.hip), which then skips them.  The rule
// and its rounding argument: sl_gp4_predecide.h; the constants: sl_gp_mean_bound.h.
//
//  * k_gp_mean_lattice, one lane per lattice point: the scaled input z_c of the reference cell -
//    by the device functions every sweep kernel forms it with - and g(z_c) with its gradient
//    dg/dz (z_c) by a plain loop over the training points (one exponential per pair, fixed order).  Runs in every sweep that uses it:
//    nothing is kept from one sweep to the next.
//  * k_gp_predecide, one lane per cell, one wavefront per 64-cell tile of the shard: state, policy,
//    scaled input, prior, V(x) and threshold by the functions of cell_bounds (sl_gp4_gen.h), then
//    gp4p::sure_fail against the nearest lattice point.  A 16-cell block whose valid cells are all
//    sure to fail writes its 16 mask bits (zeros) with the 2-byte store, folds the key of its cells
//    outside the initial set and sets its bit in the tile's byte.
//  * k_gp_open_count and k_gp_open_scatter, directly behind it: the blocks the pass left open as an
//    ascending list of block numbers (sl_gp4_open.h), which k_gp_mean_open (sl_gp4_mean.hip) works
//    through instead of walking every tile.  One workgroup per chunk of 4096 tiles counts the chunk's
//    open blocks; in the second kernel it adds up the counts of the chunks before its own and writes
//    its entries behind them.  No workgroup waits for another; both kernels do not depend on the
//    state dimension and are compiled once.
// Compiled once per state dimension like sl_gp4_mean.hip.
#include "sl_common.h"
#include "sl_gp4_predecide.h"

template <int DT, int MT>
__global__ __launch_bounds__(256) void k_gp_mean_lattice(const SlDevModel M, const SlGpDev gp, SlAux aux,
                                                         const gp4p::PreConst pc, long long npoints,
                                                         double* __restrict__ table) {
    const SlDims nd = sl_dims<DT, MT>(M);
    const int d = nd.d, p = nd.p;
    const SlGpHeadDev& hd = gp.head[0];
    const long long at = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (at >= npoints) return;
    // lattice index -> the reference cell's flat grid index (last axis fastest, as the grid's)
    long long r = at;
    int64_t cell = 0, stride = 1;
#pragma unroll
    for (int k = SL_D - 1; k >= 0; --k) {
        if (k < d) {
            const int a = (int)(r % pc.count[k]);
            r /= pc.count[k];
            cell += stride * gp4p::lattice_grid_index(a, M.m.grid.num_points[k], pc.spacing);
            stride *= M.m.grid.num_points[k];
        }
    }
    double xg[SL_P], u[SL_M], g[SL_D], J[SL_D][SL_P];
    sl_cell_state(M, d, cell, nullptr, xg);
    sl_policy_any<false>(M, nd, aux.tri, cell, xg, u);
    sl_append_action(nd, u, xg);
#pragma unroll
    for (int q = 0; q < SL_P; ++q) xg[q] = (q < p) ? xg[q] * hd.inv_ls[q] : 0.0;
#pragma unroll
    for (int j = 0; j < SL_D; ++j) {
        g[j] = 0.0;
#pragma unroll
        for (int q = 0; q < SL_P; ++q) J[j][q] = 0.0;
    }
    const int n = hd.n, n_pad = hd.n_pad, dout = hd.dout;
    for (int i = 0; i < n; ++i) {
        double r2 = 0.0, dz[SL_P];
#pragma unroll
        for (int q = 0; q < SL_P; ++q) {
            dz[q] = 0.0;
            if (q < p) {
                dz[q] = hd.xs[q * n_pad + i] - xg[q];
                r2 = fma(dz[q], dz[q], r2);
            }
        }
        const double kx = hd.variance * sl_exp_nonpos(-0.5 * r2);
#pragma unroll
        for (int j = 0; j < SL_D; ++j) {
            if (j < dout) {
                const double ak = kx * hd.alpha[i * dout + j];
                g[j] = g[j] + ak;
#pragma unroll
                for (int q = 0; q < SL_P; ++q)
                    if (q < p) J[j][q] = fma(ak, dz[q], J[j][q]);        // d/dz k(z, z_i) = k (z_i - z)
            }
        }
    }
    double* row = table + at * gp4p::row_doubles(d, p);      // z_c [p], g(z_c) [d], J [d][p]
#pragma unroll
    for (int q = 0; q < SL_P; ++q) if (q < p) row[q] = xg[q];
#pragma unroll
    for (int j = 0; j < SL_D; ++j) {
        if (j < d) {
            row[p + j] = g[j];
#pragma unroll
            for (int q = 0; q < SL_P; ++q) if (q < p) row[p + d + j * p + q] = J[j][q];
        }
    }
}

template <int DT, int MT>
__global__ __launch_bounds__(256) void k_gp_predecide(
    const SlDevModel M, const SlGpDev gp, SlAux aux, const gp4p::PreConst pc, int64_t lo, int64_t hi,
    const uint64_t* __restrict__ init_bits, const double* __restrict__ values, uint64_t* __restrict__ neg_bits,
    sl_key* __restrict__ partials, const double* __restrict__ table, unsigned char* __restrict__ tiles,
    unsigned long long* __restrict__ decided) {
    const SlDims nd = sl_dims<DT, MT>(M);
    const int d = nd.d, p = nd.p;
    const SlGpHeadDev& hd = gp.head[0];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t ntiles = (hi - lo + 63) / 64;
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    uint64_t best_v = ~0ull;
    int64_t best_i = INT64_MAX;
    unsigned count = 0u;
    for (int64_t t = (int64_t)blockIdx.x * 4 + wave; t < ntiles; t += nwaves) {
        const int64_t idx = lo + 64 * t + lane;
        const bool valid = idx < hi;
        const int64_t gidx = valid ? idx : hi - 1;
        double x[SL_P], u[SL_M], prior[SL_D], z[SL_P], lv_x[SL_D];
        sl_cell_state(M, d, gidx, nullptr, x);
        sl_policy_any<false>(M, nd, aux.tri, gidx, x, u);
        sl_append_action(nd, u, x);
        sl_rows_dot<SL_D, SL_P>(M.m.dynamics.matrix, d, p, x, prior);
#pragma unroll
        for (int q = 0; q < SL_P; ++q) z[q] = (q < p) ? x[q] * hd.inv_ls[q] : 0.0;
        const double v_x = sl_value_and_lv<SL_FAST>(M, d, aux, x, lv_x);
        const double thr = sl_threshold(M, d, lv_x, M.m.lipschitz.tau, x);
        // nearest lattice point
        int64_t ijk[SL_D];
        sl_unravel(M.m.grid, M.gf, d, gidx, ijk);
        long long at = 0;
#pragma unroll
        for (int k = 0; k < SL_D; ++k)
            if (k < d) at = at * pc.count[k] + gp4p::lattice_nearest((int)ijk[k], M.m.grid.num_points[k], pc.spacing);
        const double* row = table + at * gp4p::row_doubles(d, p);
        double z_c[SL_P], g_c[SL_D], J[SL_D * SL_P];
#pragma unroll
        for (int q = 0; q < SL_P; ++q) z_c[q] = (q < p) ? row[q] : 0.0;
#pragma unroll
        for (int j = 0; j < SL_D; ++j) g_c[j] = (j < d) ? row[p + j] : 0.0;
#pragma unroll
        for (int i = 0; i < SL_D * SL_P; ++i) J[i] = (i < d * p) ? row[p + d + i] : 0.0;
        const bool sure = valid && gp4p::sure_fail(M.m.value, d, p, pc, z, z_c, g_c, J, prior, v_x, thr);
        // a block is decided when every valid cell of it is sure to fail
        const uint64_t ok = __ballot(sure || !valid);
        unsigned dec = 0u;
#pragma unroll
        for (int jb = 0; jb < 4; ++jb)
            if (((ok >> (16 * jb)) & 0xffffull) == 0xffffull) dec |= 1u << jb;
        const bool mine = (dec >> (lane >> 4)) & 1u;
        if (mine && (lane & 15) == 0) reinterpret_cast<unsigned short*>(neg_bits)[4 * t + (lane >> 4)] = (unsigned short)0;
        bool init = false;
        if (init_bits && valid) init = (init_bits[t] >> lane) & 1ull;
        if (valid && mine && !init) sl_key_min(best_v, best_i, sl_vbits(values ? values[idx - lo] : v_x), idx);
        if (lane == 0) tiles[t] = (unsigned char)dec;
        // (a block wholly at or beyond hi is marked - the mean kernel has nothing to do there - but not counted)
        const int64_t left = hi - (lo + 64 * t);
        const unsigned live = left >= 64 ? 15u : (1u << (int)((left + 15) >> 4)) - 1u;
        count += (unsigned)__builtin_popcount(dec & live);
    }
    sl_wave_reduce_key<true>(best_v, best_i);
    if (lane == 0) {
        sl_key* out = partials + blockIdx.x * 4 + wave;
        out->vbits = best_v;
        out->index = best_i;
        if (count) atomicAdd(decided, (unsigned long long)count);
    }
}

#if !defined(SL_GP4_DIM) || SL_GP4_DIM == 4
namespace gp4o {
constexpr int LANES = 256;                                   // of a workgroup of the two list kernels
constexpr int ROUNDS = CHUNK_TILES / (4 * LANES);            // words per lane, one a round
static_assert(ROUNDS * 4 * LANES == CHUNK_TILES, "a chunk is a whole number of rounds");

// the open mask of the lane's word of round r of chunk `chunk` (0 behind the shard's last tile); t: its first tile
__device__ __forceinline__ uint32_t lane_mask(const unsigned* __restrict__ words, long long ntiles, long long chunk,
                                              int r, long long& t) {
    t = chunk * CHUNK_TILES + 4 * (long long)(r * LANES + (int)threadIdx.x);
    if (t >= ntiles) return 0u;
    const long long left = ntiles - t;
    return open_mask16(words[t >> 2], left < 4 ? (int)left : 4);
}
// sum of v over the workgroup, on every lane (part: one word per wavefront; two barriers)
__device__ __forceinline__ unsigned group_sum(unsigned v, unsigned* part) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();                                         // (the last readers of part are done)
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    return part[0] + part[1] + part[2] + part[3];
}
}  // namespace gp4o

// counts[c] = open blocks of chunk c of the tile bytes (read as words: sl_gp4_open.h)
__global__ __launch_bounds__(256) void k_gp_open_count(const unsigned* __restrict__ words, long long ntiles,
                                                       unsigned* __restrict__ counts) {
    __shared__ unsigned part[4];
    unsigned c = 0u;
#pragma unroll
    for (int r = 0; r < gp4o::ROUNDS; ++r) {
        long long t;
        c += (unsigned)__popc(gp4o::lane_mask(words, ntiles, blockIdx.x, r, t));
    }
    c = gp4o::group_sum(c, part);
    if (threadIdx.x == 0) counts[blockIdx.x] = c;
}

// The entries of chunk c at position sum(counts[0 .. c)) of the list, ascending; the workgroup of the
// last chunk writes the head.  (At most 4 ntiles entries, what the list is sized for.)
// Every workgroup adds up the counts before its own: chunks^2 / 2 word reads in all - 2 MB from L2 for
// the headline's 1 024 chunks, nothing beside the 4 MB of bytes; at the 2^29-tile limit (131 072 chunks)
// it would be 34 GB, not measured, and a shard of that size wants a prefix kernel of its own in between.
__global__ __launch_bounds__(256) void k_gp_open_scatter(const unsigned* __restrict__ words, long long ntiles,
                                                         const unsigned* __restrict__ counts,
                                                         unsigned* __restrict__ list,
                                                         unsigned long long* __restrict__ head) {
    __shared__ unsigned part[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned before = 0u;
    for (unsigned i = threadIdx.x; i < blockIdx.x; i += gp4o::LANES) before += counts[i];
    unsigned base = gp4o::group_sum(before, part);
    for (int r = 0; r < gp4o::ROUNDS; ++r) {
        long long t;
        uint32_t m = gp4o::lane_mask(words, ntiles, blockIdx.x, r, t);
        const unsigned n = (unsigned)__popc(m);
        unsigned incl = n;                                   // inclusive scan over the wavefront
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned up = __shfl_up(incl, off);
            if (lane >= off) incl += up;
        }
        __syncthreads();
        if (lane == 63) part[wave] = incl;
        __syncthreads();
        unsigned at = base + incl - n;
        for (int w = 0; w < wave; ++w) at += part[w];
        while (m) {
            const int i = __builtin_ctz(m);
            m &= m - 1u;
            list[at++] = (unsigned)(4 * t) + (unsigned)i;
        }
        base += part[0] + part[1] + part[2] + part[3];
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        head[gp4o::HEAD_LENGTH] = base;
        head[gp4o::HEAD_NTILES] = (unsigned long long)ntiles;
        head[gp4o::HEAD_BUILT] = 1ull;
    }
}
#endif

// =============================================================================================
// host side
// =============================================================================================
#if !defined(SL_GP4_DIM) || SL_GP4_DIM == 4
// The pass costs two launches and a lattice kernel that is a chain of n exponentials per lane: 0.15 ms
// on the 24^4 x 300 line (1.32 -> 1.47 ms per step with the pass, profiles/predecide.md), where the
// whole mean kernel takes less than that.  k_gp_mean_blocks costs about 10 ns per block at 1024
// points, so the pass can pay from some 10^5 blocks on: shards of at least PRE_MIN_TILES tiles (2 M
// cells).  Forced segments (sl_gp4_segment_configure: the tests) run it at any size.
constexpr int64_t PRE_MIN_TILES = 1 << 15;

bool sl_gp4_predecide_ok(const sl_ctx* ctx, const SlDevModel& model, const SlSweepArgs& a) {
    if (ctx->gp4_segment_tiles <= 0 && (a.hi - a.lo + 63) / 64 < PRE_MIN_TILES) return false;
    if (!ctx->gp4_predecide || ctx->gp4_pre_spacing < 1 || a.points || a.dbg || ctx->h_gp.nheads != 1) return false;
    const SlGpHeadHost& hh = ctx->gp_heads[0];
    if (!hh.set || !hh.mb_ok || hh.d_kernel || hh.col0 != 0 || hh.dout != model.m.grid.d) return false;
    if (model.m.value.kind != SL_V_QUADRATIC || model.m.value.negate) return false;
    // A closed-form policy only: the lattice pass evaluates the policy at cells of the WHOLE grid, and a
    // per-cell table (SL_POLICY_TABLE, also what a network policy is swapped for during a sweep) may
    // hold the cells of the shard [lo, hi) alone.
    if (model.m.policy.kind != SL_POLICY_LINEAR && model.m.policy.kind != SL_POLICY_CONST) return false;
    long long npoints = 1;
    for (int k = 0; k < model.m.grid.d; ++k) {
        if (model.m.grid.num_points[k] < 1) return false;
        npoints *= gp4p::lattice_count((int)model.m.grid.num_points[k], ctx->gp4_pre_spacing);
        if (npoints > gp4p::MAX_LATTICE) return false;
    }
    // (the design rests on a table that stays in the last-level cache)
    const int d = model.m.grid.d;
    if (npoints * gp4p::row_doubles(d, model.in_dim) * (long long)sizeof(double) > gp4p::MAX_TABLE_BYTES) return false;
    return true;
}

extern "C" int sl_gp4_predecide_configure(sl_ctx* ctx, int enable, int spacing) {
    if (!ctx) return sl_fail(nullptr, SL_ERR_INVALID, "sl_gp4_predecide_configure: NULL context");
    if (spacing < 0 || spacing > 4096)
        return sl_fail(ctx, SL_ERR_INVALID, "sl_gp4_predecide_configure: spacing %d outside [0,4096]", spacing);
    ctx->gp4_predecide = enable != 0;
    if (spacing > 0) ctx->gp4_pre_spacing = spacing;        // (0: keep)
    return SL_OK;
}
int sl_gp4_open_build(sl_ctx* ctx, const unsigned char* tiles, long long ntiles) {
    const Gp4OpenView v = sl_gp4_open_view(tiles, ntiles);
    const unsigned nchunks = (unsigned)gp4o::chunks(ntiles);
    const unsigned* words = reinterpret_cast<const unsigned*>(tiles);
    hipLaunchKernelGGL(k_gp_open_count, dim3(nchunks), dim3(gp4o::LANES), 0, ctx->stream, words, ntiles, v.counts);
    SL_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_gp_open_scatter, dim3(nchunks), dim3(gp4o::LANES), 0, ctx->stream, words, ntiles, v.counts,
                       v.list, v.head);
    SL_HIP_CHECK(ctx, hipGetLastError());
    return SL_OK;
}

extern "C" int sl_gp4_open_list(sl_ctx* ctx, uint32_t* out, int64_t cap, unsigned long long* count, int* used) {
    if (!ctx) return sl_fail(nullptr, SL_ERR_INVALID, "sl_gp4_open_list: NULL context");
    if (cap < 0 || (cap && !out)) return sl_fail(ctx, SL_ERR_INVALID, "sl_gp4_open_list: bad output (cap %lld)", (long long)cap);
    if (count) *count = 0ull;
    if (used) *used = 0;
    // The last sweep ran the pass and the mean kernel behind it.  gp4_pre_tiles alone does not say so - only
    // the first segment of a segmented sweep resets it, a later sweep on another path leaves it standing -
    // so the sweep's note is asked too: sl_sweep_any clears it for every sweep, and only launch4's
    // segmented path writes "after k_gp_mean_blocks" (those words name the mean pass whichever of its two
    // kernels ran; the tests hold the note to them).  Whoever rewords that note changes this line with it.
    // HEAD_BUILT then says whether THIS allocation holds a list (a shard of 2^29 tiles or more has none).
    if (!ctx->gp4_pre_tiles || !strstr(ctx->last_kernel, "after k_gp_mean_blocks")) return SL_OK;
    SL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    SL_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    unsigned long long head[3] = {0ull, 0ull, 0ull};
    SL_HIP_CHECK(ctx, hipMemcpy(head, ctx->gp4_pre_tiles - gp4o::HEAD_BYTES, sizeof(head), hipMemcpyDeviceToHost));
    if (head[gp4o::HEAD_BUILT] != 1ull) return SL_OK;
    const Gp4OpenView v = sl_gp4_open_view(ctx->gp4_pre_tiles, (long long)head[gp4o::HEAD_NTILES]);
    const unsigned long long n = head[gp4o::HEAD_LENGTH];
    if (count) *count = n;
    if (used) *used = 1;
    const size_t take = n < (unsigned long long)cap ? (size_t)n : (size_t)cap;
    if (take) SL_HIP_CHECK(ctx, hipMemcpy(out, v.list, take * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return SL_OK;
}
#endif

template <int DT, int MT>
static int launch_predecide(sl_ctx* ctx, const SlDevModel& model, const SlSweepArgs& a, const Gp4PreLaunch& m,
                            const unsigned char** tiles_out) {
    const SlGpHeadHost& hh = ctx->gp_heads[0];
    gp4p::PreConst pc = {};
    long long npoints = 1;
    for (int k = 0; k < DT; ++k) {
        pc.norm[k] = hh.mb_norm[k];
        pc.eps[k] = hh.mb_eps[k];
        pc.count[k] = gp4p::lattice_count((int)model.m.grid.num_points[k], ctx->gp4_pre_spacing);
        npoints *= pc.count[k];
    }
    pc.spacing = ctx->gp4_pre_spacing;
    pc.sdev = sqrt(ctx->h_gp.head[0].variance) * (1.0 + 0x1p-50);
    const int64_t ntiles = (a.hi - a.lo + 63) / 64;
    const size_t table_bytes = ((size_t)npoints * gp4p::row_doubles(DT, DT + MT) * sizeof(double) + 255) & ~(size_t)255;
    // behind the table: the open-block list's head, the tile bytes (read as words), the list's chunk
    // counts and the list itself, 16 bytes per tile for every block open (sl_gp4_open_view)
    SL_HIP_CHECK(ctx, sl_grow(ctx, &ctx->d_gp4_pre, &ctx->gp4_pre_bytes, table_bytes + gp4o::total_bytes(ntiles)));
    double* table = reinterpret_cast<double*>(ctx->d_gp4_pre);
    unsigned char* tiles = reinterpret_cast<unsigned char*>(ctx->d_gp4_pre) + table_bytes + gp4o::HEAD_BYTES;
    SL_HIP_CHECK(ctx, hipMemsetAsync(tiles - gp4o::HEAD_BYTES, 0, gp4o::HEAD_BYTES, ctx->stream));   // (no list yet)
    SlAux aux{ctx->d_tri, ctx->d_net};
    hipLaunchKernelGGL((k_gp_mean_lattice<DT, MT>), dim3((unsigned)((npoints + 255) / 256)), dim3(256), 0, ctx->stream,
                       model, ctx->h_gp, aux, pc, npoints, table);
    SL_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL((k_gp_predecide<DT, MT>), dim3((unsigned)m.workgroups), dim3(256), 0, ctx->stream, model,
                       ctx->h_gp, aux, pc, a.lo, a.hi, a.init_bits, a.values, a.neg_bits, m.partials, table, tiles,
                       m.decided);
    SL_HIP_CHECK(ctx, hipGetLastError());
    *tiles_out = tiles;
    // the blocks left open as a list for k_gp_mean_open (32-bit block numbers: larger shards walk the bytes)
    if (sl_gp4_open_fits(ntiles)) return sl_gp4_open_build(ctx, tiles, ntiles);
    return SL_OK;
}

#define SL_GP4_PRE_ENTRY(D_)                                                                                 \
    template <>                                                                                              \
    int sl_gp4_predecide_launch_dim<D_>(sl_ctx* ctx, const SlDevModel& model, const SlSweepArgs& a,          \
                                        const Gp4PreLaunch& m, const unsigned char** tiles) {                \
        return launch_predecide<D_, 1>(ctx, model, a, m, tiles);                                             \
    }
#if !defined(SL_GP4_DIM) || SL_GP4_DIM == 1
SL_GP4_PRE_ENTRY(1)
#endif
#if !defined(SL_GP4_DIM) || SL_GP4_DIM == 2
SL_GP4_PRE_ENTRY(2)
#endif
#if !defined(SL_GP4_DIM) || SL_GP4_DIM == 3
SL_GP4_PRE_ENTRY(3)
#endif
#if !defined(SL_GP4_DIM) || SL_GP4_DIM == 4
SL_GP4_PRE_ENTRY(4)
#endif
