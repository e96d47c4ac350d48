// sl_gp4_mean.hip - k_gp_mean_blocks: the posterior mean and the first decision of every 16-cell
// block of a block-mode GP sweep (k_gp_sweep4<.., EARLY = true>, sl_gp4.hip), in a kernel shaped
// for that work.
//
// Inside k_gp_sweep4 the source pass - GP inputs of the cells, run detection, 16 x (k_x chunk,
// 4 x 16 x 64 mean product), decide_block - is a chain in which every step waits for the one before
// it (L2 trip, exponentials, LDS write, LDS read, MFMA, retire), run by wavefronts that hold the 128
// accumulators of the panels and therefore sit two to a SIMD.  Here a wavefront owns nothing but
// its block:
//  * ONE wavefront per 16-cell block and no workgroup barrier: a wavefront draws a tile of four
//    blocks from a counter and works through them on an LDS slice of its own (one k_x chunk of
//    64 points x 16 cells, the cells' scaled inputs, the constants of the runs);
//  * no accumulator registers: at most 128 vector registers and 39 KB of LDS per workgroup of four
//    wavefronts, so FOUR workgroups share a CU - four wavefronts per SIMD cover each other's
//    waits.  (The chunk buffer alone is 8.25 KB per wavefront: five workgroups do not fit.)
//  * a block the bounds decide writes its 16 mask bits and folds its failing key, as in the panel
//    kernel; a block they leave open appends a stage-0 record - first cell and 16 x d means - to
//    the segment's list, position from a device counter (order free).  The panel kernel then
//    draws its stage-0 composite tiles from that list (sl_gp4_queue.h).
//
// The arithmetic of a cell is that of sl_gp4.hip statement for statement - exponential
// (sl_gp4_gen.h), recurrence, run split, direct path, the MFMA statements of the mean, the
// rotation of its four accumulators, the final (macc0 + macc1) + (macc2 + macc3), the two
// sl_cell_check calls: tests/test_gpu_gp4_mean_kernel.py holds the result against SL_GP4_EARLY=0
// bit for bit.  The statements are COPIES: the plain path's lambdas stay where they are (the
// register allocation of k_gp_sweep4<.., false> follows the shape of its source).
#include "sl_common.h"
#include "sl_gp4_gen.h"
#include "sl_gp4_mean.h"
#include "sl_gp4_queue.h"

#ifndef SL_NO_GP4

namespace gp4m {

using gp4::exp_pair;
using gp4::uniform;

constexpr int W = 4;                       // wavefronts per workgroup, each on its own
constexpr int WG_PER_CU = 4;
constexpr int RUNS = 4;                    // affine runs per block handled by the recurrence
constexpr int RUNC = SL_P + 2;             // per run: step[SL_P], a^2, Q
// k_x chunk of one wavefront: [slab pair 8][k 4][slot 16][slab of the pair 2] - cell block `wave` of
// the panel kernel's layout, the slab pairs 4 doubles apart modulo the banks as there
constexpr int KXS2 = 128 + 4;
constexpr int KXBUF = 8 * KXS2;
constexpr int SLICE = KXBUF + 16 * SL_P + RUNS * RUNC;   // doubles of LDS per wavefront
static_assert(16 * SL_D <= KXBUF, "the block's means reuse the chunk buffer");
static_assert(W * SLICE * sizeof(double) <= 40 * 1024, "four workgroups of k_gp_mean_blocks per CU");

}  // namespace gp4m

#ifdef SL_DIAG
// development builds: 16-cell blocks decided before panel 0 (sl_gp4_mean_decided_fetch: the d = 4 unit's)
static __device__ unsigned long long sl_gp4_mean_decided;
#endif

// Tiles [tile0, tile1) of the shard [lo, hi): `ticket` counts from 0 (zeroed by the launcher).
template <int DT, int MT>
__global__ __launch_bounds__(256, 4) void k_gp_mean_blocks(
    const SlDevModel M, const SlGpDev gp, SlAux aux, int64_t lo, int64_t hi, int64_t tile0, int64_t tile1,
    const uint64_t* __restrict__ init_bits, const double* __restrict__ values,
    uint64_t* __restrict__ neg_bits, sl_key* __restrict__ partials, int fold,
    const double* __restrict__ points, int skip_arg, unsigned long long* __restrict__ ticket,
    unsigned* __restrict__ list_count, long long* __restrict__ list_cell, double* __restrict__ list_mean,
    unsigned list_cap) {
    // skip (SL_GP4_SKIP; development builds only): 1 no k_x generation, 2 no mean product
#ifdef SL_DIAG
    const int skip = skip_arg;
#else
    constexpr int skip = 0;
    (void)skip_arg;
#endif
    using namespace gp4m;
    __shared__ __attribute__((aligned(16))) double smem[W * SLICE];
    const SlDims nd = sl_dims<DT, MT>(M);
    const int d = nd.d, p = nd.p;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lcol = lane & 15, lk = lane >> 4, blk = (lane >> 2) & 3, low = lane & 3;
    double* kx_l = smem + wave * SLICE;            // [KXBUF]; afterwards the block's means [16][SL_D]
    double* cell_mean = kx_l;
    double* cin = kx_l + KXBUF;                    // [16][SL_P] scaled GP inputs of the block's cells
    double* runc = cin + 16 * SL_P;                // [RUNS][RUNC]
    const int own = 2 * (16 * lk + ((lcol + 4 * (lk >> 1)) & 15));  // this lane's own (k, cell) item
    // generation writes (lane = point jj of the chunk): slab pair jj >> 3, slab (jj >> 2) & 1, k = jj & 3
    const int wbase = (lane >> 3) * KXS2 + 32 * (lane & 3) + ((lane >> 2) & 1);
    const int wswz = 4 * ((lane & 3) >> 1);
    uint64_t best_v = ~0ull;
    int64_t best_i = INT64_MAX;

    const SlGpHeadDev& hd = gp.head[0];            // (block mode: one head that fills every column)
    const int n_pad = hd.n_pad, dout = hd.dout;
    const double variance = hd.variance;
    __amdgpu_buffer_rsrc_t rs_xs = __builtin_amdgcn_make_buffer_rsrc((void*)hd.xs, 0, 0x7fffffff, 0x27000);
    __amdgpu_buffer_rsrc_t rs_alpha = __builtin_amdgcn_make_buffer_rsrc((void*)hd.alpha, 0, 0x7fffffff, 0x27000);
    constexpr int RP = 256;                        // rows per panel of k_gp_sweep4
    const int npanels = (hd.n + RP - 1) / RP;
    const int nchunks_head = npanels * (RP / 64);

    // the next tile is drawn while the current one is worked on
    auto draw = [&]() -> int64_t {
        unsigned long long t = 0ull;
        if (lane == 0) t = atomicAdd(ticket, 1ull);
        const int64_t t64 = ((int64_t)__builtin_amdgcn_readfirstlane((int)(t >> 32)) << 32) |
                            (int64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)t);
        return tile0 + t64;
    };
    int64_t tile_next = draw();
    while (tile_next < tile1) {
        const int64_t tile = tile_next;
        tile_next = draw();
        const int64_t tile_base = lo + tile * 64;
        if (tile_base >= hi) {                     // padding tile: only clears mask bits
            if (lane == 0) neg_bits[(tile_base - lo) >> 6] = 0ull;
            continue;
        }
        for (int jb = 0; jb < 4; ++jb) {
            const int64_t blk0 = tile_base + 16 * jb;
            // scaled GP input [x, policy(x)] / lengthscales of the 16 cells (lane = cell)
            if (lk == 0) {
                double xg[SL_P], u[SL_M];
                int64_t gidx = blk0 + lcol;
                gidx = gidx < hi ? gidx : hi - 1;
                sl_cell_state(M, d, gidx, points, xg);
                sl_policy_any<false>(M, nd, aux.tri, gidx, xg, u);
                sl_append_action(nd, u, xg);
#pragma unroll
                for (int q = 0; q < SL_P; ++q) cin[lcol * SL_P + q] = (q < p) ? xg[q] * hd.inv_ls[q] : 0.0;
            }
            // (LDS serves a wavefront's instructions in order: the slice is the wavefront's own, a
            // wavefront fence is all that is needed between its writes and its reads)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // maximal affine runs of the 16 cells: bit c of `runs` = cell c starts a run (sl_gp4.hip)
            unsigned runs = 1u;
            bool wide = false;
            {
                bool bend = false;
                if (lcol >= 1) {                    // |step|^2 of the scaled input between neighbours
                    double st2 = 0.0;
#pragma unroll
                    for (int q = 0; q < SL_P; ++q) {
                        if (q < p) {
                            const double st = cin[lcol * SL_P + q] - cin[(lcol - 1) * SL_P + q];
                            st2 = fma(st, st, st2);
                        }
                    }
                    wide = !(st2 <= 1.0);           // also NaN
                }
                if (lcol >= 2) {
#pragma unroll
                    for (int q = 0; q < SL_P; ++q) {
                        if (q < p) {
                            const double c0 = cin[lcol * SL_P + q];
                            const double c1 = cin[(lcol - 1) * SL_P + q];
                            const double c2 = cin[(lcol - 2) * SL_P + q];
                            bend = bend || fabs((c0 - c1) - (c1 - c2)) > 2e-14 * fmax(1.0, fabs(c0));
                        }
                    }
                }
                unsigned bends = (unsigned)(__ballot(bend) & 0xffffull);
                // a bend at c starts a run at c; c + 1 is then its second point, not a new start
                while (bends) {
                    const int c = __builtin_ctz(bends);
                    runs |= 1u << c;
                    bends &= ~(3u << c);
                }
            }
            runs = (unsigned)__builtin_amdgcn_readfirstlane((int)runs);
            const bool direct = __builtin_popcount(runs) > 4 || (__ballot(wide) & 0xffffull) != 0ull;
            // constants of the first run (the only one for most blocks) in scalar registers
            double x0[SL_P], dlt[SL_P], a2 = 0.0;
#pragma unroll
            for (int q = 0; q < SL_P; ++q) {
                if (q < p) {
                    x0[q] = uniform(cin[q]);
                    dlt[q] = uniform(cin[SL_P + q] - x0[q]);
                    a2 = fma(dlt[q], dlt[q], a2);
                }
            }
            a2 = uniform(a2);
            const double qstep = uniform(sl_exp_nonpos(-a2));
            // a block with a kink: the step, |step|^2 and Q of every run once (lane r for run r)
            if (runs != 1u && !direct) {
                if (lane < RUNS) {
                    unsigned m = runs;
                    for (int r = 0; r < lane; ++r) m &= m - 1;
                    if (m) {
                        const int c0 = __builtin_ctz(m);
                        m &= m - 1;
                        const int c1 = m ? __builtin_ctz(m) : 16;
                        const double* at = cin + c0 * SL_P;
                        const bool single = c1 - c0 < 2;
                        double a2r = 0.0;
                        double* rc = runc + lane * RUNC;
#pragma unroll
                        for (int q = 0; q < SL_P; ++q) {
                            const double step = (q < p && !single) ? at[SL_P + q] - at[q] : 0.0;
                            rc[q] = step;
                            a2r = fma(step, step, a2r);
                        }
                        rc[SL_P] = a2r;
                        rc[SL_P + 1] = sl_exp_nonpos(-a2r);
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
            double macc[4] = {0.0, 0.0, 0.0, 0.0};   // posterior-mean accumulators

            // k_x chunk `ch` -> the wavefront's buffer (lane = training point 64 ch + lane)
            auto generate = [&](int ch) {
                double* kxw = kx_l + wbase;
                double xv[SL_P];
#pragma unroll
                for (int q = 0; q < SL_P; ++q)
                    if (q < p)
                        xv[q] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(
                            rs_xs, lane * 8, (q * n_pad + 64 * ch) * 8, 0));
                if (runs == 1u) {                  // one affine run: e_{c+1} = e_c rho_c, rho_{c+1} = rho_c Q
                    double e, rho;
                    double z = 0.0, bj = 0.0;
#pragma unroll
                    for (int q = 0; q < SL_P; ++q) {
                        if (q < p) {
                            const double dq = xv[q] - x0[q];
                            z = fma(dq, dq, z);
                            bj = fma(dq, dlt[q], bj);
                        }
                    }
                    exp_pair(-0.5 * z, fmin(bj - 0.5 * a2, 700.0), e, rho);
                    e = variance * e;
                    // slot (c + wswz) & 15 with wswz 0 or 4: two bases, immediate offsets
                    double* w_lo = kxw + 2 * wswz;               // cells 0..11
                    double* w_hi = w_lo - 8 * wswz;              // cells 12..15 wrap for wswz = 4
#pragma unroll
                    for (int c = 0; c < 16; ++c) {
                        (c < 12 ? w_lo : w_hi)[2 * c] = e;
                        e *= rho;
                        rho *= qstep;
                    }
                } else if (!direct) {              // a few runs: the recurrence restarts at each
                    unsigned m = runs;
                    for (int r = 0; m; ++r) {
                        const int c0 = __builtin_ctz(m);
                        m &= m - 1;
                        const int c1 = m ? __builtin_ctz(m) : 16;
                        const double* at = cin + c0 * SL_P;
                        const double* rc = runc + r * RUNC;
                        double e, rho;
                        double z = 0.0, bj = 0.0;
#pragma unroll
                        for (int q = 0; q < SL_P; ++q) {
                            if (q < p) {
                                const double dq = xv[q] - at[q];
                                z = fma(dq, dq, z);
                                bj = fma(dq, rc[q], bj);
                            }
                        }
                        exp_pair(-0.5 * z, fmin(bj - 0.5 * rc[SL_P], 700.0), e, rho);
                        e = variance * e;
                        const double qr = rc[SL_P + 1];
                        for (int c = c0; c < c1; ++c) {
                            kxw[2 * ((c + wswz) & 15)] = e;
                            e *= rho;
                            rho *= qr;
                        }
                    }
                } else {
                    for (int c = 0; c < 16; ++c) {
                        double z = 0.0;
#pragma unroll
                        for (int q = 0; q < SL_P; ++q) {
                            if (q < p) {
                                const double dq = xv[q] - cin[c * SL_P + q];
                                z = fma(dq, dq, z);
                            }
                        }
                        kxw[2 * ((c + wswz) & 15)] = variance * sl_exp_nonpos(-0.5 * z);
                    }
                }
            };
            // mean[dd][cell] += sum_j alpha'[j][dd] k_x[j][cell] over the chunk's 64 points: A =
            // alpha'^T (row dd = lane & 3), B = the k_x values the wavefront has just written.
            // Lane (k, blk, low) ends up with the mean of output dd = k at cell 4 blk + low.
            struct MeanIn { double a0[8], a1[8]; };
            auto mean_run = [&](const MeanIn& mi) {
                const double* kxr = kx_l + own;
                sl_d2 kx[8];
#pragma unroll
                for (int s2 = 0; s2 < 8; ++s2) kx[s2] = *reinterpret_cast<const sl_d2*>(kxr + s2 * KXS2);
                // A dependent FP64 MFMA must not issue right behind its producer (no interlock):
                // four accumulators in rotation keep three MFMAs between a write and its reuse.
#pragma unroll
                for (int h = 0; h < 2; ++h)
                    asm volatile("s_nop 3\n\t"
                                 "v_mfma_f64_4x4x4_4b_f64 %0, %4, %5, %0\n\t"
                                 "v_mfma_f64_4x4x4_4b_f64 %1, %6, %7, %1\n\t"
                                 "v_mfma_f64_4x4x4_4b_f64 %2, %8, %9, %2\n\t"
                                 "v_mfma_f64_4x4x4_4b_f64 %3, %10, %11, %3\n\t"
                                 "v_mfma_f64_4x4x4_4b_f64 %0, %12, %13, %0\n\t"
                                 "v_mfma_f64_4x4x4_4b_f64 %1, %14, %15, %1\n\t"
                                 "v_mfma_f64_4x4x4_4b_f64 %2, %16, %17, %2\n\t"
                                 "v_mfma_f64_4x4x4_4b_f64 %3, %18, %19, %3"
                                 : "+v"(macc[0]), "+v"(macc[1]), "+v"(macc[2]), "+v"(macc[3])
                                 : "v"(mi.a0[4 * h]), "v"(kx[4 * h].x), "v"(mi.a1[4 * h]), "v"(kx[4 * h].y),
                                   "v"(mi.a0[4 * h + 1]), "v"(kx[4 * h + 1].x), "v"(mi.a1[4 * h + 1]), "v"(kx[4 * h + 1].y),
                                   "v"(mi.a0[4 * h + 2]), "v"(kx[4 * h + 2].x), "v"(mi.a1[4 * h + 2]), "v"(kx[4 * h + 2].y),
                                   "v"(mi.a0[4 * h + 3]), "v"(kx[4 * h + 3].x), "v"(mi.a1[4 * h + 3]), "v"(kx[4 * h + 3].y));
                // retired before any other reader (a register copy, the final sum)
                asm volatile("s_nop 15\n\ts_nop 7" : "+v"(macc[0]), "+v"(macc[1]), "+v"(macc[2]), "+v"(macc[3]));
            };
            for (int ch = 0; ch < nchunks_head; ++ch) {
                const bool with_mean = !(skip & 2);
                MeanIn mi;
                if (with_mean) {
                    // alpha' is requested together with the inputs of the generation (one trip to L2)
                    const int voff = (lk * dout + (low < dout ? low : 0)) * 8;
#pragma unroll
                    for (int s2 = 0; s2 < 8; ++s2) {
                        mi.a0[s2] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(
                            rs_alpha, voff, (64 * ch + 8 * s2) * dout * 8, 0));
                        mi.a1[s2] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(
                            rs_alpha, voff, (64 * ch + 8 * s2 + 4) * dout * 8, 0));
                    }
                }
                if (!(skip & 1)) generate(ch);
                if (with_mean) {
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    mean_run(mi);
                }
            }
            // the means of the block where the chunk was (its last reads have fed their MFMAs)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (lk < dout) cell_mean[(4 * blk + low) * SL_D + hd.col0 + lk] = (macc[0] + macc[1]) + (macc[2] + macc[3]);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();

            // decide_block(0) of sl_gp4.hip: err = 0 bounds the decrease from below, err = beta
            // sqrt(variance) from above; a block whose valid cells all agree is finished
            const int64_t idx = blk0 + lcol;
            const bool valid = lk == 0 && idx < hi;
            bool neg_hi = false, open = false;
            double v_x = 0.0;
            if (valid) {
                double x[SL_P], u[SL_M], prior[SL_D], mean[SL_D], err0[SL_D], err1[SL_D];
                sl_cell_state(M, d, idx, points, x);
                sl_policy_any<false>(M, nd, aux.tri, idx, x, u);
                sl_append_action(nd, u, x);
                sl_rows_dot<SL_D, SL_P>(M.m.dynamics.matrix, d, p, x, prior);
                const double var = variance;
                const double e = gp.beta * sqrt(var);
#pragma unroll
                for (int k = 0; k < SL_D; ++k) {
                    if (k < d) {
                        mean[k] = cell_mean[lcol * SL_D + k] + prior[k];
                        err0[k] = 0.0;
                        err1[k] = e;
                    }
                }
                const SlCellCheck c0 = sl_cell_check<SL_FAST>(M, d, aux, x, mean, err0);
                const SlCellCheck c1 = sl_cell_check<SL_FAST>(M, d, aux, x, mean, err1);
                neg_hi = c1.negative;
                // (a non-finite mean or err_hi leaves the cell, and so the block, undecided)
                open = c0.negative != c1.negative || !(fabs(c0.decrease) < INFINITY) ||
                       !(fabs(c1.decrease) < INFINITY);
                v_x = values ? values[idx - lo] : c1.v_x;
            }
            if (__ballot(open) == 0ull) {
                const unsigned word = (unsigned)(__ballot(neg_hi) & 0xffffull);
                const int64_t b16 = (blk0 - lo) >> 4;
                unsigned init = 0u;
                if (init_bits) init = reinterpret_cast<const unsigned short*>(init_bits)[b16];
                if (lane == 0) reinterpret_cast<unsigned short*>(neg_bits)[b16] = (unsigned short)word;
                const bool okc = neg_hi || ((init >> lcol) & 1u);
                if (valid && !okc) sl_key_min(best_v, best_i, sl_vbits(v_x), idx);
#ifdef SL_DIAG
                if (lane == 0) atomicAdd(&sl_gp4_mean_decided, 1ull);
#endif
            } else {
                // open: a stage-0 record - first cell, 16 x d means - at the next list position
                unsigned at = 0u;
                if (lane == 0) at = atomicAdd(list_count, 1u);
                at = (unsigned)__builtin_amdgcn_readfirstlane((int)at);
                if (at < list_cap) {               // (the launcher sizes the list for every block open)
                    if (lane == 0) list_cell[at] = blk0;
                    double* rec = list_mean + (size_t)at * 16 * d;
                    for (int i = lane; i < 16 * d; i += 64) rec[i] = cell_mean[(i / d) * SL_D + i % d];
                }
            }
            // (the slice is rewritten only by this wavefront, after these reads in program order)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
    // one key per wavefront
    sl_wave_reduce_key<true>(best_v, best_i);
    if (lane == 0) {
        sl_key* out = partials + blockIdx.x * W + wave;
        if (fold) sl_key_min(best_v, best_i, out->vbits, out->index);
        out->vbits = best_v;
        out->index = best_i;
    }
}

// =============================================================================================
// host side
// =============================================================================================
template <int DT, int MT>
static int launch_mean(sl_ctx* ctx, const SlDevModel& model, const SlSweepArgs& a, const Gp4MeanLaunch& m) {
    SlAux aux{ctx->d_tri, ctx->d_net};
    const int skip = sl_diag_flags("SL_GP4_SKIP");            // (development builds only: 0 otherwise)
    hipLaunchKernelGGL((k_gp_mean_blocks<DT, MT>), dim3((unsigned)m.workgroups), dim3(gp4m::W * 64), 0, ctx->stream,
                       model, ctx->h_gp, aux, a.lo, a.hi, (int64_t)m.tile0, (int64_t)m.tile1, a.init_bits, a.values,
                       a.neg_bits, m.partials, m.fold, a.points, skip, m.ticket, m.list_count, m.list_cell,
                       m.list_mean, m.list_cap);
    SL_HIP_CHECK(ctx, hipGetLastError());
    return SL_OK;
}

#if !defined(SL_GP4_DIM) || SL_GP4_DIM == 4
int sl_gp4_mean_workgroups(const sl_ctx* ctx, long long tiles) {
    // a wavefront works on a tile at a time: no more workgroups than quarter as many as tiles
    long long wg = (long long)ctx->num_cu * gp4m::WG_PER_CU;
    const long long need = (tiles + gp4m::W - 1) / gp4m::W;
    if (wg > need) wg = need;
    if (wg > SL_MAX_GRID / 2) wg = SL_MAX_GRID / 2;           // (4 keys per workgroup in d_partials)
    return (int)(wg < 1 ? 1 : wg);
}

unsigned long long sl_gp4_mean_decided_fetch(sl_ctx* ctx) {
    unsigned long long c = 0ull;
#ifdef SL_DIAG
    if (hipMemcpyFromSymbol(&c, HIP_SYMBOL(sl_gp4_mean_decided), sizeof(c)) != hipSuccess) return 0ull;
    const unsigned long long zero = 0ull;
    (void)hipMemcpyToSymbol(HIP_SYMBOL(sl_gp4_mean_decided), &zero, sizeof(zero));
#endif
    (void)ctx;
    return c;
}
#endif

// One entry per state dimension; the build compiles this file once per dimension like sl_gp4.hip.
#define SL_GP4_MEAN_ENTRY(D_)                                                                                \
    template <>                                                                                              \
    int sl_gp4_mean_launch_dim<D_>(sl_ctx* ctx, const SlDevModel& model, const SlSweepArgs& a,               \
                                   const Gp4MeanLaunch& m) {                                                 \
        return launch_mean<D_, 1>(ctx, model, a, m);                                                         \
    }
#if !defined(SL_GP4_DIM) || SL_GP4_DIM == 1
SL_GP4_MEAN_ENTRY(1)
#endif
#if !defined(SL_GP4_DIM) || SL_GP4_DIM == 2
SL_GP4_MEAN_ENTRY(2)
#endif
#if !defined(SL_GP4_DIM) || SL_GP4_DIM == 3
SL_GP4_MEAN_ENTRY(3)
#endif
#if !defined(SL_GP4_DIM) || SL_GP4_DIM == 4
SL_GP4_MEAN_ENTRY(4)
#endif
#endif  // SL_NO_GP4
