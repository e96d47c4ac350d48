// sl_gp4_mean.hip - k_gp_mean_blocks, k_gp_mean_open: the posterior mean and the first decision of every 16-cell
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
//    draws its stage-0 composite tiles from that list (sl_gp4_queue.h);
//  * a block that k_gp_predecide (sl_gp4_predecide.hip: a bound of the mean, in front of the first
//    segment) has already decided as failing is skipped before any input is formed: one bit of the
//    tile's byte, tested per block with a scalar load (keeping the byte across the four blocks cost
//    the d = 4 kernel five scratch operations).
//
// k_gp_mean_open is the same pass for the sweeps in which k_gp_predecide ran: behind it the open
// blocks are compacted into an ascending list of block numbers (sl_gp4_open.h; k_gp_open_count,
// k_gp_open_scatter in sl_gp4_predecide.hip), and a wavefront draws four consecutive list entries
// per ticket - every one a block of work - instead of a tile whose blocks may all be decided.  The
// segment [tile0, tile1) of the launcher then stands for the list positions [4 tile0, 4 tile1).
// k_gp_mean_blocks stays for the sweeps without the pass (table or network policies, small shards,
// appended heads) and for shards of 2^29 tiles or more, with its listing (profiles/open_list.md).
// The block body exists in both kernels, statement for statement except for three things that keep
// k_gp_mean_open free of scratch in all four dimensions (k_gp_mean_blocks<4, 1> has 60 B): the
// lane's constants are formed again per block, the failing key lives in the wavefront's LDS slice,
// and the first run's constants are row 0 of `runc`, not scalar registers.  Edit both copies together.
//
// The arithmetic of a block is that of sl_gp4.hip because it is the same source, sl_gp4_gen.h: seed
// of a run, 16-cell recurrence, direct path, alpha' and k_x fragment loads, the MFMA group of the
// mean, the final sum, the two-bound decision of a cell.  tests/test_gpu_gp4_mean_kernel.py holds
// the result against SL_GP4_EARLY=0 bit for bit.
//
// Six pieces are still written here AND in sl_gp4.hip, statement for statement, because as header
// functions they changed a kernel that the contract keeps fixed (gfx950 listings, before -> after;
// profiles/shared_block_source.md has the commands).  Edit both copies together:
//  * scaled inputs of a block: k_gp_sweep4<4, 1, false> scratch 224 -> 236 B, 94 -> 113 scratch ops,
//    another kernel descriptor at d = 2, 3, 4;
//  * run detection (`runs`, `wide`): k_gp_sweep4<4, 1, false> scratch 224 -> 268 B, 94 -> 123 scratch
//    ops (d = 2: 176 -> 200 B), another descriptor in every dimension;
//  * constants of the first run (x0, run0): k_gp_sweep4<.., false> reordered in 212 - 932 lines far
//    from the piece, at d = 1 lane-spill ops in the MFMA streams 24 -> 28 (another audit line);
//  * rows of `runc`: k_gp_sweep4<1, 1, true> scratch 156 -> 164 B, 66 -> 75 scratch ops;
//  * the recurrence of a block with kinks (the loop over c0 .. c1): k_gp_sweep4<1, 1, true> scratch
//    156 -> 164 B, 66 -> 69 scratch ops, in every argument form tried;
//  * mask store and key fold of a decided block: k_gp_mean_blocks<4, 1> has 25 scratch ops in the
//    parent; with cell_bounds alone in the header 21, with the mask store alone 25, with both 26.
#include "sl_common.h"
#include "sl_gp4_gen.h"
#include "sl_gp4_mean.h"
#include "sl_gp4_predecide.h"
#include "sl_gp4_queue.h"

#ifndef SL_NO_GP4

namespace gp4m {

using gp4::RUNC;
using gp4::RUNS;
using gp4::uniform;

constexpr int W = 4;                       // wavefronts per workgroup, each on its own
constexpr int WG_PER_CU = 4;
// k_x chunk of one wavefront: [slab pair 8][k 4][slot 16][slab of the pair 2] - cell block `wave` of
// the panel kernel's layout, the slab pairs 4 doubles apart modulo the banks as there
constexpr int KXS2 = 128 + 4;
constexpr int KXBUF = 8 * KXS2;
constexpr int SLICE = KXBUF + 16 * SL_P + RUNS * RUNC;   // doubles of LDS per wavefront
static_assert(16 * SL_D <= KXBUF, "the block's means reuse the chunk buffer");
static_assert(W * SLICE * sizeof(double) <= 40 * 1024, "four workgroups of k_gp_mean_blocks per CU");
// k_gp_mean_open keeps its failing key in LDS as well: one per cell lane (the 16 lanes that decide cells)
constexpr int KEYS = 2 * 16;
constexpr int SLICE_OPEN = SLICE + KEYS;
static_assert(W * SLICE_OPEN * sizeof(double) <= 40 * 1024, "four workgroups of k_gp_mean_open per CU");

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
    unsigned list_cap, const unsigned char* __restrict__ pre_tiles) {
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
        // blocks k_gp_predecide has decided (mask bits and key written there): one byte per tile
        for (int jb = 0; jb < 4; ++jb) {
            if (pre_tiles && ((reinterpret_cast<const unsigned*>(pre_tiles)[tile >> 2] >> (8 * (int)(tile & 3) + jb)) & 1u)) continue;
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
            double x0[SL_P], run0[RUNC], a2 = 0.0;      // run0: step, a^2, Q like a row of runc
#pragma unroll
            for (int q = 0; q < SL_P; ++q) {
                if (q < p) {
                    x0[q] = uniform(cin[q]);
                    run0[q] = uniform(cin[SL_P + q] - x0[q]);
                    a2 = fma(run0[q], run0[q], a2);
                }
            }
            run0[SL_P] = uniform(a2);
            run0[SL_P + 1] = uniform(sl_exp_nonpos(-run0[SL_P]));
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
                if (runs == 1u) {                  // one affine run
                    double e, rho;
                    gp4::run_seed(xv, x0, run0, variance, p, e, rho);
                    gp4::store_run16(kxw, wswz, rho, e, run0[SL_P + 1]);   // (rho BEFORE e: see there)
                } else if (!direct) {              // a few runs: the recurrence restarts at each
                    unsigned m = runs;
                    for (int r = 0; m; ++r) {
                        const int c0 = __builtin_ctz(m);
                        m &= m - 1;
                        const int c1 = m ? __builtin_ctz(m) : 16;
                        const double* rc = runc + r * RUNC;
                        double e, rho;
                        gp4::run_seed(xv, cin + c0 * SL_P, rc, variance, p, e, rho);
                        const double qr = rc[SL_P + 1];
                        for (int c = c0; c < c1; ++c) {
                            kxw[2 * ((c + wswz) & 15)] = e;
                            e *= rho;
                            rho *= qr;
                        }
                    }
                } else {
                    gp4::direct_run(kxw, wswz, xv, cin, 0, variance, p);
                }
            };
            for (int ch = 0; ch < nchunks_head; ++ch) {
                const bool with_mean = !(skip & 2);
                gp4::MeanIn mi;
                // alpha' is requested together with the inputs of the generation (one trip to L2)
                if (with_mean) gp4::load_alpha(mi, rs_alpha, lk, low, dout, ch);
                if (!(skip & 1)) generate(ch);
                if (with_mean) {
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    sl_d2 kx[8];
                    gp4::load_own_kx<KXS2>(kx, kx_l + own);
                    gp4::mean_mfma(kx, mi, macc);
                }
            }
            // the means of the block where the chunk was (its last reads have fed their MFMAs)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (lk < dout) cell_mean[(4 * blk + low) * SL_D + hd.col0 + lk] = gp4::mean_sum(macc);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();

            // the first decision (decide_block(0) of k_gp_sweep4: no panel yet, the whole prior
            // variance): a block whose valid cells all agree is finished
            const int64_t idx = blk0 + lcol;
            const bool valid = lk == 0 && idx < hi;
            gp4::CellBounds b{false, false, 0.0};
            // (No variance floor here: c_0, the constant of the whole factor, is 5e-7 on the headline
            // model, and reading it cost this kernel registers and scratch - profiles/variance_floor.md.)
            if (valid)
                b = gp4::cell_bounds<false>(M, nd, aux, gp.beta, idx, lo, points, values, cell_mean + lcol * SL_D, variance,
                                            0.0, 0.0);
            const bool neg_hi = b.neg_hi, open = b.open;
            const double v_x = b.v_x;
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

// The same for the blocks k_gp_predecide left open, from their list (sl_gp4_open.h, built by
// k_gp_open_count / k_gp_open_scatter behind the pass): positions [p0, p1) of it, clipped to the
// list's length *open_len.  One ticket hands out FOUR consecutive positions (p0 is a multiple of
// four, the list lies on a 16-byte boundary: one 16-byte scalar load; the draw behind the list's end
// is partly filled), and every block of a draw is work: no byte test, no padding tile, no tile
// arithmetic.  The ticket of the next draw is requested before the work of this one and read behind
// it.  `ticket` counts from 0 (the low word of the launcher's counter).  The keys are folded into
// the slots the pass has written.  The block's arithmetic is k_gp_mean_blocks', statement for
// statement: edit both copies together.
template <int DT, int MT>
__global__ __launch_bounds__(256, 4) void k_gp_mean_open(
    const SlDevModel M, const SlGpDev gp, SlAux aux, int64_t lo, int64_t hi, unsigned p0, unsigned p1,
    const unsigned* __restrict__ open_list, const unsigned long long* __restrict__ open_len,
    const uint64_t* __restrict__ init_bits, const double* __restrict__ values,
    uint64_t* __restrict__ neg_bits, sl_key* __restrict__ partials,
    const double* __restrict__ points, int skip_arg, unsigned* __restrict__ ticket,
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
    __shared__ __attribute__((aligned(16))) double smem[W * SLICE_OPEN];
    const SlDims nd = sl_dims<DT, MT>(M);
    const int d = nd.d, p = nd.p;
    const int tid = threadIdx.x, lane0 = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    double* kx_l = smem + wave * SLICE_OPEN;            // [KXBUF]; afterwards the block's means [16][SL_D]
    double* cell_mean = kx_l;
    double* cin = kx_l + KXBUF;                    // [16][SL_P] scaled GP inputs of the block's cells
    double* runc = cin + 16 * SL_P;                // [RUNS][RUNC]
    // The failing key with the least V, per cell lane, in LDS and not in four registers that live
    // across everything: with them the d = 4 kernel parks three values in scratch.
    uint64_t* keys = reinterpret_cast<uint64_t*>(runc + RUNS * RUNC);      // [16][2]: V bits, cell
    if (lane0 < 16) {
        keys[2 * lane0] = ~0ull;
        keys[2 * lane0 + 1] = (uint64_t)INT64_MAX;
    }

    const SlGpHeadDev& hd = gp.head[0];            // (block mode: one head that fills every column)
    const int n_pad = hd.n_pad, dout = hd.dout;
    const double variance = hd.variance;
    __amdgpu_buffer_rsrc_t rs_xs = __builtin_amdgcn_make_buffer_rsrc((void*)hd.xs, 0, 0x7fffffff, 0x27000);
    __amdgpu_buffer_rsrc_t rs_alpha = __builtin_amdgcn_make_buffer_rsrc((void*)hd.alpha, 0, 0x7fffffff, 0x27000);
    constexpr int RP = 256;                        // rows per panel of k_gp_sweep4
    const int npanels = (hd.n + RP - 1) / RP;
    const int nchunks_head = npanels * (RP / 64);

    {
        const unsigned long long len = open_len[0];
        if (len < (unsigned long long)p1) p1 = (unsigned)len;
    }
    if (p0 >= p1) return;                          // (the keys stay what the pass and the segments before left)
    auto request = [&]() -> unsigned {
        unsigned t = 0u;
        // (atomicInc, not atomicAdd: the compiler rewrites a uniform add for a whole wavefront's lanes
        // and reads the result back into a scalar register on the spot - the wait the prefetch avoids)
        if (lane0 == 0) t = atomicInc(ticket, 0xffffffffu);
        return t;
    };
    unsigned drawn = request();
    for (;;) {
        // (read HERE, behind the work of the draw before: without the barrier the compiler reads the
        // ticket into a scalar register right behind the atomic and waits for it there)
        asm volatile("" : "+v"(drawn));
        const unsigned pos = p0 + 4u * (unsigned)__builtin_amdgcn_readfirstlane((int)drawn);
        if (pos >= p1) break;
        drawn = request();                         // the next draw: on its way during this draw's work
        const sl_u4 entry = *reinterpret_cast<const sl_u4*>(open_list + pos);
        const int nb = p1 - pos < 4u ? (int)(p1 - pos) : 4;
        for (int jb = 0; jb < nb; ++jb) {
            const unsigned b16 = jb == 0 ? entry.x : jb == 1 ? entry.y : jb == 2 ? entry.z : entry.w;
            const int64_t blk0 = lo + 16 * (int64_t)b16;
            // The lane's constants are formed again for every block, from a lane number the compiler
            // cannot see through: kept across the loop they are fifteen registers too many, which it
            // parks in scratch.
            int lane = lane0;
            asm volatile("" : "+v"(lane));
            const int lcol = lane & 15, lk = lane >> 4, blk = (lane >> 2) & 3, low = lane & 3;
            const int own = 2 * (16 * lk + ((lcol + 4 * (lk >> 1)) & 15));  // this lane's own (k, cell) item
            // generation writes (lane = point jj of the chunk): slab pair jj >> 3, slab (jj >> 2) & 1, k = jj & 3
            const int wbase = (lane >> 3) * KXS2 + 32 * (lane & 3) + ((lane >> 2) & 1);
            const int wswz = 4 * ((lane & 3) >> 1);
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
            // (k_gp_mean_blocks keeps the constants of the first run - x0, run0 - in scalar registers; here
            // they are row 0 of `runc` and the block's first input row, the same values by the same
            // statements (gp4::block_runs says why), read from LDS: two dozen scalars fewer to carry
            // through vector lanes across the chunks)
            // the step, |step|^2 and Q of every run once (lane r for run r).  A block that is ONE run takes
            // the recurrence even when its step is wide (`direct`: generate() tests runs == 1 first, here as
            // in k_gp_mean_blocks and the plain kernel), so its row 0 is written in that case too.
            if (!direct || runs == 1u) {
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
                if (runs == 1u) {                  // one affine run
                    double e, rho;
                    gp4::run_seed(xv, cin, runc, variance, p, e, rho);
                    gp4::store_run16(kxw, wswz, rho, e, runc[SL_P + 1]);   // (rho BEFORE e: see there)
                } else if (!direct) {              // a few runs: the recurrence restarts at each
                    unsigned m = runs;
                    for (int r = 0; m; ++r) {
                        const int c0 = __builtin_ctz(m);
                        m &= m - 1;
                        const int c1 = m ? __builtin_ctz(m) : 16;
                        const double* rc = runc + r * RUNC;
                        double e, rho;
                        gp4::run_seed(xv, cin + c0 * SL_P, rc, variance, p, e, rho);
                        const double qr = rc[SL_P + 1];
                        for (int c = c0; c < c1; ++c) {
                            kxw[2 * ((c + wswz) & 15)] = e;
                            e *= rho;
                            rho *= qr;
                        }
                    }
                } else {
                    gp4::direct_run(kxw, wswz, xv, cin, 0, variance, p);
                }
            };
            for (int ch = 0; ch < nchunks_head; ++ch) {
                const bool with_mean = !(skip & 2);
                gp4::MeanIn mi;
                // alpha' is requested together with the inputs of the generation (one trip to L2)
                if (with_mean) gp4::load_alpha(mi, rs_alpha, lk, low, dout, ch);
                if (!(skip & 1)) generate(ch);
                if (with_mean) {
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    sl_d2 kx[8];
                    gp4::load_own_kx<KXS2>(kx, kx_l + own);
                    gp4::mean_mfma(kx, mi, macc);
                }
            }
            // the means of the block where the chunk was (its last reads have fed their MFMAs)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (lk < dout) cell_mean[(4 * blk + low) * SL_D + hd.col0 + lk] = gp4::mean_sum(macc);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();

            // the first decision (decide_block(0) of k_gp_sweep4: no panel yet, the whole prior
            // variance): a block whose valid cells all agree is finished
            const int64_t idx = blk0 + lcol;
            const bool valid = lk == 0 && idx < hi;
            gp4::CellBounds b{false, false, 0.0};
            // (No variance floor here: c_0, the constant of the whole factor, is 5e-7 on the headline
            // model, and reading it cost this kernel registers and scratch - profiles/variance_floor.md.)
            if (valid)
                b = gp4::cell_bounds<false>(M, nd, aux, gp.beta, idx, lo, points, values, cell_mean + lcol * SL_D, variance,
                                            0.0, 0.0);
            const bool neg_hi = b.neg_hi, open = b.open;
            const double v_x = b.v_x;
            if (__ballot(open) == 0ull) {
                const unsigned word = (unsigned)(__ballot(neg_hi) & 0xffffull);
                unsigned init = 0u;
                if (init_bits) init = reinterpret_cast<const unsigned short*>(init_bits)[b16];
                if (lane == 0) reinterpret_cast<unsigned short*>(neg_bits)[b16] = (unsigned short)word;
                const bool okc = neg_hi || ((init >> lcol) & 1u);
                if (valid && !okc) {                // (valid: lk == 0, lane = lcol)
                    uint64_t best_v = keys[2 * lcol];
                    int64_t best_i = (int64_t)keys[2 * lcol + 1];
                    sl_key_min(best_v, best_i, sl_vbits(v_x), idx);
                    keys[2 * lcol] = best_v;
                    keys[2 * lcol + 1] = (uint64_t)best_i;
                }
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
    uint64_t best_v = ~0ull;
    int64_t best_i = INT64_MAX;
    if (lane0 < 16) {
        best_v = keys[2 * lane0];
        best_i = (int64_t)keys[2 * lane0 + 1];
    }
    sl_wave_reduce_key<true>(best_v, best_i);
    if (lane0 == 0) {
        sl_key* out = partials + blockIdx.x * W + wave;
        sl_key_min(best_v, best_i, out->vbits, out->index);
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
    // The first segment of a sweep: the lattice pass and k_gp_predecide over the whole shard, in
    // front of everything else.  Its keys go to this kernel's slots (one per wavefront of as many
    // workgroups), which every segment then folds; its count to word [6] of the scratch's head.
    if (!m.fold) {
        ctx->gp4_pre_tiles = nullptr;
        ctx->gp4_pre_count = nullptr;
        if (sl_gp4_predecide_ok(ctx, model, a)) {
            const Gp4PreLaunch pl{m.workgroups, m.partials, m.ticket + 5};
            const int rc = sl_gp4_predecide_launch_dim<DT>(ctx, model, a, pl, &ctx->gp4_pre_tiles);
            if (rc) return rc;
            ctx->gp4_pre_count = m.ticket + 5;
        }
    }
    const int fold = m.fold || ctx->gp4_pre_tiles != nullptr;
    // With the pass's list of open blocks the segment [tile0, tile1) stands for the list positions
    // [4 tile0, 4 tile1): the segments partition [0, 4 ntiles), the list is no longer than that, and a
    // segment of nt tiles hands out at most 4 nt blocks - what its stage-0 list is sized for.  The
    // work of a sweep then fills the first segments; a later one finds its range empty and ends at once.
    const long long ntiles = (long long)((a.hi - a.lo + 63) / 64);
    if (ctx->gp4_pre_tiles && sl_gp4_open_fits(ntiles)) {
        const Gp4OpenView ov = sl_gp4_open_view(ctx->gp4_pre_tiles, ntiles);
        hipLaunchKernelGGL((k_gp_mean_open<DT, MT>), dim3((unsigned)m.workgroups), dim3(gp4m::W * 64), 0, ctx->stream,
                           model, ctx->h_gp, aux, a.lo, a.hi, (unsigned)(4 * m.tile0), (unsigned)(4 * m.tile1),
                           (const unsigned*)ov.list, (const unsigned long long*)(ov.head + gp4o::HEAD_LENGTH),
                           a.init_bits, a.values, a.neg_bits, m.partials, a.points, skip,
                           reinterpret_cast<unsigned*>(m.ticket), m.list_count, m.list_cell, m.list_mean, m.list_cap);
        SL_HIP_CHECK(ctx, hipGetLastError());
        return SL_OK;
    }
    hipLaunchKernelGGL((k_gp_mean_blocks<DT, MT>), dim3((unsigned)m.workgroups), dim3(gp4m::W * 64), 0, ctx->stream,
                       model, ctx->h_gp, aux, a.lo, a.hi, (int64_t)m.tile0, (int64_t)m.tile1, a.init_bits, a.values,
                       a.neg_bits, m.partials, fold, a.points, skip, m.ticket, m.list_count, m.list_cell,
                       m.list_mean, m.list_cap, ctx->gp4_pre_tiles);
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
