// sl_gp4_gen.h - the arithmetic of a 16-cell block, once, for the two kernels that form it:
// k_gp_sweep4 (sl_gp4.hip: its generate / mean_run / produce / decide_block lambdas) and
// k_gp_mean_blocks (sl_gp4_mean.hip).  A cell's k_x values, its posterior mean and its first
// decision are the same bits whichever kernel forms them because they are the same statements:
//   RUNS, RUNC               how many runs the recurrence handles, the row of constants of a run
//   exp_pair, uniform        the exponential of the recurrence, a value in scalar registers
//   run_seed                 e_0 and rho_0 of an affine run for one training point
//   store_run16              the recurrence of a one-run block into the chunk, with its slot swizzle
//   direct_run               one exponential per (point, cell)
//   MeanIn, load_alpha       the alpha' fragments of a chunk
//   load_own_kx              the k_x fragments a wavefront has just written
//   mean_mfma, mean_sum      the eight-MFMA mean group with its wait states, the final sum
//   CellBounds, cell_bounds  the two sl_cell_check calls on a cell: lower bound (with the variance
//                            floor of the stage) and upper bound
//   floor_words              where the head's floor constants lie (behind alpha')
// What differs between the kernels is an argument: where the block's inputs, run constants and
// chunk lie in LDS, the stride KXS2 of the chunk's slab pairs, the variance left after the panels.
// Only pieces both kernels use live here (the seed scratch of the plain path does not).  The
// functions are called from INSIDE the kernels' lambdas: k_gp_sweep4<.., false> must keep its kernel
// descriptor and its audit line, and the forms below are the ones under which it does (an index
// into cin instead of a row pointer, rho in front of e, the k_x loads apart from the MFMA group -
// other forms reorder its MFMA streams).  What is still written twice, and why, is listed at the
// top of sl_gp4_mean.hip; profiles/shared_block_source.md has the figures.
#pragma once
#include "sl_common.h"

typedef double sl_d2 __attribute__((ext_vector_type(2)));
typedef unsigned sl_u4 __attribute__((ext_vector_type(4)));

namespace gp4 {

constexpr int RUNS = 4;                    // affine runs per block handled by the recurrence
constexpr int RUNC = SL_P + 2;             // constants of a run: step[SL_P], a^2 = |step|^2, Q = exp(-a^2)

// exp of two arguments (sl_exp_nonpos twice), the two dependent FMA chains written alternately: a
// single wavefront per SIMD has nobody else to fill the latency of a 13-deep chain
__device__ __forceinline__ void exp_pair(double x1, double x2, double& e1, double& e2) {
    x1 = x1 < -800.0 ? -800.0 : x1;
    x2 = x2 < -800.0 ? -800.0 : x2;
    const double k1 = rint(x1 * 1.4426950408889634), k2 = rint(x2 * 1.4426950408889634);
    double r1 = fma(k1, -6.93147180369123816490e-01, x1), r2 = fma(k2, -6.93147180369123816490e-01, x2);
    r1 = fma(k1, -1.90821492927058770002e-10, r1);
    r2 = fma(k2, -1.90821492927058770002e-10, r2);
    double q1 = 1.6059043836821613e-10, q2 = 1.6059043836821613e-10;
#define SL_EXP_STEP(C) q1 = fma(q1, r1, C); q2 = fma(q2, r2, C)
    SL_EXP_STEP(2.08767569878681e-09);
    SL_EXP_STEP(2.505210838544172e-08);
    SL_EXP_STEP(2.755731922398589e-07);
    SL_EXP_STEP(2.7557319223985893e-06);
    SL_EXP_STEP(2.48015873015873e-05);
    SL_EXP_STEP(1.984126984126984e-04);
    SL_EXP_STEP(1.3888888888888889e-03);
    SL_EXP_STEP(8.333333333333333e-03);
    SL_EXP_STEP(4.1666666666666664e-02);
    SL_EXP_STEP(1.6666666666666666e-01);
    SL_EXP_STEP(0.5);
    SL_EXP_STEP(1.0);
    SL_EXP_STEP(1.0);
#undef SL_EXP_STEP
    e1 = ldexp(q1, (int)k1);
    e2 = ldexp(q2, (int)k2);
}

// a wave-uniform double held in scalar registers
__device__ __forceinline__ double uniform(double v) {
    const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
    const int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
    return __hiloint2double(hi, lo);
}

// Seed of an affine run for the training point xv: e_0 = s^2 exp(-|xv - at|^2 / 2) and rho_0 =
// exp((xv - at) . step - |step|^2 / 2), the exponent of rho capped.  `at` is the run's first cell,
// rc the run's constants [step[SL_P], |step|^2, Q] - scalar registers for the first run, a row of
// `runc` in LDS for a later one.
__device__ __forceinline__ void run_seed(const double (&xv)[SL_P], const double* at, const double* rc,
                                         double variance, int p, double& e, double& rho) {
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
}

// The recurrence e_{c+1} = e_c rho_c, rho_{c+1} = rho_c Q for the 16 cells of a block that is one
// run, into the lane's column of the chunk (kxw: its item of cell slot 0).  Cell c sits in slot
// (c + wswz) & 15 with wswz 0 or 4: two bases, immediate offsets.
// MIND THE ORDER: rho comes BEFORE e here, unlike run_seed's outputs, and all three are doubles - a
// swapped call compiles.  (The compiler orders the operands of the products after the arguments;
// with e in front every product of the plain kernel's recurrence comes out commuted, 26 lines for 2.)
// The column window [C0, C1) (a half-record of the block mode: 0 .. 8 or 8 .. 16) selects the cells
// that are STORED; the recurrence itself always starts at cell 0 of the block, so a stored value is
// the bits the whole block's generation gives it.
template <int C0 = 0, int C1 = 16>
__device__ __forceinline__ void store_run16(double* kxw, int wswz, double rho, double e, double q) {
    double* w_lo = kxw + 2 * wswz;               // cells 0..11
    double* w_hi = w_lo - 8 * wswz;              // cells 12..15 wrap for wswz = 4
#pragma unroll
    for (int c = 0; c < C1; ++c) {
        if (c >= C0) (c < 12 ? w_lo : w_hi)[2 * c] = e;
        e *= rho;
        rho *= q;
    }
}
// inputs that are not piecewise affine: one exponential per (point, cell); the block's inputs are
// rows cell0 .. cell0 + 15 of cin[][SL_P]
__device__ __forceinline__ void direct_run(double* kxw, int wswz, const double (&xv)[SL_P], const double* cin,
                                           int cell0, double variance, int p) {
    for (int c = 0; c < 16; ++c) {
        double z = 0.0;
#pragma unroll
        for (int q = 0; q < SL_P; ++q) {
            if (q < p) {
                const double dq = xv[q] - cin[(cell0 + c) * SL_P + q];
                z = fma(dq, dq, z);
            }
        }
        kxw[2 * ((c + wswz) & 15)] = variance * sl_exp_nonpos(-0.5 * z);
    }
}
// the same for the cells [c_lo, c_hi) of a block whose 16 input rows lie at cw, cs doubles a row
// (every cell on its own: a window changes no stored value)
__device__ __forceinline__ void direct_run_window(double* kxw, int wswz, const double (&xv)[SL_P], const double* cw,
                                                  int cs, double variance, int p, int c_lo, int c_hi) {
    for (int c = c_lo; c < c_hi; ++c) {
        double z = 0.0;
#pragma unroll
        for (int q = 0; q < SL_P; ++q) {
            if (q < p) {
                const double dq = xv[q] - cw[c * cs + q];
                z = fma(dq, dq, z);
            }
        }
        kxw[2 * ((c + wswz) & 15)] = variance * sl_exp_nonpos(-0.5 * z);
    }
}
// The recurrence of a block with a few runs, restarted at each (`runs`: bit c = cell c starts a
// run; rcw: the rows of run constants, cw: the block's 16 input rows of cs doubles); the cells
// [c_lo, c_hi) are stored.  The statements of k_gp_sweep4's own loop (sl_gp4.hip, generate).
__device__ __forceinline__ void store_runs_window(double* kxw, int wswz, const double (&xv)[SL_P], const double* cw,
                                                  int cs, const double* rcw, unsigned runs, double variance, int p,
                                                  int c_lo, int c_hi) {
    unsigned m = runs;
    for (int r = 0; m; ++r) {
        const int c0 = __builtin_ctz(m);
        m &= m - 1;
        const int c1 = m ? __builtin_ctz(m) : 16;
        if (c0 >= c_hi) break;
        if (c1 <= c_lo) continue;
        const double* rc = rcw + r * RUNC;
        double e, rho;
        run_seed(xv, cw + c0 * cs, rc, variance, p, e, rho);
        const double qr = rc[SL_P + 1];
        const int cend = c1 < c_hi ? c1 : c_hi;
        for (int c = c0; c < cend; ++c) {
            if (c >= c_lo) kxw[2 * ((c + wswz) & 15)] = e;
            e *= rho;
            rho *= qr;
        }
    }
}

// Run detection and run constants of a block whose 16 input rows lie at cw (cs doubles a row): the
// statements the plain path of k_gp_sweep4 and k_gp_mean_blocks apply to their own block (see there
// for the reasoning), for the records of a block-mode slot.  runs: bit c = cell c starts an affine run; direct: one
// exponential per (point, cell); rcw: [RUNS][RUNC] constants of every run - also of a block that is
// one run: its row 0 holds the values the first record keeps in scalar registers (the same
// subtraction, the same sum of squares with zeros behind p, the same exponential), read back from LDS
// so that nothing of the second record lives in registers across the MFMA streams.
__device__ __forceinline__ void block_runs(const double* cw, int cs, double* rcw, int p, int lane, unsigned& runs,
                                           bool& direct) {
    const int lcol = lane & 15;
    runs = 1u;
    bool wide = false, bend = false;
    if (lcol >= 1) {
        double st2 = 0.0;
#pragma unroll
        for (int q = 0; q < SL_P; ++q) {
            if (q < p) {
                const double st = cw[lcol * cs + q] - cw[(lcol - 1) * cs + q];
                st2 = fma(st, st, st2);
            }
        }
        wide = !(st2 <= 1.0);
    }
    if (lcol >= 2) {
#pragma unroll
        for (int q = 0; q < SL_P; ++q) {
            if (q < p) {
                const double c0 = cw[lcol * cs + q];
                const double c1 = cw[(lcol - 1) * cs + q];
                const double c2 = cw[(lcol - 2) * cs + q];
                bend = bend || fabs((c0 - c1) - (c1 - c2)) > 2e-14 * fmax(1.0, fabs(c0));
            }
        }
    }
    unsigned bends = (unsigned)(__ballot(bend) & 0xffffull);
    while (bends) {
        const int c = __builtin_ctz(bends);
        runs |= 1u << c;
        bends &= ~(3u << c);
    }
    runs = (unsigned)__builtin_amdgcn_readfirstlane((int)runs);
    direct = __builtin_popcount(runs) > 4 || (__ballot(wide) & 0xffffull) != 0ull;
    if (!direct) {
        if (lane < RUNS) {
            unsigned m = runs;
            for (int r = 0; r < lane; ++r) m &= m - 1;
            if (m) {
                const int c0 = __builtin_ctz(m);
                m &= m - 1;
                const int c1 = m ? __builtin_ctz(m) : 16;
                const double* at = cw + c0 * cs;
                const bool single = c1 - c0 < 2;
                double a2r = 0.0;
                double* rc = rcw + lane * RUNC;
#pragma unroll
                for (int q = 0; q < SL_P; ++q) {
                    const double step = (q < p && !single) ? at[cs + q] - at[q] : 0.0;
                    rc[q] = step;
                    a2r = fma(step, step, a2r);
                }
                rc[SL_P] = a2r;
                rc[SL_P + 1] = sl_exp_nonpos(-a2r);
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// alpha' of chunk `ch` from L2 through the head's buffer resource: one lane offset, the row of the
// slab in the scalar operand.  Rows dd >= dout of A hold whatever a valid column holds: row dd of
// the product depends on row dd of A only, and the rows >= dout of the result are never read.
struct MeanIn { double a0[8], a1[8]; };
__device__ __forceinline__ void load_alpha(MeanIn& mi, __amdgpu_buffer_rsrc_t rs_alpha, int lk, int low, int dout,
                                           int ch) {
    const int voff = (lk * dout + (low < dout ? low : 0)) * 8;
#pragma unroll
    for (int s2 = 0; s2 < 8; ++s2) {
        mi.a0[s2] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(
            rs_alpha, voff, (64 * ch + 8 * s2) * dout * 8, 0));
        mi.a1[s2] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(
            rs_alpha, voff, (64 * ch + 8 * s2 + 4) * dout * 8, 0));
    }
}
// this lane's own (k, cell) items of the chunk the wavefront has just written: kxr = its item of slab
// pair 0, the pairs KXS2 doubles apart
template <int KXS2>
__device__ __forceinline__ void load_own_kx(sl_d2 (&kx)[8], const double* kxr) {
#pragma unroll
    for (int s2 = 0; s2 < 8; ++s2) kx[s2] = *reinterpret_cast<const sl_d2*>(kxr + s2 * KXS2);
}
// mean[dd][cell] += sum_j alpha'[j][dd] k_x[j][cell] over the 64 points of a chunk: A = alpha'^T
// (row dd = lane & 3, the same for the four blocks), B = the k_x values the wavefront has just
// written (kx: load_own_kx).
// Lane (k, blk, low) ends up with the mean of output dd = k at cell 4 blk + low.
__device__ __forceinline__ void mean_mfma(const sl_d2 (&kx)[8], const MeanIn& mi, double (&macc)[4]) {
    // Accumulators in vector registers (the builtin would route them through a0:a1).  A dependent
    // FP64 MFMA must not issue right behind its producer (no interlock: measured, the second
    // product was lost): four accumulators in rotation keep three MFMAs between a write and its reuse.
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
}
// the mean of the lane's (output, cell) once every chunk has been added
__device__ __forceinline__ double mean_sum(const double (&macc)[4]) {
    return (macc[0] + macc[1]) + (macc[2] + macc[3]);
}

// the head's variance floor in device memory: [0] = 2 delta, [1 + s] = c_s (SlGpHeadDev::alpha)
__device__ __forceinline__ const double* floor_words(const SlGpHeadDev& hd) {
    return hd.alpha + (size_t)hd.n_pad * hd.dout;
}

// Bounds of the decrease of cell idx with `var` of the prior variance left (the panels so far
// taken off): err = beta sqrt(var) bounds it from above, and from below err = beta sqrt(var_lo)
// with the variance floor var_lo = max(0, floor_c var - floor_2d): the variance of the full sum is
// at least floor_c times the one left after these panels (floor_c = c_s of sl_gp_floor.h for the
// panel boundary, a constant of the model), and floor_2d = 2 delta allows for the rounding of both
// sums (fl(V_n) >= V_n - delta >= c (fl(V_m) - delta) - delta, delta = 64 n 2^-53 s^2).  Multiply,
// subtract, max, sqrt and the product with beta round monotonically like the operations of the
// upper bound, so a bit both bounds agree on is still the bit of the full sum.  floor_c = floor_2d
// = 0 is err = 0 (FLOOR = false: the literal, for a caller without the constants).
// mean_row: the cell's SL_D posterior means without the prior.  open: the bounds disagree, or one
// is not finite (a non-finite mean or err_hi leaves the cell, and so its block, undecided).
struct CellBounds { bool neg_hi, open; double v_x; };
template <bool FLOOR>
__device__ __forceinline__ CellBounds cell_bounds(const SlDevModel& M, const SlDims& nd, const SlAux& aux, double beta,
                                                  int64_t idx, int64_t lo, const double* points, const double* values,
                                                  const double* mean_row, double var, double floor_c, double floor_2d) {
    const int d = nd.d, p = nd.p;
    double x[SL_P], u[SL_M], prior[SL_D], mean[SL_D], err0[SL_D], err1[SL_D];
    sl_cell_state(M, d, idx, points, x);
    sl_policy_any<false>(M, nd, aux.tri, idx, x, u);
    sl_append_action(nd, u, x);
    sl_rows_dot<SL_D, SL_P>(M.m.dynamics.matrix, d, p, x, prior);
    const double e = beta * sqrt(var);
    const double e_lo = FLOOR ? beta * sqrt(fmax(floor_c * var - floor_2d, 0.0)) : 0.0;
#pragma unroll
    for (int k = 0; k < SL_D; ++k) {
        if (k < d) {
            mean[k] = mean_row[k] + prior[k];
            err0[k] = e_lo;
            err1[k] = e;
        }
    }
    const SlCellCheck c0 = sl_cell_check<SL_FAST>(M, d, aux, x, mean, err0);
    const SlCellCheck c1 = sl_cell_check<SL_FAST>(M, d, aux, x, mean, err1);
    CellBounds b;
    b.neg_hi = c1.negative;
    b.open = c0.negative != c1.negative || !(fabs(c0.decrease) < INFINITY) || !(fabs(c1.decrease) < INFINITY);
    b.v_x = values ? values[idx - lo] : c1.v_x;
    return b;
}

}  // namespace gp4
