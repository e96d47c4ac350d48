// sl_gp_likelihood.h - per-element arithmetic of the log marginal likelihood's gradient (sl_gp_likelihood.hip):
// what a host compiler can read, so that the tests can run the arithmetic of k_lml_grad and its tile / slot
// reduction on the host.
//
//   d lml / d theta = 1/2 sum_ij W_ij dK_ij / d theta,   W = B B^T - D K^-1,   B = K^-1 R
//
// theta runs over the numbers of the kernel description itself: variance[q] and inv_lengthscales[q] of every
// factor.  The entries that are not zero get a SLOT each (sl_lml_compile_slots, at most SL_LML_MAX_SLOTS); one
// more accumulator, number nslots, takes the noise variance (dK_ij = delta_ij: 1/2 tr W).  For a factor f of
// product P,  dK_ij / d theta = (the other factors of P at (i, j)) dk_f / d theta  with
//   RBF       k = v e,  e = exp(-s / 2), s = sum_q (D_q a_q)^2:          dk/dv = e,           dk/da_q = -k D_q^2 a_q
//   Matern32  r = sqrt(3) sqrt(s + 1e-12), k = v (1 + r) exp(-r):        dk/dv = (1 + r) e^-r, dk/da_q = -3 v e^-r D_q^2 a_q
//   Linear    k = sum_q v_q x_iq x_jq:                                   dk/dv_q = x_iq x_jq
// (D_q = x_iq - x_jq, a_q = inv_lengthscales[q]).  The factor values are those of sl_kernel_eval, operation for
// operation.  No fused multiply-adds of the compiler's (-ffp-contract=off).
#pragma once

#include <math.h>
#include <stdint.h>

#include "sl_model.h"

#define SL_LML_TILE 64              // a workgroup of k_lml_grad owns one 64 x 64 tile of the lower triangle
#define SL_LML_THREADS 256          // thread t: column t & 63, rows (t >> 6) + 4 e, e = 0 .. 15
#define SL_LML_MAX_SLOTS 32
#define SL_LML_MAX_ACC (SL_LML_MAX_SLOTS + 1)

enum { SL_LML_VARIANCE = 0, SL_LML_LINEAR_VARIANCE = 1, SL_LML_INV_LS = 2 };
struct sl_lml_slot {
    int32_t what, factor, q, reserved;
    double a;                       // SL_LML_INV_LS: inv_lengthscales[q] of the factor
};
struct sl_lml_slots {
    int32_t nslots, reserved;
    sl_lml_slot slot[SL_LML_MAX_SLOTS];
};

// The slots of a description in the order factor by factor, variances before inverse lengthscales, q ascending.
// Returns their number, which may exceed SL_LML_MAX_SLOTS (then `out` holds the first SL_LML_MAX_SLOTS).
inline int sl_lml_compile_slots(const sl_gp_kernel& ks, int p, sl_lml_slots* out) {
    int n = 0;
    auto add = [&](int what, int f, int q, double a) {
        if (n < SL_LML_MAX_SLOTS) out->slot[n] = sl_lml_slot{what, f, q, 0, a};
        ++n;
    };
    for (int f = 0; f < ks.nfactors; ++f) {
        const sl_gp_kernel_factor& fac = ks.factor[f];
        if (fac.kind == SL_KERNEL_LINEAR) {
            for (int q = 0; q < p; ++q)
                if (fac.variance[q] != 0.0) add(SL_LML_LINEAR_VARIANCE, f, q, 0.0);
        } else {
            if (fac.variance[0] != 0.0) add(SL_LML_VARIANCE, f, 0, 0.0);
            for (int q = 0; q < p; ++q)
                if (fac.inv_lengthscales[q] != 0.0) add(SL_LML_INV_LS, f, q, fac.inv_lengthscales[q]);
        }
    }
    out->nslots = n < SL_LML_MAX_SLOTS ? n : SL_LML_MAX_SLOTS;
    out->reserved = 0;
    return n;
}

// tiles of the lower triangle in ascending order: (I, J), J <= I, has number I (I + 1) / 2 + J
SL_HD int sl_lml_tile_index(int I, int J) { return I * (I + 1) / 2 + J; }
SL_HD int sl_lml_tiles(int64_t n) {
    const int nb = (int)((n + SL_LML_TILE - 1) / SL_LML_TILE);
    return nb * (nb + 1) / 2;
}

// what the slots of one entry (i, j) are made of
static_assert(SL_KERNEL_MAX_FACTORS == 8 && SL_P == 8, "the arrays of an entry have eight elements");
struct sl_lml_entry {
    double gv[8];                   // (the other factors of the product) x dk_f/dv       (Linear: the other factors)
    double gl[8];                   // (the other factors of the product) x (-k | -3 v e^-r)   (Linear: 0)
    double d2[8];                   // (x_iq - x_jq)^2
    double xx[8];                   // x_iq x_jq
};

SL_HD void sl_lml_entry_eval(const sl_gp_kernel& ks, int p, const double* a, const double* b, sl_lml_entry& e) {
    double val[8], dv[8], cl[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const double dq = q < p ? a[q] - b[q] : 0.0;
        e.d2[q] = dq * dq;
        e.xx[q] = q < p ? a[q] * b[q] : 0.0;
    }
#pragma unroll
    for (int f = 0; f < 8; ++f) {
        double v = 1.0, d = 0.0, c = 0.0;               // (scalars: the arrays are written once, unconditionally)
        if (f < ks.nfactors) {
            const sl_gp_kernel_factor& fac = ks.factor[f];
            if (fac.kind == SL_KERNEL_LINEAR) {
                v = 0.0;
#pragma unroll
                for (int q = 0; q < SL_P; ++q)
                    if (q < p) v = fma(a[q] * fac.variance[q], b[q], v);
                d = 1.0;
            } else {
                double r2 = 0.0;
#pragma unroll
                for (int q = 0; q < SL_P; ++q) {
                    if (q < p) {
                        const double dq = (a[q] - b[q]) * fac.inv_lengthscales[q];
                        r2 = fma(dq, dq, r2);
                    }
                }
                if (fac.kind == SL_KERNEL_RBF) {
                    d = sl_exp_nonpos(-0.5 * r2);
                    v = fac.variance[0] * d;
                    c = -v;
                } else {
                    const double r = 1.7320508075688772 * sqrt(r2 + 1e-12);
                    const double ex = sl_exp_nonpos(-r);
                    v = fac.variance[0] * (1.0 + r) * ex;
                    d = (1.0 + r) * ex;
                    c = -3.0 * fac.variance[0] * ex;
                }
            }
        }
        val[f] = v;
        dv[f] = d;
        cl[f] = c;
    }
#pragma unroll
    for (int f = 0; f < 8; ++f) {
        double others = 1.0;
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const bool same = g != f && f < ks.nfactors && g < ks.nfactors && ks.factor[g].product == ks.factor[f].product;
            others = same ? others * val[g] : others;
        }
        e.gv[f] = others * dv[f];
        e.gl[f] = others * cl[f];
    }
}

// emit(s, dK_ij / d theta of slot s) for every slot, in the order of sl_lml_compile_slots (the same conditions, so
// the numbers agree); every array index is a constant after unrolling, only the slot counter is a run-time value
template <class Emit>
SL_HD void sl_lml_walk(const sl_gp_kernel& ks, int p, const sl_lml_entry& e, Emit&& emit) {
    int s = 0;
#pragma unroll
    for (int f = 0; f < 8; ++f) {
        if (f < ks.nfactors) {
            const sl_gp_kernel_factor& fac = ks.factor[f];
            if (fac.kind == SL_KERNEL_LINEAR) {
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    if (q < p && fac.variance[q] != 0.0) emit(s++, e.gv[f] * e.xx[q]);
            } else {
                if (fac.variance[0] != 0.0) emit(s++, e.gv[f]);
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    if (q < p && fac.inv_lengthscales[q] != 0.0) emit(s++, e.gl[f] * e.d2[q] * fac.inv_lengthscales[q]);
            }
        }
    }
}

// W_ij from the rows i and j of B [n][dout] (d ascending) and K^-1_ij
SL_HD double sl_lml_w(const double* bi, const double* bj, int dout, double kinv) {
    double s = 0.0;
    for (int d = 0; d < dout; ++d) s = s + bi[d] * bj[d];
    return s - (double)dout * kinv;
}

// 1/2 w W_ij: w = 2 below the diagonal (the entry stands for (j, i) too), 1 on it, 0 above it
SL_HD double sl_lml_weight(int64_t row, int64_t col, double w) {
    return col < row ? w : (col == row ? 0.5 * w : 0.0);
}

// Who does what in the tile (I, J): wavefront `wave` of four visits the rows I 64 + wave + 4 e, e = 0 .. 15, in
// ascending order; its lane l holds column J 64 + l.  For every visited row and every slot s the 64 lanes' values
// coefficient x term are added by a butterfly (v_l + v_(l ^ 32), then ^ 16, ... ^ 1: every lane ends with the same
// sum) and the sum is added to the wavefront's running sum of the slot; accumulator nslots takes the coefficient
// of the diagonal entry.  The workgroup's partial is the four running sums in ascending order, and the tiles are
// added in ascending order.  Host and device share the pieces below, so a host program can do the same.
//
// the row of visit e, or -1 when it lies past the matrix
SL_HD int64_t sl_lml_visit_row(int64_t n, int I, int wave, int e) {
    const int64_t row = (int64_t)I * SL_LML_TILE + wave + 4 * e;
    return row < n ? row : -1;
}

// entry (row, column J 64 + lane): its slot ingredients and its coefficient 1/2 w W (0 for a lane that has no
// entry there; `ent` is finite for it)
SL_HD double sl_lml_lane(const sl_gp_kernel& ks, int64_t n, int p, int dout, const double* X, const double* B,
                         const double* kinv, int64_t row, int J, int lane, sl_lml_entry& ent) {
    const int64_t col = (int64_t)J * SL_LML_TILE + lane;
    const bool valid = col <= row;                       // (row < n, so col < n)
    const int64_t c = valid ? col : row;
    double xi[8], xj[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        xi[q] = q < p ? X[row * p + q] : 0.0;
        xj[q] = q < p ? X[c * p + q] : 0.0;
    }
    sl_lml_entry_eval(ks, p, xi, xj, ent);
    const double w = sl_lml_w(B + row * dout, B + c * dout, dout, kinv[row * n + c]);
    return valid ? sl_lml_weight(row, col, w) : 0.0;
}
