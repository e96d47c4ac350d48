// sl_polynomial.h - polynomial dynamics (SL_DYN_POLYNOMIAL): a vector field described by data.
//
// A table of terms  coef * prod_q z_q^e_q  over z = [x, u], sorted by output row, replaces the
// callable the reference accepts as dynamics (its VanDerPol, examples/utilities.py:440-519, is the
// table {-y} / {x, damping x^2 y, -damping y} with ten Euler sub-steps).  The arithmetic below is the
// ONE definition: the kernels, the host build of the tests and the NumPy restatement
// (tests/np_polynomial.py) perform the same multiplications and additions in the same order - no
// pow, no fused multiply-add (the translation units are compiled with -ffp-contract=off) - so their
// results agree bit for bit, rollouts included.
//
//   z_q = x_q * tx[q], z_{d+a} = u_a * tu[a]                 (normalised models only)
//   `substeps` times, every row from the same z:
//       acc_i = +0.0;  per term of row i, in table order:  prod = coef;
//                      for q ascending, e_q times: prod = prod * z_q;   acc_i = acc_i + prod
//       then z_i = z_i + h * acc_i for every state entry (the action entries stay)
//   substeps == 0: once, z_i = acc_i (the polynomial is the map)
//   x+_i = z_i * tx_inv[i]                                   (normalised models only)
#pragma once

#include <stdint.h>
#include <stdio.h>
#include "sl_hip.h"

#ifndef SL_HD
#if defined(__HIPCC__)
#define SL_HD __host__ __device__ __forceinline__
#else
#define SL_HD inline
#endif
#endif

// The table as the kernels read it: one copy per context in device memory, the same for every lane.
// Every index below is wavefront-uniform, so the reads are scalar loads and the exponent loops
// scalar loops around one vector multiplication.
struct SlPolyTable {
    int32_t  d, m, nterms, substeps;
    double   h;                                   // dt / substeps
    int32_t  row_start[SL_MAX_STATE_DIM + 2];     // terms of row i: [row_start[i], row_start[i + 1])
    double   coef[SL_POLY_MAX_TERMS];
    uint64_t expo[SL_POLY_MAX_TERMS];             // byte q = exponent of z_q
};

// Validates a term list and writes it sorted by row (stable: the caller's order within a row).
// Returns SL_OK, or SL_ERR_INVALID with the reason in msg.
inline int sl_poly_build(SlPolyTable* t, int d, int m, int nterms, const int32_t* rows, const double* coef,
                         const uint8_t* expo /* [nterms][SL_MAX_INPUT_DIM] */, int substeps, double h,
                         char* msg, size_t msglen) {
    if (d < 1 || d > SL_MAX_STATE_DIM || m < 1 || m > SL_MAX_ACTION_DIM || d + m > SL_MAX_INPUT_DIM) {
        snprintf(msg, msglen, "polynomial dynamics: d = %d, m = %d outside 1..%d states, 1..%d actions, %d inputs", d,
                 m, SL_MAX_STATE_DIM, SL_MAX_ACTION_DIM, SL_MAX_INPUT_DIM);
        return SL_ERR_INVALID;
    }
    if (nterms < 0 || nterms > SL_POLY_MAX_TERMS) {
        snprintf(msg, msglen, "polynomial dynamics: %d terms (at most SL_POLY_MAX_TERMS = %d)", nterms,
                 SL_POLY_MAX_TERMS);
        return SL_ERR_INVALID;
    }
    if (nterms > 0 && (!rows || !coef || !expo)) {
        snprintf(msg, msglen, "polynomial dynamics: NULL term arrays");
        return SL_ERR_INVALID;
    }
    if (substeps < 0) {
        snprintf(msg, msglen, "polynomial dynamics: %d sub-steps", substeps);
        return SL_ERR_INVALID;
    }
    for (int k = 0; k < nterms; ++k) {
        if (rows[k] < 0 || rows[k] >= d) {
            snprintf(msg, msglen, "polynomial dynamics: term %d adds to row %d of %d states", k, (int)rows[k], d);
            return SL_ERR_INVALID;
        }
        int degree = 0;
        for (int q = 0; q < SL_MAX_INPUT_DIM; ++q) {
            const int e = expo[k * SL_MAX_INPUT_DIM + q];
            if (q >= d + m && e != 0) {
                snprintf(msg, msglen, "polynomial dynamics: term %d has an exponent on input %d of %d", k, q, d + m);
                return SL_ERR_INVALID;
            }
            degree += e;
        }
        if (degree > SL_POLY_MAX_DEGREE) {
            snprintf(msg, msglen, "polynomial dynamics: term %d has total degree %d (at most SL_POLY_MAX_DEGREE = %d)",
                     k, degree, SL_POLY_MAX_DEGREE);
            return SL_ERR_INVALID;
        }
    }
    *t = SlPolyTable();
    t->d = d; t->m = m; t->nterms = nterms; t->substeps = substeps; t->h = h;
    int at = 0;
    for (int i = 0; i < d; ++i) {
        t->row_start[i] = at;
        for (int k = 0; k < nterms; ++k) {
            if (rows[k] != i) continue;
            t->coef[at] = coef[k];
            uint64_t word = 0;
            for (int q = 0; q < SL_MAX_INPUT_DIM; ++q) word |= (uint64_t)expo[k * SL_MAX_INPUT_DIM + q] << (8 * q);
            t->expo[at] = word;
            ++at;
        }
    }
    for (int i = d; i < SL_MAX_STATE_DIM + 2; ++i) t->row_start[i] = at;
    return SL_OK;
}

// x -> x+ of one (state, action) pair: zin = [x, u] (d + m entries of an SL_MAX_INPUT_DIM array), nxt [d].
// d and m are compile-time values in the kernels compiled for fixed dimensions: every `q < d` folds,
// z stays in registers (no run-time register index anywhere: the loops over q and i are unrolled, the
// loops over terms and exponents have wavefront-uniform trip counts).
SL_HD void sl_polynomial(const sl_dynamics_desc& f, const SlPolyTable& table, int d, int m, const double* zin,
                         double* nxt) {
#if defined(__HIP_DEVICE_COMPILE__)
    // The table is written by the host between launches only (sl_dynamics_polynomial_set waits for the
    // stream first): read through the constant address space its uniform reads are scalar loads even
    // in kernels that store to global memory between them (the rollouts' trajectories).
    typedef const __attribute__((address_space(4))) SlPolyTable ConstTable;
    ConstTable& T = *(ConstTable*)&table;
#else
    const SlPolyTable& T = table;
#endif
    const int p = d + m;
    double z[SL_MAX_INPUT_DIM];
#pragma unroll
    for (int q = 0; q < SL_MAX_INPUT_DIM; ++q) {
        if (q < p) {
            double v = zin[q];
            if (f.normalize) {
                if (q < d) v = v * f.tx[q];
#pragma unroll
                for (int a = 0; a < SL_MAX_ACTION_DIM; ++a)
                    if (a < m && q == d + a) v = v * f.tu[a];
            }
            z[q] = v;
        }
    }
    const int substeps = T.substeps;
    const double h = T.h;
    const int reps = substeps > 0 ? substeps : 1;
    for (int it = 0; it < reps; ++it) {
        double acc[SL_MAX_STATE_DIM];
#pragma unroll
        for (int i = 0; i < SL_MAX_STATE_DIM; ++i) {
            if (i < d) {
                double a = 0.0;
                const int t1 = T.row_start[i + 1];
                for (int t = T.row_start[i]; t < t1; ++t) {
                    double prod = T.coef[t];
                    const uint64_t e = T.expo[t];
#pragma unroll
                    for (int q = 0; q < SL_MAX_INPUT_DIM; ++q) {
                        if (q < p) {
                            const int eq = (int)((e >> (8 * q)) & 0xffu);
                            for (int r = 0; r < eq; ++r) prod = prod * z[q];
                        }
                    }
                    a = a + prod;
                }
                acc[i] = a;
            }
        }
#pragma unroll
        for (int i = 0; i < SL_MAX_STATE_DIM; ++i) {
            if (i < d) {
                if (substeps > 0) {
                    const double step = h * acc[i];
                    z[i] = z[i] + step;
                } else {
                    z[i] = acc[i];
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < SL_MAX_STATE_DIM; ++i) {
        if (i < d) nxt[i] = f.normalize ? z[i] * f.tx_inv[i] : z[i];
    }
}
