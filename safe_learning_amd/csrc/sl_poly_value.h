// sl_poly_value.h - polynomial Lyapunov / value functions (SL_V_POLYNOMIAL): a candidate described by data.
//
// A table of terms  coef * prod_q z_q^e_q  over the (scaled) state replaces the callable the reference
// accepts as a Lyapunov function (the sixth-order sum-of-squares candidate m(x)^T Q m(x) of
// examples/lyapunov_function_learning.ipynb, cell 17, is such a table once its Gram form is expanded).
// The arithmetic below is the ONE definition: the kernels, the host build of the tests and the NumPy
// restatement (tests/np_polynomial_value.py) perform the same multiplications and additions in the same
// order - no pow, no fused multiply-add (the translation units are compiled with -ffp-contract=off) - so
// their results agree bit for bit.
//
//   z_q = x_q * tx[q]                                          (normalised specs only)
//   value row:       acc = +0.0;  per term, in table order:  prod = coef;
//                    for q ascending, e_q times: prod = prod * z_q;   acc = acc + prod
//                    V = acc, or acc * -1.0 when negated
//   gradient row k:  built on the host from the value terms in their order: every term with e_k >= 1
//                    gives the coefficient coef * (double)e_k (one rounding) and the exponents with
//                    e_k - 1; evaluated like the value row, then g_k = g_k * tx[k] (normalised specs:
//                    the derivative is with respect to the function's argument x), then the sign
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
// Row 0 is the value, row 1 + k the derivative with respect to z_k.  Every index below is
// wavefront-uniform, so the reads are scalar loads and the exponent loops scalar loops around one
// vector multiplication.
struct SlPolyValue {
    int32_t  d, normalize, nterms, nentries;
    double   tx[SL_MAX_STATE_DIM];
    int32_t  row_start[SL_MAX_STATE_DIM + 2];     // entries of row r: [row_start[r], row_start[r + 1])
    double   coef[SL_POLYV_MAX_ENTRIES];
    uint64_t expo[SL_POLYV_MAX_ENTRIES];          // byte q = exponent of z_q
};

// Validates a term list and writes the value row and the d gradient rows.
// Returns SL_OK, or SL_ERR_INVALID with the reason in msg.
inline int sl_polyv_build(SlPolyValue* t, int d, int nterms, const double* coef,
                          const uint8_t* expo /* [nterms][SL_MAX_STATE_DIM] */, int normalize, const double* tx,
                          char* msg, size_t msglen) {
    if (d < 1 || d > SL_MAX_STATE_DIM) {
        snprintf(msg, msglen, "polynomial value function: d = %d outside 1..SL_MAX_STATE_DIM = %d", d,
                 SL_MAX_STATE_DIM);
        return SL_ERR_INVALID;
    }
    if (nterms < 0 || nterms > SL_POLYV_MAX_ENTRIES) {
        snprintf(msg, msglen, "polynomial value function: %d terms (at most SL_POLYV_MAX_ENTRIES = %d table entries)",
                 nterms, SL_POLYV_MAX_ENTRIES);
        return SL_ERR_INVALID;
    }
    if (nterms > 0 && (!coef || !expo)) {
        snprintf(msg, msglen, "polynomial value function: NULL term arrays");
        return SL_ERR_INVALID;
    }
    if (normalize && !tx) {
        snprintf(msg, msglen, "polynomial value function: normalised without the scales");
        return SL_ERR_INVALID;
    }
    int entries = nterms;
    for (int k = 0; k < nterms; ++k) {
        int degree = 0;
        for (int q = 0; q < SL_MAX_STATE_DIM; ++q) {
            const int e = expo[k * SL_MAX_STATE_DIM + q];
            if (q >= d && e != 0) {
                snprintf(msg, msglen, "polynomial value function: term %d has an exponent on input %d of %d", k, q, d);
                return SL_ERR_INVALID;
            }
            degree += e;
            if (e > 0) ++entries;
        }
        if (degree > SL_POLY_MAX_DEGREE) {
            snprintf(msg, msglen, "polynomial value function: term %d has total degree %d (at most SL_POLY_MAX_DEGREE = %d)",
                     k, degree, SL_POLY_MAX_DEGREE);
            return SL_ERR_INVALID;
        }
    }
    if (entries > SL_POLYV_MAX_ENTRIES) {
        snprintf(msg, msglen, "polynomial value function: %d table entries, value row and gradient rows together (at "
                 "most SL_POLYV_MAX_ENTRIES = %d)", entries, SL_POLYV_MAX_ENTRIES);
        return SL_ERR_INVALID;
    }
    *t = SlPolyValue();
    t->d = d; t->normalize = normalize ? 1 : 0; t->nterms = nterms; t->nentries = entries;
    for (int q = 0; q < SL_MAX_STATE_DIM; ++q) t->tx[q] = (normalize && q < d) ? tx[q] : 1.0;
    int at = 0;
    t->row_start[0] = 0;
    for (int k = 0; k < nterms; ++k) {
        uint64_t word = 0;
        for (int q = 0; q < SL_MAX_STATE_DIM; ++q) word |= (uint64_t)expo[k * SL_MAX_STATE_DIM + q] << (8 * q);
        t->coef[at] = coef[k];
        t->expo[at] = word;
        ++at;
    }
    for (int g = 0; g < SL_MAX_STATE_DIM; ++g) {
        t->row_start[1 + g] = at;
        if (g >= d) continue;
        for (int k = 0; k < nterms; ++k) {
            const int e = expo[k * SL_MAX_STATE_DIM + g];
            if (e < 1) continue;
            t->coef[at] = coef[k] * (double)e;
            t->expo[at] = t->expo[k] - ((uint64_t)1 << (8 * g));
            ++at;
        }
    }
    t->row_start[SL_MAX_STATE_DIM + 1] = at;
    return SL_OK;
}

#if defined(__HIP_DEVICE_COMPILE__)
// The table is written by the host between launches only (sl_value_polynomial_set waits for the stream
// first): read through the constant address space its uniform reads are scalar loads even in kernels
// that store to global memory between them.
typedef const __attribute__((address_space(4))) SlPolyValue SlPolyValueView;
#define SL_POLYV_VIEW(table) (*(SlPolyValueView*)&(table))
#else
typedef const SlPolyValue SlPolyValueView;
#define SL_POLYV_VIEW(table) (table)
#endif

// z = x * tx (normalised specs), d entries of an SL_MAX_STATE_DIM array
SL_HD void sl_polyv_scale(SlPolyValueView& T, int d, const double* x, double* z) {
    const int normalize = T.normalize;
#pragma unroll
    for (int q = 0; q < SL_MAX_STATE_DIM; ++q) {
        if (q < d) z[q] = normalize ? x[q] * T.tx[q] : x[q];
    }
}

// one row at the scaled point z.  d is a compile-time value in the kernels compiled for fixed dimensions:
// every `q < d` folds, z stays in registers (no run-time register index: the loop over q is unrolled, the
// loops over terms and exponents have wavefront-uniform trip counts).
SL_HD double sl_polyv_row(SlPolyValueView& T, int row, int d, const double* z) {
    double acc = 0.0;
    const int t1 = T.row_start[row + 1];
    for (int t = T.row_start[row]; t < t1; ++t) {
        double prod = T.coef[t];
        const uint64_t e = T.expo[t];
#pragma unroll
        for (int q = 0; q < SL_MAX_STATE_DIM; ++q) {
            if (q < d) {
                const int eq = (int)((e >> (8 * q)) & 0xffu);
                for (int r = 0; r < eq; ++r) prod = prod * z[q];
            }
        }
        acc = acc + prod;
    }
    return acc;
}

// V(x)
SL_HD double sl_polyv_value(const SlPolyValue& table, int d, int negate, const double* x) {
    SlPolyValueView& T = SL_POLYV_VIEW(table);
    double z[SL_MAX_STATE_DIM];
    sl_polyv_scale(T, d, x, z);
    const double acc = sl_polyv_row(T, 0, d, z);
    return negate ? (acc * -1.0) : acc;
}

// dV/dx(x): d entries
SL_HD void sl_polyv_gradient(const SlPolyValue& table, int d, int negate, const double* x, double* g) {
    SlPolyValueView& T = SL_POLYV_VIEW(table);
    double z[SL_MAX_STATE_DIM];
    sl_polyv_scale(T, d, x, z);
    const int normalize = T.normalize;
#pragma unroll
    for (int k = 0; k < SL_MAX_STATE_DIM; ++k) {
        if (k < d) {
            double v = sl_polyv_row(T, 1 + k, d, z);
            if (normalize) v = v * T.tx[k];
            g[k] = negate ? (v * -1.0) : v;
        }
    }
}
