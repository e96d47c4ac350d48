// sl_policy_rows.h - rows of the policy-evaluation operator, shared by the kernels
// (sl_policy_solve.hip) and the host tests.
//
// Evaluating a fixed policy pi exactly means solving V = r + gamma P V, where row i of P holds the
// barycentric weights of the value triangulation at the successor f(x_i, pi(x_i)) - the matrix
// the reference builds with Triangulation.parameter_derivative for its LP
// (reinforcement_learning.py:142-178, functions.py:1160-1259).  One row per grid vertex in ELL
// form, K = D + 1 entries, stored column by column ([K][n]) so that consecutive lanes read
// consecutive words:
//   cols[k * n + i]   vertex index of corner k of the simplex that holds the successor (int32)
//   w[k * n + i]      its weight; w[0] = 1 - (w[1] + ... + w[D]) by the ordered sum of
//                     sl_tri_locate_fast / sl_tri_reloc
//   r[i]              reward r(x_i, pi(x_i))
// The weights come from sl_tri_locate_fast, the point location of every Bellman sweep, so the row
// combine below reproduces the sweep's r + gamma V(f(x, pi(x))) bit for bit.  A value function
// V = -T (sl_value_desc.negate) stores -w: negating every product of the ordered sum negates the
// result exactly, so gamma * (sum(-w T)) == gamma * (sum(w T) * -1), the sweep's order.
//
// Plain C++ on scalars on top of sl_model.h, like that header: g++ compiles it for the tests.
#pragma once

#include "sl_model.h"

#define SL_ROW_MAX_K 16          // widest ELL row sl_value_solve takes

// Row of the successor `next` (already the dynamics' mean) in the value triangulation t.
// cols / w: K = D + 1 entries; *negative: a barycentric weight below zero (extrapolation:
// outside the grid without projection, or on the upper faces); *abs_sum: sum |w|.
template <int D>
SL_HD void sl_policy_row(const SlTri& t, const double* next, bool negate, int32_t* cols, double* w,
                         bool* negative, double* abs_sum) {
    SlTriLoc<D> loc;
    sl_tri_locate_fast<D>(t, next, loc);
    bool neg = false;
    double s = 0.0;
#pragma unroll
    for (int j = 0; j <= D; ++j) {
        cols[j] = (int32_t)(loc.row[j] / t.ncols);
        neg = neg || loc.w[j] < 0.0;
        s += fabs(loc.w[j]);
        w[j] = negate ? -loc.w[j] : loc.w[j];
    }
    *negative = neg;
    *abs_sum = s;
}

// sum_k w_k V[cols_k] in the order of sl_tri_combine: corners 1 .. K-1 fused in turn, the origin
// (corner 0) last.  vals[k] = V[cols[k]].
// KMAX: compile-time bound of k (the loop unrolls, the entries stay in registers).
template <int KMAX>
SL_HD double sl_policy_row_dot(int k, const double* w, const double* vals) {
    double acc = 0.0;
#pragma unroll
    for (int j = 1; j < KMAX; ++j)
        if (j < k) acc = fma(w[j], vals[j], acc);
    return fma(w[0], vals[0], acc);
}

// r + gamma * (P V)_i: the sweep's `q = r + gamma * v` (two roundings, never fused).
SL_HD double sl_policy_row_combine(double r, double gamma, double pv) {
    const double t = gamma * pv;
    return r + t;
}

// grids the int32 column indices can address
SL_HD bool sl_policy_rows_fit(int64_t nindex) { return nindex >= 0 && nindex <= 2147483647ll; }
