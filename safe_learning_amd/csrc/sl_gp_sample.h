// sl_gp_sample.h - block and index arithmetic of the dense FP64 factorization behind sample_gp_function
// (sl_gp_sample.hip): what a host compiler can read, so that the tests can run the same blocked algorithm on
// the host and compare the sequential pieces bit for bit.
//
// A matrix is cut into SL_GS_NB-wide blocks (the last one may be short).  Everything that is sequential by
// nature lives here, in one arithmetic order for the device and for the host:
//   sl_gs_diag_factor   Cholesky of one diagonal block held in LDS (right-looking; each entry sees its
//                       subtractions with ascending k, then one division by the square root of the pivot)
//   sl_gs_panel_row     one row of  X L_kk^T = A  (the panel under a factored diagonal block), by substitution
//   sl_gs_solve_col     one right-hand side of  L_kk x = b  or  L_kk^T x = b
// The products between blocks (trailing update, off-diagonal updates of the solves, L Z, a^T a) run on the
// matrix cores in sl_gp_sample.hip; their sums are taken in ascending k as well, four terms per instruction.
// No fused multiply-adds here (the library is built with -ffp-contract=off): a NumPy loop in the same order
// gives the same bits.
#pragma once

#include <math.h>
#include <stdint.h>

#include "sl_model.h"

#define SL_GS_NB 64                 // block width: a diagonal block is 32 KB of doubles
#define SL_GS_LD (SL_GS_NB + 1)     // leading dimension of a block in LDS (no bank conflicts down a column)
#define SL_GS_MAX_N 16384           // points of a discretization            (SL_GP_SAMPLE_MAX_N of sl_hip.h)
#define SL_GS_MAX_K 1024            // right-hand sides / samples per call   (SL_GP_SAMPLE_MAX_K)
#define SL_GS_MAX_TRAIN 4096        // observations of sl_gp_posterior_cov   (SL_GP_SAMPLE_MAX_TRAIN)

SL_HD int sl_gs_blocks(int64_t n) { return (int)((n + SL_GS_NB - 1) / SL_GS_NB); }
// rows of block b of an n-row matrix
SL_HD int sl_gs_block_rows(int64_t n, int b) {
    const int64_t rest = n - (int64_t)b * SL_GS_NB;
    return (int)(rest < SL_GS_NB ? rest : SL_GS_NB);
}

// In-place lower Cholesky factor of the nb x nb block a[i * SL_GS_LD + j] (only j <= i is read or written), by
// `nthreads` workers of which this is number `tid`; `sync` is the barrier between them (nothing for one
// worker).  Returns 0, or the 1-based column of the first pivot that is not > 0 (a NaN included): every worker
// reads the same pivot word, so all of them return together and no barrier is left waiting.
template <class Sync>
SL_HD int sl_gs_diag_factor(double* a, int nb, int tid, int nthreads, Sync&& sync) {
    for (int j = 0; j < nb; ++j) {
        const double pivot = a[j * SL_GS_LD + j];
        if (!(pivot > 0.0)) return j + 1;
        sync();                                             // every worker holds the pivot before it is replaced
        const double root = sqrt(pivot);
        for (int i = j + tid; i < nb; i += nthreads)
            a[i * SL_GS_LD + j] = (i == j) ? root : a[i * SL_GS_LD + j] / root;
        sync();
        const int m = nb - j - 1;                           // entries (i, c), j < c <= i, of the block that is left
        for (int t = tid; t < m * m; t += nthreads) {
            const int i = j + 1 + t / m, c = j + 1 + t % m;
            if (c <= i) a[i * SL_GS_LD + c] = a[i * SL_GS_LD + c] - a[i * SL_GS_LD + j] * a[c * SL_GS_LD + j];
        }
        sync();
    }
    return 0;
}

// One row x[0 .. nb) of the panel:  x L^T = a  with the factored diagonal block l[j * ldl + k]:
// x_j = (a_j - sum_{k < j} x_k l_jk) / l_jj, j and k ascending.
SL_HD void sl_gs_panel_row(double* x, const double* l, int64_t ldl, int nb) {
    for (int j = 0; j < nb; ++j) {
        double s = x[j];
        for (int k = 0; k < j; ++k) s = s - x[k] * l[j * ldl + k];
        x[j] = s / l[j * ldl + j];
    }
}

// One right-hand side x[i * stride], i < nb, of  L x = b  (transpose = 0: rows ascending) or  L^T x = b
// (rows descending); the inner sum runs over ascending j either way.
SL_HD void sl_gs_solve_col(double* x, int stride, const double* l, int64_t ldl, int nb, int transpose) {
    if (!transpose) {
        for (int i = 0; i < nb; ++i) {
            double s = x[i * stride];
            for (int j = 0; j < i; ++j) s = s - l[i * ldl + j] * x[j * stride];
            x[i * stride] = s / l[i * ldl + i];
        }
    } else {
        for (int i = nb - 1; i >= 0; --i) {
            double s = x[i * stride];
            for (int j = i + 1; j < nb; ++j) s = s - l[j * ldl + i] * x[j * stride];
            x[i * stride] = s / l[i * ldl + i];
        }
    }
}
