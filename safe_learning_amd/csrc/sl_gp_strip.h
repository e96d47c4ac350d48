// sl_gp_strip.h - the matrix-core strip of the dense FP64 linear algebra (sl_gp_sample.hip, sl_gp_likelihood.hip):
// every product between blocks is a 64 x 64 tile of a four-wavefront workgroup on v_mfma_f64_16x16x4_f64.
// Wavefront w owns the rows 16 w .. 16 w + 15 (four accumulator tiles), operands straight from global memory
// (A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15]; register r of a lane: row (lane >> 4) + 4 r,
// column lane & 15).  Device code only.
#pragma once

#include "sl_common.h"

typedef double sl_gs4 __attribute__((ext_vector_type(4)));

#define SL_GS_THREADS 256

// acc[t] += a(rows 0..15, k) b(k, columns 16 t .. 16 t + 15) over k in [0, kend): a(r, k) and b(k, c) return the
// operand or 0 outside their matrix (kend need not be a multiple of 4)
template <class FA, class FB>
__device__ __forceinline__ void gs_strip(int kend, FA a, FB b, sl_gs4 (&acc)[4]) {
    const int lane = threadIdx.x & 63, l15 = lane & 15, lk = lane >> 4;
    for (int kk = 0; kk < kend; kk += 4) {
        const double av = a(l15, kk + lk);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const double bv = b(kk + lk, 16 * t + l15);
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[t], 0, 0, 0);
        }
    }
}

#define GS_ZERO_ACC(acc)                                                      \
    sl_gs4 acc[4];                                                            \
    _Pragma("unroll") for (int t_ = 0; t_ < 4; ++t_) acc[t_] = (sl_gs4){0.0, 0.0, 0.0, 0.0}
