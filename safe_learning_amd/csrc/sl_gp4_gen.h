// sl_gp4_gen.h - pieces of the k_x generation that k_gp_sweep4 (sl_gp4.hip) and k_gp_mean_blocks
// (sl_gp4_mean.hip) share: the same exponential in both, so that a cell's k_x values - and with
// them its posterior mean - are the same bits whichever kernel forms them.
#pragma once
#include "sl_common.h"

typedef double sl_d2 __attribute__((ext_vector_type(2)));
typedef unsigned sl_u4 __attribute__((ext_vector_type(4)));

namespace gp4 {

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

}  // namespace gp4
