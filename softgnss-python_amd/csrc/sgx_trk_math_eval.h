// The fn -> call table of the evaluators of csrc/sgx_trk_math.h (include/sgx.h: sgx_trk_math_eval, sgx_trk_math_eval_batch,
// sgx_trk_math_eval_device).  ONE function, compiled for the host by sgx_core.cpp and for the device by
// sgx_trk_math_dev.hip: both evaluate literally this source, each with its own seeds, libm and code generator.
// Test support only: no tracking kernel includes this file.
#pragma once
#include "sgx_trk_math.h"

#define SGX_MATH_FN_HD_END 14      // fn 0 .. 13: sgx_trk_math.h, host and device
#define SGX_MATH_FN_DEV_FIRST 16   // fn 16 .. : sgx_trk_common.h, device only (sgx_trk_math_dev.hip)

// a, b, c, d: the operands of element i; o0, o1: its results (o1 is left alone where fn has one result).  true: fn is known.
SGX_HD bool sgx_trk_math_call(int fn, double a, double b, double c, double d, double& o0, double& o1) {
    switch (fn) {
        case 0: o0 = sgx_fast_rcp(a); return true;
        case 1: o0 = sgx_fast_div(a, b); return true;
        case 2: o0 = sgx_fast_sqrt(a); return true;
        case 3: o0 = sgx_atan_ratio(a, b); return true;
        case 4: sgx_sincos_turns_short(a, o0, o1); return true;
        case 5: o0 = (double)sgx_ceil_div(a, b); return true;
        case 6: o0 = sgx_div1(a, b); return true;
        case 7: o0 = sgx_sqrt1(a); return true;
        case 8: o0 = sgx_atan_ratio_k(a, b, sgx_atan_coef()); return true;
        case 9: sgx_rot_small(a, sgx_rot_coef(), o0, o1); return true;
        case 10: {   // a = 1023 - rem, b = codeFreq, c = fs, d = RN(1 / fs): block length, step_a
            double inv_step;
            o0 = (double)sgx_block_length(a, b, c, d, o1, inv_step);
            return true;
        }
        case 11: o0 = sgx_sqrt1_pos(a); return true;
        case 12: o0 = sgx_div_rn(a, b, c); return true;   // c = RN(1 / b)
        case 13: {   // as 10: block length, ~1 / step_a
            double step_a;
            o0 = (double)sgx_block_length(a, b, c, d, step_a, o1);
            return true;
        }
        default: return false;
    }
}
