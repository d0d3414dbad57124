// The host side of the front-end conditioning stage (include/sgx.h: sgx_cond_plan; contract: tests/cond_spec.py plan()):
// the per-block statistics of sgx_cond_block_stats smoothed into a DC per lane, a gain and a blanking threshold per block.
// Exact double arithmetic in the order the header states (the build has no contraction); needs no GPU.
#include <math.h>

#include "sgx_internal.h"

// (mult, shift) of a gain by sgx_requant_gain's rule
static void cd_mult_shift(double g, int32_t* mult, int32_t* shift) {
    *mult = 32767;
    *shift = 0;
    for (int S = 30; S >= 0; --S) {
        const double r = nearbyint(ldexp(g, S));   // ldexp is exact; round half to even (the default mode)
        if (r <= 32767.0) {
            *mult = r < 1.0 ? 1 : (int32_t)r;
            *shift = S;
            return;
        }
    }
}

extern "C" int sgx_cond_plan(const sgx_cond_stats* stats, size_t n_blocks, int32_t lanes, int32_t blank_q4,
                             double target_rms, double agc_blocks, sgx_cond_entry* plan) {
    SGX_CHECK_ARG(lanes == 1 || lanes == 2);
    SGX_CHECK_ARG(blank_q4 == 0 || (blank_q4 >= 16 && blank_q4 <= 4096));
    SGX_CHECK_ARG(target_rms > 0.0 && target_rms <= 127.0);
    SGX_CHECK_ARG(agc_blocks >= 1.0 && isfinite(agc_blocks));
    SGX_CHECK_ARG((stats && plan) || n_blocks == 0);
    for (size_t k = 0; k < n_blocks; ++k) {
        const sgx_cond_stats& s = stats[k];
        const int64_t dc_max = 1 << 20;
        if (s.kept < 1 || s.p_kept < 0 || s.p_kept / s.kept >= ((int64_t)1 << 43) || s.dc0 < -dc_max || s.dc0 > dc_max ||
            s.dc1 < -dc_max || s.dc1 > dc_max) {
            sgx_set_error("bad argument: block %zu (kept %lld, p_kept %lld, dc %lld %lld) is not what sgx_cond_block_stats makes",
                          k, (long long)s.kept, (long long)s.p_kept, (long long)s.dc0, (long long)s.dc1);
            return SGX_E_ARG;
        }
    }
    const double alpha = 1.0 / agc_blocks;
    const double q = (double)(16 * lanes * blank_q4);
    double a = 0.0, A0 = 0.0, A1 = 0.0;
    for (size_t k = 0; k < n_blocks; ++k) {
        const sgx_cond_stats& s = stats[k];
        const double v = (double)s.p_kept / ((double)s.kept * (double)lanes * 256.0);
        const double D0 = (double)s.dc0, D1 = (double)s.dc1;
        if (k == 0) {
            a = v, A0 = D0, A1 = D1;
        } else {
            a = a + alpha * (v - a);
            A0 = A0 + alpha * (D0 - A0);
            A1 = A1 + alpha * (D1 - A1);
        }
        const double g = a > 0.0 ? target_rms / sqrt(a) : 1.0;
        sgx_cond_entry& e = plan[k];
        cd_mult_shift(g, &e.mult, &e.shift);
        e.dc0 = (int32_t)nearbyint(A0);
        e.dc1 = (int32_t)nearbyint(A1);
        e.theta = blank_q4 ? (int64_t)floor(a * q) : INT64_MAX;
    }
    return SGX_OK;
}
