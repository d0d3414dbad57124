// Host side of the resampling stage: the closed-form low-pass at the stuffed rate (include/sgx.h: sgx_resamp_design).  No
// device.  The operations run in the order tests/resamp_spec.py states them (-ffp-contract=off), so the taps are the
// contract's wherever no unrounded tap sits on a rounding boundary, and fs_out is its value exactly.
#include <math.h>
#include <stdlib.h>

#include "sgx_check.h"

static int rs_gcd(int a, int b) { return b ? rs_gcd(b, a % b) : a; }

extern "C" int sgx_resamp_design(double fs, int32_t L, int32_t M, int32_t n_taps, double cutoff_hz, double gain, int16_t* taps,
                                 int32_t* shift, double* fs_out) {
    SGX_CHECK_ARG(taps && shift && fs_out);
    SGX_CHECK_ARG(isfinite(fs) && fs > 0);
    SGX_CHECK_ARG(isfinite(gain) && gain > 0);
    if (!(M >= 1 && M <= 3 && L > M && L <= 16 && rs_gcd(L, M) == 1)) {
        sgx_set_error("bad argument: L / M = %d / %d is not a pair with 1 <= M <= 3, M < L <= 16 and gcd(L, M) = 1", (int)L,
                      (int)M);
        return SGX_E_ARG;
    }
    SGX_CHECK_ARG(n_taps >= 1 && n_taps <= SGX_RESAMP_MAX_TAPS && (n_taps & 1) == 1);
    const double fu = fs * (double)L, fo = fu / (double)M;
    const double widest = (fs < fo ? fs : fo) / 2.0;
    if (!(isfinite(cutoff_hz) && cutoff_hz >= 0 && cutoff_hz <= widest)) {
        sgx_set_error("resampling design: cutoff_hz = %.6g Hz is not in 0 .. min(fs, fs L / M) / 2 = %.6g Hz", cutoff_hz, widest);
        return SGX_E_ARG;
    }
    const double fc = cutoff_hz > 0 ? cutoff_hz : widest;

    const int Lh = n_taps, c = (Lh - 1) / 2;
    const double a = (double)(1 << SGX_RESAMP_SHIFT) * gain * (double)L;
    long long sum_abs = 0;
    for (int k = 0; k < Lh; ++k) {
        const double m = (double)(k - c);
        const double t = 2.0 * fc * m / fu;
        const double sinc = (k == c) ? 1.0 : sin(M_PI * t) / (M_PI * t);
        const double win = (Lh == 1) ? 1.0 : 0.5 - 0.5 * cos(2.0 * M_PI * (double)k / (double)(Lh - 1));
        const double lp = (2.0 * fc / fu) * sinc * win;
        const double r = nearbyint(a * lp);   // round half to even (the default rounding mode)
        if (!(fabs(r) <= 32512.0)) {
            sgx_set_error("resampling design: tap %d = %.1f leaves the +-32512 the resampler takes (gain too large?)", k, r);
            return SGX_E_ARG;
        }
        taps[k] = (int16_t)r;
        sum_abs += llabs((long long)r);
    }
    if (128 * sum_abs >= (1ll << 31)) {
        sgx_set_error("resampling design: 128 sum|h| = %lld does not fit the resampler's int32 accumulator", 128 * sum_abs);
        return SGX_E_ARG;
    }
    *shift = SGX_RESAMP_SHIFT;
    *fs_out = fo;
    return SGX_OK;
}
