// Host side of the decimation stage: the closed-form band-pass design and where the band lands at the new rate
// (include/sgx.h: sgx_decim_design).  No device.  The operations run in the order tests/decim_spec.py states them
// (-ffp-contract=off), so the taps are the contract's wherever no unrounded tap sits on a rounding boundary, and fs_out,
// f_out and inverted are its values exactly.
#include <math.h>
#include <stdlib.h>

#include "sgx_check.h"

extern "C" int sgx_decim_design(double fs, double f0, double bandwidth_hz, int32_t lanes, int32_t D, int32_t n_taps,
                                double gain, int16_t* taps, int32_t* shift, double* fs_out, double* f_out,
                                int32_t* inverted) {
    SGX_CHECK_ARG(taps && shift && fs_out && f_out && inverted);
    SGX_CHECK_ARG(isfinite(fs) && fs > 0);
    SGX_CHECK_ARG(isfinite(bandwidth_hz) && bandwidth_hz > 0);
    SGX_CHECK_ARG(isfinite(f0) && isfinite(gain));
    SGX_CHECK_ARG(lanes == 1 || lanes == 2);
    SGX_CHECK_ARG(D >= 2 && D <= 16);
    SGX_CHECK_ARG(n_taps >= 1 && n_taps <= SGX_DECIM_MAX_TAPS && (n_taps & 1) == 1);

    const double fo = fs / (double)D, half = fo / 2.0;
    double f_new;
    int inv = 0;
    if (lanes == 2) {
        if (!(bandwidth_hz < fo)) {
            sgx_set_error("decimation design: bandwidth_hz = %.6g Hz does not fit the new rate fs / D = %.6g Hz", bandwidth_hz, fo);
            return SGX_E_ARG;
        }
        double r = fmod(f0 + half, fo);   // (the floor mod: the sign of the divisor)
        if (r < 0) r += fo;
        f_new = r - half;
    } else {
        const double z = floor(f0 / half);
        const double lo = f0 - bandwidth_hz / 2.0, hi = f0 + bandwidth_hz / 2.0;
        if (!(z >= 0 && z < (double)D && lo > z * half && hi < (z + 1.0) * half)) {
            sgx_set_error("decimation design: the band f0 +- bandwidth_hz / 2 = %.6g .. %.6g Hz does not lie strictly inside one "
                          "Nyquist zone of fs / D = %.6g Hz and would alias onto itself (the default record, 38.192 Msps "
                          "with the IF at 9.548 MHz, at D = 2 or 4: the IF sits on a zone edge; D = 3 or 5 clear it)",
                          lo, hi, fo);
            return SGX_E_ARG;
        }
        inv = ((long long)z) & 1;
        f_new = inv ? (z + 1.0) * half - f0 : f0 - z * half;
    }

    const double g = gain > 0 ? gain : sqrt((fs / (lanes == 2 ? 1.0 : 2.0)) / bandwidth_hz);
    const int L = n_taps, c = (L - 1) / 2;
    long long sum_abs = 0;
    for (int k = 0; k < L; ++k) {
        const double m = (double)(k - c);
        const double t = bandwidth_hz * m / fs;
        const double sinc = (k == c) ? 1.0 : sin(M_PI * t) / (M_PI * t);
        const double win = (L == 1) ? 1.0 : 0.5 - 0.5 * cos(2.0 * M_PI * (double)k / (double)(L - 1));
        const double lp = (bandwidth_hz / fs) * sinc * win;
        const double ph = 2.0 * M_PI * f0 * m / fs;
        const double a = (double)(1 << SGX_DECIM_SHIFT) * g * lp;
        double u[2];
        if (lanes == 1) {
            u[0] = a * (2.0 * cos(ph));
        } else {
            u[0] = a * cos(ph), u[1] = a * sin(ph);
        }
        for (int i = 0; i < lanes; ++i) {
            const double r = nearbyint(u[i]);   // round half to even (the default rounding mode)
            if (!(fabs(r) <= 32512.0)) {
                sgx_set_error("decimation design: tap %d = %.1f leaves the +-32512 the decimator takes (gain too large?)", k, r);
                return SGX_E_ARG;
            }
            taps[lanes * k + i] = (int16_t)r;
            sum_abs += llabs((long long)r);
        }
    }
    if (128 * sum_abs >= (1ll << 31)) {
        sgx_set_error("decimation design: 128 sum|h| = %lld does not fit the decimator's int32 accumulator", 128 * sum_abs);
        return SGX_E_ARG;
    }
    *shift = SGX_DECIM_SHIFT;
    *fs_out = fo;
    *f_out = f_new;
    *inverted = inv;
    return SGX_OK;
}
