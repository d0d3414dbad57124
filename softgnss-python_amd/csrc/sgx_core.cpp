// The exact host arithmetic of libsgx.so: error text, C/A codes, loop coefficients, the host side of the tracking-math
// evaluators, the replay's recurrence.  No HIP: the file also builds with a plain C++ compiler (tools/sanitize_host.sh).
// Compiled with -ffp-contract=off: the index math below must round exactly like the reference's
// numpy expressions.
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "sgx.h"
#include "sgx_check.h"
#include "sgx_trk_math_eval.h"

static thread_local char g_err[512] = "";

void sgx_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* sgx_version(void) { return SGX_VERSION_STR; }

extern "C" int sgx_last_error(char* buf, size_t n) {
    if (!buf || n == 0) return SGX_E_ARG;
    strncpy(buf, g_err, n - 1);
    buf[n - 1] = 0;
    return SGX_OK;
}

// ---- exact host helpers ---------------------------------------------------------------------

// G2 delays of PRN 1..32 (reference initialize.py:251-254 keeps 51 entries; only 32 reachable).
static const int kG2Delay[32] = {5,   6,   7,   8,   17,  18,  139, 140, 141, 251, 252,
                                 254, 255, 256, 257, 258, 469, 470, 471, 472, 473, 474,
                                 509, 512, 513, 514, 515, 516, 859, 860, 861, 862};

// Gold code of PRN index prn0 as +-1 chips. Bit-level statement of initialize.py:234-302:
// registers start all-ones, output = stage 10, G1 feedback 3^10, G2 feedback 2^3^6^8^9^10,
// G2 delayed by kG2Delay, chip = +1 where g1^g2 == 1.
int sgx_host_ca_code(int prn0, int8_t* out) {
    if (prn0 < 0 || prn0 > 31) return SGX_E_ARG;
    uint32_t r1 = 0x3FF, r2 = 0x3FF;   // bit i = stage i+1
    int8_t g1[1023], g2[1023];
    for (int i = 0; i < 1023; ++i) {
        g1[i] = (r1 >> 9) & 1;
        g2[i] = (r2 >> 9) & 1;
        uint32_t f1 = ((r1 >> 2) ^ (r1 >> 9)) & 1;
        uint32_t f2 = ((r2 >> 1) ^ (r2 >> 2) ^ (r2 >> 5) ^ (r2 >> 7) ^ (r2 >> 8) ^ (r2 >> 9)) & 1;
        r1 = ((r1 << 1) | f1) & 0x3FF;
        r2 = ((r2 << 1) | f2) & 0x3FF;
    }
    const int d = kG2Delay[prn0];
    for (int i = 0; i < 1023; ++i) {
        int j = i - d;
        if (j < 0) j += 1023;
        out[i] = (g1[i] ^ g2[j]) ? 1 : -1;
    }
    return SGX_OK;
}

int64_t sgx_host_samples_per_code(const sgx_settings* s) {
    // initialize.py:185: long(round(fs / (fc / codeLength))), numpy round = half to even
    return (int64_t)nearbyint(s->samplingFreq / (s->codeFreqBasis / (double)s->codeLength));
}

extern "C" int sgx_samples_per_code(const sgx_settings* s, int64_t* n) {
    SGX_CHECK_ARG(s && n);
    *n = sgx_host_samples_per_code(s);
    return SGX_OK;
}

extern "C" int sgx_generate_ca_code(int32_t prn0, double* out) {
    SGX_CHECK_ARG(out);
    int8_t c[1023];
    if (sgx_host_ca_code(prn0, c) != SGX_OK) {
        sgx_set_error("prn index %d outside 0..31", prn0);   // reference asserts (initialize.py:250)
        return SGX_E_ARG;
    }
    for (int i = 0; i < 1023; ++i) out[i] = (double)c[i];
    return SGX_OK;
}

extern "C" int sgx_make_ca_table(const sgx_settings* s, double* out) {
    SGX_CHECK_ARG(s && out);
    const int64_t n = sgx_host_samples_per_code(s);
    SGX_CHECK_ARG(n > 0 && s->codeLength == 1023);
    const double ts = 1.0 / s->samplingFreq;
    const double tc = 1.0 / s->codeFreqBasis;
    std::vector<int> idx((size_t)n);
    for (int64_t k = 1; k <= n; ++k) {
        const double v = (ts * (double)k) / tc;   // initialize.py:222: multiply, then divide
        idx[(size_t)(k - 1)] = (int)ceil(v) - 1;
    }
    idx[(size_t)(n - 1)] = 1022;                  // initialize.py:226
    for (int p = 0; p < 32; ++p) {
        int8_t c[1023];
        sgx_host_ca_code(p, c);
        double* row = out + (size_t)p * (size_t)n;
        for (int64_t k = 0; k < n; ++k) {
            const int j = idx[(size_t)k];
            if (j < 0 || j > 1022) {
                sgx_set_error("code index %d out of range at sample %lld", j, (long long)k);
                return SGX_E_ARG;
            }
            row[k] = (double)c[j];
        }
    }
    return SGX_OK;
}

extern "C" int sgx_calc_loop_coef(double lbw, double zeta, double k, double* tau1, double* tau2) {
    SGX_CHECK_ARG(tau1 && tau2);
    const double wn = lbw * 8.0 * zeta / (4.0 * (zeta * zeta) + 1);   // initialize.py:321
    *tau1 = k / (wn * wn);
    *tau2 = 2.0 * zeta / wn;
    return SGX_OK;
}

// ---- the evaluators of csrc/sgx_trk_math.h, host side ----------------------------------------------

extern "C" int sgx_trk_math_eval(int32_t fn, double a, double b, double* out) {
    SGX_CHECK_ARG(out && fn >= 0 && fn <= 10);
    // (fn 10: the block length at fs = 38.192 MHz; sgx_trk_math_eval_batch takes the rate as an operand)
    sgx_trk_math_call(fn, a, b, 38192000.0, 1.0 / 38192000.0, out[0], out[1]);
    return SGX_OK;
}

extern "C" int sgx_trk_math_eval_batch(int32_t fn, int64_t n, const double* a, const double* b, const double* c,
                                       const double* d, double* out0, double* out1) {
    SGX_CHECK_ARG(fn >= 0 && fn < SGX_MATH_FN_HD_END);
    SGX_CHECK_ARG(n >= 0 && out0 && out1);
    SGX_CHECK_ARG(n == 0 || a);
    for (int64_t i = 0; i < n; ++i) {
        double o0 = 0.0, o1 = 0.0;
        sgx_trk_math_call(fn, a[i], b ? b[i] : 0.0, c ? c[i] : 0.0, d ? d[i] : 0.0, o0, o1);
        out0[i] = o0;
        out1[i] = o1;
    }
    return SGX_OK;
}

// ---- the per-block state of a tracked channel, rebuilt from its recorded series (include/sgx.h: sgx_replay_state) ----------
// One serial recurrence per channel, in the reference's operation order (tracking.py:148-251; the build is -ffp-contract=off).
// Only the last element of the prompt linspace is needed: numpy forms it as (blk - 1) * ((stop - start) / blk) + start.
extern "C" int sgx_replay_state(const sgx_settings* s, int32_t data_type, const sgx_chan_init* ch, int32_t n_ch, int32_t ms,
                                const int32_t* ms_done, const double* series, int64_t rec_file_offset, int64_t rec_bytes,
                                sgx_replay_block* state) {
    SGX_CHECK_ARG(s && ch && series && state);
    SGX_CHECK_ARG(n_ch >= 1 && ms >= 1);
    SGX_CHECK_ARG(s->samplingFreq > 0 && s->codeFreqBasis > 0);
    if (data_type != SGX_DT_INT8 && data_type != SGX_DT_UINT8 && data_type != SGX_DT_INT16) {
        sgx_set_error("bad argument: the replay reads int8, uint8 and int16 records, not data_type %d", (int)data_type);
        return SGX_E_ARG;
    }
    if (ms_done)
        for (int i = 0; i < n_ch; ++i)
            if (ms_done[i] < 0 || ms_done[i] > ms) {
                sgx_set_error("bad argument: ms_done[%d] = %d outside [0, %d]", i, (int)ms_done[i], (int)ms);
                return SGX_E_ARG;
            }
    const long long isz = data_type == SGX_DT_INT16 ? 2 : 1;
    const double fs = s->samplingFreq;
    const double two_pi = 2.0 * M_PI;
    memset(state, 0, sizeof(sgx_replay_block) * (size_t)n_ch * (size_t)ms);
    for (int c = 0; c < n_ch; ++c) {
        if (ch[c].prn == 0) continue;
        if (ch[c].prn < 1 || ch[c].prn > 32 || !isfinite(ch[c].acquiredFreq) || !isfinite(ch[c].codePhase)) {
            sgx_set_error("bad argument: channel %d (prn %d) is not a channel of preRun", c, (int)ch[c].prn);
            return SGX_E_ARG;
        }
        const double* row_abs = series + (size_t)c * SGX_NUM_SERIES * (size_t)ms;
        const double* row_code = row_abs + ms;
        const double* row_carr = row_abs + 2 * (size_t)ms;
        long long pos = (long long)((double)s->skipNumberOfBytes + ch[c].codePhase);   // int(skip + codePhase), tracking.py:107
        double code_freq = s->codeFreqBasis, carr_freq = ch[c].acquiredFreq;
        double rem_code = 0.0, rem_carr = 0.0;
        const int done = ms_done ? ms_done[c] : ms;
        for (int k = 0; k < done; ++k) {
            const double step = code_freq / fs;
            const double nblk = ceil(((double)s->codeLength - rem_code) / step);
            if (!(isfinite(carr_freq) && nblk >= 1.0 && nblk < 2147483648.0)) {
                sgx_set_error("bad argument: channel %d block %d: the recorded rates give no block (codeFreq %g, carrFreq %g)",
                              c, k, code_freq, carr_freq);
                return SGX_E_ARG;
            }
            const long long blk = (long long)nblk;
            if (!(row_abs[k] == (double)(pos + blk * isz))) {
                sgx_set_error("bad argument: channel %d block %d: the rebuilt block ends at byte %lld, absoluteSample says %.17g "
                              "(not a tracking result of this channel)", c, k, pos + blk * isz, row_abs[k]);
                return SGX_E_ARG;
            }
            if (rec_bytes >= 0 && (pos < rec_file_offset || pos + blk * isz > rec_file_offset + rec_bytes)) {
                sgx_set_error("channel %d block %d: bytes [%lld, %lld) lie outside the record [%lld, %lld)", c, k, pos,
                              pos + blk * isz, (long long)rec_file_offset, (long long)(rec_file_offset + rec_bytes));
                return SGX_E_RANGE;
            }
            sgx_replay_block& b = state[(size_t)c * ms + k];
            b.start = pos;
            b.rem_code = rem_code;
            b.rem_carr = rem_carr;
            b.step = step;
            b.carr_freq = carr_freq;
            b.blk = (int32_t)blk;
            const double stop = nblk * step + rem_code;
            const double lin = (stop - rem_code) / nblk;
            const double tp_last = (nblk - 1.0) * lin + rem_code;
            rem_code = tp_last + step - 1023.0;
            const double arg = carr_freq * 2.0 * M_PI * (nblk / fs) + rem_carr;
            double r = fmod(arg, two_pi);             // numpy's %: the sign of the divisor
            if (r != 0.0) {
                if (r < 0.0) r += two_pi;
            } else {
                r = 0.0;
            }
            rem_carr = r;
            pos += blk * isz;
            code_freq = row_code[k];
            carr_freq = row_carr[k];
        }
    }
    return SGX_OK;
}
