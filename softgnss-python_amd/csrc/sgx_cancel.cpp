// The host side of the strong-signal cancellation (include/sgx.h: sgx_cancel_design, sgx_cancel_host; contract:
// tests/cancel_spec.py): the amplitude pairs from the prompt sums, the argument checks and block tables that the kernel of
// sgx_cancel.hip shares, and the kernel's work sample by sample with libm.  Exact double arithmetic in the contract's order
// (the build has no contraction); no HIP, needs no GPU.
#include <string.h>

#include "sgx_cancel_core.h"

extern "C" int sgx_cancel_design(const double* series, const sgx_replay_block* state, int32_t n_ch, int32_t ms,
                                 const int32_t* ms_done, int32_t smooth, double* amp) {
    SGX_CHECK_ARG(series && state && amp);
    SGX_CHECK_ARG(n_ch >= 1 && ms >= 1);
    if (smooth < 1 || smooth > CN_MAX_SMOOTH || (smooth & 1) == 0) {
        sgx_set_error("bad argument: the amplitudes are smoothed over an odd number of blocks in 1 .. %d, not %d",
                      CN_MAX_SMOOTH, (int)smooth);
        return SGX_E_ARG;
    }
    if (ms_done)
        for (int c = 0; c < n_ch; ++c)
            if (ms_done[c] < 0 || ms_done[c] > ms) {
                sgx_set_error("bad argument: ms_done[%d] = %d outside [0, %d]", c, (int)ms_done[c], (int)ms);
                return SGX_E_ARG;
            }
    const int half = (smooth - 1) / 2;
    std::vector<double> p(2 * (size_t)ms);
    for (int c = 0; c < n_ch; ++c) {
        const double* i_p = series + ((size_t)c * SGX_NUM_SERIES + 3) * (size_t)ms;
        const double* q_p = series + ((size_t)c * SGX_NUM_SERIES + 7) * (size_t)ms;
        const sgx_replay_block* b = state + (size_t)c * ms;
        double* a = amp + (size_t)c * ms * 2;
        int done = ms_done ? ms_done[c] : ms;
        while (done > 0 && b[done - 1].blk <= 0) --done;      // (a channel that is off: its state holds zeros)
        for (int k = 0; k < done; ++k) {
            if (b[k].blk <= 0) {
                sgx_set_error("bad argument: channel %d block %d has no length: not a state of sgx_replay_state", c, k);
                return SGX_E_ARG;
            }
            p[2 * k] = 2.0 * i_p[k] / (double)b[k].blk;
            p[2 * k + 1] = 2.0 * q_p[k] / (double)b[k].blk;
        }
        for (int k = 0; k < ms; ++k) {
            a[2 * k] = 0.0;
            a[2 * k + 1] = 0.0;
            if (k >= done) continue;
            const int lo = k - half < 0 ? 0 : k - half, hi = k + half >= done ? done - 1 : k + half;
            double si = 0.0, sq = 0.0;
            for (int j = lo; j <= hi; ++j) {                  // the data-bit sign of block j against block k; 0 counts as +1
                const double dot = p[2 * j] * p[2 * k] + p[2 * j + 1] * p[2 * k + 1];
                const double d = dot < 0.0 ? -1.0 : 1.0;
                si += d * p[2 * j];
                sq += d * p[2 * j + 1];
            }
            a[2 * k] = si / (double)(hi - lo + 1);
            a[2 * k + 1] = sq / (double)(hi - lo + 1);
        }
    }
    return SGX_OK;
}

int cn_check(const sgx_settings* s, int64_t rec_file_offset, int64_t rec_bytes, const sgx_chan_init* ch, int32_t n_ch,
             int32_t ms, const int32_t* ms_done, const double* series, int32_t data_type, const double* amp,
             std::vector<sgx_replay_block>* state) {
    SGX_CHECK_ARG(s && ch && series && amp);
    if (n_ch < 1 || n_ch > CN_MAX_CHANNELS) {
        sgx_set_error("bad argument: 1 .. %d channels are cancelled in one call, not %d", CN_MAX_CHANNELS, (int)n_ch);
        return SGX_E_ARG;
    }
    SGX_CHECK_ARG(ms >= 1);
    if (data_type != SGX_DT_INT8) {
        sgx_set_error("bad argument: the cancellation reads and writes int8 records, not data_type %d", (int)data_type);
        return SGX_E_ARG;
    }
    for (size_t i = 0; i < (size_t)n_ch * (size_t)ms * 2; ++i)
        if (!isfinite(amp[i])) {
            sgx_set_error("bad argument: the amplitude of channel %d block %d is not finite", (int)(i / 2 / (size_t)ms),
                          (int)(i / 2 % (size_t)ms));
            return SGX_E_ARG;
        }
    state->assign((size_t)n_ch * (size_t)ms, sgx_replay_block{});
    return sgx_replay_state(s, data_type, ch, n_ch, ms, ms_done, series, rec_file_offset, rec_bytes, state->data());
}

void cn_tables(const sgx_settings* s, int64_t rec_file_offset, const sgx_chan_init* ch, int32_t n_ch, int32_t ms,
               const int32_t* ms_done, const sgx_replay_block* state, const double* amp, CnBlock* blocks, CnChan* chan) {
    const double fs = s->samplingFreq;
    memset(blocks, 0, sizeof(CnBlock) * (size_t)n_ch * (size_t)ms);
    for (int c = 0; c < n_ch; ++c) {
        chan[c].prn = ch[c].prn;
        chan[c].done = ch[c].prn == 0 ? 0 : (ms_done ? ms_done[c] : ms);
        for (int k = 0; k < chan[c].done; ++k) {
            const sgx_replay_block& b = state[(size_t)c * ms + k];
            CnBlock& o = blocks[(size_t)c * ms + k];
            const double nblk = (double)b.blk;
            o.pos = (long long)(b.start - rec_file_offset);
            o.blk = b.blk;
            o.start = b.rem_code;
            o.lin = ((nblk * b.step + b.rem_code) - b.rem_code) / nblk;
            const double c0 = ceil(b.rem_code) - 1.0;
            double m = fmod(c0, 1023.0);
            if (m < 0.0) m += 1023.0;
            o.cb = c0 - m + 1.0;
            o.w = b.carr_freq * 2.0 * M_PI;
            o.rem_carr = b.rem_carr;
            o.rot_s = sin(o.w * (1.0 / fs));
            o.rot_c = cos(o.w * (1.0 / fs));
            o.a_i = amp[((size_t)c * ms + k) * 2];
            o.a_q = amp[((size_t)c * ms + k) * 2 + 1];
        }
    }
}

extern "C" int sgx_cancel_host(const sgx_settings* s, const int8_t* x, size_t n, int64_t rec_file_offset,
                               const sgx_chan_init* ch, int32_t n_ch, int32_t ms, const int32_t* ms_done,
                               const double* series, int32_t data_type, const double* amp, int8_t* y, int64_t* clipped) {
    SGX_CHECK_ARG(x && y && clipped);
    std::vector<sgx_replay_block> state;
    const int rc = cn_check(s, rec_file_offset, (int64_t)n, ch, n_ch, ms, ms_done, series, data_type, amp, &state);
    if (rc != SGX_OK) return rc;
    const double fs = s->samplingFreq;
    std::vector<double> v(n);
    std::vector<uint8_t> covered(n, 0);
    for (size_t i = 0; i < n; ++i) v[i] = (double)x[i];
    for (int c = 0; c < n_ch; ++c) {                          // channel order: the order of the subtractions at a sample
        if (ch[c].prn == 0) continue;
        int8_t code[1023];
        sgx_host_ca_code(ch[c].prn - 1, code);
        const int done = ms_done ? ms_done[c] : ms;
        for (int k = 0; k < done; ++k) {
            const sgx_replay_block& b = state[(size_t)c * ms + k];
            const double nblk = (double)b.blk;
            const double lin = ((nblk * b.step + b.rem_code) - b.rem_code) / nblk;
            const double w = b.carr_freq * 2.0 * M_PI;
            const double a_i = amp[((size_t)c * ms + k) * 2], a_q = amp[((size_t)c * ms + k) * 2 + 1];
            const size_t p0 = (size_t)(b.start - rec_file_offset);
            for (int i = 0; i < b.blk; ++i) {
                const double arg = w * ((double)i / fs) + b.rem_carr;
                const double t = (double)i * lin + b.rem_code;
                double m = fmod(ceil(t) - 1.0, 1023.0);
                if (m < 0.0) m += 1023.0;
                const double chip = (double)code[(int)m];
                const double sc = chip * (a_i * sin(arg) + a_q * cos(arg));
                v[p0 + i] = v[p0 + i] - sc;
                covered[p0 + i] = 1;
            }
        }
    }
    int64_t clips = 0;
    for (size_t i = 0; i < n; ++i) {
        if (!covered[i]) {
            y[i] = x[i];
            continue;
        }
        double r = nearbyint(v[i]);                           // round half to even (the default mode)
        if (r > 127.0 || r < -127.0) {
            ++clips;
            r = r > 0.0 ? 127.0 : -127.0;
        }
        y[i] = (int8_t)r;
    }
    *clipped = clips;
    return SGX_OK;
}
