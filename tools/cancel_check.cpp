// A stand-alone run of sgx_cancel_design and sgx_cancel_host (csrc/sgx_cancel.cpp) for AddressSanitizer and UBSan: host code
// only, no device.  Every array is allocated to exactly what the calls may read and write - the record ends with the last
// sample of the last block - so an access past a block is a report.  tests/test_cancel_host.py builds it with
// -fsanitize=address,undefined next to csrc/sgx_cancel.cpp and csrc/sgx_core.cpp and runs it:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -static-libasan -static-libubsan -fno-sanitize-recover=undefined \
//       -ffp-contract=off -Iinclude -Isoftgnss-python_amd/csrc tools/cancel_check.cpp softgnss-python_amd/csrc/sgx_cancel.cpp \
//       softgnss-python_amd/csrc/sgx_core.cpp -o cancel_check && ./cancel_check
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "sgx.h"

static void fail(const char* what, int rc) {
    char msg[512];
    sgx_last_error(msg, sizeof msg);
    fprintf(stderr, "%s: returned %d (%s)\n", what, rc, msg);
    exit(1);
}

int main() {
    sgx_settings s;
    memset(&s, 0, sizeof s);
    s.samplingFreq = 2.046e6;
    s.IF = 0.4e6;
    s.codeFreqBasis = 1.023e6;
    s.codeLength = 1023;
    s.numberOfChannels = 3;
    const int n_ch = 3, ms = 9;
    const int64_t off = 700;                               // the record is a window of the file
    const sgx_chan_init ch[n_ch] = {{0.4e6 + 700.0, 703.0, 5, 0}, {0.0, 0.0, 0, 0}, {0.4e6 - 1500.0, 1900.0, 21, 0}};
    const int32_t done[n_ch] = {9, 9, 6};
    // series the recurrence of sgx_replay_state accepts: rates that wander, block ends formed as it forms them
    std::vector<double> series((size_t)n_ch * SGX_NUM_SERIES * ms, 0.0);
    int64_t last = 0;
    srand(11);
    for (int c = 0; c < n_ch; ++c) {
        if (ch[c].prn == 0) continue;
        double* row = series.data() + (size_t)c * SGX_NUM_SERIES * ms;
        double cf = s.codeFreqBasis, rem = 0.0;
        int64_t pos = (int64_t)ch[c].codePhase;
        for (int k = 0; k < ms; ++k) {
            const double step = cf / s.samplingFreq;
            const double nblk = ceil((1023.0 - rem) / step);
            pos += (int64_t)nblk;
            row[k] = (double)pos;
            const double lin = ((nblk * step + rem) - rem) / nblk;
            rem = (nblk - 1.0) * lin + rem + step - 1023.0;
            cf = s.codeFreqBasis + (rand() % 2001 - 1000) * 0.01;
            row[ms + k] = cf;
            row[2 * ms + k] = ch[c].acquiredFreq + (rand() % 401 - 200) * 0.1;
            row[3 * ms + k] = (rand() % 2 ? 1.0 : -1.0) * (15000.0 + rand() % 3000);      // I_P
            row[7 * ms + k] = (double)(rand() % 4001 - 2000);                                  // Q_P
            if (k < done[c] && pos > last) last = pos;
        }
    }
    const size_t n = (size_t)(last - off);
    std::vector<sgx_replay_block> state((size_t)n_ch * ms);
    int rc = sgx_replay_state(&s, SGX_DT_INT8, ch, n_ch, ms, done, series.data(), off, (int64_t)n, state.data());
    if (rc != SGX_OK) fail("sgx_replay_state", rc);
    std::vector<int8_t> x(n), y(n);
    for (size_t i = 0; i < n; ++i) x[i] = (int8_t)(rand() % 256 - 128);
    long calls = 0, clips = 0;
    for (int smooth : {1, 5, 21, 41}) {
        std::vector<double> amp((size_t)n_ch * ms * 2);
        rc = sgx_cancel_design(series.data(), state.data(), n_ch, ms, done, smooth, amp.data());
        if (rc != SGX_OK) fail("sgx_cancel_design", rc);
        if (amp[(size_t)(2 * ms + 6) * 2] != 0.0 || amp[(size_t)ms * 2] != 0.0) fail("blocks that are not cancelled hold 0", 0);
        int64_t clipped = -1;
        rc = sgx_cancel_host(&s, x.data(), n, off, ch, n_ch, ms, done, series.data(), SGX_DT_INT8, amp.data(), y.data(), &clipped);
        if (rc != SGX_OK || clipped < 0) fail("sgx_cancel_host", rc);
        for (size_t i = 0; i < 3; ++i)
            if (y[i] != x[i]) fail("the samples in front of the first block are copied", 0);
        clips += (long)clipped;
        calls += 2;
    }
    // the refusals leave everything alone
    std::vector<double> amp((size_t)n_ch * ms * 2, 1.0);
    int64_t clipped = 0;
    if (sgx_cancel_design(series.data(), state.data(), n_ch, ms, done, 4, amp.data()) != SGX_E_ARG) fail("an even smooth", 0);
    if (sgx_cancel_host(&s, x.data(), n - 1, off, ch, n_ch, ms, done, series.data(), SGX_DT_INT8, amp.data(), y.data(), &clipped) !=
        SGX_E_RANGE)
        fail("a record one sample short", 0);
    amp[5] = NAN;
    if (sgx_cancel_host(&s, x.data(), n, off, ch, n_ch, ms, done, series.data(), SGX_DT_INT8, amp.data(), y.data(), &clipped) !=
        SGX_E_ARG)
        fail("an amplitude that is not finite", 0);
    calls += 3;
    printf("sanitized cancellation: %ld calls on %zu samples, %ld clipped, no report\n", calls, n, clips);
    return 0;
}
