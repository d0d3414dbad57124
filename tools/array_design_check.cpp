// A stand-alone run of sgx_array_design_blocks (csrc/sgx_array.cpp) for AddressSanitizer and UBSan: host code only, no
// device.  Every output array is allocated to exactly what the call may write, so a write past a block's slot is a report.
// tests/test_array_block_host.py builds it with -fsanitize=address,undefined next to csrc/sgx_array.cpp and
// csrc/sgx_core.cpp and runs it:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -static-libasan -static-libubsan -fno-sanitize-recover=undefined \
//       -ffp-contract=off -Iinclude \
//       -Isoftgnss-python_amd/csrc tools/array_design_check.cpp softgnss-python_amd/csrc/sgx_array.cpp \
//       softgnss-python_amd/csrc/sgx_core.cpp -o array_design_check && ./array_design_check
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

// The statistics of one block of `frames` frames of A streams that share one source under noise of their own: Hermitian,
// positive definite, terms at every lag
static void block_stats(int frames, int lanes, int A, int K, unsigned seed, int64_t* rho) {
    srand(seed);
    std::vector<int> x((size_t)(frames + K) * A * lanes, 0);
    for (int f = 0; f < frames; ++f) {
        const int s0 = rand() % 81 - 40, s1 = rand() % 81 - 40;
        for (int a = 0; a < A; ++a)
            for (int l = 0; l < lanes; ++l)
                x[((size_t)f * A + a) * lanes + l] = ((a + 1) * (l ? s1 : s0)) / 2 + (a & 1 ? s1 : -s0) / 3 + rand() % 13 - 6;
    }
    for (int a = 0; a < A; ++a)
        for (int b = 0; b < A; ++b)
            for (int d = 0; d < K; ++d) {
                int64_t re = 0, im = 0;
                for (int f = 0; f < frames; ++f) {
                    const int* za = &x[((size_t)(f + d) * A + a) * lanes];
                    const int* zb = &x[((size_t)f * A + b) * lanes];
                    re += (int64_t)za[0] * zb[0];
                    if (lanes == 2) re += (int64_t)za[1] * zb[1], im += (int64_t)za[1] * zb[0] - (int64_t)za[0] * zb[1];
                }
                int64_t* e = rho + ((size_t)(a * A + b) * K + d) * lanes;
                e[0] = re;
                if (lanes == 2) e[1] = im;
            }
}

int main() {
    const int64_t B = SGX_ARRAY_BLOCK_UNIT;
    long calls = 0, held_seen = 0;
    const int shapes[][3] = {{1, 4, 5}, {2, 4, 1}, {2, 8, 7}, {1, 2, 15}, {2, 3, 3}};   // (lanes, A, K)
    for (const auto& sh : shapes) {
        const int lanes = sh[0], A = sh[1], K = sh[2];
        const size_t n_val = (size_t)A * A * K * lanes, n_tap = (size_t)A * K * lanes;
        for (int n_blocks : {1, 2, 7}) {
            const int64_t F = (int64_t)(n_blocks - 1) * B + 333;                     // a short last block
            std::vector<int64_t> rho(n_val * n_blocks, 0);
            for (int j = 0; j < n_blocks; ++j) {
                const bool zero = n_blocks == 7 && (j == 0 || j == 3 || j == 4);    // a leading block and a stretch of two
                if (!zero) block_stats(j == n_blocks - 1 ? 333 : (int)B, lanes, A, K, 17u * j + A, rho.data() + n_val * j);
            }
            for (int W : {1, 3, 63}) {
                std::vector<int16_t> taps(n_tap * n_blocks);
                std::vector<double> weights(n_tap * n_blocks), gain(n_blocks), supp(n_blocks);
                std::vector<uint8_t> status(n_blocks);
                int32_t shift = -1;
                int rc = sgx_array_design_blocks(rho.data(), n_blocks, F, B, W, lanes, A, K, A - 1, 1e-3, 12.0, taps.data(), &shift,
                                                 weights.data(), gain.data(), supp.data(), status.data());
                if (rc != SGX_OK || shift != SGX_ARRAY_SHIFT) fail("sgx_array_design_blocks", rc);
                for (int j = 0; j < n_blocks; ++j) held_seen += status[j];
                if (W == 1 && n_blocks == 7 && !(status[0] && status[3] && status[4] && !status[1] && !status[2] && !status[5]))
                    fail("the hold rule", rc);
                if (W == 1 && n_blocks == 7 &&
                    (memcmp(&taps[0], &taps[n_tap], n_tap * 2) || memcmp(&taps[3 * n_tap], &taps[2 * n_tap], n_tap * 2) ||
                     memcmp(&taps[4 * n_tap], &taps[2 * n_tap], n_tap * 2)))
                    fail("the held taps", rc);
                // the optional outputs left out
                rc = sgx_array_design_blocks(rho.data(), n_blocks, F, B, W, lanes, A, K, 0, 1e-2, 3.0, taps.data(), &shift, nullptr,
                                             nullptr, nullptr, nullptr);
                if (rc != SGX_OK) fail("sgx_array_design_blocks without the optional outputs", rc);
                calls += 2;
            }
            // an all-zero record and the argument refusals leave everything alone
            std::vector<int64_t> none(n_val * n_blocks, 0);
            std::vector<int16_t> taps(n_tap * n_blocks);
            int32_t shift = 0;
            if (sgx_array_design_blocks(none.data(), n_blocks, F, B, 3, lanes, A, K, 0, 1e-3, 12.0, taps.data(), &shift, nullptr,
                                        nullptr, nullptr, nullptr) != SGX_E_ARG)
                fail("an all-zero record", 0);
            if (sgx_array_design_blocks(rho.data(), n_blocks + 1, F, B, 3, lanes, A, K, 0, 1e-3, 12.0, taps.data(), &shift, nullptr,
                                        nullptr, nullptr, nullptr) != SGX_E_ARG)
                fail("a wrong n_blocks", 0);
            calls += 2;
        }
    }
    if (!held_seen) fail("no held block was seen", 0);
    printf("sanitized block design: %ld calls, %ld held blocks, no report\n", calls, held_seen);
    return 0;
}
