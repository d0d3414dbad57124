// Host side of the multi-antenna combiner: the power-inversion weights from the record's lag statistics (include/sgx.h:
// sgx_array_design, and sgx_array_design_blocks, which runs the same steps on the statistics of a window of blocks).  No
// device.  The operations run in the order the header and tests/array_spec.py state them (-ffp-contract=off), so taps, gain,
// suppression and weights are the contract's to the bit.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "sgx_check.h"

// The refusals of the arguments that both entry points share, in sgx_array_design's order
static int ar_design_args(int32_t lanes, int32_t A, int32_t K, int32_t ref, double loading, double target_rms) {
    if (lanes != 1 && lanes != 2) {
        sgx_set_error("array design: lanes %d is not 1 (real records) or 2 (interleaved I/Q)", (int)lanes);
        return SGX_E_ARG;
    }
    if (A < 2 || A > SGX_ARRAY_MAX_ANTENNAS) {
        sgx_set_error("array design: A = %d antennas lie outside 2 .. %d", (int)A, SGX_ARRAY_MAX_ANTENNAS);
        return SGX_E_ARG;
    }
    if (K < 1 || K > SGX_ARRAY_MAX_TAPS || (K & 1) == 0) {
        sgx_set_error("array design: K = %d is not an odd number in 1 .. %d", (int)K, SGX_ARRAY_MAX_TAPS);
        return SGX_E_ARG;
    }
    if (A * K > SGX_ARRAY_MAX_WEIGHTS) {
        sgx_set_error("array design: A K = %d weights are more than %d", (int)(A * K), SGX_ARRAY_MAX_WEIGHTS);
        return SGX_E_ARG;
    }
    if (ref < 0 || ref >= A) {
        sgx_set_error("array design: ref = %d is none of the antennas 0 .. %d", (int)ref, (int)A - 1);
        return SGX_E_ARG;
    }
    if (!(isfinite(loading) && loading >= 0)) {
        sgx_set_error("array design: loading = %g is negative or not finite", loading);
        return SGX_E_ARG;
    }
    if (!(target_rms > 0 && target_rms <= 127.0)) {
        sgx_set_error("array design: target_rms = %g lies outside (0, 127]", target_rms);
        return SGX_E_ARG;
    }
    return SGX_OK;
}

// Steps 1 to 9 on one pair (rho, frames) whose arguments have passed.  where: the head of a refusal of the TAPS it makes,
// "array design" or that with the block's number.  *matrix_refused (never null): the matrix is what was refused - not
// positive definite -, which sgx_array_design_blocks answers by holding a neighbour's taps; nothing has been written then.
static int ar_design_solve(const char* where, const int64_t* rho, int64_t frames, int32_t lanes, int32_t A, int32_t K,
                           int32_t ref, double loading, double target_rms, int16_t* taps, double* weights, double* gain,
                           double* suppression_db, bool* matrix_refused) {
    *matrix_refused = true;
    const int n = A * K, c = (K - 1) / 2, m = lanes * n, at = ref * K + c;
    // 1. R = P + j Q
    std::vector<double> P((size_t)n * n), Q((size_t)n * n, 0.0);
    const double fr = (double)frames;
    for (int a = 0; a < A; ++a)
        for (int k = 0; k < K; ++k)
            for (int b = 0; b < A; ++b)
                for (int l = 0; l < K; ++l) {
                    const int d = l - k;
                    const size_t at_r = (size_t)(a * K + k) * n + (b * K + l);
                    const int64_t* e = d >= 0 ? rho + ((size_t)(a * A + b) * K + d) * lanes
                                              : rho + ((size_t)(b * A + a) * K - d) * lanes;
                    P[at_r] = (double)e[0] / fr;
                    if (lanes == 2) Q[at_r] = d >= 0 ? (double)e[1] / fr : -((double)e[1] / fr);
                }
    // 2. the loading
    double tr = 0.0;
    for (int i = 0; i < n; ++i) tr += P[(size_t)i * n + i];
    const double ld = (loading * tr) / (double)n;
    // 3. the embedding, its Cholesky factor (in place, lower triangle) and the two triangular solves
    std::vector<double> M((size_t)m * m);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const double p = P[(size_t)i * n + j] + (i == j ? ld : 0.0), q = Q[(size_t)i * n + j];
            M[(size_t)i * m + j] = p;
            if (lanes == 2) {
                M[(size_t)i * m + n + j] = -q;
                M[(size_t)(n + i) * m + j] = q;
                M[(size_t)(n + i) * m + n + j] = p;
            }
        }
    for (int j = 0; j < m; ++j)
        for (int i = j; i < m; ++i) {
            double s = M[(size_t)i * m + j];
            for (int k = 0; k < j; ++k) s -= M[(size_t)i * m + k] * M[(size_t)j * m + k];
            if (i == j) {
                if (!(s > 0)) {
                    sgx_set_error("array design: the covariance matrix is not positive definite at pivot %d (%g): an all-zero "
                                  "record, or streams that repeat each other with no loading", j, s);
                    return SGX_E_ARG;
                }
                M[(size_t)j * m + j] = sqrt(s);
            } else {
                M[(size_t)i * m + j] = s / M[(size_t)j * m + j];
            }
        }
    std::vector<double> y(m), g(m);
    for (int i = 0; i < m; ++i) {
        double s = i == at ? 1.0 : 0.0;
        for (int k = 0; k < i; ++k) s -= M[(size_t)i * m + k] * y[k];
        y[i] = s / M[(size_t)i * m + i];
    }
    for (int i = m - 1; i >= 0; --i) {
        double s = y[i];
        for (int k = i + 1; k < m; ++k) s -= M[(size_t)k * m + i] * g[k];
        g[i] = s / M[(size_t)i * m + i];
    }
    // 4. the constraint
    const double g0 = g[at];
    if (!(isfinite(g0) && g0 > 0)) {
        sgx_set_error("array design: the covariance matrix is not positive definite (the constrained weight came out as %g)", g0);
        return SGX_E_ARG;
    }
    for (int i = 0; i < m; ++i) g[i] = g[i] / g0;
    const double* gr = g.data();
    const double* gi = lanes == 2 ? g.data() + n : nullptr;
    // 5. the output power, with the unloaded R
    double p_out = 0.0;
    for (int i = 0; i < n; ++i) {
        double t_re = 0.0, t_im = 0.0;
        for (int j = 0; j < n; ++j) {
            t_re += P[(size_t)i * n + j] * gr[j];
            if (lanes == 2) {
                t_re -= Q[(size_t)i * n + j] * gi[j];
                t_im += P[(size_t)i * n + j] * gi[j];
                t_im += Q[(size_t)i * n + j] * gr[j];
            }
        }
        p_out += gr[i] * t_re;
        if (lanes == 2) p_out += gi[i] * t_im;
    }
    if (!(isfinite(p_out) && p_out > 0)) {
        sgx_set_error("array design: the covariance matrix is not positive definite (output power %g)", p_out);
        return SGX_E_ARG;
    }
    *matrix_refused = false;
    // 6. .. 9.
    const double gn = target_rms / sqrt(p_out / (double)lanes);
    const double scale = (double)(1 << SGX_ARRAY_SHIFT) * gn;
    long long sum_abs = 0;
    for (int i = 0; i < n; ++i)
        for (int l = 0; l < lanes; ++l) {
            const double h = l == 0 ? gr[i] : -gi[i];
            const double r = nearbyint(scale * h);   // round half to even (the default rounding mode)
            if (!(fabs(r) <= 32512.0)) {
                sgx_set_error("%s: tap %d of antenna %d = %.1f leaves the +-32512 the combiner takes (the gain %g is "
                              "too large: a lower target_rms, or more loading)", where, i % K, i / K, r, gn);
                return SGX_E_ARG;
            }
            taps[i * lanes + l] = (int16_t)r;
            sum_abs += llabs((long long)r);
            if (weights) weights[i * lanes + l] = h;
        }
    if (128 * sum_abs >= (1ll << 31)) {
        sgx_set_error("%s: 128 sum(|re| + |im|) = %lld does not fit the combiner's int32 accumulator", where, 128 * sum_abs);
        return SGX_E_ARG;
    }
    if (gain) *gain = gn;
    if (suppression_db) *suppression_db = 10.0 * log10(P[(size_t)at * n + at] / p_out);
    return SGX_OK;
}

extern "C" int sgx_array_design(const int64_t* rho, int64_t frames, int32_t lanes, int32_t A, int32_t K, int32_t ref,
                                double loading, double target_rms, int16_t* taps, int32_t* shift, double* weights,
                                double* gain, double* suppression_db) {
    const int rc = ar_design_args(lanes, A, K, ref, loading, target_rms);
    if (rc != SGX_OK) return rc;
    if (frames < 1) {
        sgx_set_error("array design: frames = %lld: the statistics of no frame at all", (long long)frames);
        return SGX_E_ARG;
    }
    SGX_CHECK_ARG(rho && taps && shift);
    bool matrix_refused;
    const int rs = ar_design_solve("array design", rho, frames, lanes, A, K, ref, loading, target_rms, taps, weights, gain,
                                   suppression_db, &matrix_refused);
    if (rs != SGX_OK) return rs;
    *shift = SGX_ARRAY_SHIFT;
    return SGX_OK;
}

extern "C" int sgx_array_design_blocks(const int64_t* rho_blocks, int64_t n_blocks, int64_t F, int64_t B, int32_t W,
                                       int32_t lanes, int32_t A, int32_t K, int32_t ref, double loading, double target_rms,
                                       int16_t* taps, int32_t* shift, double* weights, double* gain, double* suppression_db,
                                       uint8_t* status) {
    const int rc = ar_design_args(lanes, A, K, ref, loading, target_rms);
    if (rc != SGX_OK) return rc;
    if (B < 1 || B % SGX_ARRAY_BLOCK_UNIT) {
        sgx_set_error("array design: B = %lld frames is no positive multiple of %d", (long long)B, SGX_ARRAY_BLOCK_UNIT);
        return SGX_E_ARG;
    }
    if (W < 1 || W > SGX_ARRAY_MAX_WINDOW || (W & 1) == 0) {
        sgx_set_error("array design: W = %d is not an odd number of blocks in 1 .. %d", (int)W, SGX_ARRAY_MAX_WINDOW);
        return SGX_E_ARG;
    }
    if (F < 1) {
        sgx_set_error("array design: F = %lld frames: the statistics of no frame at all", (long long)F);
        return SGX_E_ARG;
    }
    if (n_blocks < 1 || n_blocks > SGX_ARRAY_MAX_BLOCKS || n_blocks != (F + B - 1) / B) {
        sgx_set_error("array design: n_blocks = %lld is not the ceil(F / B) = %lld blocks of F = %lld frames, or more than %d",
                      (long long)n_blocks, (long long)((F + B - 1) / B), (long long)F, SGX_ARRAY_MAX_BLOCKS);
        return SGX_E_ARG;
    }
    SGX_CHECK_ARG(rho_blocks && taps && shift);

    const size_t n_val = (size_t)A * A * K * lanes, n_tap = (size_t)A * K * lanes;
    const int64_t h = (W - 1) / 2;
    std::vector<int64_t> rho(n_val);
    std::vector<uint8_t> held((size_t)n_blocks);
    int64_t first = -1;      // the first block that was designed
    char where[64];
    for (int64_t j = 0; j < n_blocks; ++j) {
        const int64_t lo = j - h > 0 ? j - h : 0, hi = j + h + 1 < n_blocks ? j + h + 1 : n_blocks;
        memcpy(rho.data(), rho_blocks + (size_t)lo * n_val, n_val * sizeof(int64_t));
        for (int64_t w = lo + 1; w < hi; ++w) {
            const int64_t* r = rho_blocks + (size_t)w * n_val;
            for (size_t i = 0; i < n_val; ++i) rho[i] += r[i];
        }
        const int64_t frames = (hi * B < F ? hi * B : F) - lo * B;
        snprintf(where, sizeof where, "array design, block %lld", (long long)j);
        bool matrix_refused;
        const int rs = ar_design_solve(where, rho.data(), frames, lanes, A, K, ref, loading, target_rms, taps + (size_t)j * n_tap,
                                       weights ? weights + (size_t)j * n_tap : nullptr, gain ? gain + j : nullptr,
                                       suppression_db ? suppression_db + j : nullptr, &matrix_refused);
        if (rs != SGX_OK && !matrix_refused) return rs;
        held[(size_t)j] = rs != SGX_OK;
        if (rs == SGX_OK && first < 0) first = j;
    }
    if (first < 0) return SGX_E_ARG;   // (no block has a matrix the design takes: the last one's refusal is the text)
    // a held block takes what the nearest designed block before it got, the leading ones what the first designed block got
    for (int64_t j = 0, from = first; j < n_blocks; ++j) {
        if (!held[(size_t)j]) {
            from = j;
            continue;
        }
        memcpy(taps + (size_t)j * n_tap, taps + (size_t)from * n_tap, n_tap * sizeof(int16_t));
        if (weights) memcpy(weights + (size_t)j * n_tap, weights + (size_t)from * n_tap, n_tap * sizeof(double));
        if (gain) gain[j] = gain[from];
        if (suppression_db) suppression_db[j] = suppression_db[from];
    }
    if (status) memcpy(status, held.data(), (size_t)n_blocks);
    *shift = SGX_ARRAY_SHIFT;
    return SGX_OK;
}
