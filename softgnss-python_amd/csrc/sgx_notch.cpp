// Host side of the interference-excision stage: line detection on a one-sided PSD and the closed-form notch design
// (include/sgx.h: sgx_notch_design).  No device.  The operations run in the order tests/notch_spec.py states them
// (-ffp-contract=off), so the line list is the contract's exactly and the taps are its taps wherever no unrounded tap
// sits on a rounding boundary.
#include <math.h>

#include <algorithm>

#include "sgx_internal.h"

namespace {

struct NotchLine {
    int peak;
    double strength, centre_hz, width_hz;
};

const int kHalfWindow = 128;   // bins either side of a bin that its baseline's median is taken over
const int kMergeGap = 2;       // flagged bins this many unflagged bins apart (or closer) belong to one line

// b[i] = median(pxx[max(0, i-128) : min(n, i+129)]); an even count takes the mean of the two middle values
void notch_baseline(const double* pxx, int n, std::vector<double>* b) {
    b->resize((size_t)n);
    std::vector<double> w;
    for (int i = 0; i < n; ++i) {
        const int lo = std::max(0, i - kHalfWindow), hi = std::min(n, i + kHalfWindow + 1);
        w.assign(pxx + lo, pxx + hi);
        std::sort(w.begin(), w.end());
        const size_t m = w.size();
        (*b)[(size_t)i] = (m & 1) ? w[m / 2] : 0.5 * (w[m / 2 - 1] + w[m / 2]);
    }
}

void notch_detect(const double* f, const double* pxx, int n, double threshold_db, double width_hz,
                  std::vector<NotchLine>* out) {
    const double thr = pow(10.0, threshold_db / 10.0);
    std::vector<double> b;
    notch_baseline(pxx, n, &b);
    const double df = (f[1] - f[0]) * 1e6;
    std::vector<NotchLine> found;
    int first = -1, last = -1;
    auto close_run = [&]() {
        if (first < 0) return;
        int peak = first;
        for (int i = first; i <= last; ++i)
            if (pxx[i] > pxx[peak]) peak = i;
        NotchLine ln;
        ln.peak = peak;
        ln.strength = b[(size_t)peak] == 0.0 ? INFINITY : pxx[peak] / b[(size_t)peak];
        ln.centre_hz = f[peak] * 1e6;
        ln.width_hz = std::max(width_hz, (f[last] - f[first]) * 1e6 + 2.0 * df);
        found.push_back(ln);
        first = -1;
    };
    for (int i = 0; i < n; ++i) {
        if (!(pxx[i] > thr * b[(size_t)i])) continue;
        if (first >= 0 && i - last > kMergeGap + 1) close_run();
        if (first < 0) first = i;
        last = i;
    }
    close_run();
    if ((int)found.size() > SGX_NOTCH_MAX_LINES) {
        // the strongest, the lower bin first among equals; then back to ascending frequency
        std::stable_sort(found.begin(), found.end(),
                         [](const NotchLine& a, const NotchLine& c) { return a.strength > c.strength; });
        found.resize(SGX_NOTCH_MAX_LINES);
        std::sort(found.begin(), found.end(), [](const NotchLine& a, const NotchLine& c) { return a.peak < c.peak; });
    }
    out->swap(found);
}

}   // namespace

extern "C" int sgx_notch_design(const sgx_settings* s, const double* f_mhz, const double* pxx, int32_t n_bins,
                                double threshold_db, double width_hz, int32_t n_taps, int16_t* taps, int32_t* shift,
                                double* line_hz, double* line_width_hz, int32_t* n_lines) {
    SGX_CHECK_ARG(s && f_mhz && pxx && taps && shift && line_hz && line_width_hz && n_lines);
    SGX_CHECK_ARG(s->samplingFreq > 0 && isfinite(s->samplingFreq));
    SGX_CHECK_ARG(n_bins >= 2);
    SGX_CHECK_ARG(isfinite(threshold_db));
    SGX_CHECK_ARG(isfinite(width_hz) && width_hz > 0);
    SGX_CHECK_ARG(n_taps >= 1 && n_taps <= SGX_FILTER_MAX_TAPS && (n_taps & 1) == 1);
    for (int i = 0; i < n_bins; ++i) {
        if (!isfinite(pxx[i]) || !isfinite(f_mhz[i]) || pxx[i] < 0) {
            sgx_set_error("bad argument: f_mhz / pxx must be finite, pxx >= 0 (bin %d)", i);
            return SGX_E_ARG;
        }
    }
    std::vector<NotchLine> lines;
    notch_detect(f_mhz, pxx, n_bins, threshold_db, width_hz, &lines);

    const double fs = s->samplingFreq;
    const int L = n_taps, c = (L - 1) / 2;
    const int S = SGX_NOTCH_SHIFT;
    std::vector<double> h((size_t)L, 0.0);
    h[(size_t)c] = 1.0;
    for (const NotchLine& ln : lines) {
        for (int k = 0; k < L; ++k) {
            const double m = (double)(k - c);
            const double t = ln.width_hz * m / fs;
            const double sinc = (k == c) ? 1.0 : sin(M_PI * t) / (M_PI * t);
            h[(size_t)k] = h[(size_t)k] - 2.0 * (ln.width_hz / fs) * sinc * cos(2.0 * M_PI * ln.centre_hz * m / fs);
        }
    }
    long long sum_abs = 0;
    for (int k = 0; k < L; ++k) {
        const double win = (L == 1) ? 1.0 : 0.5 - 0.5 * cos(2.0 * M_PI * (double)k / (double)(L - 1));
        const double u = h[(size_t)k] * win * (double)(1 << S);
        const double r = nearbyint(u);   // round half to even (the default rounding mode)
        if (!(fabs(r) <= 32512.0)) {
            sgx_set_error("notch design: tap %d = %.1f leaves the +-32512 the filter takes (lines too wide for the band?)", k, r);
            return SGX_E_ARG;
        }
        taps[k] = (int16_t)r;
        sum_abs += llabs((long long)r);
    }
    if (128 * sum_abs >= (1ll << 31)) {
        sgx_set_error("notch design: 128 sum|h| = %lld does not fit the filter's int32 accumulator", 128 * sum_abs);
        return SGX_E_ARG;
    }
    *shift = S;
    *n_lines = (int32_t)lines.size();
    for (size_t i = 0; i < lines.size(); ++i) {
        line_hz[i] = lines[i].centre_hz;
        line_width_hz[i] = lines[i].width_hz;
    }
    return SGX_OK;
}
