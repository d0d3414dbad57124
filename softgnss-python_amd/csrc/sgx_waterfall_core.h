// The monitor's own work items on one Welch segment of sgx_probe_waterfall (sgx_waterfall.hip), around the transform of
// sgx_seg_fft.h: the window, the packing in front of it and the real-input split behind it, and the geometry of a window's
// slices and segments.  They compile for both sides, as that header's items do: the kernel hands them to the lanes of a
// workgroup between two barriers, sgx_waterfall_host runs them in a loop.
//
// A real segment of N samples is packed as the M = N / 2 point complex sequence z[m] = y[2m] + i y[2m+1] (y = window x
// detrended sample) at the bit-reversed places, transformed in place (SEG_FORWARD) and split into the N / 2 + 1 bins of the
// real transform on the way out.  tw[t] = W_N^t, t < M (seg_twiddles): the twiddles of every step, the split and, by its
// real part, the window.
#pragma once
#include "sgx_seg_fft.h"

#define WF_MIN_SEGMENT 256
#define WF_MAX_SEGMENT 16384

// Periodic Hamming window 0.54 - 0.46 cos(2 pi i / N), i < N = 2 M, from the table: cos(2 pi (i - M) / N) = -cos(2 pi i / N)
SEG_HD double wf_window(const cplx* tw, int M, int i) { return 0.54 - 0.46 * (i < M ? tw[i].x : -tw[i - M].x); }

// Packing, item m < M: z[m] to its bit-reversed place.  sum: the exact integer sum of the segment; the detrended sample
// (N x - sum) / N is an exact integer over a power of two, so a constant segment gives exactly 0.
SEG_HD void wf_pack_item(cplx* buf, const int8_t* seg, const cplx* tw, int M, int log2m, int sum, int m) {
    const int N = 2 * M;
    const double inv_n = 1.0 / (double)N;
    const double d0 = (double)(N * (int)seg[2 * m] - sum) * inv_n;
    const double d1 = (double)(N * (int)seg[2 * m + 1] - sum) * inv_n;
    buf[seg_bitrev((unsigned)m, log2m)] = make_double2(wf_window(tw, M, 2 * m) * d0, wf_window(tw, M, 2 * m + 1) * d1);
}

// The real-input split, item k <= M: |X[k]|^2 with X[k] = (Z[k] + conj Z[M-k]) / 2 - (i / 2) W_N^k (Z[k] - conj Z[M-k]),
// Z[M] = Z[0], W_N^M = -1
SEG_HD double wf_split_item(const cplx* buf, const cplx* tw, int M, int k) {
    const cplx z = buf[k & (M - 1)], y = buf[(M - k) & (M - 1)];
    const cplx e = make_double2(0.5 * (z.x + y.x), 0.5 * (z.y - y.y));
    const cplx o = make_double2(0.5 * (z.y + y.y), -0.5 * (z.x - y.x));      // -(i / 2) (z - conj y)
    const cplx w = k < M ? tw[k] : make_double2(-1.0, 0.0);
    const cplx x = seg_add(e, seg_mul(w, o));
    return x.x * x.x + x.y * x.y;
}

// The slices and segments of a window of n samples: every kept slice but perhaps the last is full
struct WfGeom {
    long long n, S;              // samples of the window and of a full slice
    long long n_slices, n_full;  // kept slices; those of them that are full
    long long k_full, k_last;    // segments of a full slice and of the last one (= k_full where that is full)
    int N, noverlap, step, log2m;
    int bins, pad;
};
// Segment g of the window, counted through the slices in order: a partial last slice has at most k_full segments, so one
// division serves every slice
SEG_HD void wf_locate(const WfGeom& g, long long seg, long long* slice, long long* start) {
    const long long j = seg / g.k_full;
    *slice = j;
    *start = j * g.S + (seg - j * g.k_full) * (long long)g.step;
}
SEG_HD long long wf_slice_segments(const WfGeom& g, long long j) { return j < g.n_full ? g.k_full : g.k_last; }
