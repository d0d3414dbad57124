// The arithmetic of one Welch segment of sgx_probe_waterfall (sgx_waterfall.hip), cut into the work items its kernel hands
// to the lanes of a workgroup between two barriers.  Each item reads and writes elements of the segment's buffer that no
// other item of the same step touches, so a host loop over the items of a step, step by step, computes what the kernel
// does: the functions compile for both sides.
//
// A real segment of N samples is packed as the M = N / 2 point complex sequence z[m] = y[2m] + i y[2m+1] (y = window x
// detrended sample), transformed in place - decimation in time on the bit-reversed sequence, radix 16 behind at most one radix-2
// and one radix-4 step (wf_step) - and split into the N / 2 + 1 bins of the real transform on the way out.
// tw[t] = W_N^t = (cos, -sin)(2 pi t / N), t < M: the twiddles of every step, the split and, by its real part, the window.
#pragma once
#include "sgx_internal.h"

#define WF_HD __host__ __device__ __forceinline__

#define WF_MIN_SEGMENT 256
#define WF_MAX_SEGMENT 16384

WF_HD unsigned wf_bitrev(unsigned v, int bits) {
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0f0f0f0fu) | ((v & 0x0f0f0f0fu) << 4);
    v = ((v >> 8) & 0x00ff00ffu) | ((v & 0x00ff00ffu) << 8);
    v = (v >> 16) | (v << 16);
    return v >> (32 - bits);
}

WF_HD cplx wf_mul(cplx a, cplx b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
WF_HD cplx wf_add(cplx a, cplx b) { return make_double2(a.x + b.x, a.y + b.y); }
WF_HD cplx wf_sub(cplx a, cplx b) { return make_double2(a.x - b.x, a.y - b.y); }

// Periodic Hamming window 0.54 - 0.46 cos(2 pi i / N), i < N = 2 M, from the table: cos(2 pi (i - M) / N) = -cos(2 pi i / N)
WF_HD double wf_window(const cplx* tw, int M, int i) { return 0.54 - 0.46 * (i < M ? tw[i].x : -tw[i - M].x); }

// Packing, item m < M: z[m] to its bit-reversed place.  sum: the exact integer sum of the segment; the detrended sample
// (N x - sum) / N is an exact integer over a power of two, so a constant segment gives exactly 0.
WF_HD void wf_pack_item(cplx* buf, const int8_t* seg, const cplx* tw, int M, int log2m, int sum, int m) {
    const int N = 2 * M;
    const double inv_n = 1.0 / (double)N;
    const double d0 = (double)(N * (int)seg[2 * m] - sum) * inv_n;
    const double d1 = (double)(N * (int)seg[2 * m + 1] - sum) * inv_n;
    buf[wf_bitrev((unsigned)m, log2m)] = make_double2(wf_window(tw, M, 2 * m) * d0, wf_window(tw, M, 2 * m + 1) * d1);
}

// The radix-2 step in front (log2 M odd), item j < M / 2: the pair (2j, 2j + 1), twiddle 1
WF_HD void wf_radix2_item(cplx* buf, int j) {
    const cplx a = buf[2 * j], b = buf[2 * j + 1];
    buf[2 * j] = wf_add(a, b);
    buf[2 * j + 1] = wf_sub(a, b);
}

// Two radix-2 steps in registers on four elements a span apart (x0 .. x3 in the order they lie): w1 = W_2h^j, w2 = W_4h^j
// for the element j of a block of h; W_4h^(j+h) = -i W_4h^j
WF_HD void wf_bfly4(cplx& x0, cplx& x1, cplx& x2, cplx& x3, cplx w1, cplx w2) {
    const cplx b = wf_mul(w1, x1), d = wf_mul(w1, x3);
    const cplx a1 = wf_add(x0, b), b1 = wf_sub(x0, b);
    const cplx c1 = wf_mul(w2, wf_add(x2, d)), t = wf_mul(w2, wf_sub(x2, d));
    const cplx d1 = make_double2(t.y, -t.x);
    x0 = wf_add(a1, c1);
    x2 = wf_sub(a1, c1);
    x1 = wf_add(b1, d1);
    x3 = wf_sub(b1, d1);
}

// A radix-4 step at span h (blocks of h become blocks of 4 h; log2h = log2 h), item q < M / 4: the elements base,
// base + h, base + 2h, base + 3h
WF_HD void wf_radix4_item(cplx* buf, const cplx* tw, int M, int h, int log2h, int q) {
    const int j = q & (h - 1);
    const int base = ((q >> log2h) << (log2h + 2)) + j;
    cplx a = buf[base], b = buf[base + h], c = buf[base + 2 * h], d = buf[base + 3 * h];
    wf_bfly4(a, b, c, d, tw[j * (M >> log2h)], tw[j * (M >> (log2h + 1))]);
    buf[base] = a;
    buf[base + h] = b;
    buf[base + 2 * h] = c;
    buf[base + 3 * h] = d;
}

// A radix-16 step at span h (blocks of h become blocks of 16 h), item q < M / 16: two radix-4 steps in registers on the
// elements base + r h, r < 16 - half the barriers and half the trips through the buffer of two radix-4 steps.  The first
// works on r = 4g .. 4g + 3 at span h, the same twiddles for every g; the second on r = u, u + 4, u + 8, u + 12 at span
// 4 h, where the element is j + u h of its block.
WF_HD void wf_radix16_item(cplx* buf, const cplx* tw, int M, int h, int log2h, int q) {
    const int j = q & (h - 1);
    const int base = ((q >> log2h) << (log2h + 4)) + j;
    cplx x[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) x[r] = buf[base + r * h];
    {
        const cplx w1 = tw[j * (M >> log2h)], w2 = tw[j * (M >> (log2h + 1))];
#pragma unroll
        for (int g = 0; g < 4; ++g) wf_bfly4(x[4 * g], x[4 * g + 1], x[4 * g + 2], x[4 * g + 3], w1, w2);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int j4 = j + u * h;                    // < 4 h
        wf_bfly4(x[u], x[u + 4], x[u + 8], x[u + 12], tw[j4 * (M >> (log2h + 2))], tw[j4 * (M >> (log2h + 3))]);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) buf[base + r * h] = x[r];
}

// The steps of a transform of M = 2^log2m points in the order they run: a radix-2 step where log2m is odd, a radix-4 step
// where what is left is no power of 16, then radix-16 steps.  step() returns the radix of step s (0: done) and its span.
WF_HD int wf_step(int log2m, int s, int* log2h) {
    int done = 0;
    if (log2m & 1) {
        if (s == 0) { *log2h = 0; return 2; }
        done = 1, --s;
    }
    if ((log2m - done) & 2) {
        if (s == 0) { *log2h = done; return 4; }
        done += 2, --s;
    }
    *log2h = done + 4 * s;
    return *log2h < log2m ? 16 : 0;
}

// The real-input split, item k <= M: |X[k]|^2 with X[k] = (Z[k] + conj Z[M-k]) / 2 - (i / 2) W_N^k (Z[k] - conj Z[M-k]),
// Z[M] = Z[0], W_N^M = -1
WF_HD double wf_split_item(const cplx* buf, const cplx* tw, int M, int k) {
    const cplx z = buf[k & (M - 1)], y = buf[(M - k) & (M - 1)];
    const cplx e = make_double2(0.5 * (z.x + y.x), 0.5 * (z.y - y.y));
    const cplx o = make_double2(0.5 * (z.y + y.y), -0.5 * (z.x - y.x));      // -(i / 2) (z - conj y)
    const cplx w = k < M ? tw[k] : make_double2(-1.0, 0.0);
    const cplx x = wf_add(e, wf_mul(w, o));
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
WF_HD void wf_locate(const WfGeom& g, long long seg, long long* slice, long long* start) {
    const long long j = seg / g.k_full;
    *slice = j;
    *start = j * g.S + (seg - j * g.k_full) * (long long)g.step;
}
WF_HD long long wf_slice_segments(const WfGeom& g, long long j) { return j < g.n_full ? g.k_full : g.k_last; }
