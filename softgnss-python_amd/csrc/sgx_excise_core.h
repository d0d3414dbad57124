// The arithmetic of the swept-interference excision stage (sgx_excise.hip; tests/excise_spec.py is the contract), cut into
// the work items its kernel hands to the lanes of a workgroup between two barriers, around the transform of sgx_seg_fft.h -
// the packing order, butterflies, step rule and twiddle table it shares with the record monitor.  Each item reads and
// writes elements that no other item of the same step touches, so a host loop over the items of a step, step by step,
// computes what the kernel does (sgx_excise_host): the functions compile for both sides, and with -ffp-contract=off both
// sides execute the same IEEE operations.
//
// A segment of N = 2 M samples lives in M complex elements `seg` from the packing to the overlap-add:
//   packed      z[m] = w[2m] x[2m] + i w[2m+1] x[2m+1], at its bit-reversed place
//   transformed Z[k], k < M                                           (the forward steps of sgx_seg_fft.h)
//   split       X[k], 1 <= k < M, the bins of the real transform; seg[0] = (X[0], X[M]), both real
//   unsplit     conj Z'[k] after the cut bins are zeroed, Z' the transform of the packed rebuilt segment
//   swapped     the same at the bit-reversed places
//   transformed M conj z'[m]: the inverse as conjugate, forward steps, conjugate; 1 / M is a power of two
// tw[t] = W_N^t = (cos, -sin)(2 pi t / N), t < M, and win[i] = sin(pi i / N), i < N, come from the plan (ex_tables).
#pragma once
#include "sgx_seg_fft.h"

#define EX_MIN_SEGMENT 64
#define EX_MAX_SEGMENT 1024
#define EX_MAX_PASSES 8
#define EX_TILE_POINTS 4096      // complex elements of a tile: 64 KB of LDS, 8192 / N segments
#define EX_CHUNK 8               // bins one item of a mean adds up; M / EX_CHUNK partial sums per segment
#define EX_PARTS (EX_TILE_POINTS / EX_CHUNK)

// Packing, item m < M: the root-Hann window from the table, no detrend
SEG_HD void ex_pack_item(cplx* seg, const int8_t* x, const double* win, int log2m, int m) {
    seg[seg_bitrev((unsigned)m, log2m)] = make_double2(win[2 * m] * (double)x[2 * m], win[2 * m + 1] * (double)x[2 * m + 1]);
}

// The real-input split in place, item k <= M / 2: the pair X[k], X[M - k] from Z[k], Z[M - k] by the formula of
// the monitor's wf_split_item, X[M - k] = conj(E - W^k O); item 0 leaves (X[0], X[M]), item M / 2 its one bin
SEG_HD void ex_split_item(cplx* seg, const cplx* tw, int M, int k) {
    if (k == 0) {
        const cplx z = seg[0];
        seg[0] = make_double2(z.x + z.y, z.x - z.y);
        return;
    }
    const cplx z = seg[k], y = seg[M - k];
    const cplx e = make_double2(0.5 * (z.x + y.x), 0.5 * (z.y - y.y));
    const cplx o = make_double2(0.5 * (z.y + y.y), -0.5 * (z.x - y.x));      // -(i / 2) (z - conj y)
    const cplx wo = seg_mul(tw[k], o);
    seg[k] = seg_add(e, wo);
    if (k != M - k) seg[M - k] = make_double2(e.x - wo.x, -(e.y - wo.y));
}

SEG_HD double ex_power(cplx x) { return x.x * x.x + x.y * x.y; }

// One pass of the mean, item c < M / EX_CHUNK: the sum and the count of the candidates 1 <= k < M of chunk c that are kept
// - all of them in the first pass, those with P_k <= tm (threshold x the last pass's mean) after it - in ascending k
SEG_HD void ex_sum_item(const cplx* seg, int c, bool all, double tm, double* sum, int* count) {
    double s = 0.0;
    int n = 0;
    for (int k = c * EX_CHUNK; k < (c + 1) * EX_CHUNK; ++k) {
        const double p = ex_power(seg[k]);
        if (k >= 1 && (all || p <= tm)) {
            s += p;
            ++n;
        }
    }
    *sum = s;
    *count = n;
}

// ... and its end, one item per segment: the partial sums in ascending chunk order, threshold x mean.  The count is never
// 0: the smallest kept bin is at most the mean and threshold >= 1.
SEG_HD double ex_fold_item(const double* sum, const int* count, int parts, double threshold) {
    double s = 0.0;
    int n = 0;
    for (int c = 0; c < parts; ++c) {
        s += sum[c];
        n += count[c];
    }
    return threshold * (s / (double)n);
}

// The cut and the inverse of the split in place, item k <= M / 2: the bins of the pair above tm zeroed (returned: how many;
// DC and Nyquist, item 0, never), then with E = (X[k] + conj X[M-k]) / 2, O = conj W^k (X[k] - conj X[M-k]) / 2:
// Z'[k] = E + i O, Z'[M-k] = conj E + i conj O, each left conjugated for the transform that follows
SEG_HD int ex_unsplit_item(cplx* seg, const cplx* tw, int M, double tm, int k) {
    if (k == 0) {
        const cplx x = seg[0];
        seg[0] = make_double2(0.5 * (x.x + x.y), -(0.5 * (x.x - x.y)));
        return 0;
    }
    cplx a = seg[k], b = seg[M - k];
    int cut = 0;
    if (!(ex_power(a) <= tm)) a = make_double2(0.0, 0.0), ++cut;
    if (k == M - k) {                                 // W^k = -i: Z' = conj X, left conjugated
        seg[k] = a;
        return cut;
    }
    if (!(ex_power(b) <= tm)) b = make_double2(0.0, 0.0), ++cut;
    const cplx e = make_double2(0.5 * (a.x + b.x), 0.5 * (a.y - b.y));
    const cplx d = make_double2(0.5 * (a.x - b.x), 0.5 * (a.y + b.y));
    const cplx w = tw[k];
    const cplx o = seg_mul(make_double2(w.x, -w.y), d);
    seg[k] = make_double2(e.x - o.y, -(e.y + o.x));
    seg[M - k] = make_double2(e.x + o.y, -(o.x - e.y));
    return cut;
}

// The bit-reversal the forward steps expect, item m < M: an exchange with the partner above
SEG_HD void ex_swap_item(cplx* seg, int log2m, int m) {
    const int r = (int)seg_bitrev((unsigned)m, log2m);
    if (m < r) {
        const cplx t = seg[m];
        seg[m] = seg[r];
        seg[r] = t;
    }
}

// Sample i < N of a rebuilt segment: the conjugate and the 1 / M of the inverse transform
SEG_HD double ex_sample(const cplx* seg, double inv_m, int i) { return (i & 1) ? -seg[i >> 1].y * inv_m : seg[i >> 1].x * inv_m; }

// The windowed overlap-add, item i < H = M of the hop between two consecutive segments: the second half of the earlier
// segment first, as the contract's accumulator takes them
SEG_HD double ex_ola_item(const cplx* seg, const cplx* next, const double* win, int M, double inv_m, int i) {
    return win[i + M] * ex_sample(seg, inv_m, i + M) + win[i] * ex_sample(next, inv_m, i);
}

// The rounding: clip(floor(o + 1/2), -127, 127); *clipped where the value lay outside in front of the clip
SEG_HD int ex_round_item(double o, bool* clipped) {
    const double q = floor(o + 0.5);
    *clipped = q < -127.0 || q > 127.0;
    return (int)(q < -127.0 ? -127.0 : (q > 127.0 ? 127.0 : q));
}

// The segments and tiles of a record of n samples: a tile holds S = EX_TILE_POINTS / M consecutive segments and owns the
// S - 1 hops between them; the last segment of a tile is the first of the next
struct ExGeom {
    long long n, J, tiles;       // samples, segments (ceil(n / H) + 1), tiles (ceil((J - 1) / (S - 1)))
    int N, M, log2m, S, passes;
    double threshold;
};
// The tile that counts segment j of tile t (its local segment s): the EARLIER of the two that hold a shared one
SEG_HD bool ex_owns(const ExGeom& g, long long t, int s) { return (s > 0 || t == 0) && t * (g.S - 1) + s < g.J; }
