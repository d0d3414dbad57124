// What the two short-time-transform stages share - the record monitor (sgx_waterfall.hip, sgx_waterfall_core.h) and the
// swept-interference excision (sgx_excise.hip, sgx_excise_core.h): the in-place transform of segments that live in LDS, cut
// into the work items a kernel hands to the lanes of a workgroup between two barriers, the loop over its steps, the twiddle
// table, and the staging of a record's bytes in LDS.  Each item reads and writes elements of the buffer that no other item
// of the same step touches, so a host loop over the items of a step, step by step, computes what the kernel does: the
// items compile for both sides, and with -ffp-contract=off both sides execute the same IEEE operations.
//
// A real segment of N samples is packed by its stage as the M = N / 2 point complex sequence z[m] = y[2m] + i y[2m+1] at
// the bit-reversed places and transformed in place - decimation in time, radix 16 behind at most one radix-2 and one
// radix-4 step (seg_step); the stage splits it into the bins of the real transform.
// tw[t] = W_N^t = (cos, -sin)(2 pi t / N), t < M (seg_twiddles): the twiddles of every step and of the splits.
#pragma once
#include <math.h>

#include "sgx_internal.h"

#define SEG_HD __host__ __device__ __forceinline__

SEG_HD unsigned seg_bitrev(unsigned v, int bits) {
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0f0f0f0fu) | ((v & 0x0f0f0f0fu) << 4);
    v = ((v >> 8) & 0x00ff00ffu) | ((v & 0x00ff00ffu) << 8);
    v = (v >> 16) | (v << 16);
    return v >> (32 - bits);
}

SEG_HD cplx seg_mul(cplx a, cplx b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
SEG_HD cplx seg_add(cplx a, cplx b) { return make_double2(a.x + b.x, a.y + b.y); }
SEG_HD cplx seg_sub(cplx a, cplx b) { return make_double2(a.x - b.x, a.y - b.y); }

// The twiddle table of segment length n_seg, on the host
static inline void seg_twiddles(int n_seg, cplx* tw) {
    for (int t = 0; t < n_seg / 2; ++t) {
        const double a = 2.0 * M_PI * (double)t / (double)n_seg;
        tw[t] = make_double2(cos(a), -sin(a));
    }
}

// The radix-2 step in front (log2 M odd), item j < M / 2: the pair (2j, 2j + 1), twiddle 1
SEG_HD void seg_radix2_item(cplx* buf, int j) {
    const cplx a = buf[2 * j], b = buf[2 * j + 1];
    buf[2 * j] = seg_add(a, b);
    buf[2 * j + 1] = seg_sub(a, b);
}

// Two radix-2 steps in registers on four elements a span apart (x0 .. x3 in the order they lie): w1 = W_2h^j, w2 = W_4h^j
// for the element j of a block of h; W_4h^(j+h) = -i W_4h^j
SEG_HD void seg_bfly4(cplx& x0, cplx& x1, cplx& x2, cplx& x3, cplx w1, cplx w2) {
    const cplx b = seg_mul(w1, x1), d = seg_mul(w1, x3);
    const cplx a1 = seg_add(x0, b), b1 = seg_sub(x0, b);
    const cplx c1 = seg_mul(w2, seg_add(x2, d)), t = seg_mul(w2, seg_sub(x2, d));
    const cplx d1 = make_double2(t.y, -t.x);
    x0 = seg_add(a1, c1);
    x2 = seg_sub(a1, c1);
    x1 = seg_add(b1, d1);
    x3 = seg_sub(b1, d1);
}

// A radix-4 step at span h (blocks of h become blocks of 4 h; log2h = log2 h), item q < M / 4: the elements base,
// base + h, base + 2h, base + 3h
SEG_HD void seg_radix4_item(cplx* buf, const cplx* tw, int M, int h, int log2h, int q) {
    const int j = q & (h - 1);
    const int base = ((q >> log2h) << (log2h + 2)) + j;
    cplx a = buf[base], b = buf[base + h], c = buf[base + 2 * h], d = buf[base + 3 * h];
    seg_bfly4(a, b, c, d, tw[j * (M >> log2h)], tw[j * (M >> (log2h + 1))]);
    buf[base] = a;
    buf[base + h] = b;
    buf[base + 2 * h] = c;
    buf[base + 3 * h] = d;
}

// A radix-16 step at span h (blocks of h become blocks of 16 h), item q < M / 16: two radix-4 steps in registers on the
// elements base + r h, r < 16 - half the barriers and half the trips through the buffer of two radix-4 steps.  The first
// works on r = 4g .. 4g + 3 at span h, the same twiddles for every g; the second on r = u, u + 4, u + 8, u + 12 at span
// 4 h, where the element is j + u h of its block.
SEG_HD void seg_radix16_item(cplx* buf, const cplx* tw, int M, int h, int log2h, int q) {
    const int j = q & (h - 1);
    const int base = ((q >> log2h) << (log2h + 4)) + j;
    cplx x[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) x[r] = buf[base + r * h];
    {
        const cplx w1 = tw[j * (M >> log2h)], w2 = tw[j * (M >> (log2h + 1))];
#pragma unroll
        for (int g = 0; g < 4; ++g) seg_bfly4(x[4 * g], x[4 * g + 1], x[4 * g + 2], x[4 * g + 3], w1, w2);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int j4 = j + u * h;                    // < 4 h
        seg_bfly4(x[u], x[u + 4], x[u + 8], x[u + 12], tw[j4 * (M >> (log2h + 2))], tw[j4 * (M >> (log2h + 3))]);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) buf[base + r * h] = x[r];
}

// The steps of a transform of M = 2^log2m points in the order they run: a radix-2 step where log2m is odd, a radix-4 step
// where what is left is no power of 16, then radix-16 steps.  step() returns the radix of step s (0: done) and its span.
SEG_HD int seg_step(int log2m, int s, int* log2h) {
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

// The forward steps of the points / M transforms of M = 2^log2m points whose (packed, bit-reversed) sequences lie one
// behind the other in buf: every step is one pass over the items of ALL of them - item q of a step belongs to transform
// q / (items per transform) - and one BARRIER.  FOR_ITEMS(q, count) is the caller's loop over q < count: a workgroup's lanes
// in a kernel, every q in a host loop.  The monitor is the case points == M.
#define SEG_FORWARD(FOR_ITEMS, BARRIER, buf, tw, M, log2m, points)                                                     \
    for (int seg_s = 0;; ++seg_s) {                                                                                    \
        int seg_log2h = 0;                                                                                             \
        const int seg_radix = seg_step(log2m, seg_s, &seg_log2h);                                                      \
        if (!seg_radix) break;                                                                                         \
        if (seg_radix == 2) {                                                                                          \
            FOR_ITEMS(q, (points) / 2) seg_radix2_item(buf, q);                                                        \
        } else if (seg_radix == 4) {                                                                                   \
            FOR_ITEMS(q, (points) / 4)                                                                                 \
                seg_radix4_item((buf) + ((q >> ((log2m) - 2)) << (log2m)), tw, M, 1 << seg_log2h, seg_log2h,           \
                                q & ((M) / 4 - 1));                                                                  \
        } else {                                                                                                       \
            FOR_ITEMS(q, (points) / 16)                                                                                \
                seg_radix16_item((buf) + ((q >> ((log2m) - 4)) << (log2m)), tw, M, 1 << seg_log2h, seg_log2h,          \
                                 q & ((M) / 16 - 1));                                                                \
        }                                                                                                              \
        BARRIER;                                                                                                       \
    }

#ifdef __HIPCC__
// Bytes lo <= b < hi of a 16-byte granule kept, the others zeroed
__device__ __forceinline__ uint4 seg_keep_bytes(uint4 v, int lo, int hi) {
    unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        unsigned m = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (4 * d + b >= lo && 4 * d + b < hi) m |= 0xffu << (8 * b);
        w[d] &= m;
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// Samples [p, p + count) of the record x of n samples, read ONCE as the aligned 16-byte granules that cover them and left in
// `stage` (LDS, room for (count + 30) / 16 granules); returned: the byte of `stage` at which sample p lies, p & 15.  x starts
// on a granule (hipMalloc's alignment; the caller checks it).  p may lie in front of the record and p + count behind it: a
// granule is loaded only where it holds a sample of the record - it then lies inside the record's allocation and its
// SGX_IF_PAD - and the bytes outside [0, n) are zeroed.  This is the one place of the two stages that reads a record's pad.
// Lane tid of nt; each(c, v): what the caller does with granule c while the lane still holds it; the caller's barrier follows.
template <class Each>
__device__ __forceinline__ int seg_stage(uint4* __restrict__ stage, const int8_t* __restrict__ x, long long n, long long p,
                                         int count, int tid, int nt, Each each) {
    const int a = (int)(p & 15);
    const int granules = (a + count + 15) / 16;
    for (int c = tid; c < granules; c += nt) {
        const long long gs = p - a + 16ll * c;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (gs >= 0 && gs < n) {                                 // (gs is a multiple of 16)
            v = *reinterpret_cast<const uint4*>(x + gs);
            if (gs + 16 > n) v = seg_keep_bytes(v, 0, (int)(n - gs));
        }
        stage[c] = v;
        each(c, v);
    }
    return a;
}
#endif
