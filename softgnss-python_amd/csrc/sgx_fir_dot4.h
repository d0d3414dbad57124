// The integer FIR core of the stages that rewrite a whole resident int8 record: the notch (sgx_filter.hip), the I/Q ->
// real-IF converter (sgx_iq.hip), the decimator (sgx_decim.hip) and the resampler (sgx_resamp.hip).  Each piece is here
// once; the files keep their tap-image layouts and their kernels.
//
// Formulation: v_dot4_i32_i8 on byte windows (DESIGN.md section 4.11 says why not the int8 matrix cores).  Each int16 tap
// is two signed bytes, h = 256 hi + lo; the two byte filters accumulate separately and are combined as 256 acc_hi + acc_lo.
// All arithmetic is modulo 2^32 and the contracts bound the true sum inside int32, so any order - and a partial sum that
// wraps - gives the exact result.  A workgroup of FIR_THREADS lanes makes FIR_TILE consecutive output bytes, 16 per lane,
// from an LDS image of W-byte slots whose first byte lies on a multiple of 16 in the record.
// Bounds: global reads are guarded per 16-byte chunk (bytes outside [0, N) are zero, never read); stores are guarded per
// lane (a 16-byte store only when all 16 outputs exist, byte stores on the record's last partial group).  The store is
// written out in each kernel: behind a helper the compiler packs the bytes before the branch and unpacks them again for
// the byte stores, a different epilogue from the one both kernels have always had.
#pragma once
#include "sgx_stage.h"

#define FIR_THREADS 256
#define FIR_TILE (FIR_THREADS * 16)   // output bytes per workgroup

// Record bytes [a, a + 16) XOR flip (0x80808080 for offset binary, a literal 0 folds away): zero outside [0, n)
__device__ __forceinline__ uint4 fir_load_chunk(const int8_t* __restrict__ x, long long a, unsigned long long n,
                                                unsigned flip) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (a >= 0 && (unsigned long long)a + 16 <= n) {
        v = *reinterpret_cast<const uint4*>(x + a);
        v.x ^= flip, v.y ^= flip, v.z ^= flip, v.w ^= flip;
    } else if (a >= 0 && (unsigned long long)a < n) {
        unsigned w[4] = {0u, 0u, 0u, 0u};
        const int left = (int)(n - (unsigned long long)a);   // 1 .. 15
        for (int b = 0; b < left; ++b) w[b >> 2] |= (((unsigned)(uint8_t)x[a + b]) ^ (flip & 0xFFu)) << ((b & 3) * 8);
        v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    return v;
}

// The register transposes of the decimator and the resampler: bytes (a >> 2 . a & 3) and (b >> 2 . b & 3) of raw[] as bytes 0 and 1 of the result
// (v_perm_b32: selector bytes 0..3 pick from the second operand, 4..7 from the first)
template <int NR>
__device__ __forceinline__ unsigned fir_pick2(const unsigned (&raw)[NR], int a, int b) {
    return __builtin_amdgcn_perm(raw[b >> 2], raw[a >> 2], (unsigned)((a & 3) | ((4 + (b & 3)) << 8)) | 0x0c0c0000u);
}

template <int W> struct FirSlot;
template <> struct FirSlot<8> {
    typedef uint2 type;
    static __device__ __forceinline__ unsigned dword(const uint2& v, int k) { return k ? v.y : v.x; }
};
template <> struct FirSlot<16> {
    typedef uint4 type;
    static __device__ __forceinline__ unsigned dword(const uint4& v, int k) {
        return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w;
    }
};

// W outputs of one lane: sum[r] = sum over steps [q_lo, q_hi) and t < W of g[W q + t] image[W (lane + q) + r + t], modulo
// 2^32.  taps: pairs (hi dword, lo dword), byte j of pair p = g[4 p + j]; wave-uniform, they come in through scalar loads.
// Per step a lane reads ONE new slot (lanes on consecutive slots: conflict-free), forms the 2 W - 4 byte-shifted dwords of
// its 2 W-byte window (every fourth is aligned, the others one v_alignbyte_b32 each) and issues W x W / 4 x 2 dot4.
template <int W>
__device__ __forceinline__ void fir_steps(const typename FirSlot<W>::type* s_x, const uint2* __restrict__ taps, int q_lo,
                                          int q_hi, int (&sum)[W]) {
    constexpr int D = W / 4;   // dwords of a slot
    int acc_hi[W], acc_lo[W];
#pragma unroll
    for (int r = 0; r < W; ++r) acc_hi[r] = acc_lo[r] = 0;
    if (q_lo < q_hi) {
        typename FirSlot<W>::type lo, hi = s_x[threadIdx.x + q_lo];   // the window: two consecutive slots
        for (int q = q_lo; q < q_hi; ++q) {
            lo = hi;
            hi = s_x[threadIdx.x + q + 1];
            unsigned w[2 * D], win[2 * W - 4];   // win[b] = image bytes [W (lane + q) + b, + 4)
#pragma unroll
            for (int k = 0; k < D; ++k) w[k] = FirSlot<W>::dword(lo, k), w[D + k] = FirSlot<W>::dword(hi, k);
#pragma unroll
            for (int b = 0; b < 2 * W - 4; ++b)
                win[b] = (b & 3) ? __builtin_amdgcn_alignbyte(w[(b >> 2) + 1], w[b >> 2], b & 3) : w[b >> 2];
#pragma unroll
            for (int t = 0; t < D; ++t) {
                const uint2 g = taps[D * q + t];   // wave-uniform
#pragma unroll
                for (int r = 0; r < W; ++r) {
                    acc_hi[r] = __builtin_amdgcn_sdot4((int)win[4 * t + r], (int)g.x, acc_hi[r], false);
                    acc_lo[r] = __builtin_amdgcn_sdot4((int)win[4 * t + r], (int)g.y, acc_lo[r], false);
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < W; ++r) sum[r] = (int)(((unsigned)acc_hi[r] << 8) + (unsigned)acc_lo[r]);
}

// The output byte of a sum: clip((+-sum + rnd) >> shift, -127, 127), rnd = 2^(shift - 1) or 0 at shift 0
__device__ __forceinline__ unsigned fir_round_clip(int sum, bool negate, long long rnd, int shift) {
    // (exact: the contract bounds |sum| below 2^31, so the negation cannot overflow; rounding in 64 bits as the contract)
    const long long s = (negate ? -(long long)sum : (long long)sum) + rnd;
    int v = (int)(s >> shift);
    v = v < -127 ? -127 : (v > 127 ? 127 : v);
    return (unsigned)(v & 0xFF);
}

// The refusals of the taps' magnitudes (no device needed): every tap splits into two signed bytes, and the sum stays in int32
static inline int fir_check_taps(const int16_t* taps, int32_t n_taps) {
    long long sum_abs = 0;
    for (int k = 0; k < n_taps; ++k) {
        const int a = taps[k] < 0 ? -(int)taps[k] : (int)taps[k];
        if (a > 32512) {
            sgx_set_error("bad argument: |taps[%d]| = %d > 32512 (a tap must split into two signed bytes)", k, a);
            return SGX_E_ARG;
        }
        sum_abs += a;
    }
    if (128 * sum_abs >= (1ll << 31)) {
        sgx_set_error("bad argument: 128 sum|taps| = %lld >= 2^31 (the int32 accumulator)", 128 * sum_abs);
        return SGX_E_ARG;
    }
    return SGX_OK;
}

// Tap h = 256 hi + lo into position j of a tap image that was zero there
static inline void fir_pack_tap(uint2* g, int j, int h) {
    const int hi = (h + 128) >> 8, lo = h - 256 * hi;
    g[j >> 2].x |= ((unsigned)(hi & 0xFF)) << ((j & 3) * 8);
    g[j >> 2].y |= ((unsigned)(lo & 0xFF)) << ((j & 3) * 8);
}

// The tap image the caller packs: the context's pinned staging area, zeroed over n_pairs (hi, lo) pairs.  The stage's
// upload (sgx_stage.h) takes it to c->d_small->fir_taps, where the kernel reads it.
static inline uint2* fir_tap_image(sgx_ctx* c, int n_pairs) {
    uint2* g = reinterpret_cast<uint2*>(c->h_small->fir_taps);
    memset(g, 0, (size_t)n_pairs * sizeof(uint2));
    return g;
}
