// The integer FIR core of the stages that rewrite a whole resident int8 record: the notch (sgx_filter.hip), the I/Q ->
// real-IF converter (sgx_iq.hip), the decimator (sgx_decim.hip), the resampler (sgx_resamp.hip) and the antenna combiner
// (sgx_array.hip).  Each piece is here once; the files keep their tap-image layouts and their kernels.  Who takes what:
//   the chunk load, fir_steps, fir_round_clip, the tap checks and the tap-image packer      all five
//   fir_split_planes (the register de-interleave into plane images)                          decimator, resampler
//   fir_plane_sums (the sum over planes, the rounding, the clip count, the packing)          decimator, combiner
//   FirLaunch, fir_dispatch, fir_check_shift, fir_run_counted (the clip count of a launch)   decimator, resampler, combiner
//
// Formulation: v_dot4_i32_i8 on byte windows (DESIGN.md section 4.11 says why not the int8 matrix cores).  Each int16 tap
// is two signed bytes, h = 256 hi + lo; the two byte filters accumulate separately and are combined as 256 acc_hi + acc_lo.
// All arithmetic is modulo 2^32 and the contracts bound the true sum inside int32, so any order - and a partial sum that
// wraps - gives the exact result.  A workgroup of FIR_THREADS lanes makes FIR_TILE consecutive output bytes, 16 per lane,
// from an LDS image of W-byte slots whose first byte lies on a multiple of 16 in the record.
// Bounds: global reads are guarded per 16-byte chunk (bytes outside [0, N) are zero, never read); stores are guarded per
// lane (a 16-byte store only when all 16 outputs exist, byte stores on the record's last partial group).  The store is
// written out in each kernel: behind a helper the compiler packs the bytes before the branch and unpacks them again for
// the byte stores, a different epilogue from the one the kernels have always had.
// Clipped outputs: counted per lane on the value before the clip; the kernel hands its lanes' counts to sgx_count_publish
// (sgx_count.h), counter 0 of the stage counters.
#pragma once
#include <limits.h>

#include <type_traits>

#include "sgx_count.h"
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

// The register transposes (fir_split_planes, the resampler's store, the combiner's ar_load_planes): bytes (a >> 2 . a & 3)
// and (b >> 2 . b & 3) of raw[] as bytes 0 and 1 of the result
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

// The register de-interleave of the decimator and the resampler.  The record's bytes from `base` (a multiple of 16) are one
// stream of P planes, plane pp holding the bytes i P + pp.  Slots [0, ns) of the P plane images, image pp at s_img + pp ns:
// a lane loads the W P / 16 consecutive chunks that hold slot s of EVERY plane (guarded per chunk) and transposes them in
// registers - output dword g of plane pp takes bytes (4 g + j) P + pp, three v_perm_b32 with constant selectors.
template <int P, int W>
__device__ __forceinline__ void fir_split_planes(const int8_t* __restrict__ x, long long base, unsigned long long n,
                                                 unsigned flip, typename FirSlot<W>::type* s_img, int ns) {
    constexpr int C = W * P / 16;   // chunks of a slot of every plane
    for (int s = threadIdx.x; s < ns; s += FIR_THREADS) {
        unsigned raw[4 * C];
#pragma unroll
        for (int d = 0; d < C; ++d) {
            const uint4 v = fir_load_chunk(x, base + (long long)s * (16 * C) + 16 * d, n, flip);
            raw[4 * d] = v.x, raw[4 * d + 1] = v.y, raw[4 * d + 2] = v.z, raw[4 * d + 3] = v.w;
        }
#pragma unroll
        for (int pp = 0; pp < P; ++pp) {
            unsigned o[W / 4];
#pragma unroll
            for (int g = 0; g < W / 4; ++g) {
                const unsigned lo = fir_pick2(raw, (4 * g) * P + pp, (4 * g + 1) * P + pp);
                const unsigned hi = fir_pick2(raw, (4 * g + 2) * P + pp, (4 * g + 3) * P + pp);
                o[g] = __builtin_amdgcn_perm(hi, lo, 0x05040100u);
            }
            if constexpr (W == 16) {
                s_img[pp * ns + s] = make_uint4(o[0], o[1], o[2], o[3]);
            } else {
                s_img[pp * ns + s] = make_uint2(o[0], o[1]);
            }
        }
    }
}

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
        // (the slot behind the lane's own as a pointer: written s_x[threadIdx.x + q + 1], a caller that runs several filters
        // in a loop keeps the sums threadIdx.x + q_lo and threadIdx.x + 1 in registers across it, two more than this way)
        const typename FirSlot<W>::type* next = s_x + threadIdx.x + 1;
        typename FirSlot<W>::type lo, hi = next[q_lo - 1];   // the window: two consecutive slots
        for (int q = q_lo; q < q_hi; ++q) {
            lo = hi;
            hi = next[q];
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

// The 16 output bytes of a lane of the decimator and the combiner, packed into out[], and how many of those below n_out
// lay outside [-127, 127] in front of the clip, added to `clipped`.  The sums run over GROUPS plane groups of `pitch`
// slots per plane, group p with its tap images of `img` pairs each.  LANES 1: a group is one plane and one image, 16 real
// outputs.  LANES 2: a group is an I plane and a Q plane with the images re, im, -im; 8 complex outputs, interleaved:
//   Re = sum_p (re_p * I_p - im_p * Q_p),   Im = sum_p (re_p * Q_p + im_p * I_p)
// o0: the lane's first output byte.
template <int LANES, int GROUPS>
__device__ __forceinline__ void fir_plane_sums(const typename FirSlot<16 / LANES>::type* s_img, int pitch,
                                               const uint2* __restrict__ taps, int img, int q_lo, int q_hi,
                                               int shift, unsigned long long o0, unsigned long long n_out, unsigned (&out)[4],
                                               unsigned& clipped) {
    typedef typename FirSlot<16 / LANES>::type slot_t;
    const long long rnd = shift ? (1ll << (shift - 1)) : 0ll;
    if constexpr (LANES == 1) {
        int tot[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) tot[r] = 0;
#pragma unroll 1
        for (int p = 0; p < GROUPS; ++p) {
            int sum[16];
            fir_steps<16>(s_img + p * pitch, taps + p * img, q_lo, q_hi, sum);
#pragma unroll
            for (int r = 0; r < 16; ++r) tot[r] = (int)((unsigned)tot[r] + (unsigned)sum[r]);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long long v = ((long long)tot[r] + rnd) >> shift;
            clipped += (o0 + r < n_out && (v < -127 || v > 127)) ? 1u : 0u;
            out[r >> 2] |= fir_round_clip(tot[r], false, rnd, shift) << ((r & 3) * 8);
        }
    } else {
        int tot_i[8], tot_q[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) tot_i[r] = tot_q[r] = 0;
#pragma unroll 1
        for (int p = 0; p < GROUPS; ++p) {
            const slot_t* s_i = s_img + (2 * p) * pitch;
            const slot_t* s_q = s_img + (2 * p + 1) * pitch;
            const uint2* g_re = taps + (3 * p) * img;
            const uint2* g_im = g_re + img;
            const uint2* g_nim = g_im + img;
            int a[8], b[8];
            fir_steps<8>(s_i, g_re, q_lo, q_hi, a);
            fir_steps<8>(s_q, g_nim, q_lo, q_hi, b);
#pragma unroll
            for (int r = 0; r < 8; ++r) tot_i[r] = (int)((unsigned)tot_i[r] + (unsigned)a[r] + (unsigned)b[r]);
            fir_steps<8>(s_q, g_re, q_lo, q_hi, a);
            fir_steps<8>(s_i, g_im, q_lo, q_hi, b);
#pragma unroll
            for (int r = 0; r < 8; ++r) tot_q[r] = (int)((unsigned)tot_q[r] + (unsigned)a[r] + (unsigned)b[r]);
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const long long vi = ((long long)tot_i[r] + rnd) >> shift, vq = ((long long)tot_q[r] + rnd) >> shift;
            // (n_out is even: a pair exists whole or not at all)
            if (o0 + 2 * r < n_out) clipped += ((vi < -127 || vi > 127) ? 1u : 0u) + ((vq < -127 || vq > 127) ? 1u : 0u);
            const unsigned e = fir_round_clip(tot_i[r], false, rnd, shift), o = fir_round_clip(tot_q[r], false, rnd, shift);
            out[r >> 1] |= (e | (o << 8)) << ((r & 1) * 16);
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
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

// The steps [lo, hi) of a tap image that hold a tap other than zero; none: 0, 0
struct FirSteps {
    int lo = 0, hi = 0;
};

// One filter into its tap image(s), which are zero there.  Position j of the image, 0 <= j < 4 img, takes tap k_of(j) of
// `taps` where that lies in [0, n_taps).  lanes 1: real taps, one image at g.  lanes 2: complex taps (re, im interleaved),
// the images re, im, -im of `img` pairs each from g.  W: the bytes of a step.  Returns `steps` grown by the steps that took
// a tap other than zero.
template <typename KOf>
static inline FirSteps fir_pack_image(const int16_t* taps, int n_taps, int lanes, int W, uint2* g, int img, KOf k_of,
                                      FirSteps steps = FirSteps()) {
    if (steps.hi == 0) steps.lo = INT_MAX;
    for (int j = 0; j < 4 * img; ++j) {
        const int k = k_of(j);
        if (k < 0 || k >= n_taps) continue;
        const int re = taps[lanes * k], im = lanes == 2 ? taps[2 * k + 1] : 0;
        if (re == 0 && im == 0) continue;
        if (re) fir_pack_tap(g, j, re);
        if (im) fir_pack_tap(g + img, j, im), fir_pack_tap(g + 2 * img, j, -im);
        if (j / W < steps.lo) steps.lo = j / W;
        if (j / W + 1 > steps.hi) steps.hi = j / W + 1;
    }
    if (steps.hi == 0) steps.lo = 0;   // no tap at all: no step
    return steps;
}

// The refusal of the shift that the decimator, the resampler and the combiner share (no device needed)
static inline int fir_check_shift(int32_t shift) {
    if (shift >= 0 && shift <= 30) return SGX_OK;
    sgx_set_error("bad argument: shift %d lies outside 0 .. 30", (int)shift);
    return SGX_E_ARG;
}

// The arguments of a launch of the decimator, the resampler or the combiner; a kernel takes the ones it has
struct FirLaunch {
    hipStream_t st;
    unsigned grid;
    const int8_t* x;
    int8_t* y = nullptr;           // the new record: set by fir_run_counted
    unsigned long long n, n_out;
    const uint2* taps;             // the stage's upload of the tap staging area, unless the stage sets its own
    int M = 0, lq = 0, cq = 0;     // (resampler; decimator and resampler: the length and the origin of a sub-filter image)
    FirSteps steps;
    int shift;
    unsigned flip;                 // 0x80808080: the input is offset binary
    unsigned long long* counts = nullptr;
    unsigned tpb = 0;              // block combiner: tiles of a block; 0: one set of taps
    FirLaunch(sgx_ctx* c, const sgx_if* rec, unsigned long long tiles, unsigned long long n_out_, int shift_, bool offset_binary)
        : st(c->stream), grid((unsigned)tiles), x(rec->d), n((unsigned long long)rec->n), n_out(n_out_),
          taps(reinterpret_cast<const uint2*>(c->d_small->fir_taps)), shift(shift_), flip(offset_binary ? 0x80808080u : 0u) {}
};

// f(std::integral_constant<int, v>) for v = value in LO .. HI (a value outside is HI: the entry points have refused it):
// the choice of a kernel instantiation from a run-time shape
template <int LO, int HI, typename F>
static inline void fir_dispatch(int value, F&& f) {
    if constexpr (LO < HI) {
        if (value != LO) return fir_dispatch<LO + 1, HI>(value, f);
    }
    f(std::integral_constant<int, LO>());
}

// sgx_stage_run of a stage whose kernel counts its clipped outputs, counter 0 of the stage counters: launch() runs with l.y
// and l.counts set, and the total goes to *clipped (may be null)
template <typename Launch>
static int fir_run_counted(sgx_ctx* c, SgxStage& st, FirLaunch& l, int64_t* clipped, Launch launch) {
    l.counts = st.count(c);
    const int rc = sgx_stage_run(c, st, [&](sgx_if* r) {
        l.y = r->d;
        launch();
    });
    if (rc == SGX_OK && clipped) *clipped = sgx_stage_count(c, 0);
    return rc;
}
