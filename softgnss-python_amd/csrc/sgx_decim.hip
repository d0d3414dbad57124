// Band selection and decimation by D = 2 .. 16 of a resident int8 record, real or interleaved I/Q (include/sgx.h:
// sgx_if_decimate; contract: tests/decim_spec.py decimate()).  The third user of the dot4 FIR core (sgx_fir_dot4.h).
//
// Polyphase.  The record's bytes are one stream of P planes, plane pp holding the bytes i P + pp: P = D for a real record,
// P = 2 D for I/Q (plane 2 p is I of phase p, plane 2 p + 1 its Q).  With input frame (m + q) D + p = frame m + q of phase p
//   lanes = 1   y[m]   = sum_p sum_q h[c - q D - p] x_p[m + q]
//   lanes = 2   Re w[m] = sum_p (re_p * I_p - im_p * Q_p)[m],   Im w[m] = sum_p (re_p * Q_p + im_p * I_p)[m]
// every term an ordinary FIR on one plane with that phase's sub-filter: fir_steps<W> as it stands, the partial sums added
// modulo 2^32 (the contract bounds the true sum inside int32).  No multiply-accumulate is issued for an output that the
// decimation drops.
//
//   * A workgroup makes FIR_TILE output bytes, 16 per lane: 16 real outputs (W = 16) or 8 complex ones (W = 8, I' and Q'
//     interleaved in registers), one 16-byte store per lane; byte stores only on the record's last partial group.
//   * The sub-filter images share one origin: G_p[j] is the tap at q = j - cq, cq = floor((c + D - 1) / D) rounded up so
//     that cq P is a multiple of 16 (dc_cq), zero where the phase has no tap; Lq (a multiple of W) covers all phases.  The
//     first byte a workgroup needs, (m0 - cq) P, is then a multiple of 16: chunk loads are aligned.
//   * De-interleave: a lane loads the D consecutive 16-byte chunks that hold slot s of EVERY plane (W P = 16 D bytes,
//     guarded per chunk: zero outside [0, N), XOR 0x80 for offset binary), transposes them in registers - output dword g of
//     plane pp takes bytes (4 g + j) P + pp, three v_perm_b32 with selectors that are constants once (LANES, D) is fixed -
//     and writes one W-byte slot to each of the P plane images.  Lanes write consecutive slots of a plane and, in the
//     filter, read consecutive slots: no bank conflict on either side.  The kernel is templated on (LANES, D), every D
//     from 2 to 16.
//   * Taps are wave-uniform: scalar loads from d_small->fir_taps, [D][Lq / 4] pairs for a real record, [D][3][Lq / 4] for
//     I/Q (re, im, -im).  All phases run over one range of steps, the union of the steps that hold a tap.
//   * Clipped outputs: counted per lane on the value before the clip, folded over the wave by shuffles and over the
//     workgroup through LDS, one integer atomic per workgroup into one of DC_COUNT_SLOTS padded slots.
#include "sgx_fir_dot4.h"

#define DC_MAX_C ((SGX_DECIM_MAX_TAPS - 1) / 2)

// The halo in front of a tile, in frames: the reach of the filter to the left, floor((c + D - 1) / D), rounded up to the
// smallest unit a that makes a (lanes D) a multiple of 16 - 16 frames for an odd D, fewer for an even one, so that a short
// sub-filter starts at the head of a step and does not straddle two.  And the padded length of a sub-filter, whole slots.
static constexpr int dc_gcd(int a, int b) { return b ? dc_gcd(b, a % b) : a; }
static constexpr int dc_cq(int lanes, int d, int c) {
    const int a = 16 / dc_gcd(16, lanes * d);
    return ((c + d - 1) / d + a - 1) / a * a;
}
static constexpr int dc_lq(int lanes, int d, int c) {
    const int w = 16 / lanes;
    return (dc_cq(lanes, d, c) + c / d + 1 + w - 1) / w * w;
}
// (hi, lo) pairs of the tap images of one call
static constexpr int dc_tap_pairs(int lanes, int d, int c) { return (lanes == 2 ? 3 : 1) * d * dc_lq(lanes, d, c) / 4; }
static constexpr bool dc_taps_fit() {
    for (int lanes = 1; lanes <= 2; ++lanes)
        for (int d = 2; d <= 16; ++d)
            for (int c = 0; c <= DC_MAX_C; ++c)
                if ((size_t)dc_tap_pairs(lanes, d, c) * sizeof(uint2) > sizeof(SgxSmall::fir_taps)) return false;
    return true;
}
static_assert(dc_taps_fit(), "the sub-filter images of the longest filter fit the tap staging at every D");

template <int LANES, int D>
__global__ __launch_bounds__(FIR_THREADS) void decim_kernel(const int8_t* __restrict__ x, int8_t* __restrict__ y,
                                                            unsigned long long n, unsigned long long n_out,
                                                            const uint2* __restrict__ taps, int lq, int cq, int q_lo,
                                                            int q_hi, int shift, unsigned flip,
                                                            unsigned long long* __restrict__ counts) {
    constexpr int W = 16 / LANES;              // bytes of a slot = outputs of a lane per plane image
    constexpr int P = LANES * D;               // planes
    constexpr int TF = FIR_TILE / LANES;       // frames of a tile
    constexpr int NS_MAX = (TF + dc_lq(LANES, D, DC_MAX_C)) / W;
    typedef typename FirSlot<W>::type slot_t;
    __shared__ slot_t s_img[P * NS_MAX];
    __shared__ unsigned s_cnt[FIR_THREADS / 64];

    const int ns = (TF + lq) / W;              // slots of a plane image: frames m0 - cq .. m0 + TF + lq - cq
    const long long base = ((long long)blockIdx.x * TF - cq) * P;   // its first byte in the record, a multiple of 16
    for (int s = threadIdx.x; s < ns; s += FIR_THREADS) {
        unsigned raw[4 * D];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const uint4 v = fir_load_chunk(x, base + (long long)s * (16 * D) + 16 * d, n, flip);
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
    __syncthreads();

    const long long rnd = shift ? (1ll << (shift - 1)) : 0ll;
    const unsigned long long o0 = (unsigned long long)blockIdx.x * FIR_TILE + 16ull * threadIdx.x;
    unsigned out[4] = {0u, 0u, 0u, 0u};
    unsigned clipped = 0;
    if constexpr (LANES == 1) {
        int tot[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) tot[r] = 0;
#pragma unroll 1
        for (int p = 0; p < D; ++p) {
            int sum[16];
            fir_steps<16>(s_img + p * ns, taps + p * (lq / 4), q_lo, q_hi, sum);
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
        for (int p = 0; p < D; ++p) {
            const slot_t* s_i = s_img + (2 * p) * ns;
            const slot_t* s_q = s_img + (2 * p + 1) * ns;
            const uint2* g_re = taps + (3 * p) * (lq / 4);
            const uint2* g_im = g_re + lq / 4;
            const uint2* g_nim = g_im + lq / 4;
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
    if (o0 + 16 <= n_out) {
        *reinterpret_cast<uint4*>(y + o0) = make_uint4(out[0], out[1], out[2], out[3]);
    } else {
        for (int r = 0; r < 16 && o0 + r < n_out; ++r) y[o0 + r] = (int8_t)((out[r >> 2] >> ((r & 3) * 8)) & 0xFF);
    }

#pragma unroll
    for (int d = 32; d > 0; d >>= 1) clipped += __shfl_down(clipped, d, 64);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = clipped;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned t = 0;
        for (int w = 0; w < FIR_THREADS / 64; ++w) t += s_cnt[w];
        if (t) atomicAdd(&counts[(size_t)(blockIdx.x % DC_COUNT_SLOTS) * DC_COUNT_STRIDE], (unsigned long long)t);
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
struct DcLaunch {
    hipStream_t st;
    unsigned grid;
    const int8_t* x;
    int8_t* y;
    unsigned long long n, n_out;
    const uint2* taps;
    int lq, cq, q_lo, q_hi, shift;
    unsigned flip;
    unsigned long long* counts;
};

template <int LANES, int D> static void dc_launch_ld(const DcLaunch& l) {
    decim_kernel<LANES, D><<<l.grid, FIR_THREADS, 0, l.st>>>(l.x, l.y, l.n, l.n_out, l.taps, l.lq, l.cq, l.q_lo, l.q_hi, l.shift,
                                                             l.flip, l.counts);
}
template <int LANES> static void dc_launch_l(int D, const DcLaunch& l) {
    switch (D) {
        case 2: return dc_launch_ld<LANES, 2>(l);
        case 3: return dc_launch_ld<LANES, 3>(l);
        case 4: return dc_launch_ld<LANES, 4>(l);
        case 5: return dc_launch_ld<LANES, 5>(l);
        case 6: return dc_launch_ld<LANES, 6>(l);
        case 7: return dc_launch_ld<LANES, 7>(l);
        case 8: return dc_launch_ld<LANES, 8>(l);
        case 9: return dc_launch_ld<LANES, 9>(l);
        case 10: return dc_launch_ld<LANES, 10>(l);
        case 11: return dc_launch_ld<LANES, 11>(l);
        case 12: return dc_launch_ld<LANES, 12>(l);
        case 13: return dc_launch_ld<LANES, 13>(l);
        case 14: return dc_launch_ld<LANES, 14>(l);
        case 15: return dc_launch_ld<LANES, 15>(l);
        default: return dc_launch_ld<LANES, 16>(l);
    }
}

extern "C" int sgx_decim_tile(int32_t* tile_bytes) {
    SGX_CHECK_ARG(tile_bytes);
    *tile_bytes = FIR_TILE;
    return SGX_OK;
}

extern "C" int sgx_decim_timing(sgx_ctx* c, float* kernel_ms) {
    SGX_CHECK_ARG(c && kernel_ms);
    *kernel_ms = c->stage_ms[SGX_STAGE_DECIM];
    return SGX_OK;
}

extern "C" int sgx_if_decimate(sgx_ctx* c, const sgx_if* rec, int32_t lanes, const int16_t* taps, int32_t n_taps,
                               int32_t shift, int32_t D, int32_t flags, sgx_if** out, int64_t* clipped) {
    // the filter and the factor first: these refusals need no device
    if (lanes != 1 && lanes != 2) {
        sgx_set_error("bad argument: lanes %d is not 1 (a real record) or 2 (interleaved I/Q)", (int)lanes);
        return SGX_E_ARG;
    }
    if (D < 2 || D > 16) {
        sgx_set_error("bad argument: D = %d lies outside 2 .. 16", (int)D);
        return SGX_E_ARG;
    }
    if (n_taps < 1 || n_taps > SGX_DECIM_MAX_TAPS || (n_taps & 1) == 0) {
        sgx_set_error("bad argument: n_taps = %d is not an odd number in 1 .. %d", (int)n_taps, SGX_DECIM_MAX_TAPS);
        return SGX_E_ARG;
    }
    if (shift < 0 || shift > 30) {
        sgx_set_error("bad argument: shift %d lies outside 0 .. 30", (int)shift);
        return SGX_E_ARG;
    }
    if (flags & ~SGX_DECIM_OFFSET_BINARY) {
        sgx_set_error("bad argument: flags 0x%x holds a bit other than SGX_DECIM_OFFSET_BINARY", (unsigned)flags);
        return SGX_E_ARG;
    }
    SGX_CHECK_ARG(taps);
    // (lanes = 2: the components of the complex taps, so the bound is on sum(|re| + |im|))
    const int bad = fir_check_taps(taps, lanes * n_taps);
    if (bad != SGX_OK) return bad;
    SGX_CHECK_ARG(c && rec && out);
    SGX_CHECK_ARG(rec->device == c->device);
    if (lanes == 2 && (rec->n & 1)) {
        sgx_set_error("bad argument: an I/Q record (lanes 2) holds whole pairs, not %zu bytes", rec->n);
        return SGX_E_ARG;
    }
    const size_t frames = rec->n / (size_t)lanes;
    const size_t n_out = (frames + (size_t)D - 1) / (size_t)D * (size_t)lanes;
    const unsigned long long tiles = ((unsigned long long)n_out + FIR_TILE - 1) / FIR_TILE;
    int rc = sgx_stage_one_launch(tiles, "bad argument: a record of %zu output bytes is beyond one launch of the decimator", n_out);
    if (rc != SGX_OK) return rc;
    rc = sgx_stage_open(c, rec, rec->n);
    if (rc != SGX_OK) return rc;

    // G_p[j] = the tap of phase p at q = j - cq: h[cc - q D - p]
    const int L = n_taps, cc = (L - 1) / 2, W = 16 / lanes;
    const int cq = dc_cq(lanes, D, cc), lq = dc_lq(lanes, D, cc), img = lq / 4, per_phase = lanes == 2 ? 3 : 1;
    uint2* g = fir_tap_image(c, dc_tap_pairs(lanes, D, cc));
    int q_lo = lq / W, q_hi = 0;
    for (int p = 0; p < D; ++p) {
        for (int j = 0; j < lq; ++j) {
            const int k = cc - (j - cq) * D - p;
            if (k < 0 || k >= L) continue;
            uint2* gp = g + (size_t)p * per_phase * img;
            bool any;
            if (lanes == 1) {
                any = taps[k] != 0;
                if (any) fir_pack_tap(gp, j, taps[k]);
            } else {
                const int re = taps[2 * k], im = taps[2 * k + 1];
                any = re != 0 || im != 0;
                if (re) fir_pack_tap(gp, j, re);
                if (im) fir_pack_tap(gp + img, j, im), fir_pack_tap(gp + 2 * img, j, -im);
            }
            if (!any) continue;
            if (j / W < q_lo) q_lo = j / W;
            if (j / W + 1 > q_hi) q_hi = j / W + 1;
        }
    }
    if (q_hi == 0) q_lo = 0;   // no tap at all: no step

    DcLaunch l;
    l.st = c->stream;
    l.grid = (unsigned)tiles;
    l.x = rec->d;
    l.n = (unsigned long long)rec->n, l.n_out = (unsigned long long)n_out;
    l.taps = reinterpret_cast<const uint2*>(c->d_small->fir_taps);
    l.lq = lq, l.cq = cq, l.q_lo = q_lo, l.q_hi = q_hi, l.shift = shift;
    l.flip = (flags & SGX_DECIM_OFFSET_BINARY) ? 0x80808080u : 0u;
    l.counts = c->d_small->decim_clip;
    unsigned long long* h_count = c->h_small->decim_clip;
    SgxStage st(SGX_STAGE_DECIM, l.grid, "decimation kernel failed: %s", out, n_out);
    st.up = {c->d_small->fir_taps, g, (size_t)dc_tap_pairs(lanes, D, cc) * sizeof(uint2)};
    st.count_into(h_count, l.counts, sizeof(SgxSmall::decim_clip));
    rc = sgx_stage_run(c, st, [&](sgx_if* r) {
        l.y = r->d;
        if (lanes == 1) {
            dc_launch_l<1>(D, l);
        } else {
            dc_launch_l<2>(D, l);
        }
    });
    if (rc != SGX_OK) return rc;
    if (clipped) *clipped = sgx_sum_slots(h_count, DC_COUNT_SLOTS, DC_COUNT_STRIDE);
    return SGX_OK;
}
