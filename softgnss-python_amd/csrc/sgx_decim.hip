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
//   * De-interleave: fir_split_planes<P, W> (sgx_fir_dot4.h), D chunks per slot of every plane, XOR 0x80 for offset binary.
//     Lanes write consecutive slots of a plane and, in the filter, read consecutive slots: no bank conflict on either
//     side.  The kernel is templated on (LANES, D), every D from 2 to 16.
//   * Taps are wave-uniform: scalar loads from d_small->fir_taps, [D][Lq / 4] pairs for a real record, [D][3][Lq / 4] for
//     I/Q (re, im, -im).  All phases run over one range of steps, the union of the steps that hold a tap.
//   * The sum over the phases, the rounding and the clip count are the header's (fir_plane_sums), the count's fold the stage
//     counters' (sgx_count.h).
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

    const int ns = (TF + lq) / W;              // slots of a plane image: frames m0 - cq .. m0 + TF + lq - cq
    const long long base = ((long long)blockIdx.x * TF - cq) * P;   // its first byte in the record, a multiple of 16
    fir_split_planes<P, W>(x, base, n, flip, s_img, ns);
    __syncthreads();

    const unsigned long long o0 = (unsigned long long)blockIdx.x * FIR_TILE + 16ull * threadIdx.x;
    unsigned out[4] = {0u, 0u, 0u, 0u};
    unsigned clipped = 0;
    fir_plane_sums<LANES, D>(s_img, ns, taps, lq / 4, q_lo, q_hi, shift, o0, n_out, out, clipped);
    if (o0 + 16 <= n_out) {
        *reinterpret_cast<uint4*>(y + o0) = make_uint4(out[0], out[1], out[2], out[3]);
    } else {
        for (int r = 0; r < 16 && o0 + r < n_out; ++r) y[o0 + r] = (int8_t)((out[r >> 2] >> ((r & 3) * 8)) & 0xFF);
    }
    const unsigned count[1] = {clipped};
    sgx_count_publish<1, FIR_THREADS / 64>(count, counts);
}

// ---- host ------------------------------------------------------------------------------------------------------------------
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
    int rc = fir_check_shift(shift);
    if (rc != SGX_OK) return rc;
    if (flags & ~SGX_DECIM_OFFSET_BINARY) {
        sgx_set_error("bad argument: flags 0x%x holds a bit other than SGX_DECIM_OFFSET_BINARY", (unsigned)flags);
        return SGX_E_ARG;
    }
    SGX_CHECK_ARG(taps);
    // (lanes = 2: the components of the complex taps, so the bound is on sum(|re| + |im|))
    rc = fir_check_taps(taps, lanes * n_taps);
    if (rc != SGX_OK) return rc;
    SGX_CHECK_ARG(c && rec && out);
    SGX_CHECK_ARG(rec->device == c->device);
    if (lanes == 2 && (rec->n & 1)) {
        sgx_set_error("bad argument: an I/Q record (lanes 2) holds whole pairs, not %zu bytes", rec->n);
        return SGX_E_ARG;
    }
    const size_t frames = rec->n / (size_t)lanes;
    const size_t n_out = (frames + (size_t)D - 1) / (size_t)D * (size_t)lanes;
    const unsigned long long tiles = ((unsigned long long)n_out + FIR_TILE - 1) / FIR_TILE;
    rc = sgx_stage_one_launch(tiles, "bad argument: a record of %zu output bytes is beyond one launch of the decimator", n_out);
    if (rc != SGX_OK) return rc;
    rc = sgx_stage_open(c, rec, rec->n);
    if (rc != SGX_OK) return rc;

    // G_p[j] = the tap of phase p at q = j - cq: h[cc - q D - p]
    const int cc = (n_taps - 1) / 2, cq = dc_cq(lanes, D, cc), lq = dc_lq(lanes, D, cc), pairs = dc_tap_pairs(lanes, D, cc);
    uint2* g = fir_tap_image(c, pairs);
    FirLaunch l(c, rec, tiles, n_out, shift, (flags & SGX_DECIM_OFFSET_BINARY) != 0);
    l.lq = lq, l.cq = cq;
    for (int p = 0; p < D; ++p)
        l.steps = fir_pack_image(taps, n_taps, lanes, 16 / lanes, g + (size_t)p * (pairs / D), lq / 4,
                                 [&](int j) { return cc - (j - cq) * D - p; }, l.steps);

    SgxStage st(SGX_STAGE_DECIM, l.grid, "decimation kernel failed: %s", out, n_out);
    st.up = {c->d_small->fir_taps, g, (size_t)pairs * sizeof(uint2)};
    return fir_run_counted(c, st, l, clipped, [&] {
        fir_dispatch<1, 2>(lanes, [&](auto la) {
            fir_dispatch<2, 16>(D, [&](auto d) {
                decim_kernel<decltype(la)::value, decltype(d)::value><<<l.grid, FIR_THREADS, 0, l.st>>>(
                    l.x, l.y, l.n, l.n_out, l.taps, l.lq, l.cq, l.steps.lo, l.steps.hi, l.shift, l.flip, l.counts);
            });
        });
    });
}
