// Interleaved I/Q baseband record -> the equivalent real IF record at twice the rate (include/sgx.h: sgx_if_from_iq,
// sgx_iq_design; contract: tests/iq_spec.py convert(), design()).
//
// The contract interpolates z = I + jQ by 2 (zero-stuffing, FIR h), shifts it up by a quarter of the new rate and keeps
// the real part.  The quarter-rate carrier is 1, j, -1, -j, so with pair index p, c = (L - 1) / 2 and x = 0 outside:
//   y[2p]     =  (-1)^p sum_d h[c - 2d]     I[p + d]      (even outputs see only I and the taps with k = c     mod 2)
//   y[2p + 1] = -(-1)^p sum_d h[c + 1 - 2d] Q[p + d]      (odd outputs see only Q and the taps with k = c + 1 mod 2)
// each rounded, shifted and clipped as sgx_if_filter does: two real polyphase FIRs over the de-interleaved bytes.
//
// The dot4 core is sgx_fir_dot4.h's, on 8-byte slots, once per branch.  Particular to this file:
//   * Both branches are written against one image origin: g_X[j] is the tap of branch X at d = j - cp, cp = floor(c / 2)
//     rounded up to 8, zero where the branch has no tap; Lp (a multiple of 8) covers both.  The first byte a workgroup
//     needs, 2 (p0 - cp), is then a multiple of 16: global loads and the record's 16-byte stores are aligned.
//   * A workgroup makes FIR_TILE output bytes = 2048 pairs.  It loads the tile's bytes plus the halo in 16-byte chunks (8
//     pairs), XORs 0x80 into them for offset binary, splits each chunk IN REGISTERS into 8 I bytes and 8 Q bytes (four
//     v_perm_b32) and writes one 8-byte slot to each of two LDS images.  Lanes write consecutive slots and, in the filter,
//     read consecutive slots (ds_write_b64 / ds_read_b64 over 512 contiguous bytes per wave): no bank conflict on either
//     side - scattering single bytes into the images would put four lanes on every bank.
//   * Lane l owns pairs 8 l .. 8 l + 7.  Per branch and step of 8 taps it reads one slot, forms 12 window dwords (9
//     v_alignbyte_b32) and issues 32 dot4.  A branch runs only over the steps that hold a non-zero tap, so the single-tap
//     branch of a half-band design costs one step.  The 8 + 8 results are interleaved in registers and leave as one
//     16-byte store.
#include <math.h>

#include "sgx_fir_dot4.h"

#define IQ_TILE_PAIRS (FIR_TILE / 2)
#define IQ_MAX_LP SGX_IQ_LP_MAX                                 // 136: cp = 64, d up to 64, rounded up to 8
#define IQ_SLOTS ((IQ_TILE_PAIRS + IQ_MAX_LP) / 8)              // 8-byte slots per image
static_assert(((((SGX_IQ_MAX_TAPS - 1) / 4 + 7) / 8) * 8 + (SGX_IQ_MAX_TAPS + 1) / 4 + 1 + 7) / 8 * 8 <= IQ_MAX_LP,
              "the padded branch length of the longest filter fits the staging area and the LDS images");

// taps: [2][lp / 4] pairs (hi dword, lo dword), the even-output (I) branch first; byte j of dword q = tap g[4 q + j].
// steps: (first, end) step of the I branch in x, y and of the Q branch in z, w.  flip: 0x80808080 for offset binary.
__global__ __launch_bounds__(FIR_THREADS) void iq_to_if_kernel(const int8_t* __restrict__ x, int8_t* __restrict__ y,
                                                               unsigned long long n, const uint2* __restrict__ taps,
                                                               int lp, int cp, int4 steps, int shift, unsigned flip,
                                                               int q_first) {
    __shared__ uint2 s_i[IQ_SLOTS];
    __shared__ uint2 s_q[IQ_SLOTS];
    const unsigned long long n0 = (unsigned long long)blockIdx.x * FIR_TILE;
    const int slots = (IQ_TILE_PAIRS + lp) / 8;
    // image byte i of a component = that component of pair n0 / 2 - cp + i; chunk i holds the pairs of slot i
    for (int i = threadIdx.x; i < slots; i += FIR_THREADS) {
        const uint4 v = fir_load_chunk(x, (long long)n0 - 2ll * cp + 16ll * i, n, flip);
        // v_perm_b32: selector bytes 0..3 pick from the second operand, 4..7 from the first
        const uint2 even = make_uint2(__builtin_amdgcn_perm(v.y, v.x, 0x06040200u), __builtin_amdgcn_perm(v.w, v.z, 0x06040200u));
        const uint2 odd = make_uint2(__builtin_amdgcn_perm(v.y, v.x, 0x07050301u), __builtin_amdgcn_perm(v.w, v.z, 0x07050301u));
        s_i[i] = q_first ? odd : even;
        s_q[i] = q_first ? even : odd;
    }
    __syncthreads();

    int sum_i[8], sum_q[8];
    fir_steps<8>(s_i, taps, steps.x, steps.y, sum_i);
    fir_steps<8>(s_q, taps + lp / 4, steps.z, steps.w, sum_q);

    const long long rnd = shift ? (1ll << (shift - 1)) : 0ll;
    unsigned out[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        // the tile starts on an even pair and a lane on a multiple of 8: (-1)^p = (-1)^r
        const unsigned e = fir_round_clip(sum_i[r], (r & 1) != 0, rnd, shift);
        const unsigned o = fir_round_clip(sum_q[r], (r & 1) == 0, rnd, shift);
        out[r >> 1] |= (e | (o << 8)) << ((r & 1) * 16);
    }
    const unsigned long long o = n0 + 16ull * threadIdx.x;
    if (o + 16 <= n) {
        *reinterpret_cast<uint4*>(y + o) = make_uint4(out[0], out[1], out[2], out[3]);
    } else {
        for (int r = 0; r < 16 && o + r < n; ++r) y[o + r] = (int8_t)((out[r >> 2] >> ((r & 3) * 8)) & 0xFF);
    }
}

extern "C" int sgx_iq_design(int32_t n_taps, int16_t* taps, int32_t* shift) {
    SGX_CHECK_ARG(taps && shift);
    SGX_CHECK_ARG(n_taps >= 1 && n_taps <= SGX_IQ_MAX_TAPS && (n_taps & 1) == 1);
    const int L = n_taps, c = (L - 1) / 2;
    for (int k = 0; k < L; ++k) {
        const int m = k - c;
        // sinc(m / 2): 1 at m = 0, exactly 0 at every other even m, (-1)^((m - 1) / 2) 2 / (pi m) at odd m
        double sinc = 0.0;
        if (m == 0) {
            sinc = 1.0;
        } else if (m & 1) {
            sinc = ((((m - 1) / 2) & 1) ? -1.0 : 1.0) * 2.0 / (M_PI * (double)m);
        }
        const double win = (L == 1) ? 1.0 : 0.5 - 0.5 * cos(2.0 * M_PI * (double)k / (double)(L - 1));
        taps[k] = (int16_t)nearbyint((double)(1 << SGX_IQ_SHIFT) * sinc * win);   // round half to even (the default mode)
    }
    *shift = SGX_IQ_SHIFT;
    return SGX_OK;
}

extern "C" int sgx_iq_tile(int32_t* tile_bytes) {
    SGX_CHECK_ARG(tile_bytes);
    *tile_bytes = FIR_TILE;
    return SGX_OK;
}

extern "C" int sgx_if_from_iq(sgx_ctx* c, const sgx_if* iq_bytes, const int16_t* taps, int32_t n_taps, int32_t shift,
                              int32_t flags, sgx_if** out) {
    // the taps and the flags first: these refusals need no device
    SGX_CHECK_ARG(taps);
    SGX_CHECK_ARG(n_taps >= 1 && n_taps <= SGX_IQ_MAX_TAPS && (n_taps & 1) == 1);
    SGX_CHECK_ARG(shift >= 0 && shift <= 30);
    SGX_CHECK_ARG((flags & ~(SGX_IQ_Q_FIRST | SGX_IQ_OFFSET_BINARY)) == 0);
    const int bad = fir_check_taps(taps, n_taps);
    if (bad != SGX_OK) return bad;
    SGX_CHECK_ARG(c && iq_bytes && out);
    SGX_CHECK_ARG(iq_bytes->device == c->device);
    if (iq_bytes->n & 1) {
        sgx_set_error("bad argument: an I/Q record holds whole pairs, not %zu bytes", iq_bytes->n);
        return SGX_E_ARG;
    }
    int rc = sgx_stage_open(c, iq_bytes, iq_bytes->n);
    if (rc != SGX_OK) return rc;
    const unsigned long long blocks = ((unsigned long long)iq_bytes->n + FIR_TILE - 1) / FIR_TILE;
    rc = sgx_stage_one_launch(blocks, "record of %zu bytes is beyond one launch of the I/Q converter", iq_bytes->n);
    if (rc != SGX_OK) return rc;

    // g_X[j] = the tap of branch X at d = j - cp: h[cc - 2 d] for the even outputs, h[cc + 1 - 2 d] for the odd ones
    const int L = n_taps, cc = (L - 1) / 2;
    const int cp = ((cc / 2 + 7) / 8) * 8;
    const int lp = ((cp + (cc + 1) / 2 + 1 + 7) / 8) * 8;
    uint2* g = fir_tap_image(c, 2 * lp / 4);
    FirSteps br[2];   // (a branch without a tap: no step)
    for (int b = 0; b < 2; ++b)
        br[b] = fir_pack_image(taps, L, 1, 8, g + b * (lp / 4), lp / 4, [&](int j) { return cc + b - 2 * (j - cp); });
    const int4 steps = make_int4(br[0].lo, br[0].hi, br[1].lo, br[1].hi);
    const uint2* d_taps = reinterpret_cast<const uint2*>(c->d_small->fir_taps);
    SgxStage st(SGX_STAGE_IQ, (unsigned)blocks, "I/Q conversion kernel failed: %s", out, iq_bytes->n);
    st.up = {c->d_small->fir_taps, g, (size_t)(2 * lp / 4) * sizeof(uint2)};
    return sgx_stage_run(c, st, [&](sgx_if* r) {
        iq_to_if_kernel<<<st.grid, FIR_THREADS, 0, c->stream>>>(
            iq_bytes->d, r->d, (unsigned long long)iq_bytes->n, d_taps, lp, cp, steps, shift,
            (flags & SGX_IQ_OFFSET_BINARY) ? 0x80808080u : 0u, (flags & SGX_IQ_Q_FIRST) ? 1 : 0);
    });
}

extern "C" int sgx_iq_timing(sgx_ctx* c, float* kernel_ms) {
    SGX_CHECK_ARG(c && kernel_ms);
    *kernel_ms = c->stage_ms[SGX_STAGE_IQ];
    return SGX_OK;
}
