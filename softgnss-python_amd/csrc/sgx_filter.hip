// Zero-phase integer FIR over a whole int8 record (include/sgx.h: sgx_if_filter; contract: tests/notch_spec.py apply()).
//
//   y[n] = clip((sum_k h[k] x[n + c - k] + rnd) >> S, -127, 127),  c = (L - 1) / 2,  x = 0 outside the record
//
// The dot4 core is sgx_fir_dot4.h's, on 16-byte slots.  Particular to this file is the tap image: the taps are reversed
// (g[j] = h[L-1-j]: y[n] = sum_j g[j] x[n - c + j]) and e = (-c) mod 16 zero taps are put in front, so that the first sample
// a workgroup needs, n0 - c - e, is a multiple of 16: global loads, LDS reads and the record's 16-byte stores are all
// aligned.  Lp = padded length, a multiple of 16.  A workgroup makes FIR_TILE consecutive outputs from ONE LDS image of
// FIR_TILE + Lp bytes; lane l owns outputs 16 l .. 16 l + 15 and per step of 16 taps reads one slot (ds_read_b128), forms
// 28 window dwords (21 v_alignbyte_b32) and issues 128 dot4.
#include "sgx_fir_dot4.h"

#define FIL_MAX_LP (((SGX_FILTER_MAX_TAPS + 15 + 15) / 16) * 16)   // 4112: L + e rounded up to 16
#define FIL_LDS_BYTES (FIR_TILE + FIL_MAX_LP)

// taps: [Lp / 4] pairs (hi dword, lo dword), four reversed taps per dword, byte j of a dword = tap 4 q + j
__global__ __launch_bounds__(FIR_THREADS) void fir_dot4_kernel(const int8_t* __restrict__ x, int8_t* __restrict__ y,
                                                               unsigned long long n, const uint2* __restrict__ taps,
                                                               int lp, int cp, int shift) {
    __shared__ uint4 s_x[FIL_LDS_BYTES / 16];
    const unsigned long long n0 = (unsigned long long)blockIdx.x * FIR_TILE;
    const int slots = (FIR_TILE + lp) / 16;
    // image byte i = x[n0 - cp + i]
    for (int i = threadIdx.x; i < slots; i += FIR_THREADS) s_x[i] = fir_load_chunk(x, (long long)n0 - cp + 16ll * i, n, 0u);
    __syncthreads();

    int sum[16];
    fir_steps<16>(s_x, taps, 0, lp / 16, sum);

    const long long rnd = shift ? (1ll << (shift - 1)) : 0ll;
    unsigned out[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int r = 0; r < 16; ++r) out[r >> 2] |= fir_round_clip(sum[r], false, rnd, shift) << ((r & 3) * 8);
    const unsigned long long o = n0 + 16ull * threadIdx.x;
    if (o + 16 <= n) {
        *reinterpret_cast<uint4*>(y + o) = make_uint4(out[0], out[1], out[2], out[3]);
    } else {
        for (int r = 0; r < 16 && o + r < n; ++r) y[o + r] = (int8_t)((out[r >> 2] >> ((r & 3) * 8)) & 0xFF);
    }
}

extern "C" int sgx_if_filter(sgx_ctx* c, const sgx_if* in, const int16_t* taps, int32_t n_taps, int32_t shift,
                             sgx_if** out) {
    // the taps first: these refusals need no device
    SGX_CHECK_ARG(taps);
    SGX_CHECK_ARG(n_taps >= 1 && n_taps <= SGX_FILTER_MAX_TAPS && (n_taps & 1) == 1);
    SGX_CHECK_ARG(shift >= 0 && shift <= 30);
    const int bad = fir_check_taps(taps, n_taps);
    if (bad != SGX_OK) return bad;
    SGX_CHECK_ARG(c && in && out);
    SGX_CHECK_ARG(in->device == c->device);
    int rc = sgx_stage_open(c, in, in->n);
    if (rc != SGX_OK) return rc;
    const unsigned long long blocks = ((unsigned long long)in->n + FIR_TILE - 1) / FIR_TILE;
    rc = sgx_stage_one_launch(blocks, "record of %zu samples is beyond one launch of the filter", in->n);
    if (rc != SGX_OK) return rc;

    // reversed taps behind e zero taps
    const int L = n_taps, cc = (L - 1) / 2;
    const int e = (16 - cc % 16) % 16, cp = cc + e;
    const int lp = ((L + e + 15) / 16) * 16;
    uint2* g = fir_tap_image(c, lp / 4);
    for (int j = 0; j < L; ++j) fir_pack_tap(g, j + e, taps[L - 1 - j]);
    const uint2* d_taps = reinterpret_cast<const uint2*>(c->d_small->fir_taps);
    SgxStage st(SGX_STAGE_FILTER, (unsigned)blocks, "filter kernel failed: %s", out, in->n);
    st.up = {c->d_small->fir_taps, g, (size_t)(lp / 4) * sizeof(uint2)};
    return sgx_stage_run(c, st, [&](sgx_if* r) {
        fir_dot4_kernel<<<st.grid, FIR_THREADS, 0, c->stream>>>(in->d, r->d, (unsigned long long)in->n, d_taps, lp, cp, shift);
    });
}

extern "C" int sgx_filter_timing(sgx_ctx* c, float* kernel_ms) {
    SGX_CHECK_ARG(c && kernel_ms);
    *kernel_ms = c->stage_ms[SGX_STAGE_FILTER];
    return SGX_OK;
}
