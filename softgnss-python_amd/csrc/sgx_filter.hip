// Zero-phase integer FIR over a whole int8 record (include/sgx.h: sgx_if_filter; contract: tests/notch_spec.py apply()).
//
//   y[n] = clip((sum_k h[k] x[n + c - k] + rnd) >> S, -127, 127),  c = (L - 1) / 2,  x = 0 outside the record
//
// Formulation: v_dot4_i32_i8 on byte windows (DESIGN.md section 4.11 says why not the int8 matrix cores).
//   * Each int16 tap is two signed bytes, h = 256 hi + lo; the two byte filters accumulate separately and are combined as
//     256 acc_hi + acc_lo.  All arithmetic is modulo 2^32 and the contract bounds the true sum inside int32, so any
//     order - and a partial sum that wraps - gives the exact result.
//   * The taps are reversed (g[j] = h[L-1-j]: y[n] = sum_j g[j] x[n - c + j]) and e = (-c) mod 16 zero taps are put in
//     front, so that the first sample a workgroup needs, n0 - c - e, is a multiple of 16: global loads, LDS reads and the
//     record's 16-byte stores are all aligned.  Lp = padded length, a multiple of 16.
//   * A workgroup of 256 lanes makes FIL_TILE = 4096 consecutive outputs from an LDS image of FIL_TILE + Lp bytes.  Lane l
//     owns outputs 16 l .. 16 l + 15.  Per step of 16 taps it reads ONE new 16-byte slot (ds_read_b128, lanes on
//     consecutive slots: conflict-free), forms the 28 byte-shifted dwords of its 32-byte window (7 are aligned, 21 are one
//     v_alignbyte_b32 each) and issues 128 dot4 (16 outputs x 4 tap dwords x hi / lo).  The tap dwords are wave-uniform and
//     come in through scalar loads.
// Bounds: global reads are guarded per 16-byte chunk (bytes outside [0, N) are zero, never read); stores are guarded per
// lane (a 16-byte store only when all 16 outputs exist, byte stores on the record's last partial group).
#include "sgx_internal.h"

int sgx_if_alloc_internal(sgx_ctx* c, size_t n, sgx_if** out);

#define FIL_THREADS 256
#define FIL_PER_LANE 16
#define FIL_TILE (FIL_THREADS * FIL_PER_LANE)                 // outputs per workgroup
#define FIL_MAX_LP (((SGX_FILTER_MAX_TAPS + 15 + 15) / 16) * 16)   // 4112: L + e rounded up to 16
#define FIL_LDS_BYTES (FIL_TILE + FIL_MAX_LP)

// taps: [Lp / 4] pairs (hi dword, lo dword), four reversed taps per dword, byte j of a dword = tap 4 q + j
__global__ __launch_bounds__(FIL_THREADS) void fir_dot4_kernel(const int8_t* __restrict__ x, int8_t* __restrict__ y,
                                                               unsigned long long n, const uint2* __restrict__ taps,
                                                               int lp, int cp, int shift) {
    __shared__ uint4 s_x[FIL_LDS_BYTES / 16];
    const unsigned long long n0 = (unsigned long long)blockIdx.x * FIL_TILE;
    const int slots = (FIL_TILE + lp) / 16;
    // image byte i = x[n0 - cp + i]
    for (int i = threadIdx.x; i < slots; i += FIL_THREADS) {
        const long long a = (long long)n0 - cp + 16ll * i;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (a >= 0 && (unsigned long long)a + 16 <= n) {
            v = *reinterpret_cast<const uint4*>(x + a);
        } else if (a >= 0 && (unsigned long long)a < n) {
            unsigned w[4] = {0u, 0u, 0u, 0u};
            const int left = (int)(n - (unsigned long long)a);   // 1 .. 15
            for (int b = 0; b < left; ++b) w[b >> 2] |= ((unsigned)(uint8_t)x[a + b]) << ((b & 3) * 8);
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        s_x[i] = v;
    }
    __syncthreads();

    int acc_hi[FIL_PER_LANE], acc_lo[FIL_PER_LANE];
#pragma unroll
    for (int r = 0; r < FIL_PER_LANE; ++r) acc_hi[r] = acc_lo[r] = 0;
    unsigned w[8];
    {
        const uint4 v = s_x[threadIdx.x];
        w[4] = v.x, w[5] = v.y, w[6] = v.z, w[7] = v.w;
    }
    const int steps = lp / 16;
    for (int q = 0; q < steps; ++q) {
        w[0] = w[4], w[1] = w[5], w[2] = w[6], w[3] = w[7];
        const uint4 v = s_x[threadIdx.x + q + 1];
        w[4] = v.x, w[5] = v.y, w[6] = v.z, w[7] = v.w;
        unsigned win[28];   // win[b] = image bytes [16 (lane + q) + b, + 4)
#pragma unroll
        for (int b = 0; b < 28; ++b)
            win[b] = (b & 3) ? __builtin_amdgcn_alignbyte(w[(b >> 2) + 1], w[b >> 2], b & 3) : w[b >> 2];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const uint2 g = taps[4 * q + t];   // wave-uniform
#pragma unroll
            for (int r = 0; r < FIL_PER_LANE; ++r) {
                acc_hi[r] = __builtin_amdgcn_sdot4((int)win[4 * t + r], (int)g.x, acc_hi[r], false);
                acc_lo[r] = __builtin_amdgcn_sdot4((int)win[4 * t + r], (int)g.y, acc_lo[r], false);
            }
        }
    }

    const long long rnd = shift ? (1ll << (shift - 1)) : 0ll;
    unsigned out[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int r = 0; r < FIL_PER_LANE; ++r) {
        // (exact: the contract bounds the sum inside int32; the rounding constant is added in 64 bits as the contract does)
        const long long sum = (long long)(int)(((unsigned)acc_hi[r] << 8) + (unsigned)acc_lo[r]) + rnd;
        int v = (int)(sum >> shift);
        v = v < -127 ? -127 : (v > 127 ? 127 : v);
        out[r >> 2] |= ((unsigned)(v & 0xFF)) << ((r & 3) * 8);
    }
    const unsigned long long o = n0 + (unsigned long long)threadIdx.x * FIL_PER_LANE;
    if (o + FIL_PER_LANE <= n) {
        *reinterpret_cast<uint4*>(y + o) = make_uint4(out[0], out[1], out[2], out[3]);
    } else {
        for (int r = 0; r < FIL_PER_LANE && o + r < n; ++r) y[o + r] = (int8_t)((out[r >> 2] >> ((r & 3) * 8)) & 0xFF);
    }
}

extern "C" int sgx_if_filter(sgx_ctx* c, const sgx_if* in, const int16_t* taps, int32_t n_taps, int32_t shift,
                             sgx_if** out) {
    // the taps first: these refusals need no device
    SGX_CHECK_ARG(taps);
    SGX_CHECK_ARG(n_taps >= 1 && n_taps <= SGX_FILTER_MAX_TAPS && (n_taps & 1) == 1);
    SGX_CHECK_ARG(shift >= 0 && shift <= 30);
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
    SGX_CHECK_ARG(c && in && out);
    {
        const int rq = sgx_if_require(in, in->n);   // a record that is still streaming in
        if (rq != SGX_OK) return rq;
    }
    SGX_HIP(hipSetDevice(c->device));

    // reversed taps behind e zero taps, split into bytes, four to a dword
    const int L = n_taps, cc = (L - 1) / 2;
    const int e = (16 - cc % 16) % 16, cp = cc + e;
    const int lp = ((L + e + 15) / 16) * 16;
    uint2* h_taps = reinterpret_cast<uint2*>(c->h_small->filter_taps);
    memset(h_taps, 0, (size_t)(lp / 4) * sizeof(uint2));
    for (int j = 0; j < L; ++j) {
        const int h = taps[L - 1 - j];
        const int hi = (h + 128) >> 8, lo = h - 256 * hi;
        const int p = j + e;
        h_taps[p >> 2].x |= ((unsigned)(hi & 0xFF)) << ((p & 3) * 8);
        h_taps[p >> 2].y |= ((unsigned)(lo & 0xFF)) << ((p & 3) * 8);
    }
    sgx_if* r = nullptr;
    const int rc = sgx_if_alloc_internal(c, in->n, &r);
    if (rc != SGX_OK) return rc;
    uint2* d_taps = reinterpret_cast<uint2*>(c->d_small->filter_taps);
    hipError_t err = hipMemcpyAsync(d_taps, h_taps, (size_t)(lp / 4) * sizeof(uint2), hipMemcpyHostToDevice, c->stream);
    c->filter_kernel_ms = 0.0f;
    const unsigned long long blocks = ((unsigned long long)in->n + FIL_TILE - 1) / FIL_TILE;
    if (err == hipSuccess && blocks > 0x7FFFFFFFull) {
        sgx_if_free(c, r);
        sgx_set_error("record of %zu samples is beyond one launch of the filter", in->n);
        return SGX_E_ARG;
    }
    if (err == hipSuccess && blocks) {
        hipEventRecord(c->ev[0], c->stream);
        fir_dot4_kernel<<<(unsigned)blocks, FIL_THREADS, 0, c->stream>>>(in->d, r->d, (unsigned long long)in->n, d_taps, lp,
                                                                         cp, shift);
        hipEventRecord(c->ev[1], c->stream);
    }
    if (err == hipSuccess) err = hipStreamSynchronize(c->stream);   // (h_small's staging is free again on return)
    if (err == hipSuccess) err = hipGetLastError();
    if (err != hipSuccess) {
        sgx_if_free(c, r);
        sgx_set_error("filter kernel failed: %s", hipGetErrorString(err));
        return SGX_E_HIP;
    }
    if (blocks) hipEventElapsedTime(&c->filter_kernel_ms, c->ev[0], c->ev[1]);
    *out = r;
    return SGX_OK;
}

extern "C" int sgx_filter_timing(sgx_ctx* c, float* kernel_ms) {
    SGX_CHECK_ARG(c && kernel_ms);
    *kernel_ms = c->filter_kernel_ms;
    return SGX_OK;
}
