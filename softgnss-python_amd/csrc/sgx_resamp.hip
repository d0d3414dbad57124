// Rational resampling by L / M (M = 1 .. 3, M < L <= 16, coprime) of a resident real int8 record (include/sgx.h:
// sgx_if_resample; contract: tests/resamp_spec.py resample()).  The fourth user of the dot4 FIR core (sgx_fir_dot4.h).
//
// Polyphase, so that no multiply-accumulate meets a stuffed zero.  Output m = r + L i (r = m mod L) takes
//   y[r + L i] = q(sum_d h[r M + c - d L] x[i M + d])            over the d with 0 <= r M + c - d L < Lh
// - stream r is a filter of the INPUT with the sub-filter of phase (r M + c) mod L, at most ceil(Lh / L) taps, evaluated at
// every M-th input.  With d = e M + p (floor) the input splits into M planes, plane p holding the samples n M + p, and
//   y[r + L i] = q(sum_p sum_e G_rp[e] x_p[i + e]),   G_rp[e] = h[r M + c - (e M + p) L]
// every term an ordinary FIR on one plane: fir_steps<16> as it stands, the partial sums added modulo 2^32 (the contract
// bounds the true sum inside int32).  Of the M L (output, input) phase pairs only the L that hold a sample are computed.
//
//   * A workgroup makes 16 consecutive i per lane of EVERY stream: FIR_TILE i, FIR_TILE L consecutive output bytes.  A
//     lane's 16 outputs of each of the L streams are the 16 L consecutive bytes from (i0 L); it keeps them packed, 4 dwords
//     per stream, transposes in registers - output byte b takes byte b / L of stream b mod L, three v_perm_b32 per dword
//     with selectors that are constants once L is fixed - and writes L 16-byte stores; byte stores only on the record's
//     last partial group.  The stream loop is unrolled for that (L filter bodies); the kernel is templated on L alone, M
//     is a kernel argument: 15 instantiations.
//   * The sub-filter images share one origin: G_rp sits at j = e + cq, cq the reach to the left in plane samples rounded up
//     so that cq M is a multiple of 16 (rs_cq); lq (a multiple of 16) covers all of them.  The first byte a workgroup
//     needs, (i0 - cq) M, is then a multiple of 16: chunk loads are aligned, guarded per chunk (zero outside [0, N)).
//   * M = 1: all L streams read ONE image of the input, filled by plain 16-byte copies.  M = 2, 3: fir_split_planes<M, 16>
//     (sgx_fir_dot4.h), M chunks per slot of every plane.  Lanes write and read consecutive slots: no bank conflict.
//   * Taps are wave-uniform: scalar loads from d_small->fir_taps, [L][M][lq / 4] pairs.  All streams run over one range of
//     steps, the union of the steps that hold a tap; a step is 16 taps, so the default 24 taps per stream (M = 1) cost 32.
//   * Clipped outputs: counted per lane on the value before the clip (in 32 bits, see the kernel), counter 0 of the stage
//     counters (sgx_count.h).
//
// What bounds it: vector-ALU issue, not HBM.  Per output byte the kernel reads 1 / L input byte and writes one, 0.33 ms at
// the copy rate for 1.4 GB of output at L = 10; it takes 1.3 ms there.  A step is 16 taps, so the default 24 taps of a stream
// cost two steps, 16 dot4 per output byte (hi and lo byte filters) beside 21 v_alignbyte_b32 per step for the window, the
// 64-bit rounding of 16 L sums and the transposes: 34-37 tera-MAC/s issued against the 61-65 of the notch's long filter.  At
// M = 3 the 8 taps of a (stream, plane) straddle two steps on each of three planes, 96 MACs issued for 24: 3.0 ms
// (DESIGN.md section 4.17 has the figures).
#include "sgx_fir_dot4.h"

#define RS_MAX_C ((SGX_RESAMP_MAX_TAPS - 1) / 2)

static constexpr int rs_gcd(int a, int b) { return b ? rs_gcd(b, a % b) : a; }
static constexpr bool rs_pair_ok(int l, int m) { return m >= 1 && m <= 3 && l > m && l <= 16 && rs_gcd(l, m) == 1; }
// The halo in front of a tile, in plane samples: the reach of stream 0 to the left, ceil((c div L) / M), rounded up to the
// smallest unit that makes cq M a multiple of 16.  And the padded length of a sub-filter image: the largest d is
// ((L - 1) M + c) div L, of stream L - 1.
static constexpr int rs_cq(int l, int m, int c) {
    const int a = 16 / rs_gcd(16, m);
    return ((c / l + m - 1) / m + a - 1) / a * a;
}
static constexpr int rs_lq(int l, int m, int c) { return (rs_cq(l, m, c) + ((l - 1) * m + c) / l / m + 1 + 15) / 16 * 16; }
// (hi, lo) pairs of the tap images of one call
static constexpr int rs_tap_pairs(int l, int m, int c) { return l * m * rs_lq(l, m, c) / 4; }
static constexpr bool rs_taps_fit() {
    for (int m = 1; m <= 3; ++m)
        for (int l = m + 1; l <= 16; ++l)
            for (int c = 0; c <= RS_MAX_C; ++c)
                if ((size_t)rs_tap_pairs(l, m, c) * sizeof(uint2) > sizeof(SgxSmall::fir_taps)) return false;
    return true;
}
static_assert(rs_taps_fit(), "the sub-filter images of the longest filter fit the tap staging at every pair");
// slots of the plane images of a tile at the longest filter, the largest over M
static constexpr int rs_img_slots(int l) {
    int most = 0;
    for (int m = 1; m <= 3; ++m) {
        const int s = m * ((FIR_TILE + rs_lq(l, m, RS_MAX_C)) / 16);
        most = s > most ? s : most;
    }
    return most;
}

template <int L>
__global__ __launch_bounds__(FIR_THREADS) void resamp_kernel(const int8_t* __restrict__ x, int8_t* __restrict__ y,
                                                             unsigned long long n, unsigned long long n_out,
                                                             const uint2* __restrict__ taps, int M, int lq, int cq, int q_lo,
                                                             int q_hi, int shift, unsigned long long* __restrict__ counts) {
    __shared__ uint4 s_img[rs_img_slots(L)];

    const int ns = (FIR_TILE + lq) / 16;       // slots of a plane image: plane samples i0 - cq .. i0 + FIR_TILE + lq - cq
    const long long base = ((long long)blockIdx.x * FIR_TILE - cq) * M;   // its first byte in the record, a multiple of 16
    if (M == 1) {
        for (int s = threadIdx.x; s < ns; s += FIR_THREADS) s_img[s] = fir_load_chunk(x, base + 16ll * s, n, 0u);
    } else if (M == 2) {
        fir_split_planes<2, 16>(x, base, n, 0u, s_img, ns);
    } else {
        fir_split_planes<3, 16>(x, base, n, 0u, s_img, ns);
    }
    __syncthreads();

    const long long rnd = shift ? (1ll << (shift - 1)) : 0ll;
    const unsigned long long i0 = (unsigned long long)blockIdx.x * FIR_TILE + 16ull * threadIdx.x;
    const unsigned long long o0 = i0 * L;      // the lane's first output byte, a multiple of 16
    const int left = o0 >= n_out ? 0 : (n_out - o0 < 16ull * L ? (int)(n_out - o0) : 16 * L);   // how many of its 16 L exist
    unsigned pk[4 * L];                        // byte 16 r + i: output i of stream r
    unsigned clipped = 0;
#pragma unroll
    for (int r = 0; r < L; ++r) {
        int tot[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) tot[i] = 0;
#pragma unroll 1
        for (int p = 0; p < M; ++p) {
            int sum[16];
            fir_steps<16>(s_img + p * ns, taps + (r * M + p) * (lq / 4), q_lo, q_hi, sum);
#pragma unroll
            for (int i = 0; i < 16; ++i) tot[i] = (int)((unsigned)tot[i] + (unsigned)sum[i]);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) pk[4 * r + g] = 0u;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const unsigned byte = fir_round_clip(tot[i], false, rnd, shift);
            // (the value in front of the clip fits 32 bits: it was clipped where it is not the byte's value)
            clipped += (i * L + r < left && (int)(((long long)tot[i] + rnd) >> shift) != (int)(int8_t)byte) ? 1u : 0u;
            pk[4 * r + (i >> 2)] |= byte << ((i & 3) * 8);
        }
        // (the stream's bytes and its count are made here: left to itself the compiler keeps every stream's 64-bit values
        // in front of the clip to the end, 32 registers a stream)
#pragma unroll
        for (int g = 0; g < 4; ++g) asm volatile("" : "+v"(pk[4 * r + g]));
        asm volatile("" : "+v"(clipped));
    }

#pragma unroll
    for (int s = 0; s < L; ++s) {
        unsigned o[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            // output byte b of the lane is output b / L of stream b mod L
            const int b = 16 * s + 4 * g;
            const unsigned lo = fir_pick2(pk, 16 * (b % L) + b / L, 16 * ((b + 1) % L) + (b + 1) / L);
            const unsigned hi = fir_pick2(pk, 16 * ((b + 2) % L) + (b + 2) / L, 16 * ((b + 3) % L) + (b + 3) / L);
            o[g] = __builtin_amdgcn_perm(hi, lo, 0x05040100u);
        }
        int8_t* at = y + o0 + 16ull * s;
        if (16 * s + 16 <= left) {
            *reinterpret_cast<uint4*>(at) = make_uint4(o[0], o[1], o[2], o[3]);
        } else {
            for (int b = 0; b < 16 && 16 * s + b < left; ++b) at[b] = (int8_t)((o[b >> 2] >> ((b & 3) * 8)) & 0xFF);
        }
    }
    const unsigned count[1] = {clipped};
    sgx_count_publish<1, FIR_THREADS / 64>(count, counts);
}

// ---- host ------------------------------------------------------------------------------------------------------------------
extern "C" int sgx_resamp_tile(int32_t* tile_bytes) {
    SGX_CHECK_ARG(tile_bytes);
    *tile_bytes = FIR_TILE * 16;
    return SGX_OK;
}

extern "C" int sgx_resamp_timing(sgx_ctx* c, float* kernel_ms) {
    SGX_CHECK_ARG(c && kernel_ms);
    *kernel_ms = c->stage_ms[SGX_STAGE_RESAMP];
    return SGX_OK;
}

extern "C" int sgx_if_resample(sgx_ctx* c, const sgx_if* rec, const int16_t* taps, int32_t n_taps, int32_t shift, int32_t L,
                               int32_t M, sgx_if** out, int64_t* clipped) {
    // the filter and the pair first: these refusals need no device
    if (!rs_pair_ok(L, M)) {
        sgx_set_error("bad argument: L / M = %d / %d is not a pair with 1 <= M <= 3, M < L <= 16 and gcd(L, M) = 1", (int)L,
                      (int)M);
        return SGX_E_ARG;
    }
    if (n_taps < 1 || n_taps > SGX_RESAMP_MAX_TAPS || (n_taps & 1) == 0) {
        sgx_set_error("bad argument: n_taps = %d is not an odd number in 1 .. %d", (int)n_taps, SGX_RESAMP_MAX_TAPS);
        return SGX_E_ARG;
    }
    int rc = fir_check_shift(shift);
    if (rc != SGX_OK) return rc;
    SGX_CHECK_ARG(taps);
    rc = fir_check_taps(taps, n_taps);
    if (rc != SGX_OK) return rc;
    SGX_CHECK_ARG(c && rec && out);
    SGX_CHECK_ARG(rec->device == c->device);
    const unsigned long long n_out = ((unsigned long long)rec->n * (unsigned)L + (unsigned)M - 1) / (unsigned)M;
    const unsigned long long per_stream = (n_out + (unsigned)L - 1) / (unsigned)L;
    const unsigned long long tiles = (per_stream + FIR_TILE - 1) / FIR_TILE;
    rc = sgx_stage_one_launch(tiles, "bad argument: a record of %zu output bytes is beyond one launch of the resampler",
                              (size_t)n_out);
    if (rc != SGX_OK) return rc;
    rc = sgx_stage_open(c, rec, rec->n);
    if (rc != SGX_OK) return rc;

    // G_rp[j] = the tap of stream r on plane p at e = j - cq: h[r M + cc - (e M + p) L]
    const int cc = (n_taps - 1) / 2, cq = rs_cq(L, M, cc), lq = rs_lq(L, M, cc), pairs = rs_tap_pairs(L, M, cc);
    uint2* g = fir_tap_image(c, pairs);
    FirLaunch l(c, rec, tiles, n_out, shift, false);
    l.M = M, l.lq = lq, l.cq = cq;
    for (int r = 0; r < L; ++r)
        for (int p = 0; p < M; ++p)
            l.steps = fir_pack_image(taps, n_taps, 1, 16, g + (size_t)(r * M + p) * (lq / 4), lq / 4,
                                     [&](int j) { return r * M + cc - ((j - cq) * M + p) * L; }, l.steps);

    SgxStage st(SGX_STAGE_RESAMP, l.grid, "resampling kernel failed: %s", out, (size_t)n_out);
    st.up = {c->d_small->fir_taps, g, (size_t)pairs * sizeof(uint2)};
    return fir_run_counted(c, st, l, clipped, [&] {
        fir_dispatch<2, 16>(L, [&](auto up) {
            resamp_kernel<decltype(up)::value><<<l.grid, FIR_THREADS, 0, l.st>>>(l.x, l.y, l.n, l.n_out, l.taps, l.M, l.lq, l.cq,
                                                                                 l.steps.lo, l.steps.hi, l.shift, l.counts);
        });
    });
}
