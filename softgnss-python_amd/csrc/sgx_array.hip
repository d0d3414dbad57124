// Multi-antenna records (include/sgx.h: sgx_array_stats, sgx_if_combine; contract: tests/array_spec.py): the exact lag
// statistics of the A streams of a resident int8 record, and the A streams through one integer FIR each, summed into one
// int8 record.  The fifth user of the dot4 FIR core (sgx_fir_dot4.h); the int8 matrix cores are left aside for the reason
// DESIGN.md section 4.11 gives.
//
// Both kernels are templated on (LANES, A) and start the same way: the record's bytes are one stream of P = A LANES planes,
// plane a LANES + l holding component l of antenna a.  ar_load_planes brings a run of frames from the interleaved bytes
// into per-plane runs in LDS: a lane loads the P dwords that hold 4 consecutive frames (guarded per dword: bytes outside
// [0, N) are zero and never read; XOR 0x80 for offset binary), picks the 4 bytes of each plane out of them - three
// v_perm_b32 with selectors that are constants once P is fixed, as the decimator's transpose - and writes one dword per
// plane.  Lanes write consecutive dwords of a plane and, afterwards, read consecutive dwords: no bank conflict.
//
// array_stats_kernel.  A workgroup takes tiles of AR_TILE frames plus 16 frames behind them (the lags reach K - 1 <= 14
// frames ahead), tile blockIdx.x, + gridDim.x, ..: frame f of the tile is the x_b[f] of its products, x_a[f + d] comes from
// the same image, and frames past the record are zero, so every product of the contract is formed once.  The A^2 pairs
// (a, b) are dealt to the four waves; a lane takes 4 frames per step - one dword of x_b, five of x_a, the K byte-shifted
// windows of x_a by v_alignbyte_b32 - and one v_dot4_i32_i8 per lag (four per lag for I/Q: II + QQ, QI, IQ).  Per tile a
// lane adds at most 8 x 2 x 2^16 into an int32 and the wave's sum stays below 2^27; it is folded over the wave by shuffles
// and added into the workgroup's int64 sums in LDS, each owned by one wave.  At the end the workgroup adds its sums into
// one of AR_SUM_SLOTS copies of rho in the context's small area, one integer atomic per value.
//
// combine_kernel.  A workgroup makes FIR_TILE output bytes, 16 per lane, from plane images of FIR_TILE / LANES + 16 frames
// that start AR_CQ = 8 frames in front of the tile, per antenna one image and one tap image G_a[j] = h_a[c + AR_CQ - j]
// (I/Q: re, im, -im).  The sum over the antennas, the rounding, the clip count and its fold are the header's
// (fir_plane_sums) and the stage counters' (sgx_count.h).
//
// Weights per block (sgx_array_block_stats, sgx_if_combine_blocks; contract: tests/array_block_spec.py): the same two kernels
// with BLOCKS set.  A block is a whole number of tiles of either kernel (SGX_ARRAY_BLOCK_UNIT), so no workgroup straddles a
// seam: the statistics kernel walks the tiles of ONE block and adds into that block's slot of a table (sgx_ctx::
// d_array_blocks) - what reaches across a seam is the halo behind a tile -, the combiner reads the tap images of the block
// its tile lies in from a table of them (sgx_ctx::d_array_taps).  BLOCKS = false is what it was before the flag.
#include "sgx_fir_dot4.h"

#define AR_TILE 2048                      // frames a workgroup of the statistics kernel sums at a time
#define AR_HALO 16                        // frames behind a tile that its lags may reach into
#define AR_MAX_GRID 2048                  // workgroups of the statistics kernel
#define AR_CQ 8                           // frames in front of a combiner tile: >= (SGX_ARRAY_MAX_TAPS - 1) / 2, a multiple of 4
#define AR_LQ 16                          // length of a tap image: AR_CQ + c + 1 <= 16
static_assert(SGX_ARRAY_MAX_TAPS - 1 < AR_HALO && AR_CQ + (SGX_ARRAY_MAX_TAPS - 1) / 2 + 1 <= AR_LQ, "the lags fit the halo");
static_assert(SGX_ARRAY_BLOCK_UNIT % AR_TILE == 0 && SGX_ARRAY_BLOCK_UNIT % FIR_TILE == 0, "a block is whole tiles of both kernels");
static_assert(AR_SUM_VALUES >= SGX_ARRAY_MAX_ANTENNAS * SGX_ARRAY_MAX_WEIGHTS * 2, "a copy of rho holds the largest case");
static_assert((size_t)SGX_ARRAY_MAX_ANTENNAS * 3 * (AR_LQ / 4) * sizeof(uint2) <= sizeof(SgxSmall::fir_taps),
              "the tap images of eight antennas fit the tap staging");

// Record bytes [a, a + 4) XOR flip, a a multiple of 4: zero outside [0, n)
__device__ __forceinline__ unsigned ar_load_dword(const int8_t* __restrict__ x, long long a, unsigned long long n,
                                                  unsigned flip) {
    unsigned v = 0u;
    if (a >= 0 && (unsigned long long)a + 4 <= n) {
        v = *reinterpret_cast<const unsigned*>(x + a) ^ flip;
    } else if (a >= 0 && (unsigned long long)a < n) {
        const int left = (int)(n - (unsigned long long)a);   // 1 .. 3
        for (int b = 0; b < left; ++b) v |= (((unsigned)(uint8_t)x[a + b]) ^ (flip & 0xFFu)) << (b * 8);
    }
    return v;
}

// Frames [frame0, frame0 + 4 units) of the record into P plane images of `pitch` dwords each; frame0 is a multiple of 4
// (or negative and one), so every dword it loads is aligned.  (Not the header's fir_split_planes: dwords of 4 frames, not
// chunks of a slot, under this alignment rule, and the statistics kernel shares it.)
template <int P>
__device__ __forceinline__ void ar_load_planes(const int8_t* __restrict__ x, unsigned long long n, unsigned flip,
                                               long long frame0, int units, int pitch, unsigned* __restrict__ s_pl) {
    for (int u = threadIdx.x; u < units; u += FIR_THREADS) {
        const long long at = (frame0 + 4ll * u) * P;
        unsigned raw[P];
#pragma unroll
        for (int i = 0; i < P; ++i) raw[i] = ar_load_dword(x, at + 4 * i, n, flip);
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const unsigned lo = fir_pick2(raw, p, P + p), hi = fir_pick2(raw, 2 * P + p, 3 * P + p);
            s_pl[p * pitch + u] = __builtin_amdgcn_perm(hi, lo, 0x05040100u);
        }
    }
}

// BLOCKS: workgroup blockIdx.x takes part blockIdx.x % parts of block blockIdx.x / parts - tiles part, part + parts, .. of the
// block's tpb tiles, as far as the record has them - and adds into the block's own slot of the table `sums`
template <int LANES, int A, bool BLOCKS>
__global__ __launch_bounds__(FIR_THREADS) void array_stats_kernel(const int8_t* __restrict__ x, unsigned long long n,
                                                                  unsigned long long tiles, int K, unsigned flip,
                                                                  unsigned long long* __restrict__ sums, unsigned tpb,
                                                                  unsigned parts) {
    constexpr int P = LANES * A;
    constexpr int PITCH = (AR_TILE + AR_HALO) / 4;     // dwords of a plane image
    constexpr int KM = SGX_ARRAY_MAX_TAPS;
    __shared__ unsigned s_pl[P * PITCH];
    __shared__ long long s_sum[A * A * KM * LANES];    // [pair][d][lane component], K of the KM used

    const int n_val = A * A * K * LANES;
    for (int i = threadIdx.x; i < n_val; i += FIR_THREADS) s_sum[i] = 0;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;

    unsigned long long tile = blockIdx.x, tile_end = tiles, step = gridDim.x;
    if constexpr (BLOCKS) {
        const unsigned long long first = (unsigned long long)(blockIdx.x / parts) * tpb;
        tile = first + blockIdx.x % parts, step = parts;
        if (first + tpb < tiles) tile_end = first + tpb;
    }
    for (; tile < tile_end; tile += step) {
        __syncthreads();                               // (the image of the tile before is read no more; s_sum is cleared)
        ar_load_planes<P>(x, n, flip, (long long)(tile * AR_TILE), PITCH, PITCH, s_pl);
        __syncthreads();
        for (int pr = wave; pr < A * A; pr += FIR_THREADS / 64) {
            const int a = pr / A, b = pr % A;
            if constexpr (LANES == 1) {
                const unsigned* pa = s_pl + a * PITCH;
                const unsigned* pb = s_pl + b * PITCH;
                int acc[KM];
#pragma unroll
                for (int d = 0; d < KM; ++d) acc[d] = 0;
                for (int u = lane; u < AR_TILE / 4; u += 64) {
                    const int xb = (int)pb[u];
                    unsigned w[5];
#pragma unroll
                    for (int i = 0; i < 5; ++i) w[i] = pa[u + i];
#pragma unroll
                    for (int d = 0; d < KM; ++d) {
                        if (d < K) {
                            const unsigned xa = (d & 3) ? __builtin_amdgcn_alignbyte(w[(d >> 2) + 1], w[d >> 2], d & 3) : w[d >> 2];
                            acc[d] = __builtin_amdgcn_sdot4((int)xa, xb, acc[d], false);
                        }
                    }
                }
#pragma unroll
                for (int d = 0; d < KM; ++d) {
                    if (d < K) {
                        const int t = sgx_wave_sum(acc[d]);
                        if (lane == 0) s_sum[pr * K + d] += (long long)t;
                    }
                }
            } else {
                const unsigned* pai = s_pl + (2 * a) * PITCH;
                const unsigned* paq = pai + PITCH;
                const unsigned* pbi = s_pl + (2 * b) * PITCH;
                const unsigned* pbq = pbi + PITCH;
                int acc_re[KM], acc_p[KM], acc_m[KM];   // II + QQ;  Q_a I_b;  I_a Q_b
#pragma unroll
                for (int d = 0; d < KM; ++d) acc_re[d] = acc_p[d] = acc_m[d] = 0;
                for (int u = lane; u < AR_TILE / 4; u += 64) {
                    const int bi = (int)pbi[u], bq = (int)pbq[u];
                    unsigned wi[5], wq[5];
#pragma unroll
                    for (int i = 0; i < 5; ++i) wi[i] = pai[u + i], wq[i] = paq[u + i];
#pragma unroll
                    for (int d = 0; d < KM; ++d) {
                        if (d < K) {
                            const unsigned ai = (d & 3) ? __builtin_amdgcn_alignbyte(wi[(d >> 2) + 1], wi[d >> 2], d & 3) : wi[d >> 2];
                            const unsigned aq = (d & 3) ? __builtin_amdgcn_alignbyte(wq[(d >> 2) + 1], wq[d >> 2], d & 3) : wq[d >> 2];
                            acc_re[d] = __builtin_amdgcn_sdot4((int)ai, bi, acc_re[d], false);
                            acc_re[d] = __builtin_amdgcn_sdot4((int)aq, bq, acc_re[d], false);
                            acc_p[d] = __builtin_amdgcn_sdot4((int)aq, bi, acc_p[d], false);
                            acc_m[d] = __builtin_amdgcn_sdot4((int)ai, bq, acc_m[d], false);
                        }
                    }
                }
#pragma unroll
                for (int d = 0; d < KM; ++d) {
                    if (d < K) {
                        const int t_re = sgx_wave_sum(acc_re[d]), t_im = sgx_wave_sum(acc_p[d] - acc_m[d]);
                        if (lane == 0) {
                            s_sum[(pr * K + d) * 2] += (long long)t_re;
                            s_sum[(pr * K + d) * 2 + 1] += (long long)t_im;
                        }
                    }
                }
            }
        }
    }
    __syncthreads();
    unsigned long long* mine = BLOCKS ? sums + (size_t)(blockIdx.x / parts) * n_val
                                      : sums + (size_t)(blockIdx.x % AR_SUM_SLOTS) * AR_SUM_VALUES;
    for (int i = threadIdx.x; i < n_val; i += FIR_THREADS) {
        const long long v = s_sum[i];
        if (v) atomicAdd(&mine[i], (unsigned long long)v);
    }
}

// BLOCKS: `taps` is a table of tap images, one set per block of tpb tiles; a workgroup reads the set of its own block
template <int LANES, int A, bool BLOCKS>
__global__ __launch_bounds__(FIR_THREADS) void combine_kernel(const int8_t* __restrict__ x, int8_t* __restrict__ y,
                                                              unsigned long long n, unsigned long long n_out,
                                                              const uint2* __restrict__ taps, int q_lo, int q_hi, int shift,
                                                              unsigned flip, unsigned long long* __restrict__ counts,
                                                              unsigned tpb) {
    constexpr int W = 16 / LANES;              // bytes of a slot = outputs of a lane per plane image
    constexpr int P = LANES * A;               // planes
    constexpr int TF = FIR_TILE / LANES;       // frames of a tile
    constexpr int NS = (TF + AR_LQ) / W;       // slots of a plane image: frames m0 - AR_CQ .. m0 + TF + AR_LQ - AR_CQ
    constexpr int IMG = AR_LQ / 4;             // pairs of a tap image
    typedef typename FirSlot<W>::type slot_t;
    __shared__ slot_t s_img[P * NS];

    if constexpr (BLOCKS) taps += (size_t)(blockIdx.x / tpb) * ((LANES == 2 ? 3 : 1) * A * IMG);
    ar_load_planes<P>(x, n, flip, (long long)blockIdx.x * TF - AR_CQ, (TF + AR_LQ) / 4, NS * (W / 4),
                      reinterpret_cast<unsigned*>(s_img));
    __syncthreads();

    const unsigned long long o0 = (unsigned long long)blockIdx.x * FIR_TILE + 16ull * threadIdx.x;
    unsigned out[4] = {0u, 0u, 0u, 0u};
    unsigned clipped = 0;
    fir_plane_sums<LANES, A>(s_img, NS, taps, IMG, q_lo, q_hi, shift, o0, n_out, out, clipped);
    if (o0 + 16 <= n_out) {
        *reinterpret_cast<uint4*>(y + o0) = make_uint4(out[0], out[1], out[2], out[3]);
    } else {
        for (int r = 0; r < 16 && o0 + r < n_out; ++r) y[o0 + r] = (int8_t)((out[r >> 2] >> ((r & 3) * 8)) & 0xFF);
    }
    const unsigned count[1] = {clipped};
    sgx_count_publish<1, FIR_THREADS / 64>(count, counts);
}

// ---- host ------------------------------------------------------------------------------------------------------------------
struct ArStats {
    hipStream_t st;
    unsigned grid;
    const int8_t* x;
    unsigned long long n, tiles;
    int K;
    unsigned flip;
    unsigned long long* sums;
    unsigned tpb = 0, parts = 0;   // block statistics: tiles of a block and the workgroups that share them; parts 0: the whole record
};

// The kernel of a launch's shape: the statistics kernel of an ArStats, the combiner of a FirLaunch
template <int LANES, int A> static void ar_launch_la(const ArStats& l) {
    if (l.parts) {
        array_stats_kernel<LANES, A, true><<<l.grid, FIR_THREADS, 0, l.st>>>(l.x, l.n, l.tiles, l.K, l.flip, l.sums, l.tpb, l.parts);
    } else {
        array_stats_kernel<LANES, A, false><<<l.grid, FIR_THREADS, 0, l.st>>>(l.x, l.n, l.tiles, l.K, l.flip, l.sums, 0u, 0u);
    }
}
template <int LANES, int A> static void ar_launch_la(const FirLaunch& l) {
    if (l.tpb) {
        combine_kernel<LANES, A, true><<<l.grid, FIR_THREADS, 0, l.st>>>(l.x, l.y, l.n, l.n_out, l.taps, l.steps.lo, l.steps.hi,
                                                                        l.shift, l.flip, l.counts, l.tpb);
    } else {
        combine_kernel<LANES, A, false><<<l.grid, FIR_THREADS, 0, l.st>>>(l.x, l.y, l.n, l.n_out, l.taps, l.steps.lo, l.steps.hi,
                                                                         l.shift, l.flip, l.counts, 0u);
    }
}
template <typename Launch> static void ar_launch(int lanes, int A, const Launch& l) {
    fir_dispatch<1, 2>(lanes, [&](auto la) {
        fir_dispatch<2, SGX_ARRAY_MAX_ANTENNAS>(A, [&](auto a) { ar_launch_la<decltype(la)::value, decltype(a)::value>(l); });
    });
}

// The refusals of the shape that both entry points share; each names its argument
static int ar_check_shape(int32_t lanes, int32_t A, int32_t K, int32_t flags) {
    if (lanes != 1 && lanes != 2) {
        sgx_set_error("bad argument: lanes %d is not 1 (real records) or 2 (interleaved I/Q)", (int)lanes);
        return SGX_E_ARG;
    }
    if (A < 2 || A > SGX_ARRAY_MAX_ANTENNAS) {
        sgx_set_error("bad argument: A = %d antennas lie outside 2 .. %d", (int)A, SGX_ARRAY_MAX_ANTENNAS);
        return SGX_E_ARG;
    }
    if (K < 1 || K > SGX_ARRAY_MAX_TAPS || (K & 1) == 0) {
        sgx_set_error("bad argument: K = %d is not an odd number in 1 .. %d", (int)K, SGX_ARRAY_MAX_TAPS);
        return SGX_E_ARG;
    }
    if (A * K > SGX_ARRAY_MAX_WEIGHTS) {
        sgx_set_error("bad argument: A K = %d weights are more than %d", (int)(A * K), SGX_ARRAY_MAX_WEIGHTS);
        return SGX_E_ARG;
    }
    if (flags & ~SGX_ARRAY_OFFSET_BINARY) {
        sgx_set_error("bad argument: flags 0x%x holds a bit other than SGX_ARRAY_OFFSET_BINARY", (unsigned)flags);
        return SGX_E_ARG;
    }
    return SGX_OK;
}

static int ar_check_record(const sgx_if* rec, int32_t lanes, int32_t A) {
    if (rec->n % (size_t)(A * lanes)) {
        sgx_set_error("bad argument: a record of %d antennas (lanes %d) holds whole frames of %d bytes, not %zu bytes", (int)A,
                      (int)lanes, (int)(A * lanes), rec->n);
        return SGX_E_ARG;
    }
    return SGX_OK;
}

// The tap images of one set of taps, into g, which is zero: G_a[j] = the tap at frame offset j - AR_CQ, h_a[cc - (j - AR_CQ)]
// (I/Q: re, im, -im per antenna).  Returns `steps` grown to the steps that hold a tap other than zero.
static int ar_tap_pairs(int32_t lanes, int32_t A) { return A * (lanes == 2 ? 3 : 1) * (AR_LQ / 4); }
static FirSteps ar_pack_taps(const int16_t* taps, int32_t lanes, int32_t A, int32_t K, uint2* g, FirSteps steps) {
    const int cc = (K - 1) / 2, per_antenna = ar_tap_pairs(lanes, 1);
    for (int a = 0; a < A; ++a)
        steps = fir_pack_image(taps + (size_t)a * K * lanes, K, lanes, 16 / lanes, g + (size_t)a * per_antenna, AR_LQ / 4,
                               [&](int j) { return cc - (j - AR_CQ); }, steps);
    return steps;
}

// The refusals of the blocks that the two block entry points share: B (no device needed), and the number of blocks that
// `frames` frames make
static int ar_check_block_length(int64_t B) {
    if (B < 1 || B % SGX_ARRAY_BLOCK_UNIT) {
        sgx_set_error("bad argument: B = %lld frames is no positive multiple of SGX_ARRAY_BLOCK_UNIT = %d", (long long)B,
                      SGX_ARRAY_BLOCK_UNIT);
        return SGX_E_ARG;
    }
    return SGX_OK;
}
static int ar_check_blocks(int64_t B, unsigned long long frames, unsigned long long* n_blocks) {
    *n_blocks = (frames + (unsigned long long)B - 1) / (unsigned long long)B;
    if (*n_blocks > SGX_ARRAY_MAX_BLOCKS) {
        sgx_set_error("bad argument: %llu blocks of B = %lld frames are more than SGX_ARRAY_MAX_BLOCKS = %d", *n_blocks,
                      (long long)B, SGX_ARRAY_MAX_BLOCKS);
        return SGX_E_ARG;
    }
    return SGX_OK;
}

extern "C" int sgx_array_stats_tile(int32_t* tile_frames) {
    SGX_CHECK_ARG(tile_frames);
    *tile_frames = AR_TILE;
    return SGX_OK;
}

extern "C" int sgx_combine_tile(int32_t* tile_bytes) {
    SGX_CHECK_ARG(tile_bytes);
    *tile_bytes = FIR_TILE;
    return SGX_OK;
}

extern "C" int sgx_array_stats_timing(sgx_ctx* c, float* kernel_ms) {
    SGX_CHECK_ARG(c && kernel_ms);
    *kernel_ms = c->stage_ms[SGX_STAGE_ARRAY_STATS];
    return SGX_OK;
}

extern "C" int sgx_combine_timing(sgx_ctx* c, float* kernel_ms) {
    SGX_CHECK_ARG(c && kernel_ms);
    *kernel_ms = c->stage_ms[SGX_STAGE_COMBINE];
    return SGX_OK;
}

extern "C" int sgx_array_stats(sgx_ctx* c, const sgx_if* rec, int32_t lanes, int32_t A, int32_t K, int32_t flags,
                               int64_t* rho) {
    int rc = ar_check_shape(lanes, A, K, flags);
    if (rc != SGX_OK) return rc;
    SGX_CHECK_ARG(c && rec && rho);
    SGX_CHECK_ARG(rec->device == c->device);
    rc = ar_check_record(rec, lanes, A);
    if (rc != SGX_OK) return rc;
    rc = sgx_stage_open(c, rec, rec->n);
    if (rc != SGX_OK) return rc;

    const unsigned long long frames = rec->n / (size_t)(A * lanes);
    ArStats l;
    l.st = c->stream;
    l.tiles = (frames + AR_TILE - 1) / AR_TILE;
    l.grid = (unsigned)(l.tiles < AR_MAX_GRID ? l.tiles : AR_MAX_GRID);
    l.x = rec->d;
    l.n = (unsigned long long)rec->n;
    l.K = K;
    l.flip = (flags & SGX_ARRAY_OFFSET_BINARY) ? 0x80808080u : 0u;
    l.sums = c->d_small->array_sum;
    unsigned long long* h_sum = c->h_small->array_sum;
    SgxStage st(SGX_STAGE_ARRAY_STATS, l.grid, "array statistics kernel failed: %s");
    st.count_into(h_sum, l.sums, sizeof(SgxSmall::array_sum));
    rc = sgx_stage_run(c, st, [&](sgx_if*) { ar_launch(lanes, A, l); });
    if (rc != SGX_OK) return rc;
    const int n_val = A * A * K * lanes;
    for (int i = 0; i < n_val; ++i) {
        unsigned long long t = 0;   // (two's complement: the copies add up modulo 2^64)
        for (int s = 0; s < AR_SUM_SLOTS; ++s) t += h_sum[(size_t)s * AR_SUM_VALUES + i];
        rho[i] = (int64_t)t;
    }
    return SGX_OK;
}

extern "C" int sgx_if_combine(sgx_ctx* c, const sgx_if* rec, int32_t lanes, int32_t A, const int16_t* taps, int32_t K,
                              int32_t shift, int32_t flags, sgx_if** out, int64_t* clipped) {
    // the shape and the taps first: these refusals need no device
    int rc = ar_check_shape(lanes, A, K, flags);
    if (rc != SGX_OK) return rc;
    rc = fir_check_shift(shift);
    if (rc != SGX_OK) return rc;
    SGX_CHECK_ARG(taps);
    // (all antennas add into one sum, so the bound is on the sum over all of them; lanes = 2: of |re| + |im|)
    rc = fir_check_taps(taps, lanes * A * K);
    if (rc != SGX_OK) return rc;
    SGX_CHECK_ARG(c && rec && out);
    SGX_CHECK_ARG(rec->device == c->device);
    rc = ar_check_record(rec, lanes, A);
    if (rc != SGX_OK) return rc;
    const size_t n_out = rec->n / (size_t)A;
    const unsigned long long tiles = ((unsigned long long)n_out + FIR_TILE - 1) / FIR_TILE;
    rc = sgx_stage_one_launch(tiles, "bad argument: a record of %zu output bytes is beyond one launch of the combiner", n_out);
    if (rc != SGX_OK) return rc;
    rc = sgx_stage_open(c, rec, rec->n);
    if (rc != SGX_OK) return rc;

    const int pairs = ar_tap_pairs(lanes, A);
    uint2* g = fir_tap_image(c, pairs);
    FirLaunch l(c, rec, tiles, n_out, shift, (flags & SGX_ARRAY_OFFSET_BINARY) != 0);
    l.steps = ar_pack_taps(taps, lanes, A, K, g, l.steps);
    SgxStage st(SGX_STAGE_COMBINE, l.grid, "combine kernel failed: %s", out, n_out);
    st.up = {c->d_small->fir_taps, g, (size_t)pairs * sizeof(uint2)};
    return fir_run_counted(c, st, l, clipped, [&] { ar_launch(lanes, A, l); });
}

extern "C" int sgx_array_block_stats_timing(sgx_ctx* c, float* kernel_ms) {
    SGX_CHECK_ARG(c && kernel_ms);
    *kernel_ms = c->stage_ms[SGX_STAGE_ARRAY_BLOCK_STATS];
    return SGX_OK;
}

extern "C" int sgx_combine_blocks_timing(sgx_ctx* c, float* kernel_ms) {
    SGX_CHECK_ARG(c && kernel_ms);
    *kernel_ms = c->stage_ms[SGX_STAGE_COMBINE_BLOCKS];
    return SGX_OK;
}

extern "C" int sgx_array_block_stats(sgx_ctx* c, const sgx_if* rec, int32_t lanes, int32_t A, int32_t K, int32_t flags,
                                     int64_t B, int64_t* rho_blocks) {
    int rc = ar_check_shape(lanes, A, K, flags);
    if (rc == SGX_OK) rc = ar_check_block_length(B);
    if (rc != SGX_OK) return rc;
    SGX_CHECK_ARG(c && rec && rho_blocks);
    SGX_CHECK_ARG(rec->device == c->device);
    rc = ar_check_record(rec, lanes, A);
    if (rc != SGX_OK) return rc;
    const unsigned long long frames = rec->n / (size_t)(A * lanes);
    unsigned long long n_blocks;
    rc = ar_check_blocks(B, frames, &n_blocks);
    if (rc != SGX_OK) return rc;
    rc = sgx_stage_open(c, rec, rec->n);
    if (rc != SGX_OK) return rc;
    const size_t bytes = (size_t)n_blocks * (size_t)(A * A * K * lanes) * sizeof(unsigned long long);
    if (bytes) rc = c->d_array_blocks.ensure(bytes);
    if (rc != SGX_OK) return rc;

    ArStats l;
    l.st = c->stream;
    l.tiles = (frames + AR_TILE - 1) / AR_TILE;
    // a block's tiles go to one workgroup, or - few blocks - to as many as fill the grid the whole-record kernel runs on
    const unsigned long long tpb = (unsigned long long)B / AR_TILE;
    l.tpb = (unsigned)(tpb < l.tiles ? tpb : l.tiles);
    l.parts = 1;
    if (n_blocks) {
        const unsigned long long want = (AR_MAX_GRID + n_blocks - 1) / n_blocks;
        l.parts = (unsigned)(want < l.tpb ? want : l.tpb);
    }
    l.grid = (unsigned)(n_blocks * l.parts);
    l.x = rec->d;
    l.n = (unsigned long long)rec->n;
    l.K = K;
    l.flip = (flags & SGX_ARRAY_OFFSET_BINARY) ? 0x80808080u : 0u;
    l.sums = c->d_array_blocks;
    SgxStage st(SGX_STAGE_ARRAY_BLOCK_STATS, l.grid, "array block statistics kernel failed: %s");
    st.count_into(rho_blocks, l.sums, bytes);   // (the table is the counters: cleared, added into, copied down)
    return sgx_stage_run(c, st, [&](sgx_if*) { ar_launch(lanes, A, l); });
}

extern "C" int sgx_if_combine_blocks(sgx_ctx* c, const sgx_if* rec, int32_t lanes, int32_t A, const int16_t* taps,
                                     int64_t n_blocks, int64_t B, int32_t K, int32_t shift, int32_t flags, sgx_if** out,
                                     int64_t* clipped) {
    // the shape and the taps of every block first: these refusals need no device
    int rc = ar_check_shape(lanes, A, K, flags);
    if (rc != SGX_OK) return rc;
    rc = fir_check_shift(shift);
    if (rc != SGX_OK) return rc;
    SGX_CHECK_ARG(taps);
    rc = ar_check_block_length(B);
    if (rc != SGX_OK) return rc;
    if (n_blocks < 0 || n_blocks > SGX_ARRAY_MAX_BLOCKS) {
        sgx_set_error("bad argument: n_blocks = %lld lies outside 0 .. SGX_ARRAY_MAX_BLOCKS = %d", (long long)n_blocks,
                      SGX_ARRAY_MAX_BLOCKS);
        return SGX_E_ARG;
    }
    const int per_block = lanes * A * K;
    for (int64_t j = 0; j < n_blocks; ++j) {
        if (fir_check_taps(taps + (size_t)j * per_block, per_block) == SGX_OK) continue;
        char why[256];
        sgx_last_error(why, sizeof why);
        sgx_set_error("%s, in the taps of block %lld", why, (long long)j);
        return SGX_E_ARG;
    }
    SGX_CHECK_ARG(c && rec && out);
    SGX_CHECK_ARG(rec->device == c->device);
    rc = ar_check_record(rec, lanes, A);
    if (rc != SGX_OK) return rc;
    const size_t n_out = rec->n / (size_t)A;
    unsigned long long blocks_of_record;
    rc = ar_check_blocks(B, (unsigned long long)(n_out / (size_t)lanes), &blocks_of_record);
    if (rc != SGX_OK) return rc;
    if (blocks_of_record != (unsigned long long)n_blocks) {
        sgx_set_error("bad argument: n_blocks = %lld sets of taps for a record of %llu blocks of B = %lld frames",
                      (long long)n_blocks, blocks_of_record, (long long)B);
        return SGX_E_ARG;
    }
    const unsigned long long tiles = ((unsigned long long)n_out + FIR_TILE - 1) / FIR_TILE;
    rc = sgx_stage_one_launch(tiles, "bad argument: a record of %zu output bytes is beyond one launch of the combiner", n_out);
    if (rc != SGX_OK) return rc;
    rc = sgx_stage_open(c, rec, rec->n);
    if (rc != SGX_OK) return rc;

    // every block's tap images, one table; the steps are those that hold a tap other than zero in ANY block (a zero tap adds
    // nothing, so each block's bytes are what its own steps would give)
    const int pairs = ar_tap_pairs(lanes, A);
    std::vector<uint2> g((size_t)n_blocks * pairs, make_uint2(0u, 0u));
    FirLaunch l(c, rec, tiles, n_out, shift, (flags & SGX_ARRAY_OFFSET_BINARY) != 0);
    for (int64_t j = 0; j < n_blocks; ++j)
        l.steps = ar_pack_taps(taps + (size_t)j * per_block, lanes, A, K, g.data() + (size_t)j * pairs, l.steps);
    if (!g.empty()) rc = c->d_array_taps.ensure(g.size() * sizeof(uint2));
    if (rc != SGX_OK) return rc;
    l.taps = c->d_array_taps;
    // (a block is a whole number of tiles; a single block longer than the record's tiles is all of them)
    const unsigned long long tpb = (unsigned long long)B * lanes / FIR_TILE;
    l.tpb = (unsigned)(tpb < tiles ? tpb : (tiles ? tiles : 1));
    SgxStage st(SGX_STAGE_COMBINE_BLOCKS, l.grid, "block combine kernel failed: %s", out, n_out);
    st.up = {c->d_array_taps.get(), g.data(), g.size() * sizeof(uint2)};
    return fir_run_counted(c, st, l, clipped, [&] { ar_launch(lanes, A, l); });
}
