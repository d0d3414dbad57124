// Block-wise front-end conditioning in front of the I/Q converter: a resident record of int8, offset-binary or little-endian
// int16 elements, L = 1 or 2 lanes per frame -> per-block statistics, and with a per-block plan (DC, gain, blanking
// threshold) -> a NEW int8 record, one byte per element (include/sgx.h: sgx_cond_block_stats, sgx_if_condition; contract:
// tests/cond_spec.py block_stats(), condition()).  Everything here is integer arithmetic, so both kernels are tested byte
// for byte.  The plan itself is host code (sgx_cond.cpp).
//
//   cond_stats_kernel  one workgroup owns one block of B frames (at most 64 KB).  Its T lanes read the block ONCE, NCH
//                      16-byte chunks per lane (chunk c of the block sits in lane c % T), and keep it in registers: 256 lanes
//                      with 1 or 4 chunks for blocks up to 4 and 16 KB, 1024 lanes with 4 chunks beyond; the last chunk of
//                      the record's last block is read byte by byte, inside the record only.
//                      Four reductions run on the resident copy: the lane sums (-> DC), sum and maximum of the frame
//                      energies, and the two clipping rounds' (count, sum).  Each is a shuffle tree over the wave and one
//                      LDS step across the waves, after which EVERY lane folds the wave partials itself (the same
//                      instructions one lane would need, and no second barrier).  No atomics; one 64-byte result per block.
//   cond_apply_kernel  a workgroup makes CD_TILE frames, 16 per lane: 1, 2 or 4 16-byte loads and 1 or 2 16-byte stores per
//                      lane.  A block is a multiple of 16 frames, so a lane's 16 frames share one plan entry; the entries of
//                      the blocks a tile and its halo touch are staged in LDS first.  Every lane leaves the hit mask of its
//                      16 frames in LDS, the first 2 CD_HALO lanes also those of the CD_HALO groups either side of the tile
//                      (read again from the record, cut at its ends); the dilation is a windowed OR over the 9 masks
//                      around a lane's own.  The group that holds the record's end loads and stores byte by byte.  Blanked
//                      frames and outputs on +-127 are counters 0 and 1 of the stage counters (sgx_count.h), one integer
//                      atomic per workgroup each.
#include <limits.h>

#include <type_traits>

#include "sgx_stage.h"

#define CD_THREADS 256
#define CD_WAVES (CD_THREADS / 64)
#define CD_GROUP 16                          // frames per lane of the apply kernel
#define CD_TILE (CD_THREADS * CD_GROUP)      // frames per workgroup of the apply kernel
#define CD_HALO 4                            // groups either side of a tile: CD_HALO * CD_GROUP >= the largest guard
#define CD_PLAN_MAX 20                       // plan entries of a tile and its halo: (255 + CD_TILE + 128) / 256 + 1 = 18
#define CD_BLOCK_MIN 256
#define CD_BLOCK_MAX 16384
#define CD_GUARD_MAX 64
#define CD_DC_MAX (1 << 20)
static_assert(CD_HALO * CD_GROUP >= CD_GUARD_MAX, "the halo covers the guard");
static_assert((CD_BLOCK_MIN - 1 + CD_TILE + 2 * CD_HALO * CD_GROUP) / CD_BLOCK_MIN + 1 <= CD_PLAN_MAX, "the staged entries");
static_assert(CD_BLOCK_MAX * 4 <= 4 * 1024 * 16, "the largest block fits 4 chunks in each of 1024 lanes");
static_assert(sizeof(sgx_cond_stats) == 64 && sizeof(sgx_cond_entry) == 24, "include/sgx.h");

// element i (a compile-time index after unrolling) of the words w of W-byte elements; offset binary was undone on loading
template <int W> __device__ __forceinline__ int cd_elem(const unsigned* w, int i) {
    if (W == 1) return (int)(signed char)((w[i >> 2] >> (8 * (i & 3))) & 0xFFu);
    return (int)(short)((w[i >> 1] >> (16 * (i & 1))) & 0xFFFFu);
}

// energy of frame i of the words: sum over the lanes of (16 x - dc)^2, below 2^43
template <int W, int L> __device__ __forceinline__ long long cd_energy(const unsigned* w, int i, int dc0, int dc1) {
    const int d0 = 16 * cd_elem<W>(w, L * i) - dc0;
    long long e = (long long)d0 * d0;
    if (L == 2) {
        const int d1 = 16 * cd_elem<W>(w, 2 * i + 1) - dc1;
        e += (long long)d1 * d1;
    }
    return e;
}

// nb < 16 * NW bytes at p as NW * 4 words, zeros beyond; byte by byte, nothing outside [p, p + nb) is read
template <int NW> __device__ __forceinline__ void cd_load_bytes(const int8_t* p, int nb, unsigned* w) {
#pragma unroll
    for (int j = 0; j < 4 * NW; ++j) w[j] = 0u;
#pragma unroll
    for (int b = 0; b < 16 * NW; ++b)
        if (b < nb) w[b >> 2] |= (unsigned)(unsigned char)p[b] << (8 * (b & 3));
}

// ---- statistics ----------------------------------------------------------------------------------------------------------
// Two values per lane -> the same two totals in every lane.  s: this reduction's own [WAVES][2] slots (each of the four
// reductions has its own, so one barrier per reduction is enough).  MAX1: the second value is a maximum, else a sum.
template <bool MAX1, int WAVES> __device__ __forceinline__ void cd_reduce2(long long& a, long long& b, long long (*s)[2]) {
    a = sgx_wave_sum(a);
    b = MAX1 ? sgx_wave_max(b) : sgx_wave_sum(b);
    if ((threadIdx.x & 63) == 0) {
        s[threadIdx.x >> 6][0] = a;
        s[threadIdx.x >> 6][1] = b;
    }
    __syncthreads();
    a = s[0][0];
    b = s[0][1];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) {
        a += s[w][0];
        b = MAX1 ? (s[w][1] > b ? s[w][1] : b) : b + s[w][1];
    }
}

// The resident copy passes through an empty asm statement between two passes over it: each pass then extracts the elements
// from the words again instead of keeping every frame's energy (two registers each) alive across the reductions.
template <int N> __device__ __forceinline__ void cd_keep_words(unsigned (*v)[4]) {
#pragma unroll
    for (int j = 0; j < N; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) asm volatile("" : "+v"(v[j][q]));
}

__device__ __forceinline__ long long cd_floor_div(long long a, long long b) {   // b > 0
    long long q = a / b;
    if (a % b != 0 && a < 0) --q;
    return q;
}

// x: the record; n_frames = F; block = B; xmask: 0x80808080 for offset binary, else 0.  out[blockIdx.x]: the block's result.
template <int W, int L, int NCH, int T>
__global__ __launch_bounds__(T) void cond_stats_kernel(const int8_t* __restrict__ x, unsigned long long n_frames,
                                                                int block, int blank_q4, unsigned xmask,
                                                                sgx_cond_stats* __restrict__ out) {
    constexpr int FB = W * L;          // bytes per frame
    constexpr int FPC = 16 / FB;       // frames per chunk
    __shared__ long long s_red[4][T / 64][2];
    const unsigned long long f0 = (unsigned long long)blockIdx.x * (unsigned long long)block;
    const unsigned long long left = n_frames - f0;
    const int nk = left < (unsigned long long)block ? (int)left : block;
    const int8_t* __restrict__ base = x + f0 * FB;
    const int nbytes = nk * FB;
    unsigned v[NCH][4];
    int nv[NCH];                       // frames of chunk j that belong to the block
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int off = 16 * ((int)threadIdx.x + j * T);
        const int rest = nbytes - off;
        nv[j] = rest <= 0 ? 0 : (rest >= 16 ? FPC : rest / FB);
        if (rest >= 16) {
            const uint4 q = *reinterpret_cast<const uint4*>(base + off);
            v[j][0] = q.x, v[j][1] = q.y, v[j][2] = q.z, v[j][3] = q.w;
        } else if (rest > 0) {
            cd_load_bytes<1>(base + off, rest, v[j]);
        } else {
            v[j][0] = v[j][1] = v[j][2] = v[j][3] = 0u;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) v[j][q] ^= xmask;
    }
    // 1: the lane sums -> the DC in 1/16 LSB
    long long s0 = 0, s1 = 0;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
#pragma unroll
        for (int i = 0; i < FPC; ++i) {
            if (i < nv[j]) {
                s0 += cd_elem<W>(v[j], L * i);
                if (L == 2) s1 += cd_elem<W>(v[j], 2 * i + 1);
            }
        }
    }
    cd_reduce2<false, T / 64>(s0, s1, s_red[0]);
    cd_keep_words<NCH>(v);
    const int dc0 = (int)cd_floor_div(16 * s0 + (nk >> 1), nk);
    const int dc1 = L == 2 ? (int)cd_floor_div(16 * s1 + (nk >> 1), nk) : 0;
    // 2: sum and maximum of the frame energies
    long long p_all = 0, e_max = 0;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
#pragma unroll
        for (int i = 0; i < FPC; ++i) {
            if (i < nv[j]) {
                const long long e = cd_energy<W, L>(v[j], i, dc0, dc1);
                p_all += e;
                e_max = e > e_max ? e : e_max;
            }
        }
    }
    cd_reduce2<true, T / 64>(p_all, e_max, s_red[1]);
    cd_keep_words<NCH>(v);
    // 3, 4: the clipping rounds
    long long kept = nk, p_kept = p_all;
    if (blank_q4) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const long long theta = ((p_kept / kept) * blank_q4) >> 4;
            long long m = 0, p = 0;
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
#pragma unroll
                for (int i = 0; i < FPC; ++i) {
                    if (i < nv[j]) {
                        const long long e = cd_energy<W, L>(v[j], i, dc0, dc1);
                        if (e <= theta) {
                            m += 1;
                            p += e;
                        }
                    }
                }
            }
            cd_reduce2<false, T / 64>(m, p, s_red[2 + r]);
            cd_keep_words<NCH>(v);
            kept = m, p_kept = p;
        }
    }
    if (threadIdx.x == 0) {
        sgx_cond_stats o;
        o.n = nk, o.kept = kept, o.dc0 = dc0, o.dc1 = dc1, o.p_kept = p_kept, o.p_all = p_all, o.e_max = e_max, o.reserved = 0;
        out[blockIdx.x] = o;
    }
}

// ---- apply -----------------------------------------------------------------------------------------------------------------
// the group of CD_GROUP frames that starts at frame f0 (a multiple of CD_GROUP, below n_frames), nv of them inside the
// record, as FB * 4 words
template <int W, int L>
__device__ __forceinline__ void cd_load_group(const int8_t* __restrict__ x, unsigned long long f0, int nv, unsigned xmask,
                                              unsigned* w) {
    constexpr int FB = W * L;
    const int8_t* __restrict__ p = x + f0 * FB;
    if (nv == CD_GROUP) {
#pragma unroll
        for (int j = 0; j < FB; ++j) {
            const uint4 q = reinterpret_cast<const uint4*>(p)[j];
            w[4 * j] = q.x, w[4 * j + 1] = q.y, w[4 * j + 2] = q.z, w[4 * j + 3] = q.w;
        }
    } else {
        cd_load_bytes<FB>(p, nv * FB, w);
    }
#pragma unroll
    for (int j = 0; j < 4 * FB; ++j) w[j] ^= xmask;
}

// bit i: frame i of the group (i < nv) is hit
template <int W, int L>
__device__ __forceinline__ unsigned cd_hits(const unsigned* w, int nv, const sgx_cond_entry& e) {
    unsigned m = 0;
#pragma unroll
    for (int i = 0; i < CD_GROUP; ++i)
        if (i < nv && cd_energy<W, L>(w, i, e.dc0, e.dc1) > (long long)e.theta) m |= 1u << i;
    return m;
}

// plan[n_plan]: one entry per block.  count: the stage counters, zeroed; counter 0 takes the blanked frames, counter 1 the
// outputs on +-127.
template <int W, int L>
__global__ __launch_bounds__(CD_THREADS) void cond_apply_kernel(const int8_t* __restrict__ x, int8_t* __restrict__ y,
                                                                unsigned long long n_frames, int block,
                                                                const sgx_cond_entry* __restrict__ plan,
                                                                unsigned long long n_plan, int guard, unsigned xmask,
                                                                unsigned long long* __restrict__ count) {
    constexpr int FB = W * L;
    __shared__ sgx_cond_entry s_plan[CD_PLAN_MAX];
    __shared__ unsigned short s_hit[CD_THREADS + 2 * CD_HALO];
    const int t = (int)threadIdx.x;
    const unsigned long long tile_f0 = (unsigned long long)blockIdx.x * CD_TILE;
    // the blocks of the tile and its halo: kfirst .. kfirst + n_ent - 1; base_f = the first frame of block kfirst
    const unsigned long long halo_f0 = tile_f0 >= CD_HALO * CD_GROUP ? tile_f0 - CD_HALO * CD_GROUP : 0ull;
    const unsigned long long kfirst = halo_f0 / (unsigned long long)block;
    const unsigned long long base_f = kfirst * (unsigned long long)block;
    const unsigned long long want_end = tile_f0 + CD_TILE + CD_HALO * CD_GROUP;
    const unsigned long long f_end = want_end < n_frames ? want_end : n_frames;     // (> tile_f0: the grid covers the record)
    const int n_ent = (int)((unsigned)(f_end - 1 - base_f) / (unsigned)block) + 1;
    if (t < n_ent && t < CD_PLAN_MAX && kfirst + t < n_plan) s_plan[t] = plan[kfirst + t];
    __syncthreads();
    // this lane's group
    const unsigned long long g_f0 = tile_f0 + (unsigned long long)(CD_GROUP * t);
    const int nv = g_f0 >= n_frames ? 0 : (n_frames - g_f0 >= CD_GROUP ? CD_GROUP : (int)(n_frames - g_f0));
    unsigned w[4 * FB];
    sgx_cond_entry ent = s_plan[0];
    if (nv > 0) {
        cd_load_group<W, L>(x, g_f0, nv, xmask, w);
        ent = s_plan[(unsigned)(g_f0 - base_f) / (unsigned)block];
    } else {
#pragma unroll
        for (int j = 0; j < 4 * FB; ++j) w[j] = 0u;
    }
    s_hit[CD_HALO + t] = (unsigned short)cd_hits<W, L>(w, nv, ent);
    if (t < 2 * CD_HALO) {
        // a halo group: CD_HALO in front of the tile, CD_HALO behind it; nothing outside the record
        const int hg = t < CD_HALO ? t - CD_HALO : CD_THREADS + (t - CD_HALO);
        unsigned m = 0;
        const bool before = hg < 0 && tile_f0 < (unsigned long long)(-hg * CD_GROUP);
        const unsigned long long h_f0 = before ? 0ull : tile_f0 + (unsigned long long)((long long)hg * CD_GROUP);
        if (!before && h_f0 < n_frames) {
            const int hv = n_frames - h_f0 >= CD_GROUP ? CD_GROUP : (int)(n_frames - h_f0);
            unsigned hw[4 * FB];
            cd_load_group<W, L>(x, h_f0, hv, xmask, hw);
            m = cd_hits<W, L>(hw, hv, s_plan[(unsigned)(h_f0 - base_f) / (unsigned)block]);
        }
        s_hit[CD_HALO + hg] = (unsigned short)m;
    }
    __syncthreads();
    // the dilation: lo = the CD_HALO groups in front of this lane's (bit p = frame p - 64 of it), hi = those behind it
    // (bit q = frame 16 + q)
    unsigned long long lo = 0, hi = 0;
#pragma unroll
    for (int j = 0; j < CD_HALO; ++j) {
        lo |= (unsigned long long)s_hit[t + j] << (16 * j);
        hi |= (unsigned long long)s_hit[t + CD_HALO + 1 + j] << (16 * j);
    }
    const unsigned own = s_hit[CD_HALO + t];
    unsigned blank = 0;
#pragma unroll
    for (int i = 0; i < CD_GROUP; ++i) {
        const int j0 = i - guard > 0 ? i - guard : 0, j1 = i + guard < CD_GROUP - 1 ? i + guard : CD_GROUP - 1;
        bool b = (own & ((2u << j1) - 1u) & ~((1u << j0) - 1u)) != 0;
        if (i < guard) b = b || (lo >> (64 + i - guard)) != 0;
        const int e = i + guard - CD_GROUP;      // the last bit of hi inside the window
        if (e >= 0) b = b || (e >= 63 ? hi : (hi & ((2ull << e) - 1ull))) != 0;
        blank |= b ? 1u << i : 0u;
    }
    const unsigned valid = nv == CD_GROUP ? 0xFFFFu : (1u << nv) - 1u;
    const unsigned n_blank = __popc(blank & valid);
    unsigned rails = 0;
    // the outputs
    if (nv > 0) {
        unsigned o[4 * L];
#pragma unroll
        for (int j = 0; j < 4 * L; ++j) o[j] = 0u;
        const long long rnd = 1ll << (ent.shift + 3);
        const int sh = ent.shift + 4;
#pragma unroll
        for (int e = 0; e < CD_GROUP * L; ++e) {
            const int i = e / L;
            const int d = 16 * cd_elem<W>(w, e) - ((L == 2 && (e & 1)) ? ent.dc1 : ent.dc0);
            long long q = ((long long)d * ent.mult + rnd) >> sh;
            q = q < -127 ? -127 : (q > 127 ? 127 : q);
            const unsigned b = ((blank >> i) & 1u) ? 0u : (unsigned)((int)q & 0xFF);
            o[e >> 2] |= b << (8 * (e & 3));
            rails += (i < nv && (b == 0x7Fu || b == 0x81u)) ? 1u : 0u;
        }
        int8_t* __restrict__ dst = y + g_f0 * L;
        if (nv == CD_GROUP) {
#pragma unroll
            for (int j = 0; j < L; ++j)
                reinterpret_cast<uint4*>(dst)[j] = make_uint4(o[4 * j], o[4 * j + 1], o[4 * j + 2], o[4 * j + 3]);
        } else {
#pragma unroll
            for (int b = 0; b < CD_GROUP * L; ++b)
                if (b < nv * L) dst[b] = (int8_t)((o[b >> 2] >> (8 * (b & 3))) & 0xFFu);
        }
    }
    const unsigned counts[2] = {n_blank, rails};
    sgx_count_publish<2, CD_WAVES>(counts, count);
}

// ---- host ------------------------------------------------------------------------------------------------------------------
struct CdShape {
    int w;                   // bytes per element
    unsigned xmask;
    size_t frames, blocks;   // F, K
};

// the arguments both device entry points share, before the record is looked at
static int cd_check_format(int32_t data_type, int32_t lanes, int32_t block, int32_t flags, CdShape* sh) {
    if (data_type != SGX_DT_INT8 && data_type != SGX_DT_INT16) {
        sgx_set_error("bad argument: data_type %d is neither SGX_DT_INT8 nor SGX_DT_INT16", (int)data_type);
        return SGX_E_ARG;
    }
    SGX_CHECK_ARG((flags & ~SGX_COND_OFFSET_BINARY) == 0);
    if ((flags & SGX_COND_OFFSET_BINARY) && data_type != SGX_DT_INT8) {
        sgx_set_error("bad argument: SGX_COND_OFFSET_BINARY is an 8-bit format, not data_type %d", (int)data_type);
        return SGX_E_ARG;
    }
    SGX_CHECK_ARG(lanes == 1 || lanes == 2);
    SGX_CHECK_ARG(block >= CD_BLOCK_MIN && block <= CD_BLOCK_MAX && block % 16 == 0);
    sh->w = data_type == SGX_DT_INT16 ? 2 : 1;
    sh->xmask = (flags & SGX_COND_OFFSET_BINARY) ? 0x80808080u : 0u;
    return SGX_OK;
}

static int cd_check_record(const sgx_if* rec, int32_t lanes, int32_t block, CdShape* sh) {
    if (rec->n % (size_t)(sh->w * lanes)) {
        sgx_set_error("bad argument: a record of %zu bytes does not hold whole frames of %d %d-byte elements", rec->n,
                      (int)lanes, sh->w);
        return SGX_E_ARG;
    }
    sh->frames = rec->n / (size_t)(sh->w * lanes);
    sh->blocks = (sh->frames + (size_t)block - 1) / (size_t)block;
    return SGX_OK;
}

extern "C" int sgx_cond_tile(int32_t* tile_frames) {
    SGX_CHECK_ARG(tile_frames);
    *tile_frames = CD_TILE;
    return SGX_OK;
}

extern "C" int sgx_cond_timing(sgx_ctx* c, float* stats_ms, float* apply_ms) {
    SGX_CHECK_ARG(c && stats_ms && apply_ms);
    *stats_ms = c->stage_ms[SGX_STAGE_COND_STATS];
    *apply_ms = c->stage_ms[SGX_STAGE_COND_APPLY];
    return SGX_OK;
}

// f(W, L) with the element width and the lanes of a frame as compile-time constants (std::integral_constant)
template <typename F>
static void cd_dispatch(int w, int lanes, F f) {
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    if (w == 1 && lanes == 1) f(I1(), I1());
    else if (w == 1) f(I1(), I2());
    else if (lanes == 1) f(I2(), I1());
    else f(I2(), I2());
}

template <int W, int L>
static void cd_launch_stats(sgx_ctx* c, const sgx_if* rec, const CdShape& sh, int block, int blank_q4, sgx_cond_stats* d_out) {
    const size_t chunks = ((size_t)block * W * L + 15) / 16;
    const unsigned grid = (unsigned)sh.blocks;
    if (chunks <= 256) {
        cond_stats_kernel<W, L, 1, 256><<<grid, 256, 0, c->stream>>>(rec->d, sh.frames, block, blank_q4, sh.xmask, d_out);
    } else if (chunks <= 4 * 256) {
        cond_stats_kernel<W, L, 4, 256><<<grid, 256, 0, c->stream>>>(rec->d, sh.frames, block, blank_q4, sh.xmask, d_out);
    } else {
        cond_stats_kernel<W, L, 4, 1024><<<grid, 1024, 0, c->stream>>>(rec->d, sh.frames, block, blank_q4, sh.xmask, d_out);
    }
}

extern "C" int sgx_cond_block_stats(sgx_ctx* c, const sgx_if* rec, int32_t data_type, int32_t lanes, int32_t block,
                                    int32_t blank_q4, int32_t flags, sgx_cond_stats* out, size_t out_cap, size_t* n_blocks) {
    CdShape sh;
    if (cd_check_format(data_type, lanes, block, flags, &sh) != SGX_OK) return SGX_E_ARG;
    SGX_CHECK_ARG(blank_q4 == 0 || (blank_q4 >= 16 && blank_q4 <= 4096));
    SGX_CHECK_ARG(c && rec && n_blocks);
    SGX_CHECK_ARG(rec->device == c->device);
    if (cd_check_record(rec, lanes, block, &sh) != SGX_OK) return SGX_E_ARG;
    if (out_cap < sh.blocks || (sh.blocks && !out)) {
        sgx_set_error("bad argument: out holds %zu entries, the record has %zu blocks", out ? out_cap : (size_t)0, sh.blocks);
        return SGX_E_ARG;
    }
    int rc = sgx_stage_one_launch(sh.blocks, "bad argument: a record of %zu blocks is beyond one launch of the statistics kernel",
                                  sh.blocks);
    if (rc == SGX_OK) rc = sgx_stage_open(c, rec, rec->n);
    if (rc != SGX_OK) return rc;
    c->stage_ms[SGX_STAGE_COND_STATS] = 0.0f;
    *n_blocks = sh.blocks;
    if (sh.blocks == 0) return SGX_OK;   // (an empty record: nothing is queued, nothing to wait for)
    rc = c->d_cond_stats.ensure(sh.blocks * sizeof(sgx_cond_stats));
    if (rc != SGX_OK) return rc;
    SgxStage st(SGX_STAGE_COND_STATS, (unsigned)sh.blocks, "conditioning statistics kernel failed: %s");
    st.down = {out, c->d_cond_stats.get(), sh.blocks * sizeof(sgx_cond_stats)};
    return sgx_stage_run(c, st, [&](sgx_if*) {
        cd_dispatch(sh.w, lanes, [&](auto W, auto L) {
            cd_launch_stats<decltype(W)::value, decltype(L)::value>(c, rec, sh, block, blank_q4, c->d_cond_stats);
        });
    });
}

extern "C" int sgx_if_condition(sgx_ctx* c, const sgx_if* rec, int32_t data_type, int32_t lanes, int32_t block, int32_t flags,
                                const sgx_cond_entry* plan, size_t n_plan, int32_t guard, sgx_if** out,
                                int64_t* blanked_frames, int64_t* clipped) {
    CdShape sh;
    if (cd_check_format(data_type, lanes, block, flags, &sh) != SGX_OK) return SGX_E_ARG;
    SGX_CHECK_ARG(guard >= 0 && guard <= CD_GUARD_MAX);
    SGX_CHECK_ARG(c && rec && out && (plan || n_plan == 0));
    SGX_CHECK_ARG(rec->device == c->device);
    if (cd_check_record(rec, lanes, block, &sh) != SGX_OK) return SGX_E_ARG;
    if (n_plan != sh.blocks) {
        sgx_set_error("bad argument: the plan has %zu entries, the record has %zu blocks", n_plan, sh.blocks);
        return SGX_E_ARG;
    }
    for (size_t k = 0; k < n_plan; ++k) {
        const sgx_cond_entry& e = plan[k];
        if (e.mult < 1 || e.mult > 32767 || e.shift < 0 || e.shift > 30 || e.dc0 < -CD_DC_MAX || e.dc0 > CD_DC_MAX ||
            e.dc1 < -CD_DC_MAX || e.dc1 > CD_DC_MAX || e.theta < 0) {
            sgx_set_error("bad argument: plan entry %zu is out of range (mult %d, shift %d, dc %d %d, theta %lld)", k,
                          (int)e.mult, (int)e.shift, (int)e.dc0, (int)e.dc1, (long long)e.theta);
            return SGX_E_ARG;
        }
    }
    const unsigned long long tiles = ((unsigned long long)sh.frames + CD_TILE - 1) / CD_TILE;
    int rc = sgx_stage_one_launch(tiles, "bad argument: a record of %zu frames is beyond one launch of the conditioning kernel",
                                  sh.frames);
    if (rc == SGX_OK) rc = sgx_stage_open(c, rec, rec->n);
    if (rc == SGX_OK && n_plan) rc = c->d_cond_plan.ensure(n_plan * sizeof(sgx_cond_entry));
    if (rc != SGX_OK) return rc;
    sgx_cond_entry* d_plan = c->d_cond_plan;
    SgxStage st(SGX_STAGE_COND_APPLY, (unsigned)tiles, "conditioning kernel failed: %s", out, sh.frames * (size_t)lanes);
    st.up = {d_plan, plan, n_plan * sizeof(sgx_cond_entry)};
    unsigned long long* d_cnt = st.count(c);
    rc = sgx_stage_run(c, st, [&](sgx_if* r) {
        cd_dispatch(sh.w, lanes, [&](auto W, auto L) {
            cond_apply_kernel<decltype(W)::value, decltype(L)::value><<<st.grid, CD_THREADS, 0, c->stream>>>(
                rec->d, r->d, sh.frames, block, d_plan, n_plan, guard, sh.xmask, d_cnt);
        });
    });
    if (rc != SGX_OK) return rc;
    if (blanked_frames) *blanked_frames = sgx_stage_count(c, 0);
    if (clipped) *clipped = sgx_stage_count(c, 1);
    return SGX_OK;
}
