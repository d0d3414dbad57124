// Unpacker, first of the record front-end stages: a resident record holding the raw bytes of a file of 1-, 2- or 4-bit
// samples -> a NEW int8 record, one byte per selected sample, through a caller's table of 2^b levels (include/sgx.h:
// sgx_unpack_table, sgx_if_unpack; contract: tests/unpack_spec.py).
//
// The host folds bit order, frame, first and take into ONE description of a period.  A period is the shortest run of whole
// bytes over which the selection repeats: P = max(F, 8 / b) fields = W = P b / 8 bytes (1, 2, 4 or 8), read as one
// little-endian word; it gives K = take P / F output bytes, output k being (word >> sh[k]) & (2^b - 1) through the table.
// N is a whole number of periods, n_out = (N / W) K.
//
//   unpack_kernel<B, W, K>  K a power of two (take is one).  A workgroup makes UP_TILE output bytes in UP_ITERS rounds; in a
//                           round a lane makes 16 of them from 16 / K periods = 16 W / K contiguous, aligned input bytes
//                           (2 .. 128: one load of that width, or 16-byte loads), and issues ONE 16-byte store, so a wave
//                           writes 1 KiB contiguously.  Everything about a lane's 16 outputs is static but the shifts, which
//                           are uniform (kernel arguments): an output costs a bit-field extract and an insert into a
//                           selector dword, and four selectors become four bytes by v_perm_b32 on the table, which sits in
//                           scalar registers (b = 4: two of them on the two halves of the table and a select).
//   unpack_any_kernel       any take: the same tiles, a lane's 16 outputs one by one with byte loads (up_slow_chunk, which
//                           is also how unpack_kernel makes the record's last partial group of 16).
//
// Code counts: a lane adds 1 << 4 code into a nibble-packed word for 8 outputs at a time, spreads the nibbles into two
// byte-packed 64-bit accumulators (even and odd codes; at most 16 UP_ITERS = 64 per byte) and keeps those over its rounds.
// At the end the 2^b counts are counters 0 .. 2^b - 1 of the stage counters (sgx_count.h): 2^b integer atomics per UP_TILE
// output bytes.
#include <type_traits>

#include "sgx_stage.h"

#define UP_THREADS 256
#define UP_ITERS 4
#define UP_TILE (UP_THREADS * 16 * UP_ITERS)   // output bytes per workgroup
static_assert(16 * UP_ITERS < 256, "a lane's count of one code fits a byte");

typedef unsigned long long up_u64;

struct UpArgs {
    unsigned tab[4];   // the table: entry c is byte c
    up_u64 sh[2];      // sh[k]: byte k & 7 of word k >> 3
    int W, K;          // bytes and outputs of a period
    unsigned mask;     // 2^b - 1
};

__device__ __forceinline__ unsigned up_shift(const UpArgs& a, unsigned k) {
    return (unsigned)((k < 8 ? a.sh[0] : a.sh[1]) >> (8 * (k & 7))) & 0xFFu;
}

// four codes, one per byte of sel -> their four table entries
template <int B> __device__ __forceinline__ unsigned up_lookup4(const UpArgs& a, unsigned sel) {
    if (B <= 2) return __builtin_amdgcn_perm(0u, a.tab[0], sel);   // selectors 0 .. 3: the bytes of the second operand
    const unsigned s7 = sel & 0x07070707u;
    const unsigned lo = __builtin_amdgcn_perm(a.tab[1], a.tab[0], s7);
    const unsigned hi = __builtin_amdgcn_perm(a.tab[3], a.tab[2], s7);
    const unsigned m = ((sel >> 3) & 0x01010101u) * 0xFFu;
    return (hi & m) | (lo & ~m);
}

// nibble-packed counts of at most 8 outputs (nibble c: code c) into the byte-packed accumulators: byte i of E is code 2 i,
// byte i of O code 2 i + 1
template <typename H> __device__ __forceinline__ void up_fold(H h, up_u64& E, up_u64& O) {
    const H m = (H)0x0F0F0F0F0F0F0F0Full;
    E += (up_u64)(h & m);
    O += (up_u64)((h >> 4) & m);
}

// The 16 output bytes from o0 on (those below n_out), one by one: any W, K
__device__ __forceinline__ void up_slow_chunk(const uint8_t* __restrict__ x, uint8_t* __restrict__ y, up_u64 o0, up_u64 n_out,
                                              const UpArgs& a, up_u64& E, up_u64& O) {
    up_u64 r = o0 / (unsigned)a.K;
    unsigned k = (unsigned)(o0 - r * (unsigned)a.K);
    unsigned out[4] = {0u, 0u, 0u, 0u};
    up_u64 h = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        if (o0 + i < n_out) {
            const unsigned s = up_shift(a, k);
            const unsigned code = ((unsigned)x[r * (unsigned)a.W + (s >> 3)] >> (s & 7)) & a.mask;
            out[i >> 2] |= (up_lookup4<4>(a, code) & 0xFFu) << (8 * (i & 3));
            h += 1ull << (4 * code);
            if (++k == (unsigned)a.K) k = 0, ++r;
        }
        if ((i & 7) == 7) up_fold(h, E, O), h = 0;
    }
    if (o0 + 16 <= n_out) {
        *reinterpret_cast<uint4*>(y + o0) = make_uint4(out[0], out[1], out[2], out[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (o0 + i < n_out) y[o0 + i] = (uint8_t)(out[i >> 2] >> (8 * (i & 3)));
    }
}

// counts: the stage counters, zeroed; counter c takes the lanes' counts of code c, bytes of E and O
template <int NC>
__device__ __forceinline__ void up_count_codes(up_u64 E, up_u64 O, up_u64* __restrict__ counts) {
    unsigned v[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) v[c] = (unsigned)(((c & 1) ? O : E) >> (8 * (c >> 1))) & 0xFFu;
    sgx_count_publish<NC, UP_THREADS / 64>(v, counts);
}

template <int B, int W, int K>
__global__ __launch_bounds__(UP_THREADS) void unpack_kernel(const uint8_t* __restrict__ x, uint8_t* __restrict__ y,
                                                            up_u64 n_out, UpArgs a, up_u64* __restrict__ counts) {
    constexpr int S = (16 / K) * W;        // input bytes of a lane's 16 outputs
    constexpr int D = (S + 3) / 4;
    typedef typename std::conditional<B == 4, up_u64, unsigned>::type nib_t;   // 2^b nibbles
    up_u64 E = 0, O = 0;
    const up_u64 chunk0 = (up_u64)blockIdx.x * (UP_THREADS * UP_ITERS) + threadIdx.x;
#pragma unroll 2
    for (int it = 0; it < UP_ITERS; ++it) {
        const up_u64 c = chunk0 + (up_u64)it * UP_THREADS;
        const up_u64 o0 = 16 * c;
        if (o0 + 16 <= n_out) {
            // periods [c 16 / K, (c + 1) 16 / K) lie inside the record: n_out = (N / W) K
            const uint8_t* src = x + c * S;
            unsigned d[D];
            if (S == 2) {
                d[0] = *reinterpret_cast<const unsigned short*>(src);
            } else if (S == 4) {
                d[0] = *reinterpret_cast<const unsigned*>(src);
            } else if (S == 8) {
                const uint2 v = *reinterpret_cast<const uint2*>(src);
                d[0] = v.x, d[1] = v.y;
            } else {
#pragma unroll
                for (int j = 0; j < S / 16; ++j) {
                    const uint4 v = reinterpret_cast<const uint4*>(src)[j];
                    d[4 * j] = v.x, d[4 * j + 1] = v.y, d[4 * j + 2] = v.z, d[4 * j + 3] = v.w;
                }
            }
            unsigned out[4];
            nib_t h = 0;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                unsigned sel = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int i = 4 * g + j;
                    const int per = i / K, k = i % K;       // static
                    const unsigned s = (unsigned)(a.sh[k >> 3] >> (8 * (k & 7))) & 0xFFu;   // uniform
                    unsigned code;
                    if (W == 8) {
                        code = (unsigned)((((up_u64)d[2 * per + 1] << 32) | d[2 * per]) >> s) & a.mask;
                    } else {
                        // a period lies inside one dword, and so does the field
                        code = (d[(per * W) / 4] >> (((per * W) % 4) * 8 + s)) & a.mask;
                    }
                    sel |= code << (8 * j);
                    h += (nib_t)1 << (4 * code);
                }
                out[g] = up_lookup4<B>(a, sel);
                if (g & 1) up_fold(h, E, O), h = 0;
            }
            *reinterpret_cast<uint4*>(y + o0) = make_uint4(out[0], out[1], out[2], out[3]);
        } else if (o0 < n_out) {
            up_slow_chunk(x, y, o0, n_out, a, E, O);    // the record's last partial group
        }
    }
    up_count_codes<(1 << B)>(E, O, counts);
}

__global__ __launch_bounds__(UP_THREADS) void unpack_any_kernel(const uint8_t* __restrict__ x, uint8_t* __restrict__ y,
                                                                up_u64 n_out, UpArgs a, up_u64* __restrict__ counts) {
    up_u64 E = 0, O = 0;
    const up_u64 chunk0 = (up_u64)blockIdx.x * (UP_THREADS * UP_ITERS) + threadIdx.x;
    for (int it = 0; it < UP_ITERS; ++it) {
        const up_u64 o0 = 16 * (chunk0 + (up_u64)it * UP_THREADS);
        if (o0 < n_out) up_slow_chunk(x, y, o0, n_out, a, E, O);
    }
    up_count_codes<16>(E, O, counts);
}

// ---- host ------------------------------------------------------------------------------------------------------------------
struct UpLaunch {
    hipStream_t st;
    unsigned grid;
    const uint8_t* x;
    uint8_t* y;
    up_u64 n_out;
    UpArgs a;
    up_u64* counts;
};

// K <= the fields of a period, 8 W / B
template <int B, int W, int K> static void up_launch_bwk(const UpLaunch& l) {
    if constexpr (K * B <= 8 * W) {
        unpack_kernel<B, W, K><<<l.grid, UP_THREADS, 0, l.st>>>(l.x, l.y, l.n_out, l.a, l.counts);
    }
}
template <int B, int W> static void up_launch_bw(const UpLaunch& l) {
    switch (l.a.K) {
        case 1: return up_launch_bwk<B, W, 1>(l);
        case 2: return up_launch_bwk<B, W, 2>(l);
        case 4: return up_launch_bwk<B, W, 4>(l);
        case 8: return up_launch_bwk<B, W, 8>(l);
        default: return up_launch_bwk<B, W, 16>(l);
    }
}
template <int B> static void up_launch_b(const UpLaunch& l) {
    switch (l.a.W) {
        case 1: return up_launch_bw<B, 1>(l);
        case 2: return up_launch_bw<B, 2>(l);
        case 4: return up_launch_bw<B, 4>(l);
        default: return up_launch_bw<B, 8>(l);
    }
}
static void up_launch(int bits, const UpLaunch& l) {
    if (l.a.K & (l.a.K - 1)) {
        unpack_any_kernel<<<l.grid, UP_THREADS, 0, l.st>>>(l.x, l.y, l.n_out, l.a, l.counts);
    } else if (bits == 1) {
        up_launch_b<1>(l);
    } else if (bits == 2) {
        up_launch_b<2>(l);
    } else {
        up_launch_b<4>(l);
    }
}

static int up_bits_ok(int32_t bits) {
    if (bits == 1 || bits == 2 || bits == 4) return 1;
    sgx_set_error("bad argument: bits %d is not 1, 2 or 4", (int)bits);
    return 0;
}

extern "C" int sgx_unpack_tile(int32_t* tile_bytes) {
    SGX_CHECK_ARG(tile_bytes);
    *tile_bytes = UP_TILE;
    return SGX_OK;
}

extern "C" int sgx_unpack_timing(sgx_ctx* c, float* kernel_ms) {
    SGX_CHECK_ARG(c && kernel_ms);
    *kernel_ms = c->stage_ms[SGX_STAGE_UNPACK];
    return SGX_OK;
}

extern "C" int sgx_unpack_table(int32_t bits, int32_t encoding, int32_t peak, int8_t* table) {
    if (!up_bits_ok(bits)) return SGX_E_ARG;
    if (encoding != SGX_UNPACK_SIGN_MAGNITUDE && encoding != SGX_UNPACK_OFFSET_BINARY && encoding != SGX_UNPACK_TWOS_COMPLEMENT) {
        sgx_set_error("bad argument: encoding %d is none of SGX_UNPACK_SIGN_MAGNITUDE, _OFFSET_BINARY, _TWOS_COMPLEMENT",
                      (int)encoding);
        return SGX_E_ARG;
    }
    const int levels = 1 << bits;
    if (peak < levels - 1 || peak > 127) {
        sgx_set_error("bad argument: peak %d lies outside %d .. 127", (int)peak, levels - 1);
        return SGX_E_ARG;
    }
    SGX_CHECK_ARG(table);
    const int scale = peak / (levels - 1);
    for (int c = 0; c < levels; ++c) {
        int level;
        if (encoding == SGX_UNPACK_SIGN_MAGNITUDE) {
            const int s = c >> (bits - 1), mu = c & ((1 << (bits - 1)) - 1);
            level = (1 - 2 * s) * (2 * mu + 1);
        } else if (encoding == SGX_UNPACK_OFFSET_BINARY) {
            level = 2 * c - (levels - 1);
        } else {
            level = 2 * (c >= levels / 2 ? c - levels : c) + 1;
        }
        table[c] = (int8_t)(level * scale);
    }
    return SGX_OK;
}

extern "C" int sgx_if_unpack(sgx_ctx* c, const sgx_if* rec, int32_t bits, int32_t flags, int32_t frame, int32_t first,
                             int32_t take, const int8_t* table, sgx_if** out, int64_t* code_counts) {
    // the format first: these refusals need no device
    if (!up_bits_ok(bits)) return SGX_E_ARG;
    if (flags & ~SGX_UNPACK_LSB_FIRST) {
        sgx_set_error("bad argument: flags 0x%x holds a bit other than SGX_UNPACK_LSB_FIRST", (unsigned)flags);
        return SGX_E_ARG;
    }
    if (frame != 1 && frame != 2 && frame != 4 && frame != 8 && frame != 16) {
        sgx_set_error("bad argument: frame %d is not 1, 2, 4, 8 or 16 fields", (int)frame);
        return SGX_E_ARG;
    }
    if (take < 1 || first < 0 || first > frame - take) {
        sgx_set_error("bad argument: first %d, take %d do not select fields of a frame of %d", (int)first, (int)take,
                      (int)frame);
        return SGX_E_ARG;
    }
    SGX_CHECK_ARG(c && rec && table && out);
    SGX_CHECK_ARG(rec->device == c->device);
    const int per_byte = 8 / bits;
    const int P = frame > per_byte ? frame : per_byte;   // fields of a period
    const int W = P * bits / 8, reps = P / frame, K = take * reps;
    if (rec->n % (size_t)W) {
        sgx_set_error("bad argument: the %zu bytes of the record do not hold whole frames of %d %d-bit fields", rec->n,
                      (int)frame, (int)bits);
        return SGX_E_ARG;
    }
    const size_t n_out = rec->n / (size_t)W * (size_t)K;
    const unsigned long long tiles = ((unsigned long long)n_out + UP_TILE - 1) / UP_TILE;
    int rc = sgx_stage_one_launch(tiles, "bad argument: a record of %zu samples is beyond one launch of the unpacker", n_out);
    if (rc != SGX_OK) return rc;
    rc = sgx_stage_open(c, rec, rec->n);
    if (rc != SGX_OK) return rc;
    UpLaunch l;
    l.st = c->stream;
    l.grid = (unsigned)tiles;
    l.x = reinterpret_cast<const uint8_t*>(rec->d);
    l.n_out = n_out;
    memset(&l.a, 0, sizeof(l.a));
    memcpy(l.a.tab, table, (size_t)1 << bits);
    l.a.W = W, l.a.K = K, l.a.mask = (1u << bits) - 1u;
    for (int rep = 0, k = 0; rep < reps; ++rep) {
        for (int t = 0; t < take; ++t, ++k) {
            const int f = rep * frame + first + t;   // the field's place in the period
            const int p = f % per_byte;
            const unsigned s = 8u * (unsigned)(f / per_byte) +
                               (unsigned)((flags & SGX_UNPACK_LSB_FIRST) ? bits * p : 8 - bits * (p + 1));
            l.a.sh[k >> 3] |= (up_u64)s << (8 * (k & 7));
        }
    }
    SgxStage st(SGX_STAGE_UNPACK, l.grid, "unpacker kernel failed: %s", out, n_out);
    l.counts = st.count(c);
    rc = sgx_stage_run(c, st, [&](sgx_if* r) {
        l.y = reinterpret_cast<uint8_t*>(r->d);
        up_launch(bits, l);
    });
    if (rc != SGX_OK) return rc;
    if (code_counts)
        for (int k = 0; k < 16; ++k) code_counts[k] = sgx_stage_count(c, k);
    return SGX_OK;
}
