// Requantiser in front of the I/Q converter: a resident record of little-endian int16 or IEEE float32 elements -> a NEW
// int8 record, one byte per element, through one fixed gain (include/sgx.h: sgx_requant_stats_of, sgx_requant_gain,
// sgx_if_requantize; contract: tests/requant_spec.py stats(), gain(), quantise()).  I and Q share the gain, so both
// kernels are elementwise and know nothing of pairs.
//
//   requant_stats_kernel  count of non-finite elements, max |x|, sum x, sum x^2 of a window of elements.  A FIXED grid of
//                         RQ_STATS_BLOCKS workgroups strides over the window's 16-byte chunks, RQ_STATS_UNROLL loads in
//                         flight per lane; a chunk that lies wholly inside the window is one 16-byte load, the (at most two)
//                         chunks that hold a window edge are read element by element, inside the window only.  Each lane
//                         accumulates its chunks in ascending order, the lanes of a wave are folded by a shuffle tree, the
//                         waves of a workgroup through LDS in wave order, and ONE partial per workgroup goes to memory; the
//                         host adds the partials in workgroup order after one small copy.  No atomics: the float sums of two
//                         calls on the same bytes and window are the same bits.  int16 sums are exact 64-bit integers (the
//                         host adds the partials in 128 bits and converts once); float32 elements are promoted to double,
//                         where the square is exact, and summed in double.  max |x| and the finite test work on the bit
//                         pattern, so they do not depend on the denormal mode.
//   requant_kernel        a lane makes 16 output bytes from 2 (int16) or 4 (float32) 16-byte loads, packs them in registers
//                         and issues one 16-byte store; the lane that holds the record's last partial group loads and stores
//                         element by element.  Nothing outside the record is read.  Outputs on +-127 are counted: counter 0
//                         of the stage counters (sgx_count.h), one integer atomic per workgroup.
#include <math.h>

#include "sgx_stage.h"

#define RQ_THREADS 256
#define RQ_TILE (RQ_THREADS * 16)   // output bytes (= elements) per workgroup
static_assert(RQ_STATS_BLOCKS * 4 * sizeof(unsigned long long) == sizeof(SgxSmall::requant_part), "one partial per workgroup");

template <int DT> struct RqType;
template <> struct RqType<SGX_DT_INT16> {
    static constexpr int W = 2;
    typedef long long sum_t;              // exact
    typedef unsigned long long sq_t;      // exact: x^2 <= 2^30
};
template <> struct RqType<SGX_DT_FLOAT32> {
    static constexpr int W = 4;
    typedef double sum_t;
    typedef double sq_t;
};

// ---- statistics ----------------------------------------------------------------------------------------------------------
template <int DT> struct RqAcc {
    typename RqType<DT>::sum_t sum;
    typename RqType<DT>::sq_t sq;
    unsigned long long bad;   // non-finite elements
    unsigned mx;              // int16: max |x|; float32: the largest bit pattern of |x| among the finite elements
};

// one element, as the 16 or 32 bits it occupies in the record
__device__ __forceinline__ void rq_add(RqAcc<SGX_DT_INT16>& a, unsigned bits) {
    const int v = (int)(short)(bits & 0xFFFFu);
    const unsigned m = (unsigned)(v < 0 ? -v : v);
    a.sum += v;
    a.sq += (unsigned long long)(m * m);
    a.mx = m > a.mx ? m : a.mx;
}
__device__ __forceinline__ void rq_add(RqAcc<SGX_DT_FLOAT32>& a, unsigned bits) {
    const unsigned m = bits & 0x7FFFFFFFu;
    const bool finite = m < 0x7F800000u;
    // a non-finite element adds +0.0 to both sums, which changes neither (they start at +0.0 and never become -0.0)
    const double d = finite ? (double)__uint_as_float(bits) : 0.0;
    a.sum += d;
    a.sq += d * d;   // exact product: 24 x 24 bits
    a.bad += finite ? 0ull : 1ull;
    a.mx = (finite && m > a.mx) ? m : a.mx;
}

template <int DT> __device__ __forceinline__ void rq_add_dword(RqAcc<DT>& a, unsigned w) {
    if (DT == SGX_DT_INT16) {
        rq_add(a, w & 0xFFFFu);
        rq_add(a, w >> 16);
    } else {
        rq_add(a, w);
    }
}

template <int DT> __device__ __forceinline__ void rq_fold(RqAcc<DT>& a, const RqAcc<DT>& b) {
    a.sum += b.sum;
    a.sq += b.sq;
    a.bad += b.bad;
    a.mx = b.mx > a.mx ? b.mx : a.mx;
}

template <typename T> __device__ __forceinline__ unsigned long long rq_bits(T v);
template <> __device__ __forceinline__ unsigned long long rq_bits<long long>(long long v) { return (unsigned long long)v; }
template <> __device__ __forceinline__ unsigned long long rq_bits<unsigned long long>(unsigned long long v) { return v; }
template <> __device__ __forceinline__ unsigned long long rq_bits<double>(double v) {
    return (unsigned long long)__double_as_longlong(v);
}

// x: the record; window = bytes [b0, b1) of it, both multiples of the element width.  part[4 blockIdx.x ..]: sum, sum of
// squares (bit patterns of the accumulators), non-finite count, max.
template <int DT>
__global__ __launch_bounds__(RQ_THREADS) void requant_stats_kernel(const int8_t* __restrict__ x, unsigned long long b0,
                                                                   unsigned long long b1,
                                                                   unsigned long long* __restrict__ part) {
    constexpr int W = RqType<DT>::W;
    __shared__ RqAcc<DT> s_wave[RQ_THREADS / 64];
    RqAcc<DT> acc;
    acc.sum = 0, acc.sq = 0, acc.bad = 0, acc.mx = 0;
    const unsigned long long c_end = (b1 + 15) / 16;   // chunk c = record bytes [16 c, 16 c + 16)
    const unsigned long long total = (unsigned long long)gridDim.x * RQ_THREADS;
    for (unsigned long long base = b0 / 16 + (unsigned long long)blockIdx.x * RQ_THREADS + threadIdx.x; base < c_end;
         base += RQ_STATS_UNROLL * total) {
        uint4 v[RQ_STATS_UNROLL];
#pragma unroll
        for (int j = 0; j < RQ_STATS_UNROLL; ++j) {
            const unsigned long long c = base + j * total;
            v[j] = make_uint4(0u, 0u, 0u, 0u);
            if (c < c_end && 16 * c >= b0 && 16 * c + 16 <= b1) v[j] = *reinterpret_cast<const uint4*>(x + 16 * c);
        }
#pragma unroll
        for (int j = 0; j < RQ_STATS_UNROLL; ++j) {
            const unsigned long long c = base + j * total;
            if (c >= c_end) break;
            if (16 * c >= b0 && 16 * c + 16 <= b1) {
                rq_add_dword(acc, v[j].x);
                rq_add_dword(acc, v[j].y);
                rq_add_dword(acc, v[j].z);
                rq_add_dword(acc, v[j].w);
            } else {
                // a chunk that holds an edge of the window: its elements inside the window, one by one
                for (int k = 0; k < 16 / W; ++k) {
                    const unsigned long long p = 16 * c + (unsigned long long)(W * k);
                    if (p < b0 || p >= b1) continue;
                    if (DT == SGX_DT_INT16) {
                        rq_add(acc, (unsigned)*reinterpret_cast<const unsigned short*>(x + p));
                    } else {
                        rq_add(acc, *reinterpret_cast<const unsigned*>(x + p));
                    }
                }
            }
        }
    }
    // lanes: a shuffle tree; waves: in wave order
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        RqAcc<DT> o;
        o.sum = __shfl_down(acc.sum, d, 64);
        o.sq = __shfl_down(acc.sq, d, 64);
        o.bad = __shfl_down(acc.bad, d, 64);
        o.mx = __shfl_down(acc.mx, d, 64);
        rq_fold(acc, o);
    }
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        RqAcc<DT> t = s_wave[0];
        for (int w = 1; w < RQ_THREADS / 64; ++w) rq_fold(t, s_wave[w]);
        unsigned long long* o = part + 4ull * blockIdx.x;
        o[0] = rq_bits(t.sum);
        o[1] = rq_bits(t.sq);
        o[2] = t.bad;
        o[3] = t.mx;
    }
}

// ---- the quantiser ---------------------------------------------------------------------------------------------------------
struct RqGain {
    int mult, rnd, shift;   // int16: y = clip((x mult + rnd) >> shift, -127, 127), rnd = (1 << shift) >> 1
    float scale;            // float32: y = clip(rint(x * scale), -127, 127), NaN -> 0
};

// the output byte of one element, given as its bits
template <int DT> __device__ __forceinline__ unsigned rq_byte(unsigned bits, const RqGain& g) {
    int v;
    if (DT == SGX_DT_INT16) {
        // exact in int32: |x mult| <= 2^15 (2^15 - 1), rnd <= 2^29; both factors fit 24 bits (v_mad_i32_i24, full rate)
        v = (__mul24((int)(short)(bits & 0xFFFFu), g.mult) + g.rnd) >> g.shift;
        v = v < -127 ? -127 : (v > 127 ? 127 : v);
    } else {
        const float p = __uint_as_float(bits) * g.scale;   // one IEEE multiply (the build has no contraction, no fast math)
        const float r = fminf(fmaxf(rintf(p), -127.0f), 127.0f);
        v = (p != p) ? 0 : (int)r;
    }
    return (unsigned)(v & 0xFF);
}

// bytes of a dword that are 0x7F or 0x81 (+-127)
__device__ __forceinline__ unsigned rq_on_rails(unsigned w) {
    unsigned n = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const unsigned v = (w >> (8 * b)) & 0xFFu;
        n += (v == 0x7Fu || v == 0x81u) ? 1u : 0u;
    }
    return n;
}

// n: elements of the record = bytes of y.  clip: the stage counters, zeroed; counter 0 takes the outputs on +-127.
template <int DT>
__global__ __launch_bounds__(RQ_THREADS) void requant_kernel(const int8_t* __restrict__ x, int8_t* __restrict__ y,
                                                             unsigned long long n, RqGain g,
                                                             unsigned long long* __restrict__ clip) {
    constexpr int W = RqType<DT>::W;
    const unsigned long long e0 = ((unsigned long long)blockIdx.x * RQ_THREADS + threadIdx.x) * 16;
    unsigned rails = 0;
    if (e0 + 16 <= n) {
        const uint4* __restrict__ src = reinterpret_cast<const uint4*>(x + e0 * W);
        uint4 v[W];
#pragma unroll
        for (int j = 0; j < W; ++j) v[j] = src[j];
        unsigned out[4];
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const unsigned w4[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
            if (DT == SGX_DT_INT16) {
                // 8 elements of this load -> output dwords 2 j, 2 j + 1
#pragma unroll
                for (int h = 0; h < 2; ++h)
                    out[2 * j + h] = rq_byte<DT>(w4[2 * h], g) | (rq_byte<DT>(w4[2 * h] >> 16, g) << 8) |
                                     (rq_byte<DT>(w4[2 * h + 1], g) << 16) | (rq_byte<DT>(w4[2 * h + 1] >> 16, g) << 24);
            } else {
                out[j] = rq_byte<DT>(w4[0], g) | (rq_byte<DT>(w4[1], g) << 8) | (rq_byte<DT>(w4[2], g) << 16) |
                         (rq_byte<DT>(w4[3], g) << 24);
            }
        }
        *reinterpret_cast<uint4*>(y + e0) = make_uint4(out[0], out[1], out[2], out[3]);
        rails = rq_on_rails(out[0]) + rq_on_rails(out[1]) + rq_on_rails(out[2]) + rq_on_rails(out[3]);
    } else if (e0 < n) {
        // the record's last partial group
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (e0 + r < n) {
                const int8_t* p = x + (e0 + r) * W;
                const unsigned bits = DT == SGX_DT_INT16 ? (unsigned)*reinterpret_cast<const unsigned short*>(p)
                                                         : *reinterpret_cast<const unsigned*>(p);
                const unsigned b = rq_byte<DT>(bits, g);
                y[e0 + r] = (int8_t)b;
                rails += (b == 0x7Fu || b == 0x81u) ? 1u : 0u;
            }
        }
    }
    const unsigned count[1] = {rails};
    sgx_count_publish<1, RQ_THREADS / 64>(count, clip);
}

// ---- host ------------------------------------------------------------------------------------------------------------------
static int rq_width(int32_t data_type) {
    if (data_type == SGX_DT_INT16) return 2;
    if (data_type == SGX_DT_FLOAT32) return 4;
    sgx_set_error("bad argument: data_type %d is neither SGX_DT_INT16 nor SGX_DT_FLOAT32", (int)data_type);
    return 0;
}

static int rq_whole_elements(const sgx_if* rec, int w) {
    if (rec->n % (size_t)w) {
        sgx_set_error("bad argument: a record of %zu bytes does not hold whole %d-byte elements", rec->n, w);
        return SGX_E_ARG;
    }
    return SGX_OK;
}

extern "C" int sgx_requant_tile(int32_t* tile_bytes) {
    SGX_CHECK_ARG(tile_bytes);
    *tile_bytes = RQ_TILE;
    return SGX_OK;
}

extern "C" int sgx_requant_timing(sgx_ctx* c, float* stats_ms, float* kernel_ms) {
    SGX_CHECK_ARG(c && stats_ms && kernel_ms);
    *stats_ms = c->stage_ms[SGX_STAGE_REQUANT_STATS];
    *kernel_ms = c->stage_ms[SGX_STAGE_REQUANT];
    return SGX_OK;
}

extern "C" int sgx_requant_gain(const sgx_requant_stats* st, int32_t data_type, double target_rms, int32_t* mult,
                                int32_t* shift, float* scale) {
    if (!rq_width(data_type)) return SGX_E_ARG;
    SGX_CHECK_ARG(target_rms > 0.0 && target_rms <= 127.0);
    SGX_CHECK_ARG(st && mult && shift && scale);
    double g = 1.0;
    if (st->n_finite > 0) {
        const double rms = sqrt(st->sum_sq / (double)st->n_finite);
        if (rms > 0.0) g = target_rms / rms;
    }
    *mult = 32767;
    *shift = 0;
    for (int S = 30; S >= 0; --S) {
        const double r = nearbyint(ldexp(g, S));   // ldexp is exact; round half to even (the default mode)
        if (r <= 32767.0) {
            *mult = r < 1.0 ? 1 : (int32_t)r;
            *shift = S;
            break;
        }
    }
    float gf = (float)g;
    gf = gf < SGX_REQUANT_SCALE_MIN ? SGX_REQUANT_SCALE_MIN : (gf > SGX_REQUANT_SCALE_MAX ? SGX_REQUANT_SCALE_MAX : gf);
    *scale = gf;
    return SGX_OK;
}

extern "C" int sgx_requant_stats_of(sgx_ctx* c, const sgx_if* rec, int32_t data_type, size_t offset, size_t count,
                                    sgx_requant_stats* out) {
    const int w = rq_width(data_type);
    if (!w) return SGX_E_ARG;
    SGX_CHECK_ARG(c && rec && out);
    SGX_CHECK_ARG(rec->device == c->device);
    if (rq_whole_elements(rec, w) != SGX_OK) return SGX_E_ARG;
    const size_t n_el = rec->n / (size_t)w;
    if (offset > n_el || count > n_el - offset) {
        sgx_set_error("bad argument: window offset %zu, count %zu lies outside the %zu elements of the record", offset, count,
                      n_el);
        return SGX_E_ARG;
    }
    int rc = sgx_stage_open(c, rec, (offset + count) * (size_t)w);
    if (rc != SGX_OK) return rc;
    c->stage_ms[SGX_STAGE_REQUANT_STATS] = 0.0f;
    memset(out, 0, sizeof(*out));
    if (count == 0) return SGX_OK;   // (an empty window: nothing is queued, nothing to wait for)
    const unsigned long long b0 = (unsigned long long)offset * w, b1 = b0 + (unsigned long long)count * w;
    unsigned long long* d_part = c->d_small->requant_part;
    unsigned long long* h_part = c->h_small->requant_part;
    SgxStage st(SGX_STAGE_REQUANT_STATS, RQ_STATS_BLOCKS, "requantiser statistics kernel failed: %s");
    st.down = {h_part, d_part, sizeof(SgxSmall::requant_part)};
    rc = sgx_stage_run(c, st, [&](sgx_if*) {
        if (data_type == SGX_DT_INT16) {
            requant_stats_kernel<SGX_DT_INT16><<<st.grid, RQ_THREADS, 0, c->stream>>>(rec->d, b0, b1, d_part);
        } else {
            requant_stats_kernel<SGX_DT_FLOAT32><<<st.grid, RQ_THREADS, 0, c->stream>>>(rec->d, b0, b1, d_part);
        }
    });
    if (rc != SGX_OK) return rc;
    // the partials in workgroup order
    unsigned long long bad = 0, mx = 0;
    if (data_type == SGX_DT_INT16) {
        __int128 sum = 0;
        unsigned __int128 sq = 0;
        for (int b = 0; b < RQ_STATS_BLOCKS; ++b) {
            sum += (long long)h_part[4 * b];
            sq += h_part[4 * b + 1];
            if (h_part[4 * b + 3] > mx) mx = h_part[4 * b + 3];
        }
        out->sum = (double)sum;   // one correctly rounded conversion of the exact integer
        out->sum_sq = (double)sq;
        out->max_abs = (double)mx;
    } else {
        double sum = 0.0, sq = 0.0;
        for (int b = 0; b < RQ_STATS_BLOCKS; ++b) {
            double v[2];
            memcpy(v, h_part + 4 * b, sizeof(v));
            sum += v[0];
            sq += v[1];
            bad += h_part[4 * b + 2];
            if (h_part[4 * b + 3] > mx) mx = h_part[4 * b + 3];
        }
        const unsigned mb = (unsigned)mx;
        float mf;
        memcpy(&mf, &mb, sizeof(mf));
        out->sum = sum;
        out->sum_sq = sq;
        out->max_abs = (double)mf;
    }
    out->n_nonfinite = (int64_t)bad;
    out->n_finite = (int64_t)count - (int64_t)bad;
    return SGX_OK;
}

extern "C" int sgx_if_requantize(sgx_ctx* c, const sgx_if* rec, int32_t data_type, int32_t mult, int32_t shift, float scale,
                                 sgx_if** out, int64_t* n_clipped) {
    // the type and the gain first: these refusals need no device
    const int w = rq_width(data_type);
    if (!w) return SGX_E_ARG;
    if (data_type == SGX_DT_INT16) {
        SGX_CHECK_ARG(mult >= 1 && mult <= 32767);
        SGX_CHECK_ARG(shift >= 0 && shift <= 30);
    } else {
        SGX_CHECK_ARG(scale >= SGX_REQUANT_SCALE_MIN && scale <= SGX_REQUANT_SCALE_MAX);   // (a NaN fails both)
    }
    SGX_CHECK_ARG(c && rec && out);
    SGX_CHECK_ARG(rec->device == c->device);
    if (rq_whole_elements(rec, w) != SGX_OK) return SGX_E_ARG;
    int rc = sgx_stage_open(c, rec, rec->n);
    if (rc != SGX_OK) return rc;
    const size_t n = rec->n / (size_t)w;
    const unsigned long long blocks = ((unsigned long long)n + RQ_TILE - 1) / RQ_TILE;
    rc = sgx_stage_one_launch(blocks, "bad argument: a record of %zu elements is beyond one launch of the requantiser", n);
    if (rc != SGX_OK) return rc;
    const RqGain g = {mult, (1 << shift) >> 1, shift, scale};
    SgxStage st(SGX_STAGE_REQUANT, (unsigned)blocks, "requantiser kernel failed: %s", out, n);
    unsigned long long* d_clip = st.count(c);
    rc = sgx_stage_run(c, st, [&](sgx_if* r) {
        if (data_type == SGX_DT_INT16) {
            requant_kernel<SGX_DT_INT16><<<st.grid, RQ_THREADS, 0, c->stream>>>(rec->d, r->d, n, g, d_clip);
        } else {
            requant_kernel<SGX_DT_FLOAT32><<<st.grid, RQ_THREADS, 0, c->stream>>>(rec->d, r->d, n, g, d_clip);
        }
    });
    if (rc != SGX_OK) return rc;
    if (n_clipped) *n_clipped = sgx_stage_count(c, 0);
    return SGX_OK;
}
