// The float front of tracking (Settings.dataType 'float32' / 'float64'; reference tracking.py:154 reads np.fromfile(fid,
// dataType, blksize) and computes in float64): one scan of the window the channels can reach, one route, and the description
// of what the call then runs on (TrkSource, sgx_trk_common.h).  The fast way for float32 is EXACT NARROWING: when every sample
// of the window is m 2^-k for one k (of either sign) and integers m that fit 8 or 16 bits - floats written from ADC samples
// (k = 0) or normalised by a power of two (int16 / 32768: k = 15) are - the integers are tracked by the int8 / int16 kernels;
// a power of two commutes with every rounding of the reference's arithmetic, so the correlator series are the integer
// record's times 2^-k exactly and everything the discriminators make of them (ratios) is untouched.  A record of arbitrary
// floats has no such k: in range it takes the latency-mode kernel, which scales every sample by a power of two on conversion.
// A channel may start inside a sample of the file (the reference seeks skipNumberOfBytes + codePhase BYTES, tracking.py:107):
// that, and whatever the other routes cannot hold, goes to the per-sample kernel of sgx_trk_any.hip, which reads every float
// where it lies.
#include "sgx_trk_common.h"

#include <algorithm>
#include <cmath>
#include <type_traits>

// What the scan leaves.  sum_abs is for a threshold only: the order of its additions is not fixed.
struct FScan {
    unsigned long long mx;   // the bits of the largest finite |x| (the bits of non-negative floats order like integers)
    unsigned lo;             // float32: smallest exponent of a sample's lowest set bit + 1024 (F_NO_BIT: no nonzero sample)
    unsigned bad;            // a sample that is not finite was seen
    double sum_abs;          // the sum of |x| over the finite samples
};
#define F_NO_BIT 0x7FFFFFFFu

template <typename F>
__global__ __launch_bounds__(256) void f_scan_kernel(const F* __restrict__ x, long long n, FScan* __restrict__ st) {
    constexpr bool f32 = sizeof(F) == 4;
    typedef typename std::conditional<f32, unsigned, unsigned long long>::type U;
    constexpr int MANT = f32 ? 23 : 52;
    constexpr U E_ALL = f32 ? 255 : 2047;
    unsigned long long mx = 0ull;
    unsigned lo = F_NO_BIT, bad = 0u;
    double sa = 0.0;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const U u = __builtin_bit_cast(U, x[i]) & ~(U(1) << (8 * sizeof(F) - 1));
        const U e = u >> MANT;
        if (e == E_ALL) bad = 1u;
        if (u == 0 || e == E_ALL) continue;
        mx = u > mx ? u : mx;
        sa += (double)__builtin_bit_cast(F, u);
        if constexpr (f32) {
            // value = (m | implicit) 2^(e - 150) (a subnormal: m 2^-149): the exponent of its lowest set bit
            const unsigned m = u & 0x7FFFFFu, full = e ? (m | 0x800000u) : m;
            const int lb = (int)(e ? e : 1u) - 150 + (__ffs((int)full) - 1);
            const unsigned key = (unsigned)(lb + 1024);
            lo = key < lo ? key : lo;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long omx = __shfl_down(mx, off);
        const unsigned olo = __shfl_down(lo, off), ob = __shfl_down(bad, off);
        mx = omx > mx ? omx : mx;
        lo = olo < lo ? olo : lo;
        bad |= ob;
        sa += __shfl_down(sa, off);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMax(&st->mx, mx);
        atomicMin(&st->lo, lo);
        if (bad) atomicOr(&st->bad, 1u);
        atomicAdd(&st->sum_abs, sa);
    }
}

// y[i] = x[i] 2^k as an 8- or 16-bit integer (exact by construction)
template <typename T>
__global__ __launch_bounds__(256) void f32_narrow_kernel(const float* __restrict__ x, long long n, int k, T* __restrict__ y) {
    const float s = ldexpf(1.0f, k);
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        y[i] = (T)(int)(x[i] * s);
}

// THE WINDOW the channels can reach, in samples of sb bytes from the description's first byte: [first, end), with the same
// allowance per block as the kernels' units (64 samples, sgx_trk.hip), cut to the record's whole samples.  false: nothing to
// scan - no channel is on, no whole sample (the kernel reports the short read), or a channel starts inside a sample of the
// file: it reads the bit patterns of bytes of two samples (the reference does), other values than a scan would see.
static bool f_window(const TrkSource& S, int sb, long long ms, long long n_code, long long& first, long long& end) {
    long long last = -1;
    first = -1;
    for (const TrkChan& h : S.hc) {
        if (h.prn == 0) continue;
        if (h.pad != 0) return false;
        first = (first < 0 || h.pos0 < first) ? h.pos0 : first;
        last = h.pos0 > last ? h.pos0 : last;
    }
    end = std::min(last + ms * (n_code + 64) + n_code, S.n / sb);
    return first >= 0 && end > first;
}

// The scan of n samples at x, launched and read back
static int f_scan(sgx_ctx* c, const int8_t* x, long long n, int kind, FScan& h) {
    DevBuf<FScan> d_st;
    const int rc = d_st.ensure(sizeof(FScan));
    if (rc != SGX_OK) return rc;
    h = FScan{0ull, F_NO_BIT, 0u, 0.0};
    hipError_t e = hipMemcpyAsync(d_st, &h, sizeof(h), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        const int grid = (int)std::min((n + 255) / 256, 4096ll);
        if (kind == SGX_DT_FLOAT32) f_scan_kernel<float><<<grid, 256, 0, c->stream>>>(reinterpret_cast<const float*>(x), n, d_st);
        else f_scan_kernel<double><<<grid, 256, 0, c->stream>>>(reinterpret_cast<const double*>(x), n, d_st);
        e = hipMemcpyAsync(&h, d_st, sizeof(h), hipMemcpyDeviceToHost, c->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) return SGX_OK;
    sgx_set_error("float%d record scan: %s", 8 * sgx_dt_bytes(kind), hipGetErrorString(e));
    return SGX_E_HIP;
}

// THE ROUTE of a scanned window of n samples: which kernel, on what
struct FRoute {
    enum Way { PER_SAMPLE, TYPED, NARROW8, NARROW16 } way;
    double fscale;   // TYPED: the power of two the kernel scales the samples by
    int k;           // NARROW8 / NARROW16: the integers are the samples times 2^k
};
static FRoute f_route(const FScan& s, long long n, int kind, const TrkEnv& E, bool multi) {
    const FRoute per_sample{FRoute::PER_SAMPLE, 1.0, 0};
    // NaN or infinite samples: numpy's arithmetic carries them, so does the per-sample kernel
    if (s.bad) return per_sample;
    const bool f32 = kind == SGX_DT_FLOAT32;
    const double mx = f32 ? (double)__builtin_bit_cast(float, (unsigned)s.mx) : __builtin_bit_cast(double, s.mx);
    // float32: every sample is a multiple of 2^lb, so an integer times 2^-k, k = -lb (negative for records of multiples of
    // 2^j, j > 0), the largest of them `peak`; integers that fit 16 bits are narrowed, to int8 where they fit 8
    // (SGX_TRK_F32_NARROW=0: never; an all-zero window: k = 0, int8)
    const int k = s.lo != F_NO_BIT ? 1024 - (int)s.lo : 0;
    const double peak = s.lo != F_NO_BIT ? ldexp(mx, k) : 0.0;
    if (f32 && E.f32_narrow && k <= 120 && k >= -120 && peak <= 32767.0)
        return FRoute{peak <= 127.0 ? FRoute::NARROW8 : FRoute::NARROW16, 1.0, k};
    // arbitrary floats: the latency-mode kernel reads them as they are (SGX_TRK_FLOAT_TYPED=0: never; nor at fewer than ~15.4
    // samples per chip, where no typed kernel runs: trk_plan) and scales them on conversion by the power of two that
    // brings the largest |sample| to at most 128 (what the typed kernels' fixed point is cut for); 1 for an all-zero window
    if (!E.float_typed || multi) return per_sample;
    if (!(mx > 0.0)) return FRoute{FRoute::TYPED, 1.0, 0};
    // The typed kernel's granules are a fixed point cut for samples of comparable size (2^-28 of the largest): a window whose
    // largest sample towers 2^12 times above the mean |x| (an outlier, a burst) would lose the small ones' last digits against
    // the reference's float64 sums - such a record takes the per-sample kernel.
    if (mx > 4096.0 * (s.sum_abs / (double)n)) return per_sample;
    int ex = 0;
    (void)frexp(mx, &ex);          // mx = m 2^ex, 1/2 <= m < 1
    // (records near the ends of the float64 range: the scale, its reciprocal or the reference's own I^2 + Q^2 would
    // leave the range - the per-sample kernel follows the reference there, overflow and all)
    if (7 - ex > 900 || 7 - ex < -900) return per_sample;
    return FRoute{FRoute::TYPED, ldexp(1.0, 7 - ex), 0};
}

// The float32 window [first, first + n) as 8- or 16-bit integers (x 2^k) in `buf`: S becomes the description of that copy -
// its first sample at byte 0, every channel where it started in the window - with the way back: the kernel's positions are
// bytes of the copy, sb per 4 of the file behind the window's first byte, and the six correlator series carry the 2^k.
static int f_narrow(sgx_ctx* c, TrkSource& S, long long first, long long n, int k, bool narrow8, DevBuf<int8_t>& buf) {
    const int sb = narrow8 ? 1 : 2;
    const size_t bytes = (size_t)n * (size_t)sb;
    const int rc = buf.ensure(bytes + SGX_IF_PAD);
    if (rc != SGX_OK) return rc;
    const float* x = reinterpret_cast<const float*>(S.d) + first;
    const int grid = (int)std::min((n + 255) / 256, 8192ll);
    if (narrow8) f32_narrow_kernel<int8_t><<<grid, 256, 0, c->stream>>>(x, n, k, buf.get());
    else f32_narrow_kernel<short><<<grid, 256, 0, c->stream>>>(x, n, k, reinterpret_cast<short*>(buf.get()));
    hipError_t e = hipMemsetAsync(buf.get() + bytes, 0, SGX_IF_PAD, c->stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) {
        sgx_set_error("float32 record narrowing: %s", hipGetErrorString(e));
        return SGX_E_HIP;
    }
    S.pos_a = 4.0 / sb;
    S.pos_b = (double)(S.file_off + first * 4);
    S.sums = ldexp(1.0, -k);
    S.d = buf.get();
    S.n = (long long)bytes;
    S.rec = nullptr;
    S.kind = narrow8 ? SGX_DT_INT8 : SGX_DT_INT16;
    S.file_off = 0;
    for (TrkChan& h : S.hc)
        if (h.prn != 0) h.pos0 -= first;
    return SGX_OK;
}

int sgx_track_float(sgx_ctx* c, const sgx_if* r, int64_t rec_file_offset, const sgx_chan_init* ch, int32_t n_ch, int32_t ms,
                    double* out, int32_t* ms_done, int kind) {
    const int sb = sgx_dt_bytes(kind);
    const TrkEnv E = sgx_trk_env();
    TrkSource S;   // (as it lies: the per-sample kernel)
    int rc = sgx_trk_source(S, c->s, r, (long long)rec_file_offset, ch, n_ch, kind);
    if (rc != SGX_OK) return rc;
    DevBuf<int8_t> narrowed;   // (the memory of a narrowed window, for the length of the call)
    long long first, end;
    if (f_window(S, sb, ms, (long long)c->n_code, first, end)) {
        rc = sgx_if_require(r, (size_t)(end * sb));   // (a streaming record: the scan needs every sample)
        if (rc != SGX_OK) return rc;
        SGX_HIP(hipSetDevice(c->device));
        FScan scan;
        rc = f_scan(c, S.d + first * sb, end - first, kind, scan);
        if (rc != SGX_OK) return rc;
        const FRoute R = f_route(scan, end - first, kind, E, sgx_trk_multi(c->s) != 0);
        if (R.way == FRoute::TYPED) {
            S.float_typed = true;
            S.fscale = R.fscale;
            S.sums = 1.0 / R.fscale;
        } else if (R.way != FRoute::PER_SAMPLE) {
            rc = f_narrow(c, S, first, end - first, R.k, R.way == FRoute::NARROW8, narrowed);
            if (rc != SGX_OK) return rc;
        }
    }
    return sgx_track_source(c, S, E, ch, n_ch, ms, out, ms_done);
}
