// The record monitor (no reference counterpart: Settings.probeData looks at the first 10 code periods only): a window of an
// int8 record cut into slices, each slice's Welch power spectral density - segments of N samples, constant detrend, periodic
// Hamming window, density scaling, one-sided, mean over the segments, as sgx_probe_stats - and the exact integer statistics
// of all its samples.  tests/waterfall_spec.py is the contract; the transform, its step loop, the twiddle table and the
// staging of the bytes are sgx_seg_fft.h's, shared with the excision stage.  sgx_probe_stats (Settings.probeData, reference
// initialize.py:330-417) is the monitor at N = 16384, overlap 1024 and one slice, and lives at the end of this file.
//
//   wf_segment_kernel  one workgroup per segment: int8 samples -> exact integer sum -> the packed N/2-point complex
//                      sequence in LDS (8192 x 16 B = 128 KB at N = 16384, the staged bytes 16 KB behind it) -> in-place transform -> real split -> the
//                      N/2 + 1 powers to the scratch row of the segment.  The complex spectrum never leaves the CU.
//   wf_average_kernel  per (slice, bin): the rows of the slice in segment order, * scale (* 2 inside the band), / segments
//   wf_hold_kernel     per bin: the maximum over the slices, in slice order
//   wf_stats_kernel    per slice: count, sum x, sum x^2, sum x^4 and the 256-bin histogram of ALL its samples, each
//                      counted once; LDS histogram per workgroup, 64-bit integer atomics to the slice's row
// The scratch holds at most WF_CHUNK_SEGMENTS rows (and at most WF_CHUNK_BYTES): a longer window runs chunk by chunk, the
// running sum of a slice cut by a chunk boundary waits in its row of the result.  No floating-point atomics: every sum has
// one order, so two runs give the same bits.
//   sgx_waterfall_host  the segments' items and the averaging in a host loop: what the kernels are held to, bit for bit
#include <math.h>

#include "sgx_waterfall_core.h"

#define WF_CHUNK_SEGMENTS 4096
#define WF_CHUNK_BYTES ((size_t)64 << 20)
#define WF_PIECE 65536             // samples one workgroup of the statistics takes at a time: its LDS counts fit 32 bits
#define WF_STATS_BLOCKS 2048
#define WF_MAX_SLICE ((size_t)1 << 32)   // 2^32 samples x 127^4 < 2^63: the sum of x^4 of a slice fits int64

// The twiddles of segment length n_seg on the host; returned: the sum of the squared window they imply
static double wf_tables(int n_seg, cplx* tw) {
    seg_twiddles(n_seg, tw);
    double w2 = 0.0;
    for (int i = 0; i < n_seg; ++i) {
        const double w = wf_window(tw, n_seg / 2, i);
        w2 += w * w;
    }
    return w2;
}

// The monitor's plan of segment length n_seg: the twiddles alone on the device, *w2 beside it
static int wf_prepare(SegPlan* plan, double* w2, int n_seg) {
    if (plan->holds(n_seg)) return SGX_OK;
    std::vector<cplx> h((size_t)n_seg / 2);
    *w2 = wf_tables(n_seg, h.data());
    return plan->upload(n_seg, reinterpret_cast<const double*>(h.data()), (size_t)n_seg);
}

#define WF_STAGE_BYTES(N) (16 * ((size_t)(N) / 16 + 1))
#define WF_LDS_BYTES(N) (sizeof(cplx) * ((size_t)(N) / 2) + WF_STAGE_BYTES(N))

// One workgroup per segment.  x: the record (on a granule), n_rec samples long; the window starts at sample `offset` of
// it.  The segment is staged in LDS behind the transform's buffer (seg_stage); the granules reach at most 15 bytes in
// front of it and 15 behind, and their bytes outside the segment are left out of the sum.
__global__ __launch_bounds__(1024) void wf_segment_kernel(const int8_t* __restrict__ x, long long n_rec, long long offset,
                                                          const cplx* __restrict__ tw, double* __restrict__ rows, WfGeom g,
                                                          long long seg0) {
    extern __shared__ __attribute__((aligned(16))) char wf_smem[];
    cplx* __restrict__ buf = reinterpret_cast<cplx*>(wf_smem);   // [N / 2]
    __shared__ int s_sum;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int M = g.N / 2;
    uint4* __restrict__ raw = reinterpret_cast<uint4*>(wf_smem + sizeof(cplx) * (size_t)M);   // [N / 16 + 1]
#define WF_LANES(q, count) for (int q = tid; q < (count); q += nt)
    long long slice, start;
    wf_locate(g, seg0 + blockIdx.x, &slice, &start);
    if (tid == 0) s_sum = 0;
    int part = 0;
    const int a = (int)((offset + start) & 15), last = (a + g.N - 1) / 16;
    seg_stage(raw, x, n_rec, offset + start, g.N, tid, nt, [&](int c, uint4 v) {
        // granule c holds the segment's bytes 16 c - a + (0 .. 15): the exact integer sum of the segment
        if (c == 0 || c == last) v = seg_keep_bytes(v, a - 16 * c, a + g.N - 16 * c);
        part = __builtin_amdgcn_sdot4((int)v.x, 0x01010101, part, false);
        part = __builtin_amdgcn_sdot4((int)v.y, 0x01010101, part, false);
        part = __builtin_amdgcn_sdot4((int)v.z, 0x01010101, part, false);
        part = __builtin_amdgcn_sdot4((int)v.w, 0x01010101, part, false);
    });
    __syncthreads();
    part = sgx_wave_sum(part);
    if ((tid & 63) == 0) atomicAdd(&s_sum, part);              // integers: any order gives the same sum
    __syncthreads();
    const int sum = s_sum;
    const int8_t* __restrict__ seg = reinterpret_cast<const int8_t*>(raw) + a;
    WF_LANES(m, M) wf_pack_item(buf, seg, tw, M, g.log2m, sum, m);
    __syncthreads();
    SEG_FORWARD(WF_LANES, __syncthreads(), buf, tw, M, g.log2m, M)
    double* __restrict__ row = rows + (size_t)blockIdx.x * (size_t)g.bins;
    WF_LANES(k, M + 1) row[k] = wf_split_item(buf, tw, M, k);
#undef WF_LANES
}

// grid (bins / WF_AVG_THREADS, slices the chunk touches): segments [seg0, seg0 + n_seg) of the window lie in the scratch.
// One wave per workgroup, so that a chunk of a few slices still spreads over the CUs; eight rows are loaded at a time and
// added in segment order.
#define WF_AVG_THREADS 64
__global__ __launch_bounds__(WF_AVG_THREADS) void wf_average_kernel(const double* __restrict__ rows, double* __restrict__ pxx, WfGeom g,
                                                         long long seg0, int n_seg, long long slice0, double scale) {
    const int k = blockIdx.x * WF_AVG_THREADS + threadIdx.x;
    if (k >= g.bins) return;
    const long long j = slice0 + blockIdx.y;
    const long long first = j * g.k_full, end = first + wf_slice_segments(g, j);
    const long long lo = first > seg0 ? first : seg0, hi = end < seg0 + n_seg ? end : seg0 + n_seg;
    if (lo >= hi) return;
    double* __restrict__ out = pxx + (size_t)j * (size_t)g.bins + k;
    const double two = (k >= 1 && k < g.bins - 1) ? 2.0 : 1.0;
    double acc = lo == first ? 0.0 : *out;
    const double* __restrict__ p = rows + (size_t)(lo - seg0) * (size_t)g.bins + k;
    long long s = lo;
    for (; s + 8 <= hi; s += 8, p += 8 * (size_t)g.bins) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = p[(size_t)u * (size_t)g.bins];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += (v[u] * scale) * two;
    }
    for (; s < hi; ++s, p += g.bins) acc += (*p * scale) * two;
    *out = hi == end ? acc / (double)(end - first) : acc;
}

__global__ __launch_bounds__(256) void wf_hold_kernel(const double* __restrict__ pxx, double* __restrict__ hold, WfGeom g) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= g.bins) return;
    double m = pxx[k];
    for (long long j = 1; j < g.n_slices; ++j) {
        const double v = pxx[(size_t)j * (size_t)g.bins + k];
        m = v > m ? v : m;
    }
    hold[k] = m;
}

// Work unit u = (slice, piece of WF_PIECE samples of it); mom: [n_slices][4], hist: [n_slices][256]
__global__ __launch_bounds__(256) void wf_stats_kernel(const int8_t* __restrict__ x, WfGeom g, long long pieces,
                                                       long long units, unsigned long long* __restrict__ mom,
                                                       unsigned long long* __restrict__ hist) {
    __shared__ unsigned s_h[256];
    const int tid = threadIdx.x;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const long long j = u / pieces, p = u - j * pieces;
        const long long end = (j + 1) * g.S < g.n ? (j + 1) * g.S : g.n;
        const long long lo = j * g.S + p * WF_PIECE;
        const long long hi = lo + WF_PIECE < end ? lo + WF_PIECE : end;
        if (lo >= hi) continue;                                  // (the same for every lane of the workgroup)
        s_h[tid] = 0;
        __syncthreads();
        long long s1 = 0;
        unsigned long long s2 = 0, s4 = 0;
        // the piece as the aligned 16-byte granules that cover it (inside the record's allocation and its pad, as the
        // segments' are); a byte outside [lo, hi) is left out
        const int a = (int)((unsigned long long)(x + lo) & 15);
        const uint4* __restrict__ src = reinterpret_cast<const uint4*>(x + lo - a);
        const int count = (int)(hi - lo), granules = (a + count + 15) / 16;
        for (int c = tid; c < granules; c += 256) {
            const uint4 v = src[c];
            const int b0 = 16 * c - a;                           // the piece's index of the granule's first byte
            const bool whole = b0 >= 0 && b0 + 16 <= count;
#pragma unroll
            for (int b = 0; b < 16; ++b) {
                const unsigned w = b < 4 ? v.x : b < 8 ? v.y : b < 12 ? v.z : v.w;
                const int val = (int)(int8_t)(w >> (8 * (b & 3)));
                if (whole || (b0 + b >= 0 && b0 + b < count)) {
                    const unsigned q = (unsigned)(val * val);
                    atomicAdd(&s_h[val + 128], 1u);
                    s1 += val;
                    s2 += q;
                    s4 += (unsigned long long)q * q;
                }
            }
        }
        s1 = sgx_wave_sum(s1);
        s2 = sgx_wave_sum(s2);
        s4 = sgx_wave_sum(s4);
        if ((tid & 63) == 0) {
            atomicAdd(&mom[j * 4 + 1], (unsigned long long)s1);  // (two's complement: the sum of the signed values)
            atomicAdd(&mom[j * 4 + 2], s2);
            atomicAdd(&mom[j * 4 + 3], s4);
        }
        __syncthreads();
        if (s_h[tid]) atomicAdd(&hist[j * 256 + tid], (unsigned long long)s_h[tid]);
        __syncthreads();
    }
}

// The geometry of a window, or the refusal: SGX_E_ARG for a segment length, overlap or slice length out of range,
// SGX_E_RANGE for a window shorter than one segment
static int wf_geometry(size_t n, int32_t nperseg, int32_t noverlap, size_t slice_len, WfGeom* g) {
    if (nperseg < WF_MIN_SEGMENT || nperseg > WF_MAX_SEGMENT || (nperseg & (nperseg - 1)) != 0) {
        sgx_set_error("the monitor's segment length is a power of two in %d .. %d, not %d", WF_MIN_SEGMENT, WF_MAX_SEGMENT,
                      (int)nperseg);
        return SGX_E_ARG;
    }
    if (noverlap < 0 || noverlap >= nperseg) {
        sgx_set_error("the monitor's overlap lies in 0 .. segment length - 1 = %d, not %d", (int)nperseg - 1, (int)noverlap);
        return SGX_E_ARG;
    }
    if (slice_len < (size_t)nperseg || slice_len > WF_MAX_SLICE) {
        // the upper bound: 2^32 samples of 127^4 each keep a slice's sum of x^4 inside int64
        sgx_set_error("a slice of the monitor holds at least one segment (%d samples) and at most 2^32 samples, not %zu",
                      (int)nperseg, slice_len);
        return SGX_E_ARG;
    }
    if (n < (size_t)nperseg) {
        sgx_set_error("ValueError: the monitor needs at least %d samples for one Welch segment, got %zu", (int)nperseg, n);
        return SGX_E_RANGE;
    }
    g->n = (long long)n;
    g->S = (long long)slice_len;
    g->N = nperseg;
    g->noverlap = noverlap;
    g->step = nperseg - noverlap;
    g->log2m = 0;
    while ((2 << g->log2m) < nperseg) ++g->log2m;
    g->bins = nperseg / 2 + 1;
    g->pad = 0;
    g->n_full = g->n / g->S;
    const long long rem = g->n - g->n_full * g->S;
    g->k_full = (g->S - noverlap) / g->step;
    const bool tail = rem >= (long long)nperseg;     // a trailing piece shorter than a segment is dropped
    g->n_slices = g->n_full + (tail ? 1 : 0);
    g->k_last = tail ? (rem - noverlap) / g->step : g->k_full;
    return SGX_OK;
}

extern "C" int sgx_waterfall_plan(size_t n, int32_t nperseg, int32_t noverlap, size_t slice_len, int64_t* n_slices) {
    SGX_CHECK_ARG(n_slices);
    WfGeom g;
    const int rc = wf_geometry(n, nperseg, noverlap, slice_len, &g);
    if (rc != SGX_OK) return rc;
    *n_slices = (int64_t)g.n_slices;
    return SGX_OK;
}

extern "C" int sgx_waterfall_timing(sgx_ctx* c, float* kernel_ms) {
    SGX_CHECK_ARG(c && kernel_ms);
    *kernel_ms = c->waterfall_ms;
    return SGX_OK;
}

// The monitor on a window the caller has checked (inside the record, geometry g): the kernels, the results to the caller's
// arrays, *kernel_ms = the HIP-event time of the kernels
static int wf_run(sgx_ctx* c, const sgx_if* rec, size_t offset, const WfGeom& g, double fs_mhz, double* f, double* pxx,
                  double* hold, int64_t* moments, int64_t* hist, int64_t* n_segments, float* kernel_ms) {
    int rc = sgx_if_require(rec, offset + (size_t)g.n);
    if (rc != SGX_OK) return rc;
    SGX_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    *kernel_ms = 0.0f;
    rc = wf_prepare(&c->plan_waterfall, &c->waterfall_w2, g.N);
    if (rc != SGX_OK) return rc;
    SGX_CHECK_ARG(((size_t)rec->d & 15) == 0);               // (every record starts on a granule: hipMalloc's alignment)
    const double scale = 1.0 / (fs_mhz * c->waterfall_w2);

    const size_t bins = (size_t)g.bins, ns = (size_t)g.n_slices;
    const long long total = g.n_full * g.k_full + (g.n_slices > g.n_full ? g.k_last : 0);
    long long chunk = (long long)(WF_CHUNK_BYTES / (sizeof(double) * bins));
    if (chunk > WF_CHUNK_SEGMENTS) chunk = WF_CHUNK_SEGMENTS;
    if (chunk > total) chunk = total;
    rc = c->d_wf_rows.ensure(sizeof(double) * bins * (size_t)chunk);
    if (rc != SGX_OK) return rc;
    // the results on the device: pxx[ns][bins] | hold[bins] | moments[ns][4] | hist[ns][256]
    const size_t pxx_bytes = sizeof(double) * bins * ns, hold_bytes = sizeof(double) * bins;
    const size_t mom_bytes = sizeof(int64_t) * 4 * ns, hist_bytes = sizeof(int64_t) * 256 * ns;
    rc = c->d_wf_out.ensure(pxx_bytes + hold_bytes + mom_bytes + hist_bytes);
    if (rc != SGX_OK) return rc;
    double* d_pxx = (double*)c->d_wf_out.get();
    double* d_hold = d_pxx + bins * ns;
    unsigned long long* d_mom = (unsigned long long*)(d_hold + bins);
    unsigned long long* d_hist = d_mom + 4 * ns;

    const int M = g.N / 2;
    const int threads = M / 8 >= 1024 ? 1024 : (M / 8 >= 64 ? M / 8 : 64);   // whole waves
    SGX_HIP(hipFuncSetAttribute((const void*)wf_segment_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)WF_LDS_BYTES(WF_MAX_SEGMENT)));
    SGX_HIP(hipMemsetAsync(d_mom, 0, mom_bytes + hist_bytes, st));
    hipEventRecord(c->ev[0], st);
    {
        const long long pieces = (g.S + WF_PIECE - 1) / WF_PIECE, units = pieces * g.n_slices;
        wf_stats_kernel<<<(unsigned)(units < WF_STATS_BLOCKS ? units : WF_STATS_BLOCKS), 256, 0, st>>>(
            rec->d + offset, g, pieces, units, d_mom, d_hist);
    }
    for (long long seg0 = 0; seg0 < total; seg0 += chunk) {
        const int n_seg = (int)(total - seg0 < chunk ? total - seg0 : chunk);
        wf_segment_kernel<<<n_seg, threads, WF_LDS_BYTES(g.N), st>>>(rec->d, (long long)rec->n, (long long)offset,
                                                                     c->plan_waterfall.tw(), c->d_wf_rows.get(), g, seg0);
        const long long slice0 = seg0 / g.k_full, slice1 = (seg0 + n_seg - 1) / g.k_full;
        wf_average_kernel<<<dim3((unsigned)((bins + WF_AVG_THREADS - 1) / WF_AVG_THREADS), (unsigned)(slice1 - slice0 + 1)),
                            WF_AVG_THREADS, 0, st>>>(
            c->d_wf_rows.get(), d_pxx, g, seg0, n_seg, slice0, scale);
    }
    wf_hold_kernel<<<(unsigned)((bins + 255) / 256), 256, 0, st>>>(d_pxx, d_hold, g);
    hipEventRecord(c->ev[1], st);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(pxx, d_pxx, pxx_bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(hold, d_hold, hold_bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(moments, d_mom, mom_bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(hist, d_hist, hist_bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        sgx_set_error("monitor kernels failed: %s", hipGetErrorString(e));
        return SGX_E_HIP;
    }
    hipEventElapsedTime(kernel_ms, c->ev[0], c->ev[1]);
    for (size_t j = 0; j < ns; ++j) {
        const long long lo = (long long)j * g.S, hi = lo + g.S < g.n ? lo + g.S : g.n;
        moments[4 * j] = (int64_t)(hi - lo);
        n_segments[j] = (int64_t)wf_slice_segments(g, (long long)j);
    }
    // np.fft.rfftfreq(N, 1 / fs): val = 1 / (n d); f = arange(n / 2 + 1) * val
    const double val = 1.0 / ((double)g.N * (1.0 / fs_mhz));
    for (int k = 0; k < g.bins; ++k) f[k] = (double)k * val;
    return SGX_OK;
}

extern "C" int sgx_probe_waterfall(sgx_ctx* c, const sgx_if* rec, size_t offset, size_t n, double fs_mhz, int32_t nperseg,
                                   int32_t noverlap, size_t slice_len, double* f, double* pxx, double* hold,
                                   int64_t* moments, int64_t* hist, int64_t* n_segments, int64_t* n_slices) {
    SGX_CHECK_ARG(c && rec && f && pxx && hold && moments && hist && n_segments && n_slices && fs_mhz > 0.0);
    SGX_CHECK_ARG(rec->device == c->device);
    if (offset > rec->n || n > rec->n - offset) {
        sgx_set_error("monitor window [%zu, %zu) outside the %zu-sample record", offset, offset + n, rec->n);
        return SGX_E_RANGE;
    }
    WfGeom g;
    int rc = wf_geometry(n, nperseg, noverlap, slice_len, &g);
    if (rc == SGX_OK) rc = wf_run(c, rec, offset, g, fs_mhz, f, pxx, hold, moments, hist, n_segments, &c->waterfall_ms);
    if (rc == SGX_OK) *n_slices = (int64_t)g.n_slices;
    return rc;
}

// The monitor's spectra without a GPU: the segments' items in a host loop, SEG_FORWARD between them, and the additions of
// wf_average_kernel in its order - acc += (p * scale) * two in segment order, then / count.  x: the window.
extern "C" int sgx_waterfall_host(const int8_t* x, size_t n, double fs_mhz, int32_t nperseg, int32_t noverlap,
                                  size_t slice_len, double* pxx, int64_t* n_segments) {
    SGX_CHECK_ARG(x && pxx && n_segments && fs_mhz > 0.0);
    WfGeom g;
    const int rc = wf_geometry(n, nperseg, noverlap, slice_len, &g);
    if (rc != SGX_OK) return rc;
    const int M = g.N / 2;
    std::vector<cplx> tw((size_t)M), buf((size_t)M);
    const double scale = 1.0 / (fs_mhz * wf_tables(g.N, tw.data()));
#define WF_ALL(q, count) for (int q = 0; q < (count); ++q)
    for (long long j = 0; j < g.n_slices; ++j) {
        const long long count = wf_slice_segments(g, j);
        double* out = pxx + (size_t)j * (size_t)g.bins;
        for (int k = 0; k < g.bins; ++k) out[k] = 0.0;
        for (long long s = 0; s < count; ++s) {
            long long slice, start;
            wf_locate(g, j * g.k_full + s, &slice, &start);
            const int8_t* seg = x + start;
            int sum = 0;
            WF_ALL(i, g.N) sum += seg[i];
            WF_ALL(m, M) wf_pack_item(buf.data(), seg, tw.data(), M, g.log2m, sum, m);
            SEG_FORWARD(WF_ALL, (void)0, buf.data(), tw.data(), M, g.log2m, M)
            WF_ALL(k, g.bins) {
                const double two = (k >= 1 && k < g.bins - 1) ? 2.0 : 1.0;
                out[k] += (wf_split_item(buf.data(), tw.data(), M, k) * scale) * two;
            }
        }
        WF_ALL(k, g.bins) out[k] /= (double)count;
        n_segments[j] = (int64_t)count;
    }
#undef WF_ALL
    return SGX_OK;
}

// ---- Settings.probeData ----------------------------------------------------------------------------------------------------
// Raw-data statistics of Settings.probeData (reference initialize.py:330-417), the step before
// acquisition: the Welch power spectral density of the first 10 code periods,
//   welch(data - mean(data), fs/1e6, hamming(16384, sym=False), nperseg 16384, noverlap 1024, nfft 16384)
// (scipy defaults: constant detrend per segment, density scaling, one-sided, mean over segments), and the histogram
// np.histogram(data, arange(-128, 128)).  That is the monitor with one slice: removing the window's mean first changes
// nothing behind a per-segment detrend, which the monitor does in exact integers.
#define PROBE_NSEG 16384
#define PROBE_NOVERLAP 1024

extern "C" int sgx_probe_stats(sgx_ctx* c, const sgx_if* rec, size_t offset, size_t n, double fs_mhz, double* f,
                               double* pxx, int64_t* hist, int32_t* n_segments) {
    SGX_CHECK_ARG(c && rec && f && pxx && hist && n_segments && fs_mhz > 0.0);
    SGX_CHECK_ARG(rec->device == c->device);
    if (offset > rec->n || n > rec->n - offset) {
        sgx_set_error("probe window [%zu, %zu) outside the %zu-sample record", offset, offset + n, rec->n);
        return SGX_E_RANGE;
    }
    if (n < (size_t)PROBE_NSEG) {
        // scipy falls back to nperseg = len(x) with a warning and then rejects the 16384-point window
        sgx_set_error("ValueError: probeData needs at least %d samples for one Welch segment, got %zu", PROBE_NSEG, n);
        return SGX_E_RANGE;
    }
    WfGeom g;
    int rc = wf_geometry(n, PROBE_NSEG, PROBE_NOVERLAP, n, &g);   // (refuses a window beyond the monitor's longest slice)
    if (rc != SGX_OK) return rc;
    std::vector<double> hold((size_t)g.bins);
    int64_t moments[4], h[256], segments = 0;
    float ms = 0.0f;                                              // (waterfall_ms stays the last sgx_probe_waterfall's)
    rc = wf_run(c, rec, offset, g, fs_mhz, f, pxx, hold.data(), moments, h, &segments, &ms);
    if (rc != SGX_OK) return rc;
    for (int b = 0; b < 255; ++b) hist[b] = h[b];
    hist[254] += h[255];                                          // np.histogram's last bin [126, 127] is closed
    *n_segments = (int32_t)segments;
    return SGX_OK;
}
