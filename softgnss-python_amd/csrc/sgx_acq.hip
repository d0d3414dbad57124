// AcquisitionResult.acquire on gfx950 (reference acquisition.py:27-204).
//
// Data flow per call (everything fp64 / complex128, int8 IF read once):
//   mix      x[n]*(sin,cos)(f_k * phasePoints[n])        -> [blocks][bins][N]      (PRN independent,
//   FFT_N                                                 -> spectra X[b][k]         computed ONCE; the
//                                                                                    reference redoes it
//                                                                                    per PRN, Q6)
//   code     table[p][n] = ca[p][ceil((ts*k)/tc)-1]      -> FFT_N -> F[p]
//   corr     conj(X[b][k]) * F[p]  -> FFT_N  (= conj(N * ifft(X conj F)))  -> |.|^2 / N^2
//   peaks    per row max / first argmax (device), block choice + exclusion list (host, tiny),
//            second peak over the exclusion list (device)
//   fine     (x - mean) * code(floor((ts*k)/tc) mod 1023), zero-padded 2^22-point FFT, argmax of |X|
// HBM-resident scratch replaces the reference's per-PRN numpy temporaries.
// A samplesPerCode with a prime factor above 31 has no transform of its own length here: its circular correlation runs
// inside a longer one (acquire_passes, "padded length").
#include <math.h>
#include <chrono>

#include "sgx_internal.h"

// ================================ limits and structs ================================
// (ACQ_MAX_BINS, ACQ_MAX_ROWS, ACQ_COH_MAX_BINS and the structs the small areas hold: sgx_internal.h)
#define ACQ_DEFAULT_CHUNK_ROWS 348   // correlation rows per chunk (the intermediate then stays in the Infinity Cache)

// The grid of a coherent multi-millisecond search (sgx_acquire_coherent; coh_grid fills it)
#define ACQ_COH_MAX_MS 20
#define ACQ_COH_MAX_WINDOWS 64
#define ACQ_COH_MAX_SPAN_MS 400
#define ACQ_COH_MAX_PHI 64
struct CohGrid {
    int T = 1, M = 1, noncoh = 0;       // coherent_ms, n_windows, rule
    double step = 500.0, f0 = 0.0;      // f_k = f0 + step k
    int n_bins = 0, n_phi = 0, path = 0;
    std::vector<int2> bin_map;          // shift path: (phi index, circular shift) per bin
    std::vector<double> phi;
    int prn_chunk = 1, runs = 1, per_run = 1;   // correlation batches (coh_plan): per_run bins (noncoh) or windows
};

// ================================ kernels ================================
struct MixArgs {
    double frq[ACQ_MAX_BINS];
    int n_bins;
    int n_blocks;
};

// acquisition.py:62-117: phasePoints[n] = ((n*2)*pi)*ts ; theta = frq*phasePoints ; I = sin*x, Q = cos*x
// (stride: elements between the rows of `out` - n, or the padded length of a row whose tail the transform takes as zero)
__global__ __launch_bounds__(256) void acq_mix_kernel(SgxSig x, cplx* __restrict__ out,
                                                      long long n, long long stride, double ts, MixArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int k = blockIdx.y % a.n_bins;
    const int b = blockIdx.y / a.n_bins;
    const double pp = ((double)(i * 2) * M_PI) * ts;
    const double th = a.frq[k] * pp;
    double s, c;
    sincos(th, &s, &c);
    const double xv = x.at((long long)b * n + i);
    out[((long long)b * a.n_bins + k) * stride + i] = make_double2(s * xv, c * xv);
}

// initialize.py:210-226 (A3) on the device, same IEEE operations: idx = ceil((ts*k)/tc) - 1
__device__ __forceinline__ double acq_code_sample(const int8_t* __restrict__ codes, int p, long long i, long long n,
                                                  double ts, double tc) {
    int idx = (int)ceil((ts * (double)(i + 1)) / tc) - 1;
    if (i == n - 1) idx = 1022;
    idx = idx < 0 ? 0 : (idx > 1022 ? 1022 : idx);
    return (double)codes[p * 1023 + idx];
}
__global__ __launch_bounds__(256) void acq_code_kernel(const int8_t* __restrict__ codes,
                                                       const int* __restrict__ prn0, cplx* __restrict__ out,
                                                       long long n, double ts, double tc) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int p = prn0[blockIdx.y];
    out[(long long)blockIdx.y * n + i] = make_double2(acq_code_sample(codes, p, i, n, ts, tc), 0.0);
}
// The code row of a padded correlation, length len >= 2 n - 1: the sampled code at [0, n), its wrap-around copy
// code[1 .. n - 1] at [len - n + 1, len), zero between them.  Against a signal that is zero from n on, the circular
// correlation of length len then reads code[(i - k) mod n] for every lag k < n: the length-n circular correlation,
// term for term.  One launch writes the whole row.
__global__ __launch_bounds__(256) void acq_code_pad_kernel(const int8_t* __restrict__ codes,
                                                           const int* __restrict__ prn0, cplx* __restrict__ out,
                                                           long long n, long long len, double ts, double tc) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= len) return;
    const int p = prn0[blockIdx.y];
    const long long j = i < n ? i : i - (len - n);   // (the copy: j = 1 .. n - 1)
    const double v = (i < n || j >= 1) ? acq_code_sample(codes, p, j, n, ts, tc) : 0.0;
    out[(long long)blockIdx.y * len + i] = make_double2(v, 0.0);
}

// rows r = (pi, b, k): Y = conj(X[b][k]) * F[pi]
__global__ __launch_bounds__(256) void acq_mul_kernel(const cplx* __restrict__ X, const cplx* __restrict__ F,
                                                      cplx* __restrict__ Y, long long n, int rows_per_prn,
                                                      int prn_base) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int r = blockIdx.y;
    const int pi = r / rows_per_prn;
    const int bk = r % rows_per_prn;
    const cplx xv = X[(long long)bk * n + i];
    const cplx fv = F[(long long)(prn_base + pi) * n + i];
    // conj(x) * f
    Y[(long long)r * n + i] =
        make_double2(__builtin_fma(xv.x, fv.x, xv.y * fv.y), __builtin_fma(xv.x, fv.y, -(xv.y * fv.x)));
}

// |fft|^2 / N^2 per output row (optionally summed over the blocks: noncoherent extension),
// plus row max and FIRST argmax (numpy argmax semantics, acquisition.py:139-143).
// (zs: elements between the rows of Z - n, or the padded length, of which the first n outputs are the correlation)
__global__ __launch_bounds__(256) void acq_power_kernel(const cplx* __restrict__ Z, double* __restrict__ P,
                                                        double* __restrict__ rowmax, int* __restrict__ rowarg,
                                                        long long n, long long zs, double inv_n, int n_bins, int n_blocks,
                                                        int noncoh) {
    const int ro = blockIdx.x;   // output row
    double best = -1.0;
    int arg = 0;
    double* __restrict__ prow = P + (long long)ro * n;
    for (long long i = threadIdx.x; i < n; i += 256) {
        double v;
        if (noncoh) {
            const int pi = ro / n_bins, k = ro % n_bins;
            v = 0.0;
            for (int b = 0; b < n_blocks; ++b) {
                const cplx z = Z[(((long long)pi * n_blocks + b) * n_bins + k) * zs + i];
                const double re = z.x * inv_n, im = z.y * inv_n;
                const double pw = re * re + im * im;
                v = (b == 0) ? pw : v + pw;
            }
        } else {
            const cplx z = Z[(long long)ro * zs + i];
            const double re = z.x * inv_n, im = z.y * inv_n;
            v = re * re + im * im;
        }
        prow[i] = v;
        if (v > best) {
            best = v;
            arg = (int)i;
        }
    }
    __shared__ double s_v[256];
    __shared__ int s_i[256];
    s_v[threadIdx.x] = best;
    s_i[threadIdx.x] = arg;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const double ov = s_v[threadIdx.x + s];
            const int oi = s_i[threadIdx.x + s];
            if (ov > s_v[threadIdx.x] || (ov == s_v[threadIdx.x] && oi < s_i[threadIdx.x])) {
                s_v[threadIdx.x] = ov;
                s_i[threadIdx.x] = oi;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        rowmax[ro] = s_v[0];
        rowarg[ro] = s_i[0];
    }
}

// finish the fused last pass: per-workgroup (max, first index) partials -> one per row
__global__ __launch_bounds__(64) void acq_rowmax_finish_kernel(const double* __restrict__ pmax,
                                                               const int* __restrict__ parg, int nblk,
                                                               double* __restrict__ rowmax, int* __restrict__ rowarg) {
    const int row = blockIdx.x;
    double best = -1.0;
    int arg = 0;
    for (int b = threadIdx.x; b < nblk; b += 64) {
        const double v = pmax[(long long)row * nblk + b];
        const int i = parg[(long long)row * nblk + b];
        if (v > best || (v == best && i < arg)) {
            best = v;
            arg = i;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_down(best, o);
        const int oi = __shfl_down(arg, o);
        if (ov > best || (ov == best && oi < arg)) {
            best = ov;
            arg = oi;
        }
    }
    if (threadIdx.x == 0) {
        rowmax[row] = best;
        rowarg[row] = arg;
    }
}


// acquisition.py:162: max of the chosen frequency row over the exclusion index list
// (grid (PRNs, SEC_SPLIT): every workgroup takes a slice of the ranges and folds its maximum into out[p] with an integer
// atomic max on the bit pattern - powers are non-negative, so the patterns order like the values; out[] starts at 0)
#define SEC_SPLIT 16
__global__ __launch_bounds__(256) void acq_second_kernel(const double* __restrict__ P, double* __restrict__ out,
                                                         long long n, const SecondArgs* __restrict__ ap) {
    const SecondArgs& a = *ap;
    const int p = blockIdx.x;
    const int t0 = blockIdx.y * 256 + threadIdx.x, ts = gridDim.y * 256;
    double best = 0.0;
    if (a.row[p] >= 0) {
        const double* __restrict__ prow = P + (long long)a.row[p] * n;
        for (int i = a.lo0[p] + t0; i < a.hi0[p]; i += ts) best = fmax(best, prow[i]);
        for (int i = a.lo1[p] + t0; i < a.hi1[p]; i += ts) best = fmax(best, prow[i]);
    }
    __shared__ double s_v[256];
    s_v[threadIdx.x] = best;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) s_v[threadIdx.x] = fmax(s_v[threadIdx.x], s_v[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicMax((unsigned long long*)&out[p], (unsigned long long)__double_as_longlong(s_v[0]));
}

// the same on a recomputed complex correlation row: |z|^2 / N^2 formed on the fly, identical arithmetic to
// the fused last pass, so peak / second peak is a ratio of consistently rounded values
// (n: elements between the rows of Z; the ranges lie inside the correlation's own length)
__global__ __launch_bounds__(256) void acq_second_cplx_kernel(const cplx* __restrict__ Z, double* __restrict__ out,
                                                              long long n, double inv_n, const SecondArgs* __restrict__ ap) {
    const SecondArgs& a = *ap;
    const int p = blockIdx.x;
    const int t0 = blockIdx.y * 256 + threadIdx.x, ts = gridDim.y * 256;
    double best = 0.0;
    if (a.row[p] >= 0) {
        const cplx* __restrict__ zrow = Z + (long long)a.row[p] * n;
        for (int i = a.lo0[p] + t0; i < a.hi0[p]; i += ts) {
            const double re = zrow[i].x * inv_n, im = zrow[i].y * inv_n;
            best = fmax(best, re * re + im * im);
        }
        for (int i = a.lo1[p] + t0; i < a.hi1[p]; i += ts) {
            const double re = zrow[i].x * inv_n, im = zrow[i].y * inv_n;
            best = fmax(best, re * re + im * im);
        }
    }
    __shared__ double s_v[256];
    s_v[threadIdx.x] = best;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) s_v[threadIdx.x] = fmax(s_v[threadIdx.x], s_v[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicMax((unsigned long long*)&out[p], (unsigned long long)__double_as_longlong(s_v[0]));
}

// integer sum of the record window (mean for acquisition.py:59): bytes up to the first 16-byte boundary, 16 bytes per
// lane from there, bytes again for the rest
__global__ __launch_bounds__(256) void acq_sum_kernel(const int8_t* __restrict__ x, long long n,
                                                      long long* __restrict__ out) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x, gsz = (long long)gridDim.x * 256;
    long long head = (16 - ((unsigned long long)x & 15)) & 15;
    if (head > n) head = n;
    const long long n16 = (n - head) / 16;
    long long acc = 0;
    if (gid < head) acc += x[gid];
    const uint4* __restrict__ x16 = reinterpret_cast<const uint4*>(x + head);
    for (long long i = gid; i < n16; i += gsz) {
        const uint4 v = x16[i];
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int d = 0; d < 4; ++d)
            acc += (int)(w[d] << 24) >> 24, acc += (int)(w[d] << 16) >> 24, acc += (int)(w[d] << 8) >> 24, acc += (int)w[d] >> 24;
    }
    for (long long i = head + n16 * 16 + gid; i < n; i += gsz) acc += x[i];
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);
    // one atomic per workgroup (a thousand 64-bit atomics on one address took most of this kernel's time)
    __shared__ long long s_acc[4];
    if ((threadIdx.x & 63) == 0) s_acc[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0)
        atomicAdd((unsigned long long*)out, (unsigned long long)(s_acc[0] + s_acc[1] + s_acc[2] + s_acc[3]));
}

// Call set-up in one launch: the PRN list and the bin map (by value) to their device tables, the accumulators zeroed.
struct AcqSetup {
    int prn[32];
    int2 bin[ACQ_MAX_BINS];
    int n_prn, n_bins;
};
__global__ __launch_bounds__(128) void acq_setup_kernel(AcqSetup a, int* __restrict__ d_prn, int2* __restrict__ d_bin,
                                                        long long* __restrict__ d_sum, double* __restrict__ d_second,
                                                        int* __restrict__ d_arrived = nullptr) {
    const int t = threadIdx.x;
    if (t < a.n_prn) d_prn[t] = a.prn[t];
    if (t < a.n_bins) d_bin[t] = a.bin[t];
    if (t < 32) d_second[t] = 0.0;
    if (t < 64 && d_arrived) d_arrived[t] = 0;   // [32] per PRN, [32] PRNs finished
    if (t == 0) d_sum[0] = 0;
}

// the same for an fp64 signal: one workgroup, fixed summation order (reproducible); the double's bits go to the same slot
__global__ __launch_bounds__(1024) void acq_sum_f64_kernel(const double* __restrict__ x, long long n,
                                                           long long* __restrict__ out) {
    __shared__ double s_v[1024];
    double acc = 0.0;
    for (long long i = threadIdx.x; i < n; i += 1024) acc += x[i];
    s_v[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) s_v[threadIdx.x] += s_v[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = __double_as_longlong(s_v[0]);
}

// acquisition.py:170-177 (A9): xCarrier = (x - mean)[c : c+10N] * code[floor((ts*k)/tc1) mod 1023].
// Two detected PRNs share one complex row (first -> real part, second -> imaginary part): the two real-input
// spectra are separated again in the argmax kernel, which halves the 2^22-point FFT work.
__global__ __launch_bounds__(256) void acq_fine_prep_kernel(SgxSig x,
                                                            const int8_t* __restrict__ codes, cplx* __restrict__ out,
                                                            long long len, long long row_stride, double mean,
                                                            double ts, double tc1, const int* __restrict__ det_prn,
                                                            const int* __restrict__ det_phase, int n_det) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= len) return;
    const int r = blockIdx.y;
    const double v = floor((ts * (double)(i + 1)) / tc1);
    const int chip = (int)((long long)v % 1023);
    const int d0 = 2 * r, d1 = 2 * r + 1;
    const double a = (x.at(det_phase[d0] + i) - mean) * (double)codes[det_prn[d0] * 1023 + chip];
    const double b = (d1 < n_det) ? (x.at(det_phase[d1] + i) - mean) * (double)codes[det_prn[d1] * 1023 + chip] : 0.0;
    out[(long long)r * row_stride + i] = make_double2(a, b);
}

// acquisition.py:182-187: argmax of |X_d[4 : uniq-5]| (first occurrence) for detection d, where the row holds
// Z = FFT(x_a + i x_b):  X_a[k] = (Z[k] + conj(Z[M-k]))/2,  X_b[k] = (Z[k] - conj(Z[M-k]))/(2i).
// Only the argmax is observable, so the common factor 1/4 of |.|^2 is dropped.
// win (coherent search, else null): detection d's own range [win[2 d], win[2 d + 1]) instead of [lo, hi)
__global__ __launch_bounds__(256) void acq_fine_argmax_kernel(const cplx* __restrict__ X, long long row_stride,
                                                              long long lo, long long hi,
                                                              double* __restrict__ pv, long long* __restrict__ pi,
                                                              const long long* __restrict__ win = nullptr) {
    const int d = blockIdx.y;
    if (win) {
        lo = win[2 * d];
        hi = win[2 * d + 1];
    }
    const cplx* __restrict__ row = X + (long long)(d >> 1) * row_stride;
    const double sgn = (d & 1) ? -1.0 : 1.0;
    double best = -1.0;
    long long arg = lo;
    for (long long i = lo + (long long)blockIdx.x * 256 + threadIdx.x; i < hi; i += (long long)gridDim.x * 256) {
        const cplx z = row[i];
        const cplx w = row[row_stride - i];           // i >= 4 > 0, so M - i is inside the row
        const double re = z.x + sgn * w.x, im = z.y - sgn * w.y;   // z +- conj(w)
        const double v = re * re + im * im;
        if (v > best) {
            best = v;
            arg = i;
        }
    }
    __shared__ double s_v[256];
    __shared__ long long s_i[256];
    s_v[threadIdx.x] = best;
    s_i[threadIdx.x] = arg;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const double ov = s_v[threadIdx.x + s];
            const long long oi = s_i[threadIdx.x + s];
            if (ov > s_v[threadIdx.x] || (ov == s_v[threadIdx.x] && oi < s_i[threadIdx.x])) {
                s_v[threadIdx.x] = ov;
                s_i[threadIdx.x] = oi;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        pv[(long long)d * gridDim.x + blockIdx.x] = s_v[0];
        pi[(long long)d * gridDim.x + blockIdx.x] = s_i[0];
    }
}

// Forward rows of the shifted-spectrum search.  The reference transforms
// x (sin th + j cos th) = j x e^(-j th), th = 2 pi f n / fs, for every Doppler bin f (acquisition.py:103-117).  With
// f N / fs = s + phi (s integer, 0 <= phi < 1) that transform is j X_phi[(m + s) mod N], X_phi = fft(x e^(-j 2 pi phi n / N)):
// bins that share phi share ONE forward spectrum, read with a circular shift (|j| = 1 drops out of |.|^2).  For the
// default front end (fs / N = 1 kHz, 500 Hz grid) phi is 0 or 1/2: two forward transforms per 1-ms block instead of 29.
struct PhiArgs {
    double phi[4];
    int n_phi;
};
__global__ __launch_bounds__(256) void acq_mixphi_kernel(SgxSig x, cplx* __restrict__ out,
                                                         long long n, PhiArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int j = blockIdx.y % a.n_phi;
    const int b = blockIdx.y / a.n_phi;
    const double xv = x.at((long long)b * n + i);
    double s = 0.0, c = 1.0;
    if (a.phi[j] != 0.0) sincospi((2.0 * a.phi[j]) * ((double)i / (double)n), &s, &c);
    out[(long long)blockIdx.y * n + i] = make_double2(c * xv, -(s * xv));
}

// The front of a call in ONE launch (round 4; int8 records): the first kernels of a call are a few microseconds each and
// the host cannot queue them faster than they run, so four launches cost four launch latencies.  Workgroup roles by index:
// [0, n_mix) acq_mixphi_kernel's tiles, [n_mix, n_mix + n_code) acq_code_kernel's (PRN list by value), then ACQ_SUM_WGS
// of acq_sum_kernel's, then one of acq_setup_kernel's.  The record sum goes to the slot `sum_now`, which the PREVIOUS
// call's set-up workgroup zeroed (two slots alternate; the host keeps track and clears a slot itself when it cannot know).
#define ACQ_SUM_WGS 64
__global__ __launch_bounds__(256) void acq_front_kernel(AcqSetup su, SgxSig x, PhiArgs pa, const int8_t* __restrict__ codes,
                                                        cplx* __restrict__ out, long long n, int rows_fwd, double ts,
                                                        double tc, long long n_samples, int* __restrict__ d_prn,
                                                        int2* __restrict__ d_bin, long long* __restrict__ sum_now,
                                                        long long* __restrict__ sum_next, double* __restrict__ d_second,
                                                        int* __restrict__ d_arrived) {
    const int gx = (int)((n + 255) / 256);
    const int n_mix = rows_fwd * gx, n_code = su.n_prn * gx;
    int blk = blockIdx.x;
    const int t = threadIdx.x;
    if (blk < n_mix) {
        const int row = blk / gx;
        const long long i = (long long)(blk - row * gx) * 256 + t;
        if (i >= n) return;
        const int j = row % pa.n_phi;
        const int b = row / pa.n_phi;
        const double xv = x.at((long long)b * n + i);
        double s = 0.0, c = 1.0;
        if (pa.phi[j] != 0.0) sincospi((2.0 * pa.phi[j]) * ((double)i / (double)n), &s, &c);
        out[(long long)row * n + i] = make_double2(c * xv, -(s * xv));
        return;
    }
    blk -= n_mix;
    if (blk < n_code) {
        const int row = blk / gx;
        const long long i = (long long)(blk - row * gx) * 256 + t;
        if (i >= n) return;
        const int p = su.prn[row];
        int idx = (int)ceil((ts * (double)(i + 1)) / tc) - 1;
        if (i == n - 1) idx = 1022;
        idx = idx < 0 ? 0 : (idx > 1022 ? 1022 : idx);
        out[(long long)(rows_fwd + row) * n + i] = make_double2((double)codes[p * 1023 + idx], 0.0);
        return;
    }
    blk -= n_code;
    if (blk < ACQ_SUM_WGS) {
        const int8_t* __restrict__ xs = x.i8;
        const long long gid = (long long)blk * 256 + t, gsz = (long long)ACQ_SUM_WGS * 256;
        long long head = (16 - ((unsigned long long)xs & 15)) & 15;
        if (head > n_samples) head = n_samples;
        const long long n16 = (n_samples - head) / 16;
        long long acc = 0;
        if (gid < head) acc += xs[gid];
        const uint4* __restrict__ x16 = reinterpret_cast<const uint4*>(xs + head);
        for (long long i = gid; i < n16; i += gsz) {
            const uint4 v = x16[i];
            const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int d = 0; d < 4; ++d)
                acc += (int)(w[d] << 24) >> 24, acc += (int)(w[d] << 16) >> 24, acc += (int)(w[d] << 8) >> 24, acc += (int)w[d] >> 24;
        }
        for (long long i = head + n16 * 16 + gid; i < n_samples; i += gsz) acc += xs[i];
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);
        __shared__ long long s_acc[4];
        if ((t & 63) == 0) s_acc[t >> 6] = acc;
        __syncthreads();
        if (t == 0) atomicAdd((unsigned long long*)sum_now, (unsigned long long)(s_acc[0] + s_acc[1] + s_acc[2] + s_acc[3]));
        return;
    }
    if (t < su.n_prn) d_prn[t] = su.prn[t];
    if (t < su.n_bins) d_bin[t] = su.bin[t];
    if (t < 32) d_second[t] = 0.0;
    if (t < 64) d_arrived[t] = 0;   // [32] rows finished per PRN, [32] PRNs finished
    if (t == 0) sum_next[0] = 0;
}

// Direct path of the coherent search: window w of bin k folded as the contract states it (include/sgx.h), every
// (window, bin) row on its own - the same IEEE operations as acq_mix_kernel, which is the case T = 1:
//   out[w][k][n] = sum_{m < T} x[(w T + m) n_code + n] (sin + j cos)(frq[k] (((n + m n_code) 2) pi ts))
__global__ __launch_bounds__(256) void acq_fold_direct_kernel(SgxSig x, cplx* __restrict__ out, long long n,
                                                              long long stride, double ts,
                                                              const double* __restrict__ frq, int n_bins, int T) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int k = blockIdx.y % n_bins;
    const int w = blockIdx.y / n_bins;
    const double f = frq[k];
    double re = 0.0, im = 0.0;
    for (int m = 0; m < T; ++m) {
        const double pp = ((double)((i + (long long)m * n) * 2) * M_PI) * ts;
        double sn, cs;
        sincos(f * pp, &sn, &cs);
        const double xv = x.at(((long long)w * T + m) * n + i);
        re += sn * xv;
        im += cs * xv;
    }
    out[(long long)blockIdx.y * stride + i] = make_double2(re, im);
}

// Shift path of the coherent search.  With f_k n_code ts = shift_k + phi_k the window's carrier is
// j e^(-j 2 pi shift_k n / n_code) e^(-j 2 pi phi_k (n / n_code + m)) (e^(-j 2 pi shift_k m) = 1): bins that share phi share
// ONE folded row, whose spectrum they read with a circular shift (acq_mixphi_kernel's trick, across the window).  One
// workgroup reads its 256 samples of each of the window's T blocks once and writes all n_phi folded rows of them:
//   out[w][j][n] = e^(-j 2 pi phi_j n / n_code) sum_{m < T} x[(w T + m) n_code + n] e^(-j 2 pi phi_j m)
struct FoldArgs {
    double phi[ACQ_COH_MAX_PHI];
    int n_phi, T;
};
__global__ __launch_bounds__(256) void acq_fold_phi_kernel(SgxSig x, cplx* __restrict__ out, long long n, FoldArgs a) {
    __shared__ cplx s_rot[ACQ_COH_MAX_PHI * ACQ_COH_MAX_MS];   // e^(-j 2 pi phi_j m)
    for (int t = threadIdx.x; t < a.n_phi * a.T; t += 256) {
        const int j = t / a.T, m = t % a.T;
        double sn = 0.0, cs = 1.0;
        if (a.phi[j] != 0.0 && m != 0) sincospi(2.0 * a.phi[j] * (double)m, &sn, &cs);
        s_rot[t] = make_double2(cs, -sn);
    }
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int w = blockIdx.y;
    double xv[ACQ_COH_MAX_MS];
#pragma unroll
    for (int m = 0; m < ACQ_COH_MAX_MS; ++m) xv[m] = m < a.T ? x.at(((long long)w * a.T + m) * n + i) : 0.0;
    for (int j = 0; j < a.n_phi; ++j) {
        const cplx* __restrict__ rot = s_rot + j * a.T;
        double re = 0.0, im = 0.0;
#pragma unroll
        for (int m = 0; m < ACQ_COH_MAX_MS; ++m) {
            if (m < a.T) {
                re = __builtin_fma(xv[m], rot[m].x, re);
                im = __builtin_fma(xv[m], rot[m].y, im);
            }
        }
        double sn = 0.0, cs = 1.0;
        if (a.phi[j] != 0.0) sincospi((2.0 * a.phi[j]) * ((double)i / (double)n), &sn, &cs);
        // (re + j im) (cs - j sn)
        out[((long long)w * a.n_phi + j) * n + i] = make_double2(__builtin_fma(re, cs, im * sn), __builtin_fma(im, cs, -(re * sn)));
    }
}

// Peak logic of one PRN (acquisition.py:129-162) in pieces a wave can share; the round-1 passes run the same pieces on the
// host.
// One bin's candidate: block choice (A7) and its row's maximum / first index.
struct AcqCand {
    double v;
    int k, a, b;
};
// (the row maxima come from other workgroups of the SAME launch, acq_rowmax_peak_kernel: written and read past the
// per-XCD L2s with device-scope accesses, no cache write-back or invalidation; the host reads its own copy)
#ifdef __HIP_DEVICE_COMPILE__
#define ACQ_LD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#else
#define ACQ_LD(p) (*(p))
#endif
#define ACQ_ST(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
__host__ __device__ static inline AcqCand acq_peak_bin(const double* __restrict__ rowmax, const int* __restrict__ rowarg,
                                                       int n_bins, int n_blocks, bool noncoh, int k) {
    int row = k, bsel = 0;
    if (!noncoh) {
        int best = 0;   // acquisition.py:129-133 generalised left to right, later block wins ties
        for (int b = 1; b < n_blocks; ++b) {
            const double vb = ACQ_LD(rowmax + best * n_bins + k);
            const double vn = ACQ_LD(rowmax + b * n_bins + k);
            if (!(vb > vn)) best = b;
        }
        row = best * n_bins + k;
        bsel = best;
    }
    AcqCand c;
    c.v = ACQ_LD(rowmax + row);
    c.a = ACQ_LD(rowarg + row);
    c.k = k;
    c.b = bsel;
    return c;
}
// A scan over the bins in ascending k keeps: the maximum, the FIRST bin attaining it (results.max(1).argmax()), that
// bin's block, and the SMALLEST column among the bins attaining it (results.max(0).argmax()) - A8.  The same as a
// combination of two partial scans (k < 0: an empty one):
__host__ __device__ static inline AcqCand acq_peak_join(const AcqCand& x, const AcqCand& y) {
    if (y.k < 0) return x;
    if (x.k < 0) return y;
    if (x.v > y.v) return x;
    if (y.v > x.v) return y;
    AcqCand c = (x.k < y.k) ? x : y;
    c.a = x.a < y.a ? x.a : y.a;
    return c;
}
// The exclusion list around the peak's code phase (A8b, acquisition.py:135-162).  Returns 1 where the reference raises
// IndexError (Q5), else 0.
__host__ __device__ static inline int acq_peak_ranges(int gc, long long N, int spc, int* lo0, int* hi0, int* lo1, int* hi1) {
    *lo0 = *hi0 = *lo1 = *hi1 = 0;
    const int e1 = gc - spc, e2 = gc + spc;
    if (e1 <= 0) {
        if ((long long)N + e1 + 1 > N) return 1;   // index N would be read: the reference's IndexError (Q5)
        *lo0 = e2;
        *hi0 = (int)(N + e1 + 1);
    } else if (e2 >= N - 1) {
        const int lo = (int)(e2 - N);
        if (lo < 0) {   // arange starts at -1: numpy wraps it to N-1
            *lo0 = 0;
            *hi0 = e1;
            *lo1 = (int)N - 1;
            *hi1 = (int)N;
        } else {
            *lo0 = lo;
            *hi0 = e1;
        }
    } else {
        *lo0 = 0;
        *hi0 = e1 + 1;
        *lo1 = e2;
        *hi1 = (int)N;
    }
    return 0;
}

// SAME_LAUNCH: the peaks were written by other waves of this launch (device-scope stores): read them the same way.
template <bool SAME_LAUNCH>
__device__ __forceinline__ void acq_publish_body(const PeakOut* __restrict__ po, const double* __restrict__ second, int n_prn,
                                                 CoarseLook* __restrict__ host, const int* __restrict__ prn_list,
                                                 double threshold, long long fine_len, long long n_samples,
                                                 AcqDet* __restrict__ det, int t) {
    const int* src = reinterpret_cast<const int*>(po);
    int* dst = reinterpret_cast<int*>(&host->po);
    for (int i = t; i < (int)(sizeof(PeakOut) / sizeof(int)); i += 64) dst[i] = SAME_LAUNCH ? ACQ_LD(src + i) : src[i];
    double sec = 0.0, pk = 0.0;
    int ie = 0, cp = 0;
    if (t < n_prn) {
        sec = SAME_LAUNCH ? ACQ_LD(second + t) : second[t];
        pk = SAME_LAUNCH ? ACQ_LD(po->peak + t) : po->peak[t];
        ie = SAME_LAUNCH ? ACQ_LD(po->index_error + t) : po->index_error[t];
        cp = SAME_LAUNCH ? ACQ_LD(po->cph + t) : po->cph[t];
        host->second[t] = sec;
    }
    if (det) {
        // acquisition.py:164-166: detected iff peak / second peak > acqThreshold; the list in ascending PRN position
        const bool hit = t < n_prn && ie == 0 && (pk / sec) > threshold;
        const unsigned long long m = __builtin_amdgcn_ballot_w64(hit);
        const int d = __builtin_popcountll(m & ((1ull << t) - 1ull));
        const bool out = hit && (long long)cp + fine_len > n_samples;   // (the reference would fail to broadcast)
        const unsigned long long mo = __builtin_amdgcn_ballot_w64(out);
        if (hit) {
            det->prn[d] = prn_list[t];
            det->phase[d] = cp;
            host->det_slot[d] = t;
            host->det_phase[d] = cp;
        }
        if (t == 0) {
            det->fine_done = 0;                                 // fine_rows_kernel's arrival counter
            det->n_det = mo ? 0 : __builtin_popcountll(m);      // (an error: the fine kernels have nothing to do)
            host->n_det = __builtin_popcountll(m);
            host->range_error = mo ? 1 + __builtin_ctzll(mo) : 0;
            host->seq = 0ull;   // device-led: `host` is a device-side copy of the page; fine_rows_kernel's last workgroup
        }                       // copies it to the real one and the host waits for seq2
    }
}

// (det: an AcqDet, or null; an int* in the signature, which is part of the kernel's name in traces and profiles)
__global__ __launch_bounds__(64) void acq_publish_kernel(const PeakOut* __restrict__ po, const double* __restrict__ second,
                                                         int n_prn, CoarseLook* __restrict__ host, unsigned long long seq,
                                                         const int* __restrict__ prn_list, double threshold,
                                                         long long fine_len, long long n_samples, int* __restrict__ det) {
    const int t = threadIdx.x;
    acq_publish_body<false>(po, second, n_prn, host, prn_list, threshold, fine_len, n_samples, reinterpret_cast<AcqDet*>(det), t);
    if (det) return;
    __threadfence_system();
    __syncthreads();
    if (t == 0) __hip_atomic_store(&host->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The peak of one PRN, a lane per Doppler bin (one lane per PRN scanning its rows was a chain of dependent loads: 12 us);
// lane 0 holds the result.
__device__ __forceinline__ AcqCand acq_peak_reduce(const double* __restrict__ pm, const int* __restrict__ pa, int lane,
                                                   int n_bins, int n_blocks, int noncoh) {
    AcqCand c;
    c.v = -1.0;
    c.k = -1;
    c.a = c.b = 0;
    for (int k = lane; k < n_bins; k += 64) c = acq_peak_join(c, acq_peak_bin(pm, pa, n_bins, n_blocks, noncoh != 0, k));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        AcqCand o;
        o.v = __shfl_down(c.v, off);
        o.k = __shfl_down(c.k, off);
        o.a = __shfl_down(c.a, off);
        o.b = __shfl_down(c.b, off);
        c = acq_peak_join(c, o);
    }
    return c;
}
// ... and on every lane of the wave
__device__ __forceinline__ AcqCand acq_peak_scan(const double* __restrict__ pm, const int* __restrict__ pa, int lane,
                                                 int n_bins, int n_blocks, int noncoh) {
    AcqCand c = acq_peak_reduce(pm, pa, lane, n_bins, n_blocks, noncoh);
    c.v = __shfl(c.v, 0);
    c.k = __shfl(c.k, 0);
    c.a = __shfl(c.a, 0);
    c.b = __shfl(c.b, 0);
    return c;
}

// One WAVE per PRN: its peak, exclusion list and the row the second-peak search transforms again.
__device__ __forceinline__ void acq_peak_one(const double* __restrict__ rowmax, const int* __restrict__ rowarg, int pi,
                                             int lane, int n_prn, int out_per_prn, int n_bins, int n_blocks, int noncoh,
                                             long long N, int spc, PeakOut* __restrict__ po, SecondArgs* __restrict__ sa,
                                             int2* __restrict__ row_map) {
    if (pi >= n_prn) {
        if (lane == 0) {
            sa->row[pi] = -1;
            sa->lo0[pi] = sa->hi0[pi] = sa->lo1[pi] = sa->hi1[pi] = 0;
        }
        return;
    }
    const AcqCand c = acq_peak_reduce(rowmax + (long long)pi * out_per_prn, rowarg + (long long)pi * out_per_prn, lane, n_bins,
                                      n_blocks, noncoh);
    if (lane != 0) return;
    int lo0, hi0, lo1, hi1;
    const int bad = acq_peak_ranges(c.a, N, spc, &lo0, &hi0, &lo1, &hi1);
    po->peak[pi] = c.v;
    po->cph[pi] = c.a;
    po->fbi[pi] = c.k;
    po->index_error[pi] = bad;
    sa->row[pi] = bad ? -1 : pi;
    sa->lo0[pi] = bad ? 0 : lo0;
    sa->hi0[pi] = bad ? 0 : hi0;
    sa->lo1[pi] = bad ? 0 : lo1;
    sa->hi1[pi] = bad ? 0 : hi1;
    if (noncoh) {
        for (int b = 0; b < n_blocks; ++b) row_map[pi * n_blocks + b] = make_int2(b * n_bins + c.k, pi);
    } else {
        row_map[pi] = make_int2(c.b * n_bins + c.k, pi);
    }
}

// A wave finishes one output row from its `n` partial (maximum, first index) pairs, stores it and counts the arrival at
// its PRN *pi_out (arrival counter per PRN, zeroed by the call's set-up).  Returns, on every lane, whether this was the
// LAST row of the PRN.
__device__ __forceinline__ int acq_row_finish(const double* __restrict__ pv, const int* __restrict__ pidx, int n, int row,
                                              int lane, double* __restrict__ rowmax, int* __restrict__ rowarg,
                                              int* __restrict__ arrived, int out_per_prn, int* pi_out) {
    double best = -1.0;
    int arg = 0;
    for (int b = lane; b < n; b += 64) {
        const double v = pv[(long long)row * n + b];
        const int i = pidx[(long long)row * n + b];
        if (v > best || (v == best && i < arg)) {
            best = v;
            arg = i;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_down(best, o);
        const int oi = __shfl_down(arg, o);
        if (ov > best || (ov == best && oi < arg)) {
            best = ov;
            arg = oi;
        }
    }
    const int pi = row / out_per_prn;
    *pi_out = pi;
    int last = 0;
    if (lane == 0) {
        ACQ_ST(rowmax + row, best);
        ACQ_ST(rowarg + row, arg);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // both written through before the arrival is counted
        last = __hip_atomic_fetch_add(arrived + pi, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1 == out_per_prn;
    }
    return __builtin_amdgcn_readfirstlane(last);
}

// acq_rowmax_finish_kernel and the peak step in one launch (round 4): a wave finishes one output row; the wave that
// finishes the LAST row of a PRN goes on to that PRN's block choice, global peak and exclusion list.  The last PRN's wave
// also fills the unused slots of the second-peak arguments.
__global__ __launch_bounds__(64) void acq_rowmax_peak_kernel(const double* __restrict__ pmax, const int* __restrict__ parg,
                                                             int nblk, double* __restrict__ rowmax, int* __restrict__ rowarg,
                                                             int* __restrict__ arrived, int n_prn, int out_per_prn,
                                                             int n_bins, int n_blocks, int noncoh, long long N, int spc,
                                                             PeakOut* __restrict__ po, SecondArgs* __restrict__ sa,
                                                             int2* __restrict__ row_map) {
    const int row = blockIdx.x, lane = threadIdx.x;
    int pi;
    if (!acq_row_finish(pmax, parg, nblk, row, lane, rowmax, rowarg, arrived, out_per_prn, &pi)) return;
    acq_peak_one(rowmax, rowarg, pi, lane, n_prn, out_per_prn, n_bins, n_blocks, noncoh, N, spc, po, sa, row_map);
    if (pi == n_prn - 1 && n_prn + lane < 32)
        acq_peak_one(rowmax, rowarg, n_prn + lane, 0, n_prn, out_per_prn, n_bins, n_blocks, noncoh, N, spc, po, sa, row_map);
}

struct PublishArgs {
    CoarseLook* stage;          // device-side copy of the result page, or null: a publish kernel follows
    const int* prn_list;
    double threshold;
    long long fine_len, n_samples;
    AcqDet* det;
};

// Round 5: row maxima, peak, SECOND PEAK and the detection list in one launch, from the rows kernel's per-residue
// (maximum, maximum of the others, first index) triples - the winning row is not transformed again (two launches, 39 us
// of the 8-rank shard of config 4) and no publish kernel follows (10 us).  A wave finishes one output row; the wave that
// finishes the last row of a PRN goes on to that PRN's block choice, global peak, exclusion list (acquisition.py:129-162)
// and the maximum over the allowed indices: the excluded ones are fewer than `nres` consecutive indices, at most one per
// residue, so a residue contributes its maximum if that is allowed and else the maximum of its others - the same powers
// the first pass formed.  The wave that finishes the last PRN decides the detections (acquisition.py:164-166).
__global__ __launch_bounds__(64) void acq_rowtop2_peak_kernel(const double* __restrict__ b1, const double* __restrict__ b2,
                                                              const int* __restrict__ i1, int nres,
                                                              double* __restrict__ rowmax, int* __restrict__ rowarg,
                                                              int* __restrict__ arrived, int n_prn, int out_per_prn,
                                                              int n_bins, int n_blocks, int noncoh, long long N, int spc,
                                                              PeakOut* __restrict__ po, double* __restrict__ second,
                                                              PublishArgs pub) {
    const int row = blockIdx.x, lane = threadIdx.x;
    int pi;
    if (!acq_row_finish(b1, i1, nres, row, lane, rowmax, rowarg, arrived, out_per_prn, &pi)) return;
    const AcqCand c = acq_peak_scan(rowmax + (long long)pi * out_per_prn, rowarg + (long long)pi * out_per_prn, lane, n_bins,
                                    n_blocks, noncoh);
    int lo0, hi0, lo1, hi1;
    const int bad = acq_peak_ranges(c.a, N, spc, &lo0, &hi0, &lo1, &hi1);
    double sec = 0.0;
    if (!bad) {
        const long long wrow = ((long long)pi * out_per_prn + (noncoh ? c.k : c.b * n_bins + c.k)) * nres;
        for (int r = lane; r < nres; r += 64) {
            const int idx = i1[wrow + r];
            const double v1 = b1[wrow + r], v2 = b2[wrow + r];   // (both: three independent loads)
            const bool in = (idx >= lo0 && idx < hi0) || (idx >= lo1 && idx < hi1);
            sec = fmax(sec, in ? v1 : v2);
        }
    }
    for (int o = 32; o > 0; o >>= 1) sec = fmax(sec, __shfl_down(sec, o));
    int done = 0;
    if (lane == 0) {
        ACQ_ST(po->peak + pi, c.v);
        ACQ_ST(po->cph + pi, c.a);
        ACQ_ST(po->fbi + pi, c.k);
        ACQ_ST(po->index_error + pi, bad);
        ACQ_ST(second + pi, sec);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        done = __hip_atomic_fetch_add(arrived + 32, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1 == n_prn;
    }
    done = __builtin_amdgcn_readfirstlane(done);
    if (!done || !pub.stage) return;
    acq_publish_body<true>(po, second, n_prn, pub.stage, pub.prn_list, pub.threshold, pub.fine_len, pub.n_samples, pub.det,
                           lane);
}

// ================================ round 6: deferred acquisition, preRun on the device ================================
// The reference's caller (initialize.py:484-506) runs acquire -> preRun -> track and looks at each result in between.  A
// caller that only wants the tracking results can queue all three: sgx_acquire_begin queues the search and returns,
// sgx_track_chained (sgx_trk.hip) queues preRun - the kernel below - and the tracking kernel behind it and waits ONCE;
// sgx_acquire_end then decodes the search's page (no waiting left).  Outputs are those of the eager calls, bit for bit:
// the same kernels in the same order, and the kernel below repeats the host's arithmetic (one IEEE multiplication and
// division for carrFreq, one division for peakMetric, a stable descending sort).
// acquisition.py:259-306 on the device.  One wave; lane p = PRN index p of the 32-entry result arrays.
__global__ __launch_bounds__(64) void acq_prerun_kernel(const CoarseLook* __restrict__ stage, const long long* __restrict__ fine_bi,
                                                        const int* __restrict__ prn_list, int n_prn, double fs, double npts,
                                                        TrkChan* __restrict__ d_ch, int n_ch, long long skip_bytes,
                                                        long long rec_file_offset, int sample_bytes,
                                                        StepLook* __restrict__ look) {
    __shared__ double s_met[32], s_carr[32], s_cph[32];
    __shared__ int s_err;
    const int t = threadIdx.x;
    if (t < 32) {
        s_met[t] = 0.0;
        s_carr[t] = 0.0;
        s_cph[t] = 0.0;
    }
    if (t == 0) s_err = 0;
    __syncthreads();
    if (t < n_prn) {
        s_met[prn_list[t]] = stage->po.peak[t] / stage->second[t];   // acquisition.py:164
        if (stage->po.index_error[t]) atomicOr(&s_err, 2);
    }
    if (t == 0 && stage->range_error) atomicOr(&s_err, 2);
    __syncthreads();
    const int n_det = stage->n_det;
    if (t < n_det && s_err == 0) {
        const long long m = fine_bi[t] - 4;                          // acquisition.py:187-191 (Q3)
        const int p = prn_list[stage->det_slot[t]];
        s_carr[p] = ((double)m * fs) / npts;
        s_cph[p] = (double)stage->det_phase[t];
    }
    __syncthreads();
    // sorted(enumerate(peakMetric), key = metric, reverse = True): stable, descending (acquisition.py:289-290)
    int rank = 0, nan = 0;
    if (t < 32) {
        const double mine = s_met[t];
        nan = (mine != mine) ? 1 : 0;
        for (int q = 0; q < 32; ++q) {
            const double o = s_met[q];
            rank += (o > mine || (o == mine && q < t)) ? 1 : 0;
        }
    }
    const unsigned long long any_nan = __builtin_amdgcn_ballot_w64(nan != 0);
    const int count = __builtin_popcountll(__builtin_amdgcn_ballot_w64(t < 32 && s_carr[t] > 0.0));   // sum(carrFreq > 0)
    int flags = s_err | (any_nan ? 1 : 0);
    const int n_act = flags ? 0 : (count < n_ch ? count : n_ch);
    // channels that are off (acquisition.py:281-284); the lanes holding ranks < n_act then fill theirs
    if (t < n_ch) {
        d_ch[t].acquiredFreq = 0.0;
        d_ch[t].pos0 = 0;
        d_ch[t].prn = 0;
        d_ch[t].pad = 0;
        if (t < 32) {
            look->prn[t] = 0;
            look->acquiredFreq[t] = 0.0;
            look->codePhase[t] = 0.0;
        }
    }
    __syncthreads();
    int before = 0;
    if (t < 32 && rank < n_act) {
        const long long p0 = skip_bytes + (long long)s_cph[t] - rec_file_offset;   // tracking.py:107
        if (p0 < 0) before = 1;
        d_ch[rank].acquiredFreq = s_carr[t];
        d_ch[rank].pos0 = p0 / sample_bytes;
        d_ch[rank].prn = t + 1;
        d_ch[rank].pad = (int)(p0 % sample_bytes);
        look->prn[rank] = t + 1;
        look->acquiredFreq[rank] = s_carr[t];
        look->codePhase[rank] = s_cph[t];
    }
    if (__builtin_amdgcn_ballot_w64(before != 0)) {
        flags |= 4;
        __syncthreads();
        if (t < n_ch) d_ch[t].prn = 0;      // (nothing is tracked; the host reports the channel)
    }
    if (t == 0) {
        look->n_ch = n_ch;
        look->n_active = n_act;
        look->flags = flags;
    }
}

// The sharded search's rank-local peaks as 40-byte records (PeakRec), packed on the device behind the search
__global__ __launch_bounds__(64) void acq_pack_kernel(const CoarseLook* __restrict__ stage, const long long* __restrict__ fine_bi,
                                                      const int* __restrict__ prn_list, int n_prn, double fs, double npts,
                                                      PeakRec* __restrict__ out, int slots) {
    const int t = threadIdx.x;
    if (t >= slots) return;
    PeakRec r;
    r.prn0 = 0; r.freqBin = -1; r.carrFreq = 0.0; r.codePhase = 0.0; r.peakMetric = 0.0; r.fineIdx = -1; r.valid = 0;
    if (t < n_prn) {
        r.prn0 = prn_list[t];
        r.freqBin = stage->po.fbi[t];
        r.peakMetric = stage->po.peak[t] / stage->second[t];
        r.valid = stage->po.index_error[t] ? -1 : 1;
        if (stage->range_error == 1 + t) r.valid = -2;
        if (r.valid < 0) r.codePhase = (double)stage->po.cph[t];   // (for the error text)
        const int n_det = stage->n_det;
        for (int d = 0; d < n_det; ++d)
            if (stage->det_slot[d] == t && r.valid == 1 && stage->range_error == 0) {
                const long long m = fine_bi[d] - 4;
                r.carrFreq = ((double)m * fs) / npts;
                r.codePhase = (double)stage->det_phase[d];
                r.fineIdx = (int)m;
            }
    }
    out[t] = r;
}

// gathered records -> the result page (LookPage::gather), then the word the host spins on
__global__ __launch_bounds__(256) void acq_gather_publish_kernel(const int* __restrict__ src, int n_words, int* __restrict__ dst,
                                                                 unsigned long long* __restrict__ word, unsigned long long seq) {
    for (int i = threadIdx.x; i < n_words; i += 256) dst[i] = src[i];
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(word, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ================================ environment and plans ================================
// The environment an acquisition call reads, once at its entry: diagnosis switches, and the cross-references of
// test_acquire_variants_agree.  Each of the older paths is also the only one for some input.
struct AcqEnv {
    bool v1;              // SGX_ACQ_V1=1: the round-1 passes (else: lengths the four-step transform does not take)
    bool one_queue;       // SGX_ACQ_STREAMS=1: the correlation batches on one queue (else: where the plan says so)
    bool top2_off;        // SGX_ACQ_TOP2=0: the round-4 second-peak search (else: sampling rates above 111 MHz)
    bool front_off;       // SGX_ACQ_FRONT=0: the four-launch front (else: fp64 signals)
    bool fine_v1;         // SGX_ACQ_FINE_V1=1: the fine search on the pass-per-launch transform
    bool device_led_off;  // SGX_ACQ_DEVICE_LED=0: the host looks between the coarse and the fine search
    bool split_event;     // SGX_ACQ_SPLIT_EVENT=1: an event between them, so that the split is measured
    bool spin;            // SGX_ACQ_SPIN=0 clears it: the look goes straight to the stream synchronisation
    int chunk_rows;       // SGX_ACQ_CHUNK_ROWS: correlation rows per chunk
};
static AcqEnv acq_env() {
    auto is = [](const char* name, char v) {
        const char* e = getenv(name);
        return e && e[0] == v;
    };
    AcqEnv e;
    e.v1 = is("SGX_ACQ_V1", '1');
    e.one_queue = is("SGX_ACQ_STREAMS", '1');
    e.top2_off = is("SGX_ACQ_TOP2", '0');
    e.front_off = is("SGX_ACQ_FRONT", '0');
    e.fine_v1 = is("SGX_ACQ_FINE_V1", '1');
    e.device_led_off = is("SGX_ACQ_DEVICE_LED", '0');
    e.split_event = is("SGX_ACQ_SPLIT_EVENT", '1');
    e.spin = !is("SGX_ACQ_SPIN", '0');
    e.chunk_rows = ACQ_DEFAULT_CHUNK_ROWS;
    const char* ce = getenv("SGX_ACQ_CHUNK_ROWS");
    if (ce && atoi(ce) > 0) e.chunk_rows = atoi(ce);
    return e;
}

// How the correlation batch of a call is cut (round 5).  Rows are ordered (PRN, block, bin) - coherent - or (PRN, bin, block)
// - non-coherent sums; a chunk is whole PRNs (prn_chunk of them) or, for non-coherent sums whose PRN does not fit half a
// chunk, ONE PRN's rows of a run of Doppler bins (bin_runs runs per PRN: a run is a batch of its own with fewer bins).
// The chunks alternate between `queues` HIP streams, each with its own intermediate of chunk_rows / queues rows: the columns
// kernel is bound by its stores and the rows kernel by its loads, and with two chunks in flight the one's stores overlap
// the other's loads (0.85 -> 0.77 ms for config 2, 3.21 -> 2.89 ms for config 4; both kernels move their bytes at 3-5 TB/s
// over the same fabric - the intermediate lives in the Infinity Cache - so a producer / consumer fusion has no more to win).
struct AcqPlan {
    int prn_chunk, bin_runs, bins_per_run, queues;
};
static AcqPlan acq_plan(int n_prn, int n_bins, int n_blocks, bool noncoh, int chunk_rows, int max_queues) {
    if (chunk_rows > ACQ_MAX_ROWS) chunk_rows = ACQ_MAX_ROWS;
    if (chunk_rows < 1) chunk_rows = 1;
    const int rows_per_prn = n_bins * n_blocks;
    AcqPlan p;
    p.bin_runs = 1;
    p.queues = (max_queues >= 2 && n_prn >= 2 && chunk_rows / 2 >= rows_per_prn) ? 2 : 1;
    if (max_queues >= 2 && p.queues == 1 && noncoh && rows_per_prn > chunk_rows / 2 && rows_per_prn <= chunk_rows && n_bins >= 2) {
        int runs = (rows_per_prn + chunk_rows / 2 - 1) / (chunk_rows / 2);
        if (runs > n_bins) runs = n_bins;
        if (runs >= 2) {
            p.bin_runs = runs;
            p.queues = 2;
        }
    }
    if (p.queues == 2 && p.bin_runs == 1) chunk_rows /= 2;
    p.prn_chunk = p.bin_runs > 1 ? 1 : chunk_rows / rows_per_prn;   // (a run of bins belongs to ONE PRN)
    if (p.prn_chunk < 1) p.prn_chunk = 1;
    if (p.prn_chunk > n_prn) p.prn_chunk = n_prn;
    if (p.queues == 2 && p.bin_runs == 1 && p.prn_chunk > (n_prn + 1) / 2) p.prn_chunk = (n_prn + 1) / 2;   // (both queues get work)
    p.bins_per_run = (n_bins + p.bin_runs - 1) / p.bin_runs;
    return p;
}
extern "C" int sgx_acquire_plan(int32_t n_prn, int32_t n_bins, int32_t n_blocks, int32_t noncoh, int32_t chunk_rows,
                                int32_t max_queues, int32_t* prn_chunk, int32_t* bin_runs, int32_t* bins_per_run,
                                int32_t* queues) {
    SGX_CHECK_ARG(n_prn >= 1 && n_bins >= 1 && n_blocks >= 1 && prn_chunk && bin_runs && bins_per_run && queues);
    const AcqPlan p = acq_plan(n_prn, n_bins, n_blocks, noncoh != 0, chunk_rows > 0 ? chunk_rows : ACQ_DEFAULT_CHUNK_ROWS, max_queues);
    *prn_chunk = p.prn_chunk;
    *bin_runs = p.bin_runs;
    *bins_per_run = p.bins_per_run;
    *queues = p.queues;
    return SGX_OK;
}

// PRNs per correlation batch of acquire_passes: whole PRNs, ACQ_MAX_ROWS rows at most - and, on a padded length len > n, no
// more rows than keep a batch's intermediate at the bytes ACQ_MAX_ROWS rows of the code's own length take (padding at
// least doubles a row; the batch shrinks instead of the context's two intermediates growing).  A batch is never less than
// one PRN: where one PRN's rows alone exceed that share (more than about 1 000 blocks x bins, a large coherent grid on
// the direct path), its intermediate is rows_per_prn padded rows, up to twice those bytes.
static int acq_passes_chunk(long long n, long long len, int rows_per_prn, int n_prn) {
    const long long max_rows = len > n ? (long long)ACQ_MAX_ROWS * n / len : ACQ_MAX_ROWS;
    int chunk = (int)(max_rows / rows_per_prn);
    if (chunk < 1) chunk = 1;
    if (chunk > n_prn) chunk = n_prn;
    return chunk;
}

extern "C" int sgx_acquire_fft_length(int64_t n_code, int64_t* length) {
    SGX_CHECK_ARG(length);
    const int64_t len = sgx_fft_corr_length(n_code);
    if (len == 0) {
        sgx_set_error("bad argument: %lld samples per code (2 .. 2^29)", (long long)n_code);
        return SGX_E_ARG;
    }
    *length = len;
    return SGX_OK;
}

extern "C" int sgx_acquire_fft_passes(int64_t n_code, int32_t* radices_out, int32_t* n_passes, int64_t* length,
                                      int32_t* last_pass_blocks, int32_t* tpb_out) {
    SGX_CHECK_ARG(radices_out && n_passes && length && last_pass_blocks && tpb_out);
    const int64_t len = sgx_fft_corr_length(n_code);
    if (len == 0) {
        sgx_set_error("bad argument: %lld samples per code (2 .. 2^29)", (long long)n_code);
        return SGX_E_ARG;
    }
    FftPlan p;   // (host fields only: no tables, nothing to destroy)
    std::vector<int> tpb;
    if (!sgx_fft_pass_list(len, &p.radices, &tpb) || p.radices.size() > SGX_FFT_MAX_PASSES) {
        sgx_set_error("no pass list for length %lld", (long long)len);
        return SGX_E_ARG;
    }
    p.n = len;
    for (size_t i = 0; i < p.radices.size(); ++i) {
        radices_out[i] = p.radices[i];
        tpb_out[i] = tpb[i];
    }
    *n_passes = (int32_t)p.radices.size();
    *length = len;
    *last_pass_blocks = sgx_fft_last_pass_blocks(&p);
    return SGX_OK;
}

// The radix passes on caller data (include/sgx.h): the tests' way to the kernels behind sgx_fft_forward_fused, through the
// plan and the pass loop the search uses.  Everything is allocated and freed here; the context lends device and stream.
namespace {
struct ProbeBufs {
    static constexpr int kMax = 12;   // (the fused form with a row map and maxima takes nine)
    void* p[kMax] = {nullptr};
    int n = 0;
    ~ProbeBufs() {
        for (int i = 0; i < n; ++i) hipFree(p[i]);
    }
    int get(void** out, size_t bytes) {
        *out = nullptr;
        if (n >= kMax) {
            sgx_set_error("sgx_fft_run_passes: more than %d buffers", kMax);
            return SGX_E_NOMEM;
        }
        hipError_t e = hipMalloc(out, bytes);
        if (e != hipSuccess) {
            sgx_set_error("hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
            return SGX_E_NOMEM;
        }
        p[n++] = *out;
        return SGX_OK;
    }
};
struct ProbePlan {
    FftPlan plan;
    ~ProbePlan() { sgx_fft_plan_destroy(&plan); }
};
}   // namespace

extern "C" int sgx_fft_run_passes(sgx_ctx* c, int64_t n, int32_t rows, const double* in, int64_t nonzero_len,
                                  const double* mul_x, int32_t n_x, const double* mul_f, int32_t n_f, int32_t rows_per_prn,
                                  int32_t prn_base, const int32_t* row_map, int64_t n_valid, double* out_rows,
                                  double* out_max, int32_t* out_arg) {
    SGX_CHECK_ARG(c && n >= 2 && n <= (1ll << 24) && rows >= 1 && rows <= 4096);
    const bool fused = mul_x != nullptr;
    if (fused) {
        SGX_CHECK_ARG(mul_f && !in && n_x >= 1 && n_x <= 4096 && n_f >= 1 && n_f <= 4096 && n_valid >= 0 && n_valid <= n);
        SGX_CHECK_ARG((out_max != nullptr) == (out_arg != nullptr) && (out_max != nullptr) != (out_rows != nullptr));
        if (row_map) {
            for (int r = 0; r < rows; ++r)
                SGX_CHECK_ARG(row_map[2 * r] >= 0 && row_map[2 * r] < n_x && row_map[2 * r + 1] >= 0 && row_map[2 * r + 1] < n_f);
        } else {
            SGX_CHECK_ARG(rows_per_prn >= 1 && rows_per_prn <= n_x && prn_base >= 0 &&
                          prn_base + (rows - 1) / rows_per_prn < n_f);
        }
    } else {
        SGX_CHECK_ARG(in && out_rows && !mul_f && !out_max && !out_arg && nonzero_len >= 1 && nonzero_len <= n);
    }
    SGX_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    ProbePlan pp;
    int rc = sgx_fft_plan_create(&pp.plan, n);   // (refuses what the search's plan refuses)
    if (rc != SGX_OK) return rc;
    const size_t row_bytes = sizeof(cplx) * (size_t)n;
    ProbeBufs bufs;
    cplx *wa = nullptr, *wb = nullptr, *res = nullptr;
    if ((rc = bufs.get((void**)&wa, (size_t)rows * row_bytes)) != SGX_OK) return rc;
    if ((rc = bufs.get((void**)&wb, (size_t)rows * row_bytes)) != SGX_OK) return rc;
    if (!fused) {
        SGX_HIP(hipMemcpyAsync(wa, in, (size_t)rows * row_bytes, hipMemcpyHostToDevice, st));
        rc = sgx_fft_forward(&pp.plan, wa, wb, rows, st, &res, nonzero_len);
        if (rc != SGX_OK) return rc;
        SGX_HIP(hipMemcpyAsync(out_rows, res, (size_t)rows * row_bytes, hipMemcpyDeviceToHost, st));
        SGX_HIP(hipStreamSynchronize(st));
        return SGX_OK;
    }
    cplx *dx = nullptr, *df = nullptr;
    if ((rc = bufs.get((void**)&dx, (size_t)n_x * row_bytes)) != SGX_OK) return rc;
    if ((rc = bufs.get((void**)&df, (size_t)n_f * row_bytes)) != SGX_OK) return rc;
    SGX_HIP(hipMemcpyAsync(dx, mul_x, (size_t)n_x * row_bytes, hipMemcpyHostToDevice, st));
    SGX_HIP(hipMemcpyAsync(df, mul_f, (size_t)n_f * row_bytes, hipMemcpyHostToDevice, st));
    FftFuse fu;
    fu.mul_x = dx;
    fu.mul_f = df;
    fu.rows_per_prn = row_map ? 1 : rows_per_prn;
    fu.prn_base = row_map ? 0 : prn_base;
    if (row_map) {
        int2* dm = nullptr;
        if ((rc = bufs.get((void**)&dm, sizeof(int2) * (size_t)rows)) != SGX_OK) return rc;
        SGX_HIP(hipMemcpyAsync(dm, row_map, sizeof(int2) * (size_t)rows, hipMemcpyHostToDevice, st));
        fu.row_map = dm;
    }
    if (out_rows) {
        rc = sgx_fft_forward_fused(&pp.plan, wa, wb, rows, st, &res, n, &fu);
        if (rc != SGX_OK) return rc;
        SGX_HIP(hipMemcpyAsync(out_rows, res, (size_t)rows * row_bytes, hipMemcpyDeviceToHost, st));
        SGX_HIP(hipStreamSynchronize(st));
        return SGX_OK;
    }
    const int nblk = sgx_fft_last_pass_blocks(&pp.plan);
    double *d_pmax = nullptr, *d_max = nullptr;
    int *d_parg = nullptr, *d_arg = nullptr;
    if ((rc = bufs.get((void**)&d_pmax, sizeof(double) * (size_t)rows * (size_t)nblk)) != SGX_OK) return rc;
    if ((rc = bufs.get((void**)&d_parg, sizeof(int) * (size_t)rows * (size_t)nblk)) != SGX_OK) return rc;
    if ((rc = bufs.get((void**)&d_max, sizeof(double) * (size_t)rows)) != SGX_OK) return rc;
    if ((rc = bufs.get((void**)&d_arg, sizeof(int) * (size_t)rows)) != SGX_OK) return rc;
    fu.pmax = d_pmax;
    fu.parg = d_parg;
    fu.inv_n = 1.0 / (double)n;
    fu.n_valid = n_valid;
    rc = sgx_fft_forward_fused(&pp.plan, wa, wb, rows, st, &res, n, &fu);
    if (rc != SGX_OK) return rc;
    acq_rowmax_finish_kernel<<<rows, 64, 0, st>>>(d_pmax, d_parg, nblk, d_max, d_arg);
    SGX_HIP(hipGetLastError());
    SGX_HIP(hipMemcpyAsync(out_max, d_max, sizeof(double) * (size_t)rows, hipMemcpyDeviceToHost, st));
    SGX_HIP(hipMemcpyAsync(out_arg, d_arg, sizeof(int) * (size_t)rows, hipMemcpyDeviceToHost, st));
    SGX_HIP(hipStreamSynchronize(st));
    return SGX_OK;
}

extern "C" int sgx_acquire_plan_limits(int32_t* default_chunk_rows, int32_t* max_rows) {
    SGX_CHECK_ARG(default_chunk_rows && max_rows);
    *default_chunk_rows = ACQ_DEFAULT_CHUNK_ROWS;
    *max_rows = ACQ_MAX_ROWS;
    return SGX_OK;
}
// How the correlation batch is cut: whole PRNs while one PRN's rows fit a chunk (ACQ_DEFAULT_CHUNK_ROWS), else one PRN
// per batch in runs - of bins for non-coherent sums (rows (bin, window): a run's output rows are whole bins), of windows
// for the reference rule (rows (window, bin): a run's output rows are whole windows).
static void coh_plan(CohGrid* g, int n_prn, long long N) {
    const int chunk = ACQ_DEFAULT_CHUNK_ROWS;
    const int rows_per_prn = g->M * g->n_bins;
    if (g->path == 0) {   // (acquire_passes: its own chunks of whole PRNs)
        g->prn_chunk = acq_passes_chunk(N, sgx_fft_corr_length(N), rows_per_prn, n_prn);
        g->runs = 1;
        g->per_run = g->noncoh ? g->n_bins : g->M;
    } else if (rows_per_prn <= chunk) {
        g->prn_chunk = chunk / rows_per_prn;
        g->runs = 1;
        g->per_run = g->noncoh ? g->n_bins : g->M;
    } else {
        g->prn_chunk = 1;
        const int total = g->noncoh ? g->n_bins : g->M;
        const int other = g->noncoh ? g->M : g->n_bins;
        g->per_run = chunk / other < 1 ? 1 : chunk / other;
        g->runs = (total + g->per_run - 1) / g->per_run;
    }
    if (g->prn_chunk < 1) g->prn_chunk = 1;
    if (g->prn_chunk > n_prn) g->prn_chunk = n_prn;
}

// f N / fs = shift + phi (shift integer, 0 <= phi < 1) for every bin f0 + step k of a grid: the distinct fractions to
// *phi, (phi index, circular shift) per bin to *bin_map.  Returns the number of distinct fractions; a path that shares
// forward spectra takes the grid if they are few enough for it.
static int acq_phi_split(double f0, double step, int n_bins, long long N, double fs, std::vector<double>* phi,
                         std::vector<int2>* bin_map) {
    phi->clear();
    bin_map->assign((size_t)n_bins, make_int2(0, 0));
    for (int k = 0; k < n_bins; ++k) {
        const double f = f0 + step * k;
        const double ratio = f * (double)N / fs;
        const double sh = floor(ratio + 1e-9);
        double ph = ratio - sh;
        if (ph < 1e-9) ph = 0.0;
        int j = -1;
        for (size_t q = 0; q < phi->size() && j < 0; ++q)
            if (fabs((*phi)[q] - ph) < 1e-9) j = (int)q;
        if (j < 0) {
            j = (int)phi->size();
            phi->push_back(ph);
        }
        long long shm = (long long)sh % N;
        if (shm < 0) shm += N;
        (*bin_map)[(size_t)k] = make_int2(j, (int)shm);
    }
    return (int)phi->size();
}

// Parameters -> grid, phi decomposition, path and batches.  SGX_E_ARG (with the reason) for anything out of range.
static int coh_grid(const sgx_settings& S, long long N, const sgx_acq_params* p, int n_prn, CohGrid* g) {
    if (!p) {
        sgx_set_error("bad argument: no sgx_acq_params");
        return SGX_E_ARG;
    }
    const int T = p->coherent_ms, M = p->n_windows;
    const double step = p->bin_step_hz;
    if (T < 1 || T > ACQ_COH_MAX_MS || M < 1 || M > ACQ_COH_MAX_WINDOWS || (long long)T * M > ACQ_COH_MAX_SPAN_MS) {
        sgx_set_error("bad argument: coherent_ms %d x n_windows %d (coherent_ms 1..%d, n_windows 1..%d, product <= %d ms)",
                      T, M, ACQ_COH_MAX_MS, ACQ_COH_MAX_WINDOWS, ACQ_COH_MAX_SPAN_MS);
        return SGX_E_ARG;
    }
    if ((p->noncoh != 0 && p->noncoh != 1) || p->reserved != 0) {
        sgx_set_error("bad argument: noncoh %d (0 or 1), reserved %d (0)", p->noncoh, p->reserved);
        return SGX_E_ARG;
    }
    if (!(step > 0.0) || !std::isfinite(step)) {
        sgx_set_error("bad argument: bin_step_hz %g (must be > 0)", step);
        return SGX_E_ARG;
    }
    const double nb = nearbyint(S.acqSearchBand * 1000.0 / step) + 1;
    if (!(nb >= 1.0 && nb <= (double)ACQ_COH_MAX_BINS)) {
        sgx_set_error("bad argument: a %g kHz band at %g Hz steps is %.0f Doppler bins (at most %d)", S.acqSearchBand, step,
                      nb, ACQ_COH_MAX_BINS);
        return SGX_E_ARG;
    }
    if (sgx_fft_corr_length(N) == 0) {
        sgx_set_error("bad argument: %lld samples per code", N);
        return SGX_E_ARG;
    }
    g->T = T;
    g->M = M;
    g->noncoh = p->noncoh;
    g->step = step;
    g->f0 = S.IF - S.acqSearchBand / 2 * 1000;
    g->n_bins = (int)nb;
    g->n_phi = acq_phi_split(g->f0, step, g->n_bins, N, S.samplingFreq, &g->phi, &g->bin_map);
    g->path = (sgx_fft4_supported(N) && g->n_phi <= ACQ_COH_MAX_PHI) ? 1 : 0;
    if (g->path == 0 && (long long)M * g->n_bins > ACQ_MAX_ROWS) {
        sgx_set_error("bad argument: the direct path (%d distinct Doppler fractions, %lld samples per code) takes at most "
                      "%d windows x bins, asked for %d x %d", g->n_phi, N, ACQ_MAX_ROWS, M, g->n_bins);
        return SGX_E_ARG;
    }
    coh_plan(g, n_prn, N);
    return SGX_OK;
}

// The fine search's lengths (acquisition.py:167-187): 10 ms of signal, the padded transform, its one-sided spectrum
struct FineGeom {
    long long len, npts, uniq;
};
static FineGeom acq_fine_geom(long long N) {
    FineGeom f;
    f.len = 10 * N;
    f.npts = 8ll << (long long)ceil(log2((double)f.len));
    f.uniq = (long long)ceil((double)(f.npts + 1) / 2.0);
    return f;
}

// Detection d's fine-search range for T > 1: the spectrum indices i of the 2^k-point transform (frequency i fs / npts)
// within one bin step of its coarse bin, inside the reference's [4, uniq - 5).
static std::vector<long long> coh_fine_windows(const CohGrid& g, const sgx_settings& S, long long N,
                                               const std::vector<int>& det_bin) {
    const FineGeom fg = acq_fine_geom(N);
    const long long npts = fg.npts, uniq = fg.uniq;
    std::vector<long long> win;
    for (int k : det_bin) {
        const double fk = g.f0 + g.step * k;
        long long lo = (long long)ceil(((fk - g.step) * (double)npts) / S.samplingFreq);
        long long hi = (long long)floor(((fk + g.step) * (double)npts) / S.samplingFreq) + 1;
        if (lo < 4) lo = 4;
        if (hi > uniq - 5) hi = uniq - 5;
        if (hi <= lo) hi = lo + 1;
        win.push_back(lo);
        win.push_back(hi);
    }
    return win;
}

// ================================ stages ================================
// One call as every stage and path sees it
struct AcqCall {
    sgx_ctx* c;
    SgxSig x;
    size_t n_samples;
    const int32_t* prn0;
    int n_prn;
    AcqOut out;   // [n_prn]
    AcqEnv env;
};
static AcqCall acq_call(sgx_ctx* c, SgxSig x, size_t n_samples, const int32_t* prn0, int32_t n_prn, const AcqOut& out,
                        const AcqEnv& env) {
    AcqCall a;
    a.c = c;
    a.x = x;
    a.n_samples = n_samples;
    a.prn0 = prn0;
    a.n_prn = n_prn;
    a.out = out;
    a.env = env;
    return a;
}
// The detections of a call (acquisition.py:164-166) in ascending position of its PRN list
struct AcqDets {
    std::vector<int> prn, phase, slot;
};

static int acq_check_prns(const int32_t* prn0, int32_t n_prn) {
    SGX_CHECK_ARG(n_prn >= 1 && n_prn <= 32);
    for (int i = 0; i < n_prn; ++i) SGX_CHECK_ARG(prn0[i] >= 0 && prn0[i] < 32);
    return SGX_OK;
}

// The record's window as the kernels read it, once it is resident
static int acq_record_sig(sgx_ctx* c, const sgx_if* r, size_t offset, size_t n_samples, SgxSig* x) {
    const int rq = sgx_if_require(r, offset + n_samples);   // a record that is still streaming in
    if (rq != SGX_OK) return rq;
    SGX_HIP(hipSetDevice(c->device));
    x->i8 = r->d + offset;
    x->f64 = nullptr;
    return SGX_OK;
}

// acquire() on a signal that is not int8 (acquisition.py:55-59 takes whatever real dtype numpy hands it): the caller's
// fp64 samples are copied to HBM and every kernel reads them instead of the int8 record; the arithmetic is the same
// fp64 arithmetic either way.
static int acq_upload_f64(sgx_ctx* c, const double* signal, size_t n_samples, SgxSig* x) {
    SGX_HIP(hipSetDevice(c->device));
    const int rc = c->d_sig64.ensure(sizeof(double) * (n_samples + 64));
    if (rc != SGX_OK) return rc;
    SGX_HIP(hipMemcpyAsync(c->d_sig64, signal, sizeof(double) * n_samples, hipMemcpyHostToDevice, c->stream));
    SGX_HIP(hipStreamSynchronize(c->stream));   // the caller may free `signal` on return
    x->i8 = nullptr;
    x->f64 = c->d_sig64;
    return SGX_OK;
}

// Where a search's samples come from: n_samples at `offset` of a resident record, or (r null) of the caller's fp64 signal
struct AcqSource {
    const sgx_if* r;
    size_t offset;
    const double* signal;
    size_t n_samples;
};
static int acq_source_sig(sgx_ctx* c, const AcqSource& src, SgxSig* x) {
    return src.r ? acq_record_sig(c, src.r, src.offset, src.n_samples, x) : acq_upload_f64(c, src.signal, src.n_samples, x);
}

// What the searches on the reference's grid check before they touch the device: PRN list, blocks, the source's length
static int acq_open_source(sgx_ctx* c, const AcqSource& src, const int32_t* prn0, int32_t n_prn, int32_t n_blocks, SgxSig* x) {
    SGX_CHECK_ARG(c && (src.r || src.signal) && prn0);
    SGX_CHECK_ARG(n_blocks >= 1 && n_blocks <= 64);
    const int rc = acq_check_prns(prn0, n_prn);
    if (rc != SGX_OK) return rc;
    const long long need = (long long)n_blocks * c->n_code;
    const bool outside = src.r && (src.offset > src.r->n || src.n_samples > src.r->n - src.offset);
    if (outside || (long long)src.n_samples < need) {
        if (src.r)
            sgx_set_error("record window too short: %zu samples at offset %zu, %lld needed for the coarse search",
                          src.n_samples, src.offset, need);
        else
            sgx_set_error("signal too short: %zu samples, %lld needed for the coarse search", src.n_samples, need);
        return SGX_E_RANGE;
    }
    return acq_source_sig(c, src, x);
}

static bool acq_out_non_null(const AcqOut& o) {
    return o.carrFreq && o.codePhase && o.peakMetric && o.freqBin && o.fineIdx;
}
static void acq_reset_outputs(const AcqOut& o, int n) {
    for (int i = 0; i < n; ++i) {
        o.carrFreq[i] = 0.0;
        o.codePhase[i] = 0.0;
        o.peakMetric[i] = 0.0;
        o.freqBin[i] = -1;
        o.fineIdx[i] = -1;
    }
}
static void acq_copy_results(const AcqOut& dst, const AcqOut& src, int n) {
    for (int i = 0; i < n; ++i) {
        dst.carrFreq[i] = src.carrFreq[i];
        dst.codePhase[i] = src.codePhase[i];
        dst.peakMetric[i] = src.peakMetric[i];
        dst.freqBin[i] = src.freqBin[i];
        dst.fineIdx[i] = src.fineIdx[i];
    }
}

// Device times of a call from its events ev[0] (start), ev[1] (between coarse and fine search), ev[2] (end).  An event
// between the coarse and the fine kernels holds the fine search back by 6-8 us, so the device-led sequence records it on
// request only (SGX_ACQ_SPLIT_EVENT=1); without it the split is NOT measured: NaN, not total / 0
static void acq_event_times(sgx_ctx* c, bool split_measured) {
    hipEventElapsedTime(&c->timing.acquire_ms, c->ev[0], c->ev[2]);
    if (split_measured) {
        hipEventElapsedTime(&c->timing.acq_coarse_ms, c->ev[0], c->ev[1]);
        hipEventElapsedTime(&c->timing.acq_fine_ms, c->ev[1], c->ev[2]);
    } else {
        c->timing.acq_coarse_ms = __builtin_nanf("");
        c->timing.acq_fine_ms = __builtin_nanf("");
    }
}

// The reference's IndexError (Q5; acquisition.py:152-162) and its failure to broadcast (acquisition.py:177) as errors
static int acq_index_error(long long N, int prn, int code_phase) {
    sgx_set_error("IndexError: index %lld is out of bounds for axis 1 with size %lld "
                  "(PRN index %d, codePhase %d; reference acquisition.py:152-162)", N, N, prn, code_phase);
    return SGX_E_INDEX;
}
static int acq_fine_range_error(long long end, size_t n_samples) {
    sgx_set_error("fine search needs codePhase + 10 ms = %lld samples, record window has %zu "
                  "(reference acquisition.py:177 would fail to broadcast)", end, n_samples);
    return SGX_E_RANGE;
}

// The first of PRNs [first, first + n) of the call at which the reference raises (po: entry i = PRN first + i)
static int acq_look_index_error(const AcqCall& a, const PeakOut& po, int first, int n) {
    for (int i = 0; i < n; ++i)
        if (po.index_error[i]) return acq_index_error(a.c->n_code, a.prn0[first + i], po.cph[i]);
    return SGX_OK;
}

// The look decoded: peaks and second peaks of PRNs [first, first + n) -> peakMetric, freqBin and the detections
// (acquisition.py:164-166), or the reference's IndexError
static int acq_look_decode(const AcqCall& a, const PeakOut& po, const double* second, int first, int n, AcqDets* det) {
    const int rc = acq_look_index_error(a, po, first, n);
    if (rc != SGX_OK) return rc;
    for (int i = 0; i < n; ++i) {
        const int o = first + i;
        const double ratio = po.peak[i] / second[i];
        a.out.peakMetric[o] = ratio;
        a.out.freqBin[o] = po.fbi[i];
        if (ratio > a.c->s.acqThreshold) {
            det->prn.push_back(a.prn0[o]);
            det->phase.push_back(po.cph[i]);
            det->slot.push_back(o);
        }
    }
    return SGX_OK;
}

// Waits for a result word in the pinned page (acq_publish_kernel's `seq`, the fine search's `seq2`, the gathered peaks' word)
static int acq_look_wait(sgx_ctx* c, const unsigned long long* word, unsigned long long seq, bool spin) {
    return sgx_look_wait(c->stream, word, seq, spin, 0.05, 1024, "acquisition: the search's result page was not written", nullptr);
}

// The second queue of the correlation batches and its two events, created on first use
static int acq_second_queue(sgx_ctx* c, hipStream_t* st2) {
    if (!c->acq_stream2) {
        // (into locals; the context gets them only when ALL exist - a half-made second queue would fail every later call)
        int least = 0, greatest = 0;
        SGX_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
        hipStream_t ns = nullptr;
        hipEvent_t ne[2] = {nullptr, nullptr};
        hipError_t ce = (c->priority == 0) ? hipStreamCreateWithFlags(&ns, hipStreamNonBlocking)
                                           : hipStreamCreateWithPriority(&ns, hipStreamNonBlocking, c->priority < 0 ? greatest : least);
        for (int i = 0; i < 2 && ce == hipSuccess; ++i) ce = hipEventCreateWithFlags(&ne[i], hipEventDisableTiming);
        if (ce != hipSuccess) {
            for (int i = 0; i < 2; ++i)
                if (ne[i]) hipEventDestroy(ne[i]);
            if (ns) hipStreamDestroy(ns);
            sgx_set_error("acquisition: the second queue could not be created: %s", hipGetErrorString(ce));
            return SGX_E_HIP;
        }
        c->acq_stream2 = ns;
        c->acq_ev2[0] = ne[0];
        c->acq_ev2[1] = ne[1];
    }
    *st2 = c->acq_stream2;
    return SGX_OK;
}

// The correlation of the paths that read shifted forward spectra (four-step, coherent shift): its geometry, and where in
// the reduction buffer (c->d_pow) its kernels leave their results
struct AcqCorr {
    int n_bins, n_phi, n_blocks, noncoh;   // (blocks: 1-ms blocks, or the coherent search's windows)
    int out_per_prn, rows_out_all;
    bool top2;                             // peak and second peak from one pass (acq_rowtop2_peak_kernel)
    int nblk, nres;
    const cplx* d_codefd;                  // code spectra, behind the forward spectra in c->d_fwd
    // [per-workgroup maxima | their indices] or [per-residue maxima | second maxima | indices], [row maxima | row indices],
    // then (non-coherent, round-4 sequence) the second-peak power rows
    double* pmax;
    int* parg;
    double *t2b1, *t2b2;
    int* t2i1;
    double* rowmax;
    int* rowarg;
    double* power;
};
static int acq_corr_carve(sgx_ctx* c, AcqCorr* k, size_t pow_need) {
    const size_t rows = (size_t)k->rows_out_all;
    const size_t part_bytes = ((rows * (k->top2 ? (size_t)k->nres * 20 : (size_t)k->nblk * 12)) + 255) / 256 * 256;
    const size_t red_bytes = (part_bytes + rows * 12 + 1023) / 256 * 256;
    const int rc = c->d_pow.ensure(red_bytes + pow_need);
    if (rc != SGX_OK) return rc;
    char* red = (char*)c->d_pow.get();
    k->pmax = (double*)red;
    k->parg = (int*)(red + rows * k->nblk * 8);
    k->t2b1 = (double*)red;
    k->t2b2 = k->t2b1 + rows * k->nres;
    k->t2i1 = (int*)(k->t2b2 + rows * k->nres);
    k->rowmax = (double*)(red + part_bytes);
    k->rowarg = (int*)(red + part_bytes + rows * 8);
    k->power = (double*)(red + red_bytes);
    return SGX_OK;
}
// The scratch of such a correlation - two intermediates of work_rows rows (the forward batch's rows at least) and d_fwd =
// [forward | code] spectra - and its AcqCorr.  power_rows: room behind the reductions for the round-4 sequence's second-peak
// power rows.
static int acq_corr_setup(sgx_ctx* c, AcqCorr* k, int n_prn, int n_bins, int n_phi, int n_blocks, int noncoh, bool top2,
                          size_t work_rows, bool power_rows) {
    const size_t N = (size_t)c->n_code, row_bytes = sizeof(cplx) * N;
    const size_t rows_fwd = (size_t)n_blocks * n_phi;
    if (work_rows < rows_fwd + n_prn) work_rows = rows_fwd + n_prn;
    int rc;
    if ((rc = c->d_work[0].ensure(work_rows * row_bytes)) != SGX_OK) return rc;
    if ((rc = c->d_work[1].ensure(work_rows * row_bytes)) != SGX_OK) return rc;
    if ((rc = c->d_fwd.ensure((rows_fwd + n_prn) * row_bytes)) != SGX_OK) return rc;
    k->n_bins = n_bins;
    k->n_phi = n_phi;
    k->n_blocks = n_blocks;
    k->noncoh = noncoh;
    k->out_per_prn = noncoh ? n_bins : n_blocks * n_bins;
    k->rows_out_all = n_prn * k->out_per_prn;
    k->nblk = sgx_fft4_row_blocks();
    k->nres = sgx_fft4_residues();
    k->top2 = top2;
    k->d_codefd = c->d_fwd + rows_fwd * N;
    size_t pow_need = 0;
    if (power_rows) {
        pow_need = (size_t)k->rows_out_all * k->nblk * 12 + 4096;
        if (noncoh && pow_need < (size_t)n_prn * sizeof(double) * N) pow_need = (size_t)n_prn * sizeof(double) * N;
    }
    return acq_corr_carve(c, k, pow_need);
}

// One correlation batch: PRNs [p0, p0 + np) x bins [bin0, bin0 + nb) x blocks [blk0, blk0 + nblocks) -> its Fft4Fuse (a
// run of bins is a batch of its own with fewer bins; a run of blocks reads its blocks' forward rows) and the transform,
// through intermediate `work` on queue `st`.  Rows are ordered (PRN, block, bin), or (PRN, bin, block) for non-coherent
// sums, which take all blocks of a bin in one batch.
static int acq_corr_batch(sgx_ctx* c, const AcqCorr& k, int p0, int np, int bin0, int nb, int blk0, int nblocks, cplx* work,
                          hipStream_t st) {
    Fft4Fuse fu;
    fu.mul_x = c->d_fwd + (size_t)blk0 * k.n_phi * (size_t)c->n_code;
    fu.mul_f = k.d_codefd;
    fu.bin_map = c->d_small->bin_map + bin0;
    fu.n_bins = nb;
    fu.n_phi = k.n_phi;
    fu.rows_per_prn = nb * nblocks;
    fu.prn_base = p0;
    fu.n_blocks = nblocks;
    fu.blocks_fast = k.noncoh ? 1 : 0;
    const size_t out0 = (size_t)p0 * k.out_per_prn + (k.noncoh ? (size_t)bin0 : (size_t)blk0 * k.n_bins + (size_t)bin0);
    if (k.top2) {
        fu.t2_b1 = k.t2b1 + out0 * k.nres;
        fu.t2_b2 = k.t2b2 + out0 * k.nres;
        fu.t2_i1 = k.t2i1 + out0 * k.nres;
    } else {
        fu.pmax = k.pmax + out0 * k.nblk;
        fu.parg = k.parg + out0 * k.nblk;
    }
    fu.inv_n = 1.0 / (double)c->n_code;
    fu.sum_blocks = k.noncoh ? nblocks : 1;
    return sgx_fft4_forward(&c->plan_code, nullptr, work, nullptr, (int64_t)np * fu.rows_per_prn, st, &fu);
}

// Row maxima, block choice, global peak, exclusion list and second peak of every PRN in one launch; with a stage in
// `pub` the detections too, else a publish kernel follows
static void acq_queue_top2(const AcqCall& a, const AcqCorr& k, int spc, const PublishArgs& pub) {
    SgxSmall* dsm = a.c->d_small;
    acq_rowtop2_peak_kernel<<<k.rows_out_all, 64, 0, a.c->stream>>>(k.t2b1, k.t2b2, k.t2i1, k.nres, k.rowmax, k.rowarg,
                                                                    dsm->arrived, a.n_prn, k.out_per_prn, k.n_bins, k.n_blocks,
                                                                    k.noncoh, a.c->n_code, spc, &dsm->peak_out, dsm->second, pub);
}
// The coarse search's outcome to `page` (the pinned one; or, device-led with `det`, its device-side copy)
static void acq_queue_publish(const AcqCall& a, CoarseLook* page, unsigned long long seq, long long fine_len, AcqDet* det) {
    SgxSmall* dsm = a.c->d_small;
    acq_publish_kernel<<<1, 64, 0, a.c->stream>>>(&dsm->peak_out, dsm->second, a.n_prn, page, seq, dsm->prn, a.c->s.acqThreshold,
                                                  fine_len, (long long)a.n_samples, reinterpret_cast<int*>(det));
}

// Fine frequency search (acquisition.py:167-193) for the detected PRNs; records event ev[2] and synchronises.
// win (coherent search, else null): [2 d], [2 d + 1] = detection d's own arg-max range in place of [4, uniq - 5)
static int acquire_fine(const AcqCall& a, const AcqDets& det, long long* d_sum, const std::vector<long long>* win) {
    sgx_ctx* c = a.c;
    const SgxSig x = a.x;
    const size_t n_samples = a.n_samples;
    hipStream_t st = c->stream;
    const sgx_settings& S = c->s;
    const double ts = 1.0 / S.samplingFreq;
    SgxSmall* dsm = c->d_small;
    SgxSmall* hsm = c->h_small;
    int rc = SGX_OK;
    const int n_det = (int)det.prn.size();
    if (n_det == 0) {
        hipEventRecord(c->ev[2], st);
        SGX_HIP(hipStreamSynchronize(st));
        return SGX_OK;
    }
    const FineGeom fg = acq_fine_geom(c->n_code);
    const long long len = fg.len, npts = fg.npts, uniq = fg.uniq;
    for (int d = 0; d < n_det; ++d)
        if ((long long)det.phase[d] + len > (long long)n_samples) return acq_fine_range_error((long long)det.phase[d] + len, n_samples);
    rc = sgx_fft_plan_create(&c->plan_fine, npts);
    if (rc != SGX_OK) return rc;
    const int n_rows = (n_det + 1) / 2;   // two real signals per complex row
    if ((rc = c->d_fine[0].ensure((size_t)n_rows * sizeof(cplx) * (size_t)npts)) != SGX_OK)
        return rc;
    if ((rc = c->d_fine[1].ensure((size_t)n_rows * sizeof(cplx) * (size_t)npts)) != SGX_OK)
        return rc;
    const double tc1 = 1.0 / S.codeFreqBasis;
    const bool fine2 = sgx_fft_fine_supported(npts) && !a.env.fine_v1;
    double mean = 0.0;
    if (!fine2) {
        long long h_sum = 0;
        SGX_HIP(hipMemcpyAsync(&h_sum, d_sum, 8, hipMemcpyDeviceToHost, st));
        SGX_HIP(hipStreamSynchronize(st));
        double h_sumd;
        memcpy(&h_sumd, &h_sum, 8);
        mean = (x.f64 ? h_sumd : (double)h_sum) / (double)n_samples;   // longSignal.mean(), acquisition.py:59
    }
    int nblk = 256;
    // per-detection ranges (coherent search): to device memory, and their union as the common range
    long long* d_win = nullptr;
    long long win_lo = 4, win_hi = uniq - 5;
    if (win) {
        d_win = dsm->fine_win;
        memcpy(hsm->fine_win, win->data(), sizeof(long long) * 2 * (size_t)n_det);
        SGX_HIP(hipMemcpyAsync(d_win, hsm->fine_win, sizeof(long long) * 2 * (size_t)n_det, hipMemcpyHostToDevice, st));
        win_lo = (*win)[0];
        win_hi = (*win)[1];
        for (int d = 1; d < n_det; ++d) {
            win_lo = (*win)[2 * (size_t)d] < win_lo ? (*win)[2 * (size_t)d] : win_lo;
            win_hi = (*win)[2 * (size_t)d + 1] > win_hi ? (*win)[2 * (size_t)d + 1] : win_hi;
        }
    }
    if (fine2) {
        // two kernels with LDS-resident sub-transforms, input built on the fly (the mean comes from the device-side
        // sum: no host look), arg-max fused (sgx_fft.hip)
        nblk = sgx_fft_fine_partials();
        FineSearch f;
        f.x = x;
        f.codes = c->d_codes;
        f.len = len;
        f.d_sum = d_sum;
        f.n_mean = (double)n_samples;
        f.ts = ts;
        f.tc1 = tc1;
        f.work = c->d_fine[0];
        f.n_det = n_det;
        f.det_prn = det.prn.data();
        f.det_phase = det.phase.data();
        f.lo = win_lo;
        f.hi = win_hi;
        f.win = d_win;
        f.pv = dsm->fine_pv;
        f.pi = dsm->fine_pi;
        rc = sgx_fft_fine_search(&c->plan_fine, f, st);
        if (rc != SGX_OK) return rc;
    } else {
        SGX_HIP(hipMemcpyAsync(dsm->det_prn, det.prn.data(), sizeof(int) * (size_t)n_det, hipMemcpyHostToDevice, st));
        SGX_HIP(hipMemcpyAsync(dsm->det_phase, det.phase.data(), sizeof(int) * (size_t)n_det, hipMemcpyHostToDevice, st));
        dim3 grid((unsigned)((len + 255) / 256), (unsigned)n_rows);
        acq_fine_prep_kernel<<<grid, 256, 0, st>>>(x, c->d_codes, c->d_fine[0], len, npts, mean, ts, tc1, dsm->det_prn,
                                                   dsm->det_phase, n_det);
        cplx* res = nullptr;
        rc = sgx_fft_forward(&c->plan_fine, c->d_fine[0], c->d_fine[1], n_rows, st, &res, len);
        if (rc != SGX_OK) return rc;
        dim3 g2((unsigned)nblk, (unsigned)n_det);
        acq_fine_argmax_kernel<<<g2, 256, 0, st>>>(res, npts, 4, uniq - 5, dsm->fine_pv, dsm->fine_pi, d_win);
    }
    const double* h_pv = hsm->fine_pv;
    const long long* h_pi = hsm->fine_pi;
    SGX_HIP(hipMemcpyAsync(hsm->fine_pv, dsm->fine_pv, sizeof(double) * (size_t)n_det * nblk, hipMemcpyDeviceToHost, st));
    SGX_HIP(hipMemcpyAsync(hsm->fine_pi, dsm->fine_pi, sizeof(long long) * (size_t)n_det * nblk, hipMemcpyDeviceToHost, st));
    hipEventRecord(c->ev[2], st);
    SGX_HIP(hipStreamSynchronize(st));
    for (int d = 0; d < n_det; ++d) {
        double bv = -1.0;
        long long bi = 0;
        for (int b = 0; b < nblk; ++b) {
            const double v = h_pv[d * nblk + b];
            const long long i = h_pi[d * nblk + b];
            if (v > bv || (v == bv && i < bi)) {
                bv = v;
                bi = i;
            }
        }
        const long long m = bi - 4;   // index inside the [4:uniq-5] slice (acquisition.py:187)
        const int o = det.slot[d];
        a.out.carrFreq[o] = ((double)m * S.samplingFreq) / (double)npts;   // acquisition.py:189-191 (Q3)
        a.out.codePhase[o] = (double)det.phase[d];
        a.out.fineIdx[o] = (int)m;
    }
    return SGX_OK;
}

// The tail of a host-led call: the detections' fine search (for a coherent grid with T > 1: inside one bin step of each
// detection's coarse bin) and the device times
static int acq_fine_and_times(const AcqCall& a, const AcqDets& det, long long* d_sum, const CohGrid* g) {
    std::vector<long long> win;
    if (g && g->T > 1) {
        std::vector<int> det_bin;
        for (int o : det.slot) det_bin.push_back(a.out.freqBin[o]);
        win = coh_fine_windows(*g, a.c->s, a.c->n_code, det_bin);
    }
    const int rc = acquire_fine(a, det, d_sum, win.empty() ? nullptr : &win);
    if (rc != SGX_OK) return rc;
    acq_event_times(a.c, true);
    return SGX_OK;
}
// ... behind the host's look at the page the publish kernel wrote with `seq`, decoded into the detections
static int acq_host_tail(const AcqCall& a, unsigned long long seq, long long* d_sum, const CohGrid* g) {
    const CoarseLook* look = &a.c->h_look->coarse;
    int rc = acq_look_wait(a.c, &look->seq, seq, a.env.spin);
    if (rc != SGX_OK) return rc;
    AcqDets det;
    rc = acq_look_decode(a, look->po, look->second, 0, a.n_prn, &det);
    if (rc != SGX_OK) return rc;
    return acq_fine_and_times(a, det, d_sum, g);
}

// ================================ the three paths ================================
// The round-1 path: one launch per radix pass, every Doppler bin mixed separately (any samplesPerCode).
// Padded length: N with a prime factor above 31 has no transform here, and the search needs none - it needs the circular
// correlation of length N.  That one is computed inside a circular correlation of length L = sgx_fft_corr_length(N) >=
// 2 N - 1: the mixed rows hold the signal at [0, N) and count as zero from there (the first pass reads no further: nothing
// is filled), the code rows hold the code and its wrap-around copy (acq_code_pad_kernel), and outputs k < N of the length-L
// correlation are the reference's ifft(fft(x) conj(fft(c)))[k], the same N products each.  Everything below then runs on
// rows of L elements scaled by 1 / L, and only looks at k < N.  L = N: the path as it always was.
// g (coherent search, direct path; else null): n_blocks = the windows, each folded from g->T blocks per Doppler bin of g's
// grid (acq_fold_direct_kernel) in place of the 1-ms mix
static int acquire_passes(const AcqCall& a, int n_blocks, int noncoh, const CohGrid* g = nullptr) {
    sgx_ctx* c = a.c;
    const SgxSig x = a.x;
    const int n_prn = a.n_prn;
    const long long N = c->n_code;
    const sgx_settings& S = c->s;
    hipStream_t st = c->stream;

    // A4 frequency grid (acquisition.py:68,99-101)
    const int n_bins = g ? g->n_bins : (int)(nearbyint(S.acqSearchBand * 2) + 1);
    SGX_CHECK_ARG(n_bins >= 1 && n_bins <= (g ? ACQ_COH_MAX_BINS : ACQ_MAX_BINS));
    MixArgs ma;
    ma.n_bins = n_bins;
    ma.n_blocks = n_blocks;
    for (int k = 0; k < n_bins && !g; ++k) ma.frq[k] = S.IF - S.acqSearchBand / 2 * 1000 + 500.0 * k;
    const double ts = 1.0 / S.samplingFreq;
    const double tc = 1.0 / S.codeFreqBasis;
    const int spc = (int)llround(S.samplingFreq / S.codeFreqBasis);   // acquisition.py:145

    const long long L = sgx_fft_corr_length(N);   // rows and transforms have this length
    if (L == 0) {
        sgx_set_error("bad argument: %lld samples per code (2 .. 2^29)", N);
        return SGX_E_ARG;
    }
    const bool padded = L != N;
    int rc = sgx_fft_plan_create(&c->plan_code, L);
    if (rc != SGX_OK) return rc;

    // ---- scratch ------------------------------------------------------------------------------
    const int rows_fwd = n_blocks * n_bins;
    const int rows_per_prn = rows_fwd;
    SGX_CHECK_ARG(rows_per_prn <= ACQ_MAX_ROWS);
    const int prn_chunk = acq_passes_chunk(N, L, rows_per_prn, n_prn);
    const size_t row_bytes = sizeof(cplx) * (size_t)L;
    size_t work_rows = (size_t)prn_chunk * rows_per_prn;
    if (work_rows < (size_t)rows_fwd) work_rows = rows_fwd;
    if (work_rows < (size_t)n_prn) work_rows = n_prn;
    if ((rc = c->d_work[0].ensure(work_rows * row_bytes)) != SGX_OK) return rc;
    if ((rc = c->d_work[1].ensure(work_rows * row_bytes)) != SGX_OK) return rc;
    if ((rc = c->d_fwd.ensure((size_t)rows_fwd * row_bytes)) != SGX_OK) return rc;
    if ((rc = c->d_codefd.ensure((size_t)n_prn * row_bytes)) != SGX_OK) return rc;
    // per-workgroup maxima of the fused last pass live in the (otherwise unused) power buffer: what the plan's last pass
    // writes for the rows of one batch, whatever the length (acq_rowmax_finish_kernel strides over any number of them)
    const int nblk_last = sgx_fft_last_pass_blocks(&c->plan_code);
    const size_t part_slots = work_rows * (size_t)nblk_last;
    const size_t pow_need = noncoh ? work_rows * sizeof(double) * (size_t)N : part_slots * 12 + 4096;
    if ((rc = c->d_pow.ensure(pow_need)) != SGX_OK) return rc;

    SgxSmall* dsm = c->d_small;
    SgxSmall* hsm = c->h_small;
    double* d_pmax = c->d_pow;
    int* d_parg = (int*)(c->d_pow + part_slots);
    hipEventRecord(c->ev[0], st);
    SGX_HIP(hipMemsetAsync(&dsm->sum, 0, 8, st));
    SGX_HIP(hipMemcpyAsync(dsm->prn, a.prn0, sizeof(int) * (size_t)n_prn, hipMemcpyHostToDevice, st));
    if (x.f64) acq_sum_f64_kernel<<<1, 1024, 0, st>>>(x.f64, (long long)a.n_samples, &dsm->sum);
    else acq_sum_kernel<<<256, 256, 0, st>>>(x.i8, (long long)a.n_samples, &dsm->sum);

    // ---- PRN-independent part: mix + forward FFTs ------------------------------------------------
    {
        dim3 grid((unsigned)((N + 255) / 256), (unsigned)rows_fwd);
        if (g) {
            for (int k = 0; k < n_bins; ++k) hsm->frq[k] = g->f0 + g->step * k;
            SGX_HIP(hipMemcpyAsync(dsm->frq, hsm->frq, sizeof(double) * (size_t)n_bins, hipMemcpyHostToDevice, st));
            acq_fold_direct_kernel<<<grid, 256, 0, st>>>(x, c->d_work[0], N, L, ts, dsm->frq, n_bins, g->T);
        } else {
            acq_mix_kernel<<<grid, 256, 0, st>>>(x, c->d_work[0], N, L, ts, ma);
        }
        cplx* res = nullptr;
        rc = sgx_fft_forward(&c->plan_code, c->d_work[0], c->d_work[1], rows_fwd, st, &res, N);
        if (rc != SGX_OK) return rc;
        SGX_HIP(hipMemcpyAsync(c->d_fwd, res, (size_t)rows_fwd * row_bytes, hipMemcpyDeviceToDevice, st));
    }
    // ---- code spectra ---------------------------------------------------------------------------
    {
        dim3 grid((unsigned)((L + 255) / 256), (unsigned)n_prn);
        if (padded) acq_code_pad_kernel<<<grid, 256, 0, st>>>(c->d_codes, dsm->prn, c->d_work[0], N, L, ts, tc);
        else acq_code_kernel<<<grid, 256, 0, st>>>(c->d_codes, dsm->prn, c->d_work[0], N, ts, tc);
        cplx* res = nullptr;
        rc = sgx_fft_forward(&c->plan_code, c->d_work[0], c->d_work[1], n_prn, st, &res, L);
        if (rc != SGX_OK) return rc;
        SGX_HIP(hipMemcpyAsync(c->d_codefd, res, (size_t)n_prn * row_bytes, hipMemcpyDeviceToDevice, st));
    }

    // ---- correlation + peak search, PRN chunk by chunk ---------------------------------------------
    AcqDets det;
    int status = SGX_OK;
    acq_reset_outputs(a.out, a.n_prn);
    const double inv_n = 1.0 / (double)L;
    const int out_per_prn = noncoh ? n_bins : rows_per_prn;
    for (int p0 = 0; p0 < n_prn && status == SGX_OK; p0 += prn_chunk) {
        const int np = (p0 + prn_chunk <= n_prn) ? prn_chunk : (n_prn - p0);
        const int rows = np * rows_per_prn;
        const int rows_out = np * out_per_prn;
        cplx* res = nullptr;
        if (noncoh) {
            // extension path: the blocks' powers are summed per sample, so rows are materialised
            dim3 grid((unsigned)((L + 255) / 256), (unsigned)rows);
            acq_mul_kernel<<<grid, 256, 0, st>>>(c->d_fwd, c->d_codefd, c->d_work[0], L, rows_per_prn, p0);
            rc = sgx_fft_forward(&c->plan_code, c->d_work[0], c->d_work[1], rows, st, &res, L);
            if (rc != SGX_OK) return rc;
            acq_power_kernel<<<rows_out, 256, 0, st>>>(res, c->d_pow, dsm->rowmax, dsm->rowarg, N, L, inv_n, n_bins, n_blocks, 1);
        } else {
            // reference path, fused: conj(X)*F formed in the first radix pass, |.|^2 and the per-workgroup
            // maxima taken in the last one; no product rows, no power rows
            FftFuse fu;
            fu.mul_x = c->d_fwd;
            fu.mul_f = c->d_codefd;
            fu.rows_per_prn = rows_per_prn;
            fu.prn_base = p0;
            fu.pmax = d_pmax;
            fu.parg = d_parg;
            fu.inv_n = inv_n;
            fu.n_valid = padded ? N : 0;
            rc = sgx_fft_forward_fused(&c->plan_code, c->d_work[0], c->d_work[1], rows, st, &res, L, &fu);
            if (rc != SGX_OK) return rc;
            acq_rowmax_finish_kernel<<<rows, 64, 0, st>>>(d_pmax, d_parg, nblk_last, dsm->rowmax, dsm->rowarg);
        }
        SGX_HIP(hipMemcpyAsync(hsm->rowmax, dsm->rowmax, sizeof(double) * (size_t)rows_out, hipMemcpyDeviceToHost, st));
        SGX_HIP(hipMemcpyAsync(hsm->rowarg, dsm->rowarg, sizeof(int) * (size_t)rows_out, hipMemcpyDeviceToHost, st));
        SGX_HIP(hipStreamSynchronize(st));

        // host: block choice (A7), global peak (A8), exclusion list (A8b) - the device's peak logic, bin by bin
        SecondArgs sa;
        PeakOut po;
        for (int pi = 0; pi < 32; ++pi) sa.row[pi] = -1, sa.lo0[pi] = sa.hi0[pi] = sa.lo1[pi] = sa.hi1[pi] = 0;
        memset(&po, 0, sizeof(po));
        for (int pi = 0; pi < np; ++pi) {
            AcqCand cand = {-1.0, -1, 0, 0};
            for (int k = 0; k < n_bins; ++k)
                cand = acq_peak_join(cand, acq_peak_bin(hsm->rowmax + pi * out_per_prn, hsm->rowarg + pi * out_per_prn, n_bins,
                                                        n_blocks, noncoh != 0, k));
            po.peak[pi] = cand.v;
            po.cph[pi] = cand.a;
            po.fbi[pi] = cand.k;
            po.index_error[pi] = acq_peak_ranges(cand.a, N, spc, &sa.lo0[pi], &sa.hi0[pi], &sa.lo1[pi], &sa.hi1[pi]);
            if (po.index_error[pi]) break;
            sa.row[pi] = pi * out_per_prn + (noncoh ? cand.k : cand.b * n_bins + cand.k);
        }
        status = acq_look_index_error(a, po, p0, np);
        if (status != SGX_OK) break;
        if (noncoh) {
            SGX_HIP(hipMemcpyAsync(&dsm->second_args, &sa, sizeof(sa), hipMemcpyHostToDevice, st));
            SGX_HIP(hipMemsetAsync(dsm->second, 0, sizeof(double) * 32, st));
            acq_second_kernel<<<dim3((unsigned)np, SEC_SPLIT), 256, 0, st>>>(c->d_pow, dsm->second, N, &dsm->second_args);
        } else {
            // recompute only the np rows the second-peak search reads (one per PRN)
            for (int pi = 0; pi < np; ++pi) {
                hsm->row_map[pi] = make_int2(sa.row[pi] % rows_per_prn, p0 + pi);   // row = (pi*blocks + b)*bins + k
                sa.row[pi] = pi;
            }
            SGX_HIP(hipMemcpyAsync(dsm->row_map, hsm->row_map, sizeof(int2) * (size_t)np, hipMemcpyHostToDevice, st));
            FftFuse fu;
            fu.mul_x = c->d_fwd;
            fu.mul_f = c->d_codefd;
            fu.row_map = dsm->row_map;
            cplx* r2 = nullptr;
            rc = sgx_fft_forward_fused(&c->plan_code, c->d_work[0], c->d_work[1], np, st, &r2, L, &fu);
            if (rc != SGX_OK) return rc;
            SGX_HIP(hipMemcpyAsync(&dsm->second_args, &sa, sizeof(sa), hipMemcpyHostToDevice, st));
            SGX_HIP(hipMemsetAsync(dsm->second, 0, sizeof(double) * 32, st));
            acq_second_cplx_kernel<<<dim3((unsigned)np, SEC_SPLIT), 256, 0, st>>>(r2, dsm->second, L, inv_n, &dsm->second_args);
        }
        SGX_HIP(hipMemcpyAsync(hsm->second, dsm->second, sizeof(double) * (size_t)np, hipMemcpyDeviceToHost, st));
        SGX_HIP(hipStreamSynchronize(st));
        status = acq_look_decode(a, po, hsm->second, p0, np, &det);
    }
    hipEventRecord(c->ev[1], st);
    if (status != SGX_OK) {
        hipStreamSynchronize(st);
        return status;
    }
    // ---- fine frequency search (acquisition.py:167-193) -----------------------------------------------
    return acq_fine_and_times(a, det, &dsm->sum, g);
}

// The acquisition on the four-step transform (sgx_fft.hip): every 38192-point transform is two kernels with register-resident
// sub-transforms, the mixed-signal spectra are computed once per (block, phi) and read with a circular shift, results
// land where they are needed (no device-to-device copies) and the host looks at the device ONCE, at the very end of the
// call (round 4: peaks, second peaks, the detections and their fine-search results arrive in one pinned page), whatever the
// number of PRN chunks.
static int acquire_four_step(const AcqCall& a, int n_blocks, int noncoh, bool* handled, bool defer = false) {
    *handled = false;
    sgx_ctx* c = a.c;
    const SgxSig x = a.x;
    const int n_prn = a.n_prn;
    const size_t n_samples = a.n_samples;
    const long long N = c->n_code;
    const sgx_settings& S = c->s;
    if (a.env.v1 || !sgx_fft4_supported(N)) return SGX_OK;
    const int n_bins = (int)(nearbyint(S.acqSearchBand * 2) + 1);
    if (n_bins < 1 || n_bins > ACQ_MAX_BINS) return SGX_OK;
    // f N / fs = shift + phi for every bin of the A4 grid (acquisition.py:68,99-101); the path needs few distinct phi
    // (more than PhiArgs holds: the direct path mixes every bin)
    std::vector<double> phi;
    std::vector<int2> bin_map;
    const int n_phi = acq_phi_split(S.IF - S.acqSearchBand / 2 * 1000, 500.0, n_bins, N, S.samplingFreq, &phi, &bin_map);
    if (n_phi > 4 || (n_phi >= n_bins && n_bins > 1)) return SGX_OK;
    *handled = true;
    PhiArgs pa;
    pa.n_phi = n_phi;
    for (int j = 0; j < n_phi; ++j) pa.phi[j] = phi[(size_t)j];

    hipStream_t st = c->stream;
    const double ts = 1.0 / S.samplingFreq;
    const double tc = 1.0 / S.codeFreqBasis;
    const int spc = (int)llround(S.samplingFreq / S.codeFreqBasis);   // acquisition.py:145
    int rc = sgx_fft_plan_create(&c->plan_code, N);
    if (rc != SGX_OK) return rc;

    // ---- scratch ------------------------------------------------------------------------------
    const int rows_fwd = n_blocks * n_phi;
    const int rows_per_prn = n_blocks * n_bins;
    SGX_CHECK_ARG(rows_per_prn <= ACQ_MAX_ROWS);
    // PRN chunks of ~350 rows: a chunk's intermediate (213 MB) then stays in the 256 MiB Infinity Cache between the
    // columns kernel that writes it and the rows kernel that reads it, and the next chunk overwrites it there.  With the
    // round-3 kernels - bound by their stores and by the dirty lines on their way out, not by instruction issue or LDS
    // any more - that is 0.94 -> 0.80 ms for config 2 and 3.43 -> 3.24 ms for config 4 (tools/acq_chunk_probe.py; the
    // round-2 kernels measured no difference).
    const AcqPlan plan = acq_plan(n_prn, n_bins, n_blocks, noncoh != 0, a.env.chunk_rows, a.env.one_queue ? 1 : 2);
    const bool two_q = plan.queues == 2;
    const int bin_runs = plan.bin_runs, prn_chunk = plan.prn_chunk;
    size_t work_rows = (size_t)prn_chunk * rows_per_prn;
    if (work_rows < (size_t)n_prn * (noncoh ? n_blocks : 1)) work_rows = (size_t)n_prn * (noncoh ? n_blocks : 1);
    // Round 5: peak and second peak from ONE pass (acq_rowtop2_peak_kernel) when the exclusion list leaves out fewer than
    // `nres` consecutive indices (2 spc of them at most: any sampling rate below 111 MHz); SGX_ACQ_TOP2=0: the round-4
    // sequence, which transforms each PRN's winning row a second time
    const bool top2 = 2 * spc + 1 <= sgx_fft4_residues() && !a.env.top2_off;
    AcqCorr k;
    if ((rc = acq_corr_setup(c, &k, n_prn, n_bins, n_phi, n_blocks, noncoh, top2, work_rows, true)) != SGX_OK) return rc;

    SgxSmall* dsm = c->d_small;
    long long* d_sum = &dsm->sum;

    hipEventRecord(c->ev[0], st);
    {
        // ---- set-up, record sum, mixed rows (n_blocks x n_phi, PRN independent) and code rows (n_prn): one launch for
        //      int8 records; then the forward spectra of all of them as ONE batch, straight into d_fwd = [forward | code]
        AcqSetup su;
        memset(&su, 0, sizeof(su));
        su.n_prn = n_prn;
        su.n_bins = n_bins;
        for (int i = 0; i < n_prn; ++i) su.prn[i] = a.prn0[i];
        for (int b = 0; b < n_bins; ++b) su.bin[b] = bin_map[(size_t)b];
        static_assert(ACQ_MAX_BINS <= 256, "the set-up workgroup has 256 threads");
        if (!x.f64 && !a.env.front_off) {
            const int ph = c->acq_sum_phase & 1;
            long long* sum_now = dsm->sum2 + ph;
            long long* sum_next = dsm->sum2 + (ph ^ 1);
            if (!c->acq_sum_clean[ph]) SGX_HIP(hipMemsetAsync(sum_now, 0, 8, st));
            const unsigned gx = (unsigned)((N + 255) / 256);
            acq_front_kernel<<<(unsigned)(rows_fwd + n_prn) * gx + ACQ_SUM_WGS + 1, 256, 0, st>>>(
                su, x, pa, c->d_codes, c->d_work[1], N, rows_fwd, ts, tc, (long long)n_samples, dsm->prn, dsm->bin_map, sum_now,
                sum_next, dsm->second, dsm->arrived);
            c->acq_sum_clean[ph] = false;
            c->acq_sum_clean[ph ^ 1] = true;
            c->acq_sum_phase = ph ^ 1;
            d_sum = sum_now;
        } else {
            acq_setup_kernel<<<1, 128, 0, st>>>(su, dsm->prn, dsm->bin_map, d_sum, dsm->second, dsm->arrived);
            if (x.f64) acq_sum_f64_kernel<<<1, 1024, 0, st>>>(x.f64, (long long)n_samples, d_sum);
            else acq_sum_kernel<<<64, 256, 0, st>>>(x.i8, (long long)n_samples, d_sum);
            dim3 grid((unsigned)((N + 255) / 256), (unsigned)rows_fwd);
            acq_mixphi_kernel<<<grid, 256, 0, st>>>(x, c->d_work[1], N, pa);
            dim3 grid2((unsigned)((N + 255) / 256), (unsigned)n_prn);
            acq_code_kernel<<<grid2, 256, 0, st>>>(c->d_codes, dsm->prn, c->d_work[1] + (size_t)rows_fwd * (size_t)N, N, ts, tc);
        }
        rc = sgx_fft4_forward(&c->plan_code, c->d_work[1], c->d_work[0], c->d_fwd, rows_fwd + n_prn, st, nullptr);
        if (rc != SGX_OK) return rc;
    }
    acq_reset_outputs(a.out, a.n_prn);
    // ---- correlation, all PRN chunks queued back to back; row maxima of every PRN collected on the device -----------
    hipStream_t st2 = st;
    if (two_q) {
        if ((rc = acq_second_queue(c, &st2)) != SGX_OK) return rc;
        // (the second queue's intermediate is the buffer the forward transforms read: they are queued in front)
        SGX_HIP(hipEventRecord(c->acq_ev2[0], st));
        SGX_HIP(hipStreamWaitEvent(st2, c->acq_ev2[0], 0));
    }
    int chunk_no = 0;
    const int bins_per_run = plan.bins_per_run;
    for (int p0 = 0; p0 < n_prn; p0 += prn_chunk)
        for (int bin0 = 0; bin0 < n_bins; bin0 += bins_per_run, ++chunk_no) {
            const int np = (p0 + prn_chunk <= n_prn) ? prn_chunk : (n_prn - p0);
            const int nb = bin_runs == 1 ? n_bins : (bin0 + bins_per_run <= n_bins ? bins_per_run : n_bins - bin0);
            const int q = two_q ? (chunk_no & 1) : 0;
            rc = acq_corr_batch(c, k, p0, np, bin0, nb, 0, n_blocks, c->d_work[q], q ? st2 : st);
            if (rc != SGX_OK) {
                // (the second queue may still hold chunks that write d_work[1]: nothing of the next call may overtake them)
                if (two_q) hipStreamSynchronize(st2);
                return rc;
            }
        }
    if (two_q) {
        SGX_HIP(hipEventRecord(c->acq_ev2[1], st2));
        SGX_HIP(hipStreamWaitEvent(st, c->acq_ev2[1], 0));
    }
    // ---- the fine search is queued right behind the coarse one: the detections are decided on the device
    //      (acquisition.py:164-166) and the fine kernels read their list, so the host looks ONCE, at the very end ----------
    const unsigned long long seq = ++c->look_seq;
    const FineGeom fg = acq_fine_geom(N);
    const bool device_led = sgx_fft_fine_supported(fg.npts) && !a.env.fine_v1 && !a.env.device_led_off && n_prn <= 32;
    if (device_led) {
        // (before the last coarse kernels are queued: nothing of the host's between them and the fine kernels)
        rc = sgx_fft_plan_create(&c->plan_fine, fg.npts);
        if (rc != SGX_OK) return rc;
        const int max_rows = (n_prn + 1) / 2;   // two real signals per complex row; only the detections' rows are touched
        if ((rc = c->d_fine[0].ensure((size_t)max_rows * sizeof(cplx) * (size_t)fg.npts)) != SGX_OK) return rc;
    }
    // (device-led: into a device-side copy of the page - a kernel that writes host memory ends with a flush the next one
    // waits for, 5 us in front of the fine search)
    CoarseLook* const d_stage = &dsm->stage;
    CoarseLook* const d_look = &c->d_look->coarse;
    // ---- device: row maxima, then per PRN block choice, global peak, exclusion list, second peak -----------------------
    if (k.top2) {
        PublishArgs pub;
        pub.stage = device_led ? d_stage : nullptr;
        pub.prn_list = dsm->prn;
        pub.threshold = S.acqThreshold;
        pub.fine_len = fg.len;
        pub.n_samples = (long long)n_samples;
        pub.det = &dsm->det;
        acq_queue_top2(a, k, spc, pub);
    } else {
        acq_rowmax_peak_kernel<<<k.rows_out_all, 64, 0, st>>>(k.pmax, k.parg, k.nblk, k.rowmax, k.rowarg, dsm->arrived, n_prn,
                                                              k.out_per_prn, n_bins, n_blocks, noncoh, N, spc, &dsm->peak_out,
                                                              &dsm->second_args, dsm->row_map);
        // the rows the second-peak search reads, transformed again
        const int rows2 = n_prn * (noncoh ? n_blocks : 1);
        Fft4Fuse fu;
        fu.mul_x = c->d_fwd;
        fu.mul_f = k.d_codefd;
        fu.bin_map = dsm->bin_map;
        fu.row_map = dsm->row_map;
        fu.n_bins = n_bins;
        fu.n_phi = n_phi;
        fu.n_blocks = n_blocks;
        // the rows kernel folds each row's maximum over the exclusion list into d_second itself (the same powers, formed
        // by the same arithmetic, as the first pass: peak / second peak is a ratio of consistently rounded values);
        // neither the rows nor their powers are stored
        static_assert(sizeof(SecondArgs) == 5 * 32 * sizeof(int), "row / lo0 / hi0 / lo1 / hi1, 32 each");
        fu.sec = reinterpret_cast<const int*>(&dsm->second_args);
        fu.second_out = dsm->second;
        fu.inv_n = 1.0 / (double)N;
        fu.sum_blocks = noncoh ? n_blocks : 1;
        rc = sgx_fft4_forward(&c->plan_code, nullptr, c->d_work[0], nullptr, rows2, st, &fu);
        if (rc != SGX_OK) return rc;
    }
    if (!k.top2 || !device_led) acq_queue_publish(a, device_led ? d_stage : d_look, seq, fg.len, device_led ? &dsm->det : nullptr);
    // (an event between the coarse and the fine kernels holds the fine search back by 6-8 us: recorded on request only)
    if (a.env.split_event || !device_led) hipEventRecord(c->ev[1], st);
    SGX_HIP(hipGetLastError());
    if (device_led) {
        FineSearch f;
        f.x = x;
        f.codes = c->d_codes;
        f.len = fg.len;
        f.d_sum = d_sum;
        f.n_mean = (double)n_samples;
        f.ts = ts;
        f.tc1 = 1.0 / S.codeFreqBasis;
        f.work = c->d_fine[0];
        f.n_det = n_prn;
        f.lo = 4;
        f.hi = fg.uniq - 5;
        f.d_det = &dsm->det;
        f.stage_src = reinterpret_cast<const int*>(d_stage);
        f.stage_dst = reinterpret_cast<int*>(d_look);
        f.stage_words = (int)(offsetof(CoarseLook, fine_bi) / sizeof(int));
        f.out_bi = d_look->fine_bi;
        f.out_seq = &d_look->seq2;
        f.seq = seq;
        f.pv = dsm->fine_pv;
        f.pi = dsm->fine_pi;
        rc = sgx_fft_fine_search(&c->plan_fine, f, st);
        if (rc != SGX_OK) return rc;
        hipEventRecord(c->ev[2], st);
        SGX_HIP(hipGetLastError());
        // everything is queued; what the look needs to be decoded later (sgx_acquire_finish)
        AcqPending& P = c->acq_pending;
        P.mode = 1;
        P.seq = seq;
        P.n_prn = n_prn;
        for (int i = 0; i < n_prn; ++i) P.prn0[i] = a.prn0[i];
        P.npts = fg.npts;
        P.fine_len = fg.len;
        P.n_samples = n_samples;
        P.split_event = a.env.split_event;
        P.spin = a.env.spin;
        if (defer) return SGX_OK;
        return sgx_acquire_finish(c, a.out);
    }
    return acq_host_tail(a, seq, d_sum, nullptr);
}

// The host's ONE look at a device-led acquisition (queued by acquire_four_step; c->acq_pending says what was asked): waits
// for the result page's second word, then decodes peaks, detections and fine frequencies exactly as the eager call did.
int sgx_acquire_finish(sgx_ctx* c, const AcqOut& out) {
    AcqPending& P = c->acq_pending;
    if (P.mode == 2) {   // (the search could not be deferred and ran eagerly: its outputs were kept)
        P.mode = 0;
        acq_copy_results(out, P.res.out(), P.n_prn);
        return P.rc;
    }
    if (P.mode != 1) {
        sgx_set_error("sgx_acquire_end: no acquisition is pending on this context");
        return SGX_E_ARG;
    }
    P.mode = 0;
    const sgx_settings& S = c->s;
    AcqEnv env{};   // (only what the queued call left for its look: the environment is not read again)
    env.split_event = P.split_event;
    env.spin = P.spin;
    const AcqCall a = acq_call(c, SgxSig{nullptr, nullptr}, P.n_samples, P.prn0, P.n_prn, out, env);
    acq_reset_outputs(a.out, a.n_prn);
    const CoarseLook* look = &c->h_look->coarse;
    int rc = acq_look_wait(c, &look->seq2, P.seq, P.spin);
    if (rc != SGX_OK) return rc;
    AcqDets det;
    rc = acq_look_decode(a, look->po, look->second, 0, a.n_prn, &det);
    if (rc != SGX_OK) return rc;
    if (look->range_error) return acq_fine_range_error((long long)look->po.cph[look->range_error - 1] + P.fine_len, P.n_samples);
    if (look->n_det != (int)det.slot.size()) {   // (the same comparison on the same doubles: cannot differ)
        sgx_set_error("acquisition: device found %d detections, host %d", look->n_det, (int)det.slot.size());
        return SGX_E_HIP;
    }
    for (int d = 0; d < look->n_det; ++d) {
        const long long m = look->fine_bi[d] - 4;   // index inside the [4:uniq-5] slice (acquisition.py:187)
        const int o = look->det_slot[d];
        out.carrFreq[o] = ((double)m * S.samplingFreq) / (double)P.npts;   // acquisition.py:189-191 (Q3)
        out.codePhase[o] = (double)look->det_phase[d];
        out.fineIdx[o] = (int)m;
    }
    // (the result word is stored a moment before the last kernel retires: the device times below need its event)
    SGX_HIP(hipEventSynchronize(c->ev[2]));
    acq_event_times(c, P.split_event);
    return SGX_OK;
}

// The shift path of the coherent search: folded rows per (window, phi), their forward spectra once, the correlation
// batches of acquire_four_step (Fft4Fuse reads each bin's row with its circular shift), the same peak kernels, then one
// host look and the fine search.  All on one queue.
static int acquire_coherent_shift(const AcqCall& a, const CohGrid& g) {
    sgx_ctx* c = a.c;
    const SgxSig x = a.x;
    const int n_prn = a.n_prn;
    const long long N = c->n_code;
    const sgx_settings& S = c->s;
    hipStream_t st = c->stream;
    const double ts = 1.0 / S.samplingFreq;
    const double tc = 1.0 / S.codeFreqBasis;
    const int spc = (int)llround(S.samplingFreq / S.codeFreqBasis);   // acquisition.py:145
    const int n_bins = g.n_bins, n_phi = g.n_phi, M = g.M, noncoh = g.noncoh;
    int rc = sgx_fft_plan_create(&c->plan_code, N);
    if (rc != SGX_OK) return rc;

    // ---- scratch ------------------------------------------------------------------------------
    const int rows_fwd = M * n_phi;
    const int rows_per_prn = M * n_bins;
    const int run_rows = g.runs == 1 ? g.prn_chunk * rows_per_prn : g.per_run * (noncoh ? M : n_bins);
    // peak and second peak from one pass (acq_rowtop2_peak_kernel): the four-step length has 217 residues, so any exclusion
    // list (2 spc + 1 = 75 indices at that length's rate) fits
    if (2 * spc + 1 > sgx_fft4_residues()) {
        sgx_set_error("coherent acquisition: %d samples per chip exceed the one-pass second-peak search", spc);
        return SGX_E_ARG;
    }
    AcqCorr k;
    if ((rc = acq_corr_setup(c, &k, n_prn, n_bins, n_phi, M, noncoh, true, (size_t)run_rows, false)) != SGX_OK) return rc;

    SgxSmall* dsm = c->d_small;
    SgxSmall* hsm = c->h_small;
    // (host staging in the pinned small buffer: the copies are queued, the buffer is not touched again before the look)
    for (int i = 0; i < n_prn; ++i) hsm->stage_prn[i] = a.prn0[i];
    for (int b = 0; b < n_bins; ++b) hsm->stage_bin_map[b] = g.bin_map[(size_t)b];

    hipEventRecord(c->ev[0], st);
    {
        SGX_HIP(hipMemcpyAsync(dsm->prn, hsm->stage_prn, sizeof(int) * (size_t)n_prn, hipMemcpyHostToDevice, st));
        SGX_HIP(hipMemcpyAsync(dsm->bin_map, hsm->stage_bin_map, sizeof(int2) * (size_t)n_bins, hipMemcpyHostToDevice, st));
        SGX_HIP(hipMemsetAsync(&dsm->sum, 0, 8, st));
        SGX_HIP(hipMemsetAsync(dsm->second, 0, sizeof(double) * 32, st));
        SGX_HIP(hipMemsetAsync(dsm->arrived, 0, sizeof(int) * 64, st));
        if (x.f64) acq_sum_f64_kernel<<<1, 1024, 0, st>>>(x.f64, (long long)a.n_samples, &dsm->sum);
        else acq_sum_kernel<<<64, 256, 0, st>>>(x.i8, (long long)a.n_samples, &dsm->sum);
        FoldArgs fa;
        memset(&fa, 0, sizeof(fa));
        fa.n_phi = n_phi;
        fa.T = g.T;
        for (int j = 0; j < n_phi; ++j) fa.phi[j] = g.phi[(size_t)j];
        const unsigned gx = (unsigned)((N + 255) / 256);
        acq_fold_phi_kernel<<<dim3(gx, (unsigned)M), 256, 0, st>>>(x, c->d_work[1], N, fa);
        acq_code_kernel<<<dim3(gx, (unsigned)n_prn), 256, 0, st>>>(c->d_codes, dsm->prn, c->d_work[1] + (size_t)rows_fwd * (size_t)N,
                                                                   N, ts, tc);
        rc = sgx_fft4_forward(&c->plan_code, c->d_work[1], c->d_work[0], c->d_fwd, rows_fwd + n_prn, st, nullptr);
        if (rc != SGX_OK) return rc;
    }
    acq_reset_outputs(a.out, a.n_prn);
    // ---- correlation: batches of whole PRNs, or one PRN in runs of bins (noncoh) / windows (reference rule) ----------
    const int total = noncoh ? n_bins : M;
    for (int p0 = 0; p0 < n_prn; p0 += g.prn_chunk)
        for (int r0 = 0; r0 < total; r0 += (g.runs == 1 ? total : g.per_run)) {
            const int np = (p0 + g.prn_chunk <= n_prn) ? g.prn_chunk : (n_prn - p0);
            const int nr = g.runs == 1 ? total : (r0 + g.per_run <= total ? g.per_run : total - r0);
            rc = noncoh ? acq_corr_batch(c, k, p0, np, r0, nr, 0, M, c->d_work[0], st)
                        : acq_corr_batch(c, k, p0, np, 0, n_bins, r0, nr, c->d_work[0], st);
            if (rc != SGX_OK) return rc;
        }
    // ---- row maxima, block (window) choice, global peak, exclusion list, second peak: acquire_four_step's kernels -------
    const unsigned long long seq = ++c->look_seq;
    PublishArgs pub;
    memset(&pub, 0, sizeof(pub));   // (no stage: the publish kernel below writes the page)
    acq_queue_top2(a, k, spc, pub);
    acq_queue_publish(a, &c->d_look->coarse, seq, acq_fine_geom(N).len, nullptr);
    hipEventRecord(c->ev[1], st);
    SGX_HIP(hipGetLastError());
    return acq_host_tail(a, seq, &dsm->sum, &g);
}

// ================================ entry points ================================
static int acquire_any(const AcqCall& a, int n_blocks, int noncoh) {
    // the four-step path (sub-transforms in registers and LDS, shifted forward spectra) where it applies
    bool handled = false;
    const int rc4 = acquire_four_step(a, n_blocks, noncoh, &handled);
    if (handled) return rc4;
    return acquire_passes(a, n_blocks, noncoh);
}

// ONE search may be pending per context, and c->acq_pending belongs to the search that ran last: every search's kernels
// write the result page and d_small->stage, so every entry point drops what an earlier sgx_acquire_begin left before it
// touches the device.  sgx_track_chained then answers SGX_E_DEFER and sgx_acquire_end SGX_E_ARG, as for "nothing pending".
static void acq_drop_pending(sgx_ctx* c) { c->acq_pending.mode = 0; }

static int acquire_source(sgx_ctx* c, const AcqSource& src, const int32_t* prn0, int32_t n_prn, int32_t n_blocks, int32_t noncoh,
                          const AcqOut& out, const AcqEnv& env) {
    SGX_CHECK_ARG(c);
    acq_drop_pending(c);
    SGX_CHECK_ARG(acq_out_non_null(out));
    SgxSig x;
    const int rc = acq_open_source(c, src, prn0, n_prn, n_blocks, &x);
    if (rc != SGX_OK) return rc;
    return acquire_any(acq_call(c, x, src.n_samples, prn0, n_prn, out, env), n_blocks, noncoh);
}
extern "C" int sgx_acquire(sgx_ctx* c, const sgx_if* r, size_t offset, size_t n_samples, const int32_t* prn0,
                           int32_t n_prn, int32_t n_blocks, int32_t noncoh, double* carrFreq, double* codePhase,
                           double* peakMetric, int32_t* freqBin, int32_t* fineIdx) {
    const AcqOut out{carrFreq, codePhase, peakMetric, freqBin, fineIdx};
    return acquire_source(c, AcqSource{r, offset, nullptr, n_samples}, prn0, n_prn, n_blocks, noncoh, out, acq_env());
}
extern "C" int sgx_acquire_f64(sgx_ctx* c, const double* signal, size_t n_samples, const int32_t* prn0, int32_t n_prn,
                               int32_t n_blocks, int32_t noncoh, double* carrFreq, double* codePhase, double* peakMetric,
                               int32_t* freqBin, int32_t* fineIdx) {
    const AcqOut out{carrFreq, codePhase, peakMetric, freqBin, fineIdx};
    return acquire_source(c, AcqSource{nullptr, 0, signal, n_samples}, prn0, n_prn, n_blocks, noncoh, out, acq_env());
}

int sgx_prerun_enqueue(sgx_ctx* c, TrkChan* d_ch, int n_ch, long long skip_bytes, long long rec_file_offset, int sample_bytes) {
    const AcqPending& P = c->acq_pending;
    if (P.mode != 1 || n_ch < 1 || n_ch > 32) return SGX_E_DEFER;
    acq_prerun_kernel<<<1, 64, 0, c->stream>>>(&c->d_small->stage, c->d_look->coarse.fine_bi, c->d_small->prn, P.n_prn,
                                               c->s.samplingFreq, (double)P.npts, d_ch, n_ch, skip_bytes, rec_file_offset,
                                               sample_bytes, &c->d_look->step);
    SGX_HIP(hipGetLastError());
    return SGX_OK;
}

// ---- deferred acquisition (round 6) ----
// The reference's caller (initialize.py:484-506) runs acquire -> preRun -> track and looks at each result in between.  A
// caller that only wants the tracking results can queue all three: sgx_acquire_begin queues the search and returns,
// sgx_track_chained (sgx_trk.hip) queues preRun - acq_prerun_kernel - and the tracking kernel behind it and waits ONCE;
// sgx_acquire_end then decodes the search's page (no waiting left).  Outputs are those of the eager calls, bit for bit:
// the same kernels in the same order, and acq_prerun_kernel repeats the host's arithmetic.
static int acquire_begin(sgx_ctx* c, const sgx_if* r, size_t offset, size_t n_samples, const int32_t* prn0, int32_t n_prn,
                         int32_t n_blocks, int32_t noncoh, const AcqEnv& env) {
    SGX_CHECK_ARG(c);
    acq_drop_pending(c);
    SgxSig x;
    int rc = acq_open_source(c, AcqSource{r, offset, nullptr, n_samples}, prn0, n_prn, n_blocks, &x);
    if (rc != SGX_OK) return rc;
    AcqPending& P = c->acq_pending;
    const AcqCall a = acq_call(c, x, n_samples, prn0, n_prn, P.res.out(), env);
    bool handled = false;
    rc = acquire_four_step(a, n_blocks, noncoh, &handled, true);
    if (handled && P.mode == 1) return rc;          // queued; nothing has been looked at
    if (!handled) rc = acquire_passes(a, n_blocks, noncoh);
    // (a path without the device-led sequence: it ran eagerly; sgx_acquire_end hands its outputs over)
    P.mode = 2;
    P.n_prn = n_prn;
    P.rc = rc;
    return SGX_OK;
}
extern "C" int sgx_acquire_begin(sgx_ctx* c, const sgx_if* r, size_t offset, size_t n_samples, const int32_t* prn0,
                                 int32_t n_prn, int32_t n_blocks, int32_t noncoh) {
    return acquire_begin(c, r, offset, n_samples, prn0, n_prn, n_blocks, noncoh, acq_env());
}

extern "C" int sgx_acquire_end(sgx_ctx* c, double* carrFreq, double* codePhase, double* peakMetric, int32_t* freqBin,
                               int32_t* fineIdx) {
    const AcqOut out{carrFreq, codePhase, peakMetric, freqBin, fineIdx};
    SGX_CHECK_ARG(c && acq_out_non_null(out));
    SGX_HIP(hipSetDevice(c->device));
    return sgx_acquire_finish(c, out);
}

// ================================ round 6: the sharded search as ONE call ================================
// BASELINE configs[3]: the PRN loop (acquisition.py:92) shards over the ranks, the peaks are gathered.  Rounds 1-5 did the
// pack, the gather and the merge in Python around sgx_acquire (softgnss-python_amd/shard.py): 0.17-0.28 ms of host time per
// call next to a 0.45 ms shard.  Here the rank's search is queued, its peaks are packed into 40-byte records ON THE DEVICE
// behind it, one ncclAllGather follows on the same stream, a small kernel copies the gathered records to the result page and
// the host looks ONCE; the merge into the 32-entry arrays is a loop over at most 32 records.
extern "C" int sgx_acquire_sharded(sgx_ctx* c, sgx_comm* comm, int32_t rank, int32_t world, const sgx_if* r, size_t offset,
                                   size_t n_samples, int32_t n_prn_total, int32_t n_blocks, int32_t noncoh, double* carrFreq,
                                   double* codePhase, double* peakMetric, int32_t* freqBin, int32_t* fineIdx) {
    const AcqOut out{carrFreq, codePhase, peakMetric, freqBin, fineIdx};
    SGX_CHECK_ARG(c);
    // (the rank's search is queued by acquire_begin and looked at in here: nothing is pending after ANY return)
    struct DropPending {
        sgx_ctx* c;
        ~DropPending() { acq_drop_pending(c); }
    } drop{c};
    SGX_CHECK_ARG(r && acq_out_non_null(out));
    SGX_CHECK_ARG(world >= 1 && rank >= 0 && rank < world && n_prn_total >= 1 && n_prn_total <= 32);
    SGX_CHECK_ARG(!comm || (comm->n_ranks == world && comm->rank == rank && comm->ctx == c));
    const AcqEnv env = acq_env();
    acq_reset_outputs(out, 32);
    // contiguous balanced partition (shard.plan_shards)
    const int base = n_prn_total / world, extra = n_prn_total % world;
    const int first = rank * base + (rank < extra ? rank : extra);
    const int n_mine = base + (rank < extra ? 1 : 0);
    const int slots = (n_prn_total + world - 1) / world;
    int32_t prn0[32];
    for (int i = 0; i < n_mine; ++i) prn0[i] = first + i;
    SGX_HIP(hipSetDevice(c->device));
    const size_t rec_bytes = sizeof(PeakRec) * (size_t)slots;
    // where the packed records go: the communicator's send buffer, or (no communicator: one rank, or a shard run alone)
    // the context's small device area
    SgxSmall* dsm = c->d_small;
    PeakRec* d_send = comm ? (PeakRec*)comm->d_send.get() : dsm->shard;
    const PeakRec* d_all = comm ? (const PeakRec*)comm->d_recv.get() : d_send;
    const int n_ranks_seen = comm ? world : 1;
    std::vector<PeakRec> host_pack;      // a search that could not be queued: packed on the host
    bool queued = false;
    if (n_mine > 0) {
        const int rb = acquire_begin(c, r, offset, n_samples, prn0, n_mine, n_blocks, noncoh, env);
        if (rb != SGX_OK) return rb;
        queued = c->acq_pending.mode == 1;
        if (!queued) {
            AcqResults mine;
            const int re = sgx_acquire_finish(c, mine.out());
            if (re != SGX_OK && re != SGX_E_INDEX && re != SGX_E_RANGE) return re;
            host_pack.resize((size_t)slots);
            memset(host_pack.data(), 0, rec_bytes);
            for (int i = 0; i < n_mine; ++i) host_pack[(size_t)i] = peak_rec_pack(prn0[i], mine.out(), i);
            if (re != SGX_OK) host_pack[0].valid = re == SGX_E_INDEX ? -1 : -2;   // (every rank learns of it)
        }
    }
    hipStream_t st = c->stream;
    if (queued) {
        const AcqPending& P = c->acq_pending;
        acq_pack_kernel<<<1, 64, 0, st>>>(&dsm->stage, c->d_look->coarse.fine_bi, dsm->prn, P.n_prn, c->s.samplingFreq, (double)P.npts, d_send, slots);
    } else {
        if (host_pack.empty()) {
            host_pack.resize((size_t)slots);
            memset(host_pack.data(), 0, rec_bytes);
        }
        SGX_HIP(hipMemcpyAsync(d_send, host_pack.data(), rec_bytes, hipMemcpyHostToDevice, st));
    }
    if (comm) {
        const int rg = sgx_comm_allgather_device(comm, rec_bytes);
        if (rg != SGX_OK) return rg;
    }
    const int n_rec = slots * n_ranks_seen;
    if ((size_t)n_rec > sizeof(GatherLook::rec) / sizeof(PeakRec)) {
        sgx_set_error("sgx_acquire_sharded: %d ranks x %d slots do not fit the result page", world, slots);
        return SGX_E_ARG;
    }
    const unsigned long long seq = ++c->look_seq;
    GatherLook* const d_gather = &c->d_look->gather;
    const GatherLook* gather = &c->h_look->gather;
    acq_gather_publish_kernel<<<1, 256, 0, st>>>((const int*)d_all, (int)(sizeof(PeakRec) * (size_t)n_rec / 4), (int*)d_gather->rec,
                                                 &d_gather->seq, seq);
    SGX_HIP(hipGetLastError());
    const int rl = acq_look_wait(c, &gather->seq, seq, env.spin);   // the one look
    if (rl != SGX_OK) return rl;
    if (queued) {   // (device time of this rank's search; the search's own page is complete: the gather came behind it)
        SGX_HIP(hipEventSynchronize(c->ev[2]));
        acq_event_times(c, false);
    }
    for (int i = 0; i < n_rec; ++i) {
        const PeakRec& q = gather->rec[i];
        if (q.valid == 0) continue;
        if (q.valid == -1) return acq_index_error(c->n_code, q.prn0, (int)q.codePhase);
        if (q.valid == -2) return acq_fine_range_error((long long)q.codePhase + acq_fine_geom(c->n_code).len, n_samples);
        if (q.prn0 < 0 || q.prn0 >= 32) continue;
        peak_rec_merge(q, out);
    }
    return SGX_OK;
}

// ---- coherent multi-millisecond acquisition ----
// (include/sgx.h, sgx_acquire_coherent; tests/coherent_acq_spec.py is the contract in numpy.)  The search of the reference
// (acquisition.py:62-166) with T-ms windows in place of its 1-ms blocks, on a finer Doppler grid.
static int acquire_coherent_any(const AcqCall& a, const CohGrid& g) {
    if (g.path == 1) return acquire_coherent_shift(a, g);
    return acquire_passes(a, g.M, g.noncoh, &g);
}

// Everything an entry point checks before it touches the device: arguments, grid, record length.
static int coherent_checks(sgx_ctx* c, size_t n_samples, const int32_t* prn0, int32_t n_prn, const sgx_acq_params* p,
                           CohGrid* g, bool* legacy) {
    int rc = acq_check_prns(prn0, n_prn);
    if (rc != SGX_OK) return rc;
    rc = coh_grid(c->s, c->n_code, p, n_prn, g);
    if (rc != SGX_OK) return rc;
    const long long need = (long long)g->T * g->M * c->n_code;
    if ((long long)n_samples < need) {
        sgx_set_error("record window too short: %zu samples, coherent_ms %d x n_windows %d need %lld (%lld short)",
                      n_samples, g->T, g->M, need, need - (long long)n_samples);
        return SGX_E_RANGE;
    }
    *legacy = g->T == 1 && g->step == 500.0;   // the reference's grid: sgx_acquire itself
    return SGX_OK;
}

static int acquire_coherent_source(sgx_ctx* c, const AcqSource& src, const int32_t* prn0, int32_t n_prn, const sgx_acq_params* p,
                                   const AcqOut& out) {
    SGX_CHECK_ARG(c);
    acq_drop_pending(c);
    SGX_CHECK_ARG((src.r || src.signal) && prn0 && p && acq_out_non_null(out));
    if (src.r) SGX_CHECK_ARG(src.offset <= src.r->n && src.n_samples <= src.r->n - src.offset);
    const AcqEnv env = acq_env();
    CohGrid g;
    bool legacy = false;
    int rc = coherent_checks(c, src.n_samples, prn0, n_prn, p, &g, &legacy);
    if (rc != SGX_OK) return rc;
    if (legacy) return acquire_source(c, src, prn0, n_prn, g.M, g.noncoh, out, env);
    SgxSig x;
    if ((rc = acq_source_sig(c, src, &x)) != SGX_OK) return rc;
    return acquire_coherent_any(acq_call(c, x, src.n_samples, prn0, n_prn, out, env), g);
}
extern "C" int sgx_acquire_coherent(sgx_ctx* c, const sgx_if* r, size_t offset, size_t n_samples, const int32_t* prn0,
                                    int32_t n_prn, const sgx_acq_params* p, double* carrFreq, double* codePhase,
                                    double* peakMetric, int32_t* freqBin, int32_t* fineIdx) {
    const AcqOut out{carrFreq, codePhase, peakMetric, freqBin, fineIdx};
    return acquire_coherent_source(c, AcqSource{r, offset, nullptr, n_samples}, prn0, n_prn, p, out);
}
extern "C" int sgx_acquire_coherent_f64(sgx_ctx* c, const double* signal, size_t n_samples, const int32_t* prn0,
                                        int32_t n_prn, const sgx_acq_params* p, double* carrFreq, double* codePhase,
                                        double* peakMetric, int32_t* freqBin, int32_t* fineIdx) {
    const AcqOut out{carrFreq, codePhase, peakMetric, freqBin, fineIdx};
    return acquire_coherent_source(c, AcqSource{nullptr, 0, signal, n_samples}, prn0, n_prn, p, out);
}

extern "C" int sgx_acquire_coherent_plan(const sgx_settings* s, const sgx_acq_params* p, int32_t* n_bins, int32_t* n_phi,
                                         int32_t* path, int32_t* prn_chunk, int32_t* bin_runs) {
    SGX_CHECK_ARG(s && p && n_bins && n_phi && path && prn_chunk && bin_runs);
    SGX_CHECK_ARG(s->codeLength > 0 && s->codeFreqBasis > 0 && s->samplingFreq > 0);
    CohGrid g;
    const int rc = coh_grid(*s, sgx_host_samples_per_code(s), p, 32, &g);
    if (rc != SGX_OK) return rc;
    *n_bins = g.n_bins;
    *n_phi = g.n_phi;
    *path = g.path;
    *prn_chunk = g.prn_chunk;
    *bin_runs = g.runs;
    return SGX_OK;
}
