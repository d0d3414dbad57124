// The acquisition's device code (sgx_acq.hip includes it, nothing else does: one translation unit, no launcher layer):
// the kernels, the structs they take by value and the __device__ bodies they share.  Every routine is here once - a tile
// of a front role, a (maximum, first index) reduction over a wave or a workgroup, a second-peak fold - and the kernels
// that need it call it; kernel names and signatures are what profiles and the trace tools select by.
#pragma once
#include "sgx_internal.h"

// The limits of a coherent multi-millisecond search (sgx_acquire_coherent)
#define ACQ_COH_MAX_MS 20
#define ACQ_COH_MAX_WINDOWS 64
#define ACQ_COH_MAX_SPAN_MS 400
#define ACQ_COH_MAX_PHI 64

// ================================ shared reductions ================================
// "v at index i beats the best so far": the larger value, the smaller index among equals (numpy's FIRST argmax)
template <typename I>
__device__ __forceinline__ void acq_argmax_take(double& best, I& arg, double v, I i) {
    if (v > best || (v == best && i < arg)) {
        best = v;
        arg = i;
    }
}
// (maximum, first index) over the n partial pairs of `row`, a wave at work; lane 0 holds the result
__device__ __forceinline__ void acq_wave_argmax(const double* __restrict__ pv, const int* __restrict__ pidx, int n, int row,
                                                int lane, double& best, int& arg) {
    best = -1.0;
    arg = 0;
    for (int b = lane; b < n; b += 64) acq_argmax_take(best, arg, pv[(long long)row * n + b], pidx[(long long)row * n + b]);
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_down(best, o);
        const int oi = __shfl_down(arg, o);
        acq_argmax_take(best, arg, ov, oi);
    }
}
// (maximum, first index) over the 256 lanes' pairs of a workgroup; thread 0 holds the result
template <typename I>
__device__ __forceinline__ void acq_block_argmax(double& best, I& arg) {
    __shared__ double s_v[256];
    __shared__ I s_i[256];
    s_v[threadIdx.x] = best;
    s_i[threadIdx.x] = arg;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const double ov = s_v[threadIdx.x + s];
            const I oi = s_i[threadIdx.x + s];
            if (ov > s_v[threadIdx.x] || (ov == s_v[threadIdx.x] && oi < s_i[threadIdx.x])) {
                s_v[threadIdx.x] = ov;
                s_i[threadIdx.x] = oi;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        best = s_v[0];
        arg = s_i[0];
    }
}

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
// element i of row `row` of `out`: PRN index p's sampled code
__device__ __forceinline__ void acq_code_tile(const int8_t* __restrict__ codes, int p, cplx* __restrict__ out, int row,
                                              long long i, long long n, double ts, double tc) {
    out[(long long)row * n + i] = make_double2(acq_code_sample(codes, p, i, n, ts, tc), 0.0);
}
__global__ __launch_bounds__(256) void acq_code_kernel(const int8_t* __restrict__ codes,
                                                       const int* __restrict__ prn0, cplx* __restrict__ out,
                                                       long long n, double ts, double tc) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    acq_code_tile(codes, prn0[blockIdx.y], out, blockIdx.y, i, n, ts, tc);
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
    acq_block_argmax(best, arg);
    if (threadIdx.x == 0) {
        rowmax[ro] = best;
        rowarg[ro] = arg;
    }
}

// finish the fused last pass: per-workgroup (max, first index) partials -> one per row
__global__ __launch_bounds__(64) void acq_rowmax_finish_kernel(const double* __restrict__ pmax,
                                                               const int* __restrict__ parg, int nblk,
                                                               double* __restrict__ rowmax, int* __restrict__ rowarg) {
    const int row = blockIdx.x;
    double best;
    int arg;
    acq_wave_argmax(pmax, parg, nblk, row, threadIdx.x, best, arg);
    if (threadIdx.x == 0) {
        rowmax[row] = best;
        rowarg[row] = arg;
    }
}

// acquisition.py:162: max of the chosen frequency row over the exclusion index list
// (grid (PRNs, SEC_SPLIT): every workgroup takes a slice of the ranges and folds its maximum into out[p] with an integer
// atomic max on the bit pattern - powers are non-negative, so the patterns order like the values; out[] starts at 0)
#define SEC_SPLIT 16
// power(row, i): the power at index i of the row, however the kernel forms it
template <typename Power>
__device__ __forceinline__ void acq_second_body(const SecondArgs& a, double* __restrict__ out, Power power) {
    const int p = blockIdx.x;
    const int t0 = blockIdx.y * 256 + threadIdx.x, ts = gridDim.y * 256;
    double best = 0.0;
    if (a.row[p] >= 0) {
        const int row = a.row[p];
        for (int i = a.lo0[p] + t0; i < a.hi0[p]; i += ts) best = fmax(best, power(row, i));
        for (int i = a.lo1[p] + t0; i < a.hi1[p]; i += ts) best = fmax(best, power(row, i));
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
__global__ __launch_bounds__(256) void acq_second_kernel(const double* __restrict__ P, double* __restrict__ out,
                                                         long long n, const SecondArgs* __restrict__ ap) {
    acq_second_body(*ap, out, [=](int row, int i) { return P[(long long)row * n + i]; });
}

// the same on a recomputed complex correlation row: |z|^2 / N^2 formed on the fly, identical arithmetic to
// the fused last pass, so peak / second peak is a ratio of consistently rounded values
// (n: elements between the rows of Z; the ranges lie inside the correlation's own length)
__global__ __launch_bounds__(256) void acq_second_cplx_kernel(const cplx* __restrict__ Z, double* __restrict__ out,
                                                              long long n, double inv_n, const SecondArgs* __restrict__ ap) {
    acq_second_body(*ap, out, [=](int row, int i) {
        const cplx z = Z[(long long)row * n + i];
        const double re = z.x * inv_n, im = z.y * inv_n;
        return re * re + im * im;
    });
}

// integer sum of the record window (mean for acquisition.py:59): bytes up to the first 16-byte boundary, 16 bytes per
// lane from there, bytes again for the rest
// (thread gid of gsz, t its index in a workgroup of 256)
__device__ __forceinline__ void acq_sum_part(const int8_t* __restrict__ x, long long n, long long gid, long long gsz, int t,
                                             long long* __restrict__ out) {
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
    if ((t & 63) == 0) s_acc[t >> 6] = acc;
    __syncthreads();
    if (t == 0) atomicAdd((unsigned long long*)out, (unsigned long long)(s_acc[0] + s_acc[1] + s_acc[2] + s_acc[3]));
}
__global__ __launch_bounds__(256) void acq_sum_kernel(const int8_t* __restrict__ x, long long n,
                                                      long long* __restrict__ out) {
    acq_sum_part(x, n, (long long)blockIdx.x * 256 + threadIdx.x, (long long)gridDim.x * 256, threadIdx.x, out);
}

// Call set-up in one launch: the PRN list and the bin map (by value) to their device tables, the accumulators zeroed.
struct AcqSetup {
    int prn[32];
    int2 bin[ACQ_MAX_BINS];
    int n_prn, n_bins;
};
__device__ __forceinline__ void acq_setup_part(const AcqSetup& a, int* __restrict__ d_prn, int2* __restrict__ d_bin,
                                               long long* __restrict__ d_sum, double* __restrict__ d_second,
                                               int* __restrict__ d_arrived, int t) {
    if (t < a.n_prn) d_prn[t] = a.prn[t];
    if (t < a.n_bins) d_bin[t] = a.bin[t];
    if (t < 32) d_second[t] = 0.0;
    if (t < 64) d_arrived[t] = 0;   // [32] rows finished per PRN, [32] PRNs finished
    if (t == 0) d_sum[0] = 0;
}
__global__ __launch_bounds__(128) void acq_setup_kernel(AcqSetup a, int* __restrict__ d_prn, int2* __restrict__ d_bin,
                                                        long long* __restrict__ d_sum, double* __restrict__ d_second,
                                                        int* __restrict__ d_arrived) {
    acq_setup_part(a, d_prn, d_bin, d_sum, d_second, d_arrived, threadIdx.x);
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
    acq_block_argmax(best, arg);
    if (threadIdx.x == 0) {
        pv[(long long)d * gridDim.x + blockIdx.x] = best;
        pi[(long long)d * gridDim.x + blockIdx.x] = arg;
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
// element i of forward row `row` = (block, phi)
__device__ __forceinline__ void acq_mixphi_tile(SgxSig x, cplx* __restrict__ out, long long n, const PhiArgs& a, int row,
                                                long long i) {
    const int j = row % a.n_phi;
    const int b = row / a.n_phi;
    const double xv = x.at((long long)b * n + i);
    double s = 0.0, c = 1.0;
    if (a.phi[j] != 0.0) sincospi((2.0 * a.phi[j]) * ((double)i / (double)n), &s, &c);
    out[(long long)row * n + i] = make_double2(c * xv, -(s * xv));
}
__global__ __launch_bounds__(256) void acq_mixphi_kernel(SgxSig x, cplx* __restrict__ out,
                                                         long long n, PhiArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    acq_mixphi_tile(x, out, n, a, blockIdx.y, i);
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
        acq_mixphi_tile(x, out, n, pa, row, i);
        return;
    }
    blk -= n_mix;
    if (blk < n_code) {
        const int row = blk / gx;
        const long long i = (long long)(blk - row * gx) * 256 + t;
        if (i >= n) return;
        acq_code_tile(codes, su.prn[row], out, rows_fwd + row, i, n, ts, tc);
        return;
    }
    blk -= n_code;
    if (blk < ACQ_SUM_WGS) {
        acq_sum_part(x.i8, n_samples, (long long)blk * 256 + t, (long long)ACQ_SUM_WGS * 256, t, sum_now);
        return;
    }
    acq_setup_part(su, d_prn, d_bin, sum_next, d_second, d_arrived, t);
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
// (bad: bit b set - block b of the signal holds a sample that is not finite, so every power of the block is NaN in the
// reference (numpy's max then is NaN, its argmax 0); the kernels' "v > best" reductions skip NaN, so the block's rows are
// taken as (NaN, 0) here, where the reference's block rule meets them.  Only an fp64 signal can set a bit.)
__host__ __device__ static inline AcqCand acq_peak_bin(const double* __restrict__ rowmax, const int* __restrict__ rowarg,
                                                       int n_bins, int n_blocks, bool noncoh, int k,
                                                       unsigned long long bad = 0ull) {
    int row = k, bsel = 0;
    bool nan_row = noncoh && bad != 0ull;
    if (!noncoh) {
        int best = 0;   // acquisition.py:129-133 generalised left to right, later block wins ties
        for (int b = 1; b < n_blocks; ++b) {
            const double vb = ACQ_LD(rowmax + best * n_bins + k);
            const double vn = ACQ_LD(rowmax + b * n_bins + k);
            if (!(vb > vn) || (((bad >> best) | (bad >> b)) & 1ull)) best = b;   // (a NaN maximum on either side: not larger)
        }
        row = best * n_bins + k;
        bsel = best;
        nan_row = ((bad >> best) & 1ull) != 0ull;
    }
    AcqCand c;
    c.v = ACQ_LD(rowmax + row);
    c.a = ACQ_LD(rowarg + row);
    if (nan_row) {
        c.v = __builtin_nan("");
        c.a = 0;
    }
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
                                                   int n_bins, int n_blocks, int noncoh, unsigned long long bad) {
    AcqCand c;
    c.v = -1.0;
    c.k = -1;
    c.a = c.b = 0;
    for (int k = lane; k < n_bins; k += 64) c = acq_peak_join(c, acq_peak_bin(pm, pa, n_bins, n_blocks, noncoh != 0, k, bad));
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
                                                 int n_bins, int n_blocks, int noncoh, unsigned long long bad) {
    AcqCand c = acq_peak_reduce(pm, pa, lane, n_bins, n_blocks, noncoh, bad);
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
                                             int2* __restrict__ row_map, unsigned long long bad_rows) {
    if (pi >= n_prn) {
        if (lane == 0) {
            sa->row[pi] = -1;
            sa->lo0[pi] = sa->hi0[pi] = sa->lo1[pi] = sa->hi1[pi] = 0;
        }
        return;
    }
    const AcqCand c = acq_peak_reduce(rowmax + (long long)pi * out_per_prn, rowarg + (long long)pi * out_per_prn, lane, n_bins,
                                      n_blocks, noncoh, bad_rows);
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
    double best;
    int arg;
    acq_wave_argmax(pv, pidx, n, row, lane, best, arg);
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
                                                             int2* __restrict__ row_map, unsigned long long bad_rows) {
    const int row = blockIdx.x, lane = threadIdx.x;
    int pi;
    if (!acq_row_finish(pmax, parg, nblk, row, lane, rowmax, rowarg, arrived, out_per_prn, &pi)) return;
    acq_peak_one(rowmax, rowarg, pi, lane, n_prn, out_per_prn, n_bins, n_blocks, noncoh, N, spc, po, sa, row_map, bad_rows);
    if (pi == n_prn - 1 && n_prn + lane < 32)
        acq_peak_one(rowmax, rowarg, n_prn + lane, 0, n_prn, out_per_prn, n_bins, n_blocks, noncoh, N, spc, po, sa, row_map, bad_rows);
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
                                                              PublishArgs pub, unsigned long long bad_rows) {
    const int row = blockIdx.x, lane = threadIdx.x;
    int pi;
    if (!acq_row_finish(b1, i1, nres, row, lane, rowmax, rowarg, arrived, out_per_prn, &pi)) return;
    const AcqCand c = acq_peak_scan(rowmax + (long long)pi * out_per_prn, rowarg + (long long)pi * out_per_prn, lane, n_bins,
                                    n_blocks, noncoh, bad_rows);
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
// (sgx_acq.hip, "deferred acquisition", says who queues it.)  acquisition.py:259-306 on the device, repeating the host's
// arithmetic: one IEEE multiplication and division for carrFreq, one division for peakMetric, a stable descending sort.
// One wave; lane p = PRN index p of the 32-entry result arrays.
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
