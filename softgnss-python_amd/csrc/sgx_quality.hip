// Per-channel C/N0 estimate and lock detector on the tracking output (include/sgx.h, sgx_track_quality): the hook the
// reference leaves at tracking.py:276-278 ("it can be update by a lock detector if implemented").
//
//   per window of W ms   R = sum(I^2 - Q^2), X = sum(2 I Q), P = sum(I^2 + Q^2)            (fp64)
//                        phi = atan2(X, R) / 2,  A = sum |I cos phi + Q sin phi|           (second pass, from LDS)
//                        CNo = 10 log10(Psig / ((Ptot - Psig) T)),  Psig = (A/W)^2, Ptot = P/W
//                        carrLock = R / sqrt(R^2 + X^2)
//   per channel          f = 0; fail: f + 1, pass: max(f - 1, 0); lost = first window with f >= max_fail
//
// One workgroup per channel walks the channel in tiles: a tile's I/Q stretch is loaded into LDS with coalesced reads,
// G lanes (a power of two <= min(W, 64)) reduce one window with xor shuffles, and wave 0 runs the counter over the
// tile's pass flags as a scan of the steps x -> max(x + a, b), which compose to steps of the same form.  The restatement
// in numpy is tests/lock_spec.py.
#include <math.h>

#include "sgx_internal.h"

#define QL_THREADS 256
#define QL_STAGE_MS 2048   // ms of I and of Q held in LDS per tile (2 x 16 KiB); a longer window is read from HBM
#define QL_MAX_TILE 1024   // windows per tile at most: QL_STAGE_MS / 2

// (R, X, P, A) of one window; wi / wq point at its first ms, g = this lane's place in its group of G lanes.  Every lane
// of the group returns the same sums (the xor butterfly adds the same pairs on both sides).
__device__ __forceinline__ void ql_window(const double* wi, const double* wq, int W, int g, int G, double& R, double& X,
                                          double& P, double& A) {
    double r = 0.0, x = 0.0, p = 0.0;
    for (int k = g; k < W; k += G) {
        const double i = wi[k], q = wq[k];
        r += i * i - q * q;
        x += 2.0 * i * q;
        p += i * i + q * q;
    }
    for (int o = G >> 1; o > 0; o >>= 1) {
        r += __shfl_xor(r, o);
        x += __shfl_xor(x, o);
        p += __shfl_xor(p, o);
    }
    double s, c;
    sincos(0.5 * atan2(x, r), &s, &c);
    double a = 0.0;
    for (int k = g; k < W; k += G) a += fabs(wi[k] * c + wq[k] * s);
    for (int o = G >> 1; o > 0; o >>= 1) a += __shfl_xor(a, o);
    R = r;
    X = x;
    P = p;
    A = a;
}

template <bool kStaged>
__global__ __launch_bounds__(QL_THREADS) void quality_kernel(const double* __restrict__ I, const double* __restrict__ Q,
                                                             int ms, const int* __restrict__ ms_done, sgx_lock_params lp,
                                                             int n_win, int G, int log2G, double* __restrict__ cno,
                                                             double* __restrict__ carr, uint8_t* __restrict__ pass,
                                                             int* __restrict__ lost) {
    __shared__ double s_i[kStaged ? QL_STAGE_MS : 1];
    __shared__ double s_q[kStaged ? QL_STAGE_MS : 1];
    __shared__ uint8_t s_pass[QL_MAX_TILE];
    const int ch = blockIdx.x;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int W = lp.window;
    const int n_c = (ms_done ? ms_done[ch] : ms) / W;            // whole windows this channel has
    const int tile = kStaged ? QL_STAGE_MS / W : QL_THREADS / G;  // windows per tile
    const double* __restrict__ row_i = I + (long long)ch * ms;
    const double* __restrict__ row_q = Q + (long long)ch * ms;
    const long long out0 = (long long)ch * n_win;
    const int g = tid & (G - 1);
    int f = 0, lost_j = -1;                                       // the counter: meaningful in wave 0
    for (int t0 = 0; t0 < n_win; t0 += tile) {
        const int count = min(tile, n_win - t0);
        const int valid = max(0, min(count, n_c - t0));
        if (kStaged) {
            const int n = valid * W;                              // <= QL_STAGE_MS, and t0 W + n <= ms_done
            for (int k = tid; k < n; k += QL_THREADS) {
                s_i[k] = row_i[(long long)t0 * W + k];
                s_q[k] = row_q[(long long)t0 * W + k];
            }
            __syncthreads();
        }
        for (int w = tid >> log2G; w < count; w += QL_THREADS / G) {   // uniform across each group of G lanes
            double c_no = NAN, cl = NAN;
            uint8_t ok = 0;
            if (w < valid) {
                const double* wi = kStaged ? s_i + w * W : row_i + (long long)(t0 + w) * W;
                const double* wq = kStaged ? s_q + w * W : row_q + (long long)(t0 + w) * W;
                double R, X, P, A;
                ql_window(wi, wq, W, g, G, R, X, P, A);
                const double psig = (A / W) * (A / W);
                const double ptot = P / W;
                if (P == 0.0)
                    c_no = NAN;
                else if (psig == 0.0)
                    c_no = -INFINITY;
                else if (ptot - psig <= 0.0)
                    c_no = INFINITY;
                else
                    c_no = 10.0 * log10(psig / ((ptot - psig) * lp.T));
                cl = R / sqrt(R * R + X * X);
                ok = (c_no >= lp.cno_min && cl >= lp.carr_lock_min) ? 1 : 0;   // a NaN fails
            }
            if (g == 0) {
                cno[out0 + t0 + w] = c_no;
                carr[out0 + t0 + w] = cl;
                pass[out0 + t0 + w] = ok;
                s_pass[w] = ok;
            }
        }
        __syncthreads();
        if (tid < 64 && lost_j < 0) {
            // inclusive scan of the steps (a, b): x -> max(x + a, b); fail (1, 0), pass (-1, 0), past the tile the
            // identity (0, -inf).  (a1, b1) then (a2, b2) is (a1 + a2, max(b1 + a2, b2)).
            for (int base = 0; base < valid; base += 64) {
                const int j = base + lane;
                int a = 0, b = -(1 << 30);
                if (j < valid) {
                    a = s_pass[j] ? -1 : 1;
                    b = 0;
                }
                for (int d = 1; d < 64; d <<= 1) {
                    const int pa = __shfl_up(a, d);
                    const int pb = __shfl_up(b, d);
                    if (lane >= d) {
                        b = max(pb + a, b);
                        a = pa + a;
                    }
                }
                const int fj = max(f + a, b);
                const unsigned long long hit = __ballot(j < valid && fj >= lp.max_fail);
                if (hit) {
                    lost_j = t0 + base + __ffsll((long long)hit) - 1;
                    break;
                }
                f = __shfl(fj, 63);
            }
        }
        __syncthreads();   // the next tile overwrites s_i, s_q and s_pass
    }
    if (tid == 0) lost[ch] = lost_j;
}

extern "C" int sgx_track_quality(sgx_ctx* c, const double* I_P, const double* Q_P, int64_t row_stride, int32_t n_ch,
                                 int32_t ms, const int32_t* ms_done, const sgx_lock_params* p, double* cno,
                                 double* carr_lock, uint8_t* pass, int32_t* lost) {
    SGX_CHECK_ARG(c && I_P && Q_P && p && cno && carr_lock && pass && lost);
    SGX_CHECK_ARG(n_ch >= 1 && ms >= 1);
    const sgx_lock_params lp = *p;
    if (lp.window < 2 || lp.window > ms) {
        sgx_set_error("bad argument: window %d ms must lie in [2, ms = %d]", (int)lp.window, (int)ms);
        return SGX_E_ARG;
    }
    if (lp.max_fail < 1) {
        sgx_set_error("bad argument: max_fail %d must be >= 1", (int)lp.max_fail);
        return SGX_E_ARG;
    }
    if (!(isfinite(lp.T) && lp.T > 0.0)) {
        sgx_set_error("bad argument: T = %g s must be finite and > 0", lp.T);
        return SGX_E_ARG;
    }
    if (row_stride < ms) {
        sgx_set_error("bad argument: row_stride %lld < ms %d", (long long)row_stride, (int)ms);
        return SGX_E_ARG;
    }
    if (ms_done)
        for (int i = 0; i < n_ch; ++i)
            if (ms_done[i] < 0 || ms_done[i] > ms) {
                sgx_set_error("bad argument: ms_done[%d] = %d outside [0, %d]", i, (int)ms_done[i], (int)ms);
                return SGX_E_ARG;
            }
    SGX_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int W = lp.window;
    const int n_win = ms / W;
    int G = 1, log2G = 0;
    while (G * 2 <= W && G < 64) {
        G *= 2;
        ++log2G;
    }
    const size_t n_in = (size_t)n_ch * (size_t)ms, n_out = (size_t)n_ch * (size_t)n_win;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_in = up(n_in * sizeof(double)), b_out = up(n_out * sizeof(double));
    const size_t b_pass = up(n_out), b_ch = up((size_t)n_ch * sizeof(int32_t));
    DevBuf<char> d;
    const int rc = d.ensure(2 * b_in + 2 * b_out + b_pass + 2 * b_ch);
    if (rc != SGX_OK) return rc;
    double* d_i = (double*)d.get();
    double* d_q = (double*)(d + b_in);
    double* d_cno = (double*)(d + 2 * b_in);
    double* d_carr = (double*)(d + 2 * b_in + b_out);
    uint8_t* d_pass = (uint8_t*)(d + 2 * b_in + 2 * b_out);
    int32_t* d_lost = (int32_t*)(d + 2 * b_in + 2 * b_out + b_pass);
    int32_t* d_done = ms_done ? (int32_t*)(d + 2 * b_in + 2 * b_out + b_pass + b_ch) : nullptr;
    const size_t pitch = (size_t)ms * sizeof(double), spitch = (size_t)row_stride * sizeof(double);
    hipError_t e = hipMemcpy2DAsync(d_i, pitch, I_P, spitch, pitch, (size_t)n_ch, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpy2DAsync(d_q, pitch, Q_P, spitch, pitch, (size_t)n_ch, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && d_done) e = hipMemcpyAsync(d_done, ms_done, (size_t)n_ch * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {   // (n_win >= 1: window <= ms)
        if (W <= QL_STAGE_MS)
            quality_kernel<true><<<n_ch, QL_THREADS, 0, st>>>(d_i, d_q, ms, d_done, lp, n_win, G, log2G, d_cno, d_carr,
                                                              d_pass, d_lost);
        else
            quality_kernel<false><<<n_ch, QL_THREADS, 0, st>>>(d_i, d_q, ms, d_done, lp, n_win, G, log2G, d_cno, d_carr,
                                                               d_pass, d_lost);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(cno, d_cno, n_out * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(carr_lock, d_carr, n_out * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(pass, d_pass, n_out, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(lost, d_lost, (size_t)n_ch * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        sgx_set_error("sgx_track_quality failed: %s", hipGetErrorString(e));
        return SGX_E_HIP;
    }
    return SGX_OK;
}
