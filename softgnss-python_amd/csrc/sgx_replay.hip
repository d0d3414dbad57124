// Multi-correlator replay of tracked channels (include/sgx.h: sgx_track_replay; the contract in numpy: tests/replay_spec.py).
//
// A tracked channel's blocks are on record: sgx_replay_state (sgx_core.cpp) rebuilds, per block, its start byte, length,
// code and carrier remainders and rates from the series sgx_track_ex wrote.  Nothing chains the blocks any more, so ONE
// launch covers every (channel, block): workgroup b = channel * ms + block, 256 threads, thread t takes the samples
// n = t, t + 256, ... of its block (a wave reads 64 consecutive samples per load).
//
//   once per sample   the load; the carrier (cos, sin)(arg_n): fp64 sincos at n = t in the contract's own arithmetic
//                     (carr_freq 2.0 pi (n / fs) + rem_carr), then turned by the angle of 256 samples per step (two
//                     multiplications and two fused multiply-adds; <= 150 turns per block at 38 samples per chip)
//   per tap           t_n = n steplin + start with the contract's roundings (steplin = (stop - start) / blk per tap, the
//                     multiplication and the addition unfused: the build is -ffp-contract=off), ceil, and the chip read
//                     from an LDS table of the code as +-1.0 doubles laid out twice: index ceil(t_n) - cb with
//                     cb = ceil(start) - (ceil(start) - 1) mod 1023 lies in [0, 2047), no modulus per sample.
//                     I += chip sin x, Q += chip cos x as fused multiply-adds (chip = +-1: the product is exact)
//
// Taps run in register chunks of KT <= 4 (2 KT accumulators and 3 KT tap constants per lane); a bank of more taps walks its
// block once per chunk (the block is 38 KB and stays in L2).  Sums: lanes in stride order, xor butterfly per wave, the
// four waves added in wave order by one thread: the same bytes on every call.
#include <math.h>

#include <vector>

#include "sgx_internal.h"

#define RP_THREADS 256
#define RP_TABLE 2048        // doubles of the doubled code table (2 x 1023 + 2)

template <int DT>
__device__ __forceinline__ double rp_sample(const int8_t* __restrict__ p, long long n) {
    if (DT == SGX_DT_INT8) return (double)p[n];
    if (DT == SGX_DT_UINT8) return (double)(uint8_t)p[n];
    const int lo = (uint8_t)p[2 * n], hi = p[2 * n + 1];   // little endian, at any byte
    return (double)(hi * 256 + lo);
}

template <int KT, int DT>
__global__ __launch_bounds__(RP_THREADS) void replay_kernel(const int8_t* __restrict__ rec, long long rec_n,
                                                            long long rec_file_offset, const int8_t* __restrict__ codes,
                                                            const sgx_replay_block* __restrict__ state,
                                                            const int* __restrict__ prn, const int* __restrict__ done,
                                                            const double* __restrict__ taps, int n_taps, int ms, double fs,
                                                            double* __restrict__ out) {
    __shared__ double s_code[RP_TABLE];
    __shared__ double s_red[RP_THREADS / 64][2 * KT];
    const int ch = blockIdx.x / ms;
    const int k = blockIdx.x - ch * ms;
    if (k >= done[ch]) return;                       // (the output was zeroed; channels that are off have done = 0)
    const int tid = threadIdx.x;
    const sgx_replay_block b = state[blockIdx.x];
    const int blk = b.blk;
    const long long isz = DT == SGX_DT_INT16 ? 2 : 1;
    const long long i0 = b.start - rec_file_offset;
    if (i0 < 0 || i0 + blk * isz > rec_n) return;    // (the host has checked it: sgx_replay_state)
    const int8_t* __restrict__ x0 = rec + i0;
    const int8_t* __restrict__ code = codes + (prn[ch] - 1) * 1023;
    for (int i = tid; i < RP_TABLE; i += RP_THREADS) s_code[i] = (double)code[i % 1023];
    __syncthreads();
    const double nblk = (double)blk;
    const double w = b.carr_freq * 2.0 * M_PI;
    double rs, rc;                                   // the turn of 256 samples
    sincos(w * ((double)RP_THREADS / fs), &rs, &rc);
    for (int j0 = 0; j0 < n_taps; j0 += KT) {
        double start[KT], lin[KT], cb[KT], acc_i[KT], acc_q[KT];
#pragma unroll
        for (int u = 0; u < KT; ++u) {
            const double d = taps[min(j0 + u, n_taps - 1)];
            start[u] = b.rem_code + d;
            const double stop = nblk * b.step + b.rem_code + d;
            lin[u] = (stop - start[u]) / nblk;
            const double c0 = ceil(start[u]) - 1.0;
            double m = fmod(c0, 1023.0);
            if (m < 0.0) m += 1023.0;
            cb[u] = c0 - m + 1.0;
            acc_i[u] = 0.0;
            acc_q[u] = 0.0;
        }
        double sn, cs;
        sincos(w * ((double)tid / fs) + b.rem_carr, &sn, &cs);
        double nd = (double)tid;
        for (int n = tid; n < blk; n += RP_THREADS) {
            const double x = rp_sample<DT>(x0, n);
            const double xi = sn * x, xq = cs * x;
#pragma unroll
            for (int u = 0; u < KT; ++u) {
                const double t = nd * lin[u] + start[u];
                const int idx = min(max((int)(ceil(t) - cb[u]), 0), RP_TABLE - 1);
                const double chip = s_code[idx];
                acc_i[u] = fma(chip, xi, acc_i[u]);
                acc_q[u] = fma(chip, xq, acc_q[u]);
            }
            const double c2 = fma(cs, rc, -(sn * rs));
            sn = fma(sn, rc, cs * rs);
            cs = c2;
            nd += (double)RP_THREADS;
        }
#pragma unroll
        for (int u = 0; u < KT; ++u) {
            for (int o = 32; o > 0; o >>= 1) {
                acc_i[u] += __shfl_xor(acc_i[u], o);
                acc_q[u] += __shfl_xor(acc_q[u], o);
            }
            if ((tid & 63) == 0) {
                s_red[tid >> 6][2 * u] = acc_i[u];
                s_red[tid >> 6][2 * u + 1] = acc_q[u];
            }
        }
        __syncthreads();
        if (tid < 2 * KT && j0 + (tid >> 1) < n_taps) {
            double v = s_red[0][tid];
            for (int wv = 1; wv < RP_THREADS / 64; ++wv) v += s_red[wv][tid];
            out[(((size_t)ch * n_taps + (j0 + (tid >> 1))) * 2 + (tid & 1)) * (size_t)ms + k] = v;
        }
        __syncthreads();                             // the next chunk overwrites s_red
    }
}

template <int DT>
static void replay_launch(int kt, int grid, hipStream_t st, const int8_t* rec, long long rec_n, long long off,
                          const int8_t* codes, const sgx_replay_block* state, const int* prn, const int* done,
                          const double* taps, int n_taps, int ms, double fs, double* out) {
    switch (kt) {
    case 1: replay_kernel<1, DT><<<grid, RP_THREADS, 0, st>>>(rec, rec_n, off, codes, state, prn, done, taps, n_taps, ms, fs, out); break;
    case 2: replay_kernel<2, DT><<<grid, RP_THREADS, 0, st>>>(rec, rec_n, off, codes, state, prn, done, taps, n_taps, ms, fs, out); break;
    case 3: replay_kernel<3, DT><<<grid, RP_THREADS, 0, st>>>(rec, rec_n, off, codes, state, prn, done, taps, n_taps, ms, fs, out); break;
    default: replay_kernel<4, DT><<<grid, RP_THREADS, 0, st>>>(rec, rec_n, off, codes, state, prn, done, taps, n_taps, ms, fs, out); break;
    }
}

extern "C" int sgx_track_replay(sgx_ctx* c, const sgx_if* r, int64_t rec_file_offset, const sgx_chan_init* ch, int32_t n_ch,
                                int32_t ms, const int32_t* ms_done, const double* series, int32_t data_type,
                                const double* taps, int32_t n_taps, double* out) {
    SGX_CHECK_ARG(c && r && ch && series && taps && out);
    SGX_CHECK_ARG(n_ch >= 1 && ms >= 1 && (long long)n_ch * ms <= 0x7fffffffLL);
    if (n_taps < 1 || n_taps > SGX_REPLAY_MAX_TAPS) {
        sgx_set_error("bad argument: n_taps %d outside [1, %d]", (int)n_taps, SGX_REPLAY_MAX_TAPS);
        return SGX_E_ARG;
    }
    for (int j = 0; j < n_taps; ++j)
        if (!isfinite(taps[j])) {
            sgx_set_error("bad argument: tap %d is not finite", j);
            return SGX_E_ARG;
        }
    if (data_type != SGX_DT_INT8 && data_type != SGX_DT_UINT8 && data_type != SGX_DT_INT16) {
        sgx_set_error("bad argument: the replay reads int8, uint8 and int16 records, not data_type %d", (int)data_type);
        return SGX_E_ARG;
    }
    const int rq = sgx_if_require(r, r->n);          // the whole record resident, as sgx_if_wait
    if (rq != SGX_OK) return rq;
    const size_t n_blocks = (size_t)n_ch * (size_t)ms;
    std::vector<sgx_replay_block> state(n_blocks);
    const int rs = sgx_replay_state(&c->s, data_type, ch, n_ch, ms, ms_done, series, rec_file_offset, (int64_t)r->n,
                                    state.data());
    if (rs != SGX_OK) return rs;
    std::vector<int> meta(2 * (size_t)n_ch);         // prn, then blocks done (0 for a channel that is off)
    for (int i = 0; i < n_ch; ++i) {
        meta[i] = ch[i].prn;
        meta[n_ch + i] = ch[i].prn == 0 ? 0 : (ms_done ? ms_done[i] : ms);
    }
    SGX_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_state = up(n_blocks * sizeof(sgx_replay_block)), b_meta = up(meta.size() * sizeof(int));
    const size_t b_taps = up((size_t)n_taps * sizeof(double));
    const size_t n_out = n_blocks * (size_t)n_taps * 2;
    DevBuf<char> d;
    const int rd = d.ensure(b_state + b_meta + b_taps + n_out * sizeof(double));
    if (rd != SGX_OK) return rd;
    sgx_replay_block* d_state = (sgx_replay_block*)d.get();
    int* d_meta = (int*)(d + b_state);
    double* d_taps = (double*)(d + b_state + b_meta);
    double* d_out = (double*)(d + b_state + b_meta + b_taps);
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipError_t e = hipSuccess;
    for (int i = 0; i < 4 && e == hipSuccess; ++i) e = hipEventCreate(&ev[i]);
    if (e == hipSuccess) e = hipEventRecord(ev[0], st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_state, state.data(), n_blocks * sizeof(sgx_replay_block), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_meta, meta.data(), meta.size() * sizeof(int), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_taps, taps, (size_t)n_taps * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(d_out, 0, n_out * sizeof(double), st);
    if (e == hipSuccess) e = hipEventRecord(ev[1], st);
    if (e == hipSuccess) {
        const int kt = n_taps < 4 ? n_taps : 4;
        const int grid = (int)n_blocks;
        const long long rec_n = (long long)r->n;
        if (data_type == SGX_DT_INT8)
            replay_launch<SGX_DT_INT8>(kt, grid, st, r->d, rec_n, rec_file_offset, c->d_codes, d_state, d_meta, d_meta + n_ch,
                                       d_taps, n_taps, ms, c->s.samplingFreq, d_out);
        else if (data_type == SGX_DT_UINT8)
            replay_launch<SGX_DT_UINT8>(kt, grid, st, r->d, rec_n, rec_file_offset, c->d_codes, d_state, d_meta, d_meta + n_ch,
                                        d_taps, n_taps, ms, c->s.samplingFreq, d_out);
        else
            replay_launch<SGX_DT_INT16>(kt, grid, st, r->d, rec_n, rec_file_offset, c->d_codes, d_state, d_meta, d_meta + n_ch,
                                        d_taps, n_taps, ms, c->s.samplingFreq, d_out);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(ev[2], st);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, n_out * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipEventRecord(ev[3], st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) {
        (void)hipEventElapsedTime(&c->replay_kernel_ms, ev[1], ev[2]);
        (void)hipEventElapsedTime(&c->replay_device_ms, ev[0], ev[3]);
    }
    for (int i = 0; i < 4; ++i)
        if (ev[i]) (void)hipEventDestroy(ev[i]);
    if (e != hipSuccess) {
        sgx_set_error("sgx_track_replay failed: %s", hipGetErrorString(e));
        return SGX_E_HIP;
    }
    return SGX_OK;
}
