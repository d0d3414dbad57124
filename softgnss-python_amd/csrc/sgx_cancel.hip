// Strong-signal cancellation (no reference counterpart): the signals of tracked channels rebuilt from their recorded blocks
// and subtracted from a real int8 record, so that a search of the new record finds what they hid.  tests/cancel_spec.py is the
// contract, sgx_cancel.cpp the host twin and the tables, DESIGN.md section 4.23 the account.
//
//   cancel_kernel  tiles the OUTPUT: a workgroup of 256 lanes owns CN_TILE = 4096 consecutive samples, lane t the 16 from
//                  t0 + 16 t on - one 16-byte load, one 16-byte store, every byte written once by one lane.  Nothing crosses a
//                  workgroup but the clip count (integer atomics, sgx_count.h).
//     blocks       a channel's blocks are contiguous in the record: thread c < n_ch finds by binary search over the block
//                  ends the first block of channel c that reaches the tile; every lane walks on from there to its own 16
//                  samples, and through them: a block run is the part of one block inside the 16 - none, one or (at a
//                  boundary) two of them, and as many as there are where blocks are shorter than that.
//     per run      the carrier (sin, cos)(w (i / fs) + rem_carr) by fp64 sincos at the lane's first sample, in the contract's
//                  own arithmetic, then turned by the block's angle of one sample (sgx_cancel.cpp forms it); the chip from an
//                  LDS table of the channel's code laid out twice, index ceil(i lin + start) - cb as replay_kernel's.
//     per sample   v -= chip (a_I sin + a_Q cos), channels in channel order: two calls give the same bytes.
//   The 16 sums stay in registers: every loop over them is unrolled and a run's samples are selected, not indexed.
#include <math.h>

#include "sgx_cancel_core.h"
#include "sgx_stage.h"

#define CN_THREADS 256
#define CN_LANE 16
#define CN_TILE (CN_THREADS * CN_LANE)

__global__ __launch_bounds__(CN_THREADS) void cancel_kernel(const int8_t* __restrict__ x, int8_t* __restrict__ y, long long n,
                                                            const CnBlock* __restrict__ blocks,
                                                            const CnChan* __restrict__ chan, int n_ch, int ms,
                                                            const int8_t* __restrict__ codes, double fs,
                                                            unsigned long long* __restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) int8_t s_code[];   // [n_ch][CN_TABLE]
    __shared__ int s_first[CN_MAX_CHANNELS];
    const int tid = threadIdx.x;
    const long long t0 = (long long)blockIdx.x * CN_TILE;
    for (int i = tid; i < n_ch * CN_TABLE; i += CN_THREADS) {
        const int prn = chan[i / CN_TABLE].prn;
        s_code[i] = prn ? codes[(prn - 1) * 1023 + (i % CN_TABLE) % 1023] : (int8_t)0;
    }
    if (tid < n_ch) {           // the first block of channel tid that ends behind the tile's first sample; done: none does
        const CnBlock* __restrict__ b = blocks + (size_t)tid * ms;
        int lo = 0, hi = chan[tid].done;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (b[mid].pos + b[mid].blk <= t0) lo = mid + 1;
            else hi = mid;
        }
        s_first[tid] = lo;
    }
    __syncthreads();
    const long long p0 = t0 + (long long)tid * CN_LANE;
    unsigned clipped = 0;
    if (p0 < n) {
        const bool whole = p0 + CN_LANE <= n;
        unsigned in[4] = {0u, 0u, 0u, 0u};
        if (whole) {
            const uint4 q = *reinterpret_cast<const uint4*>(x + p0);
            in[0] = q.x, in[1] = q.y, in[2] = q.z, in[3] = q.w;
        } else {
#pragma unroll
            for (int e = 0; e < CN_LANE; ++e)
                if (p0 + e < n) in[e >> 2] |= (unsigned)(uint8_t)x[p0 + e] << (8 * (e & 3));
        }
        double v[CN_LANE];
#pragma unroll
        for (int e = 0; e < CN_LANE; ++e) v[e] = (double)(int8_t)((in[e >> 2] >> (8 * (e & 3))) & 0xFFu);
        unsigned covered = 0;
        for (int c = 0; c < n_ch; ++c) {
            const int done = chan[c].done;
            const CnBlock* __restrict__ b = blocks + (size_t)c * ms;
            const int8_t* __restrict__ code = s_code + c * CN_TABLE;
            int k = s_first[c];
            while (k < done && b[k].pos + b[k].blk <= p0) ++k;
            while (k < done) {
                const CnBlock g = b[k];
                if (g.pos >= p0 + CN_LANE) break;
                // samples [e0, e1) of the 16 lie in block k; sample e is sample ia + e of the block (ia < 0: the block
                // starts inside the 16)
                const int ia = (int)(p0 - g.pos);
                const int e0 = ia < 0 ? -ia : 0;
                const long long left = g.pos + g.blk - p0;
                const int e1 = left < CN_LANE ? (int)left : CN_LANE;
                double sn, cs;
                sincos(g.w * ((double)ia / fs) + g.rem_carr, &sn, &cs);
                double nd = (double)ia;
#pragma unroll
                for (int e = 0; e < CN_LANE; ++e) {
                    const double t = nd * g.lin + g.start;
                    const int idx = min(max((int)(ceil(t) - g.cb), 0), CN_TABLE - 1);
                    const double chip = (double)code[idx];
                    const double sc = chip * (g.a_i * sn + g.a_q * cs);
                    if (e >= e0 && e < e1) v[e] = v[e] - sc;
                    const double c2 = fma(cs, g.rot_c, -(sn * g.rot_s));
                    sn = fma(sn, g.rot_c, cs * g.rot_s);
                    cs = c2;
                    nd += 1.0;
                }
                covered |= ((1u << e1) - 1u) & ~((1u << e0) - 1u);
                if (left > CN_LANE) break;
                ++k;
            }
        }
        unsigned o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < CN_LANE; ++e) {
            const unsigned raw = (in[e >> 2] >> (8 * (e & 3))) & 0xFFu;
            double r = rint(v[e]);
            const bool on = (covered >> e) & 1u;          // (a lane's samples beyond the record are never covered)
            const bool clip = on && (r > 127.0 || r < -127.0);
            clipped += clip ? 1u : 0u;
            r = fmin(fmax(r, -127.0), 127.0);
            o[e >> 2] |= (on ? (unsigned)((int)r & 0xFF) : raw) << (8 * (e & 3));
        }
        if (whole) {
            *reinterpret_cast<uint4*>(y + p0) = make_uint4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int e = 0; e < CN_LANE; ++e)
                if (p0 + e < n) y[p0 + e] = (int8_t)((o[e >> 2] >> (8 * (e & 3))) & 0xFFu);
        }
    }
    const unsigned cnt[1] = {clipped};
    sgx_count_publish<1, CN_THREADS / 64>(cnt, counts);
}

extern "C" int sgx_cancel_timing(sgx_ctx* c, float* kernel_ms) {
    SGX_CHECK_ARG(c && kernel_ms);
    *kernel_ms = c->stage_ms[SGX_STAGE_CANCEL];
    return SGX_OK;
}

extern "C" int sgx_if_cancel(sgx_ctx* c, const sgx_if* rec, int64_t rec_file_offset, const sgx_chan_init* ch, int32_t n_ch,
                             int32_t ms, const int32_t* ms_done, const double* series, int32_t data_type, const double* amp,
                             sgx_if** out, int64_t* clipped) {
    SGX_CHECK_ARG(c && rec && out && clipped);
    SGX_CHECK_ARG(rec->device == c->device);
    if (rec->n == 0) {
        sgx_set_error("bad argument: the cancellation needs a record of at least one sample");
        return SGX_E_ARG;
    }
    const unsigned long long tiles = ((unsigned long long)rec->n + CN_TILE - 1) / CN_TILE;
    int rc = sgx_stage_one_launch(tiles, "bad argument: a record of %zu samples is beyond one launch of the cancellation kernel",
                                  rec->n);
    if (rc == SGX_OK) rc = sgx_stage_open(c, rec, rec->n);       // the whole record resident, as the replay
    if (rc != SGX_OK) return rc;
    std::vector<sgx_replay_block> state;
    rc = cn_check(&c->s, rec_file_offset, (int64_t)rec->n, ch, n_ch, ms, ms_done, series, data_type, amp, &state);
    if (rc != SGX_OK) return rc;
    SGX_CHECK_ARG(((size_t)rec->d & 15) == 0);                   // (every record starts on a granule: hipMalloc's alignment)
    const size_t n_blocks = (size_t)n_ch * (size_t)ms;
    const size_t b_blocks = (n_blocks * sizeof(CnBlock) + 255) & ~(size_t)255;
    std::vector<char> h(b_blocks + sizeof(CnChan) * (size_t)n_ch);
    cn_tables(&c->s, rec_file_offset, ch, n_ch, ms, ms_done, state.data(), amp, reinterpret_cast<CnBlock*>(h.data()),
              reinterpret_cast<CnChan*>(h.data() + b_blocks));
    rc = c->d_cancel.ensure(h.size());
    if (rc != SGX_OK) return rc;
    SGX_HIP(hipMemcpy(c->d_cancel.get(), h.data(), h.size(), hipMemcpyHostToDevice));
    const CnBlock* d_blocks = reinterpret_cast<const CnBlock*>(c->d_cancel.get());
    const CnChan* d_chan = reinterpret_cast<const CnChan*>(c->d_cancel.get() + b_blocks);
    const size_t lds = (size_t)n_ch * CN_TABLE;                  // at most 64 KB, beside the few static words
    SGX_HIP(hipFuncSetAttribute((const void*)cancel_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                CN_MAX_CHANNELS * CN_TABLE));
    const long long n = (long long)rec->n;
    const double fs = c->s.samplingFreq;
    SgxStage st(SGX_STAGE_CANCEL, (unsigned)tiles, "cancellation kernel failed: %s", out, rec->n);
    unsigned long long* d_cnt = st.count(c);
    rc = sgx_stage_run(c, st, [&](sgx_if* r) {
        cancel_kernel<<<st.grid, CN_THREADS, lds, c->stream>>>(rec->d, r->d, n, d_blocks, d_chan, n_ch, ms, c->d_codes, fs,
                                                               d_cnt);
    });
    if (rc != SGX_OK) return rc;
    *clipped = sgx_stage_count(c, 0);
    return SGX_OK;
}
