// Bit-aligned coherent tracking of weak signals (include/sgx.h: sgx_track_coherent; the contract in numpy is
// tests/coh_track_spec.py): the kernel and its host side.
//
// Every block is the reference's block (tracking.py:148-219), mapped, reduced and recorded by the block pieces of
// sgx_trk_block.h, which the per-sample body shares (sgx_trk_persample.h with one member per channel computes the same bits
// while every block is updated); only WHEN the two loop filters run changes, and that schedule is this file's own.  Blocks
// k < k0 are updated one by one (the reference); at the end of block k0 - 1 both filters restart from the mean of their last H
// NCO values; from k0 on the sums of T blocks are added and the filters run once per group with PDI = T ms, the rates held in
// between.  k0 sits on a navigation-bit edge, given or found by the 20 hypotheses of the bit synchronisation during the pull-in.
//
// ONE workgroup per channel and no exchange between workgroups: nothing in this kernel polls memory another workgroup
// writes, so no wait can fail to end and no launch is repeated.  Four waves:
//   every lane   maps the block's groups of 16 samples (sample by sample below ~15.4 samples per chip, one chip switch per
//                ramp and group above), six partial sums -> s_red
//   wave 0       folds I_E / Q_E; PLL side: group sums of I_P / Q_P, discriminator, filter, hand-over, next block's phasors
//   wave 1       folds I_P / Q_P; DLL side: group sums of the early and late arms, discriminator, filter, hand-over, next ramps
//   wave 2       folds I_L / Q_L; stores the previous block's row
//   wave 3       the carrier phase at the block's end; lanes 0..19 the 20 bit-synchronisation hypotheses
#include "sgx_trk_block.h"

#define COH_MAX_H 1000
#define COH_K0_NONE 0x7FFFFFFF

struct CohConst {
    double k_code_a, k_code_b, k_carr_a, k_carr_b;   // tau2 / tau1 and T ms / tau1 of the coherent loops
    int T, P, H;
    // where the call's results beside the series go, [n_ch] each (the energies [n_ch][20]), and the launch's error word
    const int* edge_in;
    int *edge_out, *k0_out, *ms_done, *err;
    double* energy;
};

// The hand-over at the end of the pull-in: the mean of the last nh NCO values, the block's own (nco, not in the ring yet)
// the latest of them (block k's value sits at ring[k % H])
static __device__ __forceinline__ double coh_ring_mean(const double (&ring)[COH_MAX_H], int it, int nh, int H, double nco) {
    double acc = 0.0;
    for (int q = it + 1 - nh; q < it; ++q) acc += ring[q % H];
    acc += nco;
    return acc / (double)nh;
}

__global__ __launch_bounds__(TRK_THREADS, 1) void trk_kernel_coh(const int8_t* __restrict__ rec, const int8_t* __restrict__ codes,
    const TrkChan* __restrict__ chans, double* __restrict__ out, const TrkConst Kin, const CohConst Cin) {
    // The call's constants live in LDS, not in scalar registers: the filter waves read a field when they need it (a
    // broadcast read), and nothing is held across the map - with them as kernel arguments 54 scalars were kept in vector lanes
    __shared__ TrkConst s_K;
    __shared__ CohConst s_C;
    __shared__ unsigned s_code_hi[1028];   // trk_code_table
    __shared__ TrkBlock s_blk;
    __shared__ double s_red[6][TRK_THREADS];
    __shared__ double s_tot[2][6];         // block sums by block parity, order I_E Q_E I_P Q_P I_L Q_L
    __shared__ TrkState s_st;
    __shared__ double s_rc;                // carrier phase at the end of the current block (wave 3 -> wave 0)
    __shared__ double s_out[2][8];         // scalar outputs of a block, staged for wave 2 to store one block later
    __shared__ double s_ring[2][COH_MAX_H];   // carrNco / codeNco of the last H blocks of the pull-in (block k at k % H)
    __shared__ double s_energy[20];
    __shared__ int s_edge, s_k0;

    const int ch = blockIdx.x;
    if (ch >= Kin.n_ch) return;
    const int tid = threadIdx.x;
    if (tid == 0) {
        s_K = Kin;
        s_C = Cin;
    }
    __syncthreads();
    const TrkConst& K = s_K;
    const CohConst& C = s_C;
    const int wave = tid >> 6, lane = tid & 63;
    const TrkChan cc = chans[ch];
    const int edge0 = C.edge_in[ch];
    if (cc.prn == 0) {
        if (tid == 0) {
            C.ms_done[ch] = 0;
            C.edge_out[ch] = edge0;
            C.k0_out[ch] = -1;
        }
        if (tid < 20) C.energy[ch * 20 + tid] = 0.0;
        return;
    }
    const int T = C.T, P = C.P, H = C.H;
    const bool find = edge0 < 0;
    trk_code_table(s_code_hi, codes, cc.prn, tid, TRK_THREADS);
    if (tid == 0) {
        trk_state_start(s_st, K, cc);
        s_edge = edge0;
        s_k0 = (!find && T > 1) ? P + (((edge0 - P) % 20) + 20) % 20 : COH_K0_NONE;
    }
    __syncthreads();
    if (wave == 0) prep_carr(K, s_st.w, s_st.remCarr, (int)(cc.pos0 & 15), s_blk, lane);
    if (wave == 1) prep_code(K, s_st.codeFreq, s_st.remCode, s_st.pos, s_st, s_blk, lane == 0);
    __syncthreads();

    const long long limit = K.rec_alloc - 16;
    const long long lane_off = (long long)tid * 16;
    uint4 cur = load_group(rec, (s_blk.pos & ~15ll) + lane_off, limit);
    double* __restrict__ o = out + (long long)ch * SGX_NUM_SERIES * K.ms;
    const long long m = K.ms;
    int done = 0;
    // loop state, uniform in the wave that owns it.  wave 0: f = carrFreq, (n0, e0) the filter's memory, (rn, re) the values
    // of the latest update as the series show them, g0 / g1 the group sums of I_P / Q_P.  wave 1: the same for the code
    // loop, g0 .. g3 the group sums of I_E / Q_E / I_L / Q_L.  wave 3, lanes 0..19: the hypothesis' sum and energy.
    double f = (wave == 0) ? cc.acquiredFreq : K.code_basis;
    double n0 = 0.0, e0 = 0.0, rn = 0.0, re = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0, g3 = 0.0;
    double a_re = 0.0, a_im = 0.0, a_en = 0.0;
    for (int it = 0; it < K.ms; ++it) {
        const long long pos = s_blk.pos;
        const int blk = s_blk.blk;
        if (s_blk.stop) break;   // short read (tracking.py:159-163), or rates that are NaN
        if ((int)(pos & 15) + blk > K.n_units * TRK_UNIT) {
            // the code NCO drove the block past the units of the launch: samples would be dropped silently
            if (tid == 0) atomicExch(C.err, TRK_ERR_RANGE | (1 + ch));
            break;
        }
        const int k0 = s_k0;
        const TrkRamps R = trk_ramps(s_blk);
        const long long abase = pos & ~15ll;
        const long long abase_next = (pos + blk) & ~15ll;
        const int head = (int)(pos - abase);              // bytes of the first group before the block
        const int n_groups = (head + blk + 15) >> 4;
        TrkSums sum = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        // carrier phasor of the lane's group inside a unit: W1[tid & 15] * W2[tid >> 4]
        double lc, ls;
        {
            const double2 a = s_blk.W1[tid & 15], c2 = s_blk.W2[tid >> 4];
            lc = __builtin_fma(a.x, c2.x, -(a.y * c2.y));
            ls = __builtin_fma(a.x, c2.y, a.y * c2.x);
        }
#pragma unroll 1
        for (int u = 0; u < K.n_units; ++u) {
            // issue the load of the lane's next unit (this block's, or the first one of the next block)
            const int un = u + 1;
            const uint4 nxt = (un < K.n_units) ? load_group(rec, abase + (long long)(tid + un * TRK_THREADS) * 16, limit)
                                               : load_group(rec, abase_next + lane_off, limit);
            const int g = tid + u * TRK_THREADS;
            if (g < n_groups) {
                const int i0 = g * 16 - head;             // sample index of byte 0 of this group
                unsigned wd[4] = {cur.x, cur.y, cur.z, cur.w};
                trk_mask_group(wd, i0, blk);
                // group-start phasor G = (lane part) * W3[u]
                const double2 w3 = s_blk.W3[u];
                const double gc = __builtin_fma(lc, w3.x, -(ls * w3.y));
                const double gs = __builtin_fma(lc, w3.y, ls * w3.x);
                // (the carrier table of a group is read from LDS where it is used, and the rare route of a one-switch group
                // unrolled by four: this kernel holds its loop state in registers across the map, 256 of them)
                if (!K.multi) {
                    double xd[16];
#pragma unroll
                    for (int b = 0; b < 16; ++b) xd[b] = trk_byte(wd, b);
                    trk_map_one_switch<4>(sum, xd, s_blk.B, s_code_hi, R, i0, gc, gs);
                } else {
                    trk_map_by_sample(sum, s_blk.B, s_code_hi, R, i0, blk, gc, gs, [&](int b, int) { return trk_byte(wd, b); });
                }
            }
            cur = nxt;
        }
        sum.publish(s_red, tid);
        if (wave == 3) {
            const double rc = trk_end_phase(K, s_st.w, s_st.remCarr, blk);
            if (lane == 0) s_rc = rc;
        }
        __syncthreads();
        if (wave < 3) {
            const double acc = trk_fold(s_red, wave, lane);
            if ((lane & 31) == 0) s_tot[it & 1][2 * wave + (lane >> 5)] = acc;
        }
        __syncthreads();
        const bool more = (it + 1 < K.ms);
        const bool syncing = find && it < P;
        if (wave == 3 && syncing && lane < 20) {
            // the bit synchronisation: hypothesis h = lane adds z = I_P + j Q_P from block h on, and every 20 blocks the
            // energy of its sum
            const double zr = s_tot[it & 1][2], zi = s_tot[it & 1][3];
            if (it >= lane) {
                a_re += zr;
                a_im += zi;
                if ((it - lane) % 20 == 19) {
                    a_en += a_re * a_re + a_im * a_im;
                    a_re = a_im = 0.0;
                }
            }
            if (it == P - 1) s_energy[lane] = a_en;
        }
        if (syncing && it == P - 1) {
            // the edge: the lowest h with the largest energy; k0 follows, and block P - 1 may be the one that hands over
            __syncthreads();
            if (tid == 0) {
                int best = 0;
                for (int h = 1; h < 20; ++h)
                    if (s_energy[h] > s_energy[best]) best = h;
                s_edge = best;
                if (T > 1) s_k0 = P + (((best - P) % 20) + 20) % 20;
            }
            __syncthreads();
        }
        const int k0n = (syncing && it == P - 1) ? s_k0 : k0;
        const bool coh = it >= k0;                               // (k0 of the block's start: a group never begins at P - 1)
        const int j = coh ? (it - k0) % T : 0;
        const bool update = !coh || j == T - 1;
        const bool hand = !coh && k0n == it + 1 && more;
        const int nh = H < k0n ? H : k0n;                         // H' = min(H, k0)
        if (wave == 0) {
            // the PLL of the block's sums, or of the group's; carrier parameters of the next block
            const double I_P = s_tot[it & 1][2], Q_P = s_tot[it & 1][3];
            g0 = (coh && j > 0) ? g0 + I_P : I_P;
            g1 = (coh && j > 0) ? g1 + Q_P : Q_P;
            if (update) {
                n0 = rn = trk_pll_update(g0, g1, n0, e0, coh ? C.k_carr_a : K.k_carr_a, coh ? C.k_carr_b : K.k_carr_b, K.inv_pi, re);
                e0 = re;
                if (!coh && lane == 0) s_ring[0][it % H] = rn;
                if (hand) {
                    n0 = coh_ring_mean(s_ring[0], it, nh, H, rn);
                    e0 = 0.0;
                }
                f = s_st.carrBasis + n0;
            }
            const double w_new = (f * 2.0) * M_PI;
            const double rc = s_rc;
            if (more) prep_carr(K, w_new, rc, (int)((pos + blk) & 15), s_blk, lane);
            if (lane == 0) {
                s_st.w = w_new;
                s_st.remCarr = rc;
                s_out[it & 1][0] = f;       // T9 record (tracking.py:255-275), stored by wave 2
                s_out[it & 1][1] = re;
                s_out[it & 1][2] = rn;
            }
        } else if (wave == 1) {
            // the DLL likewise, then block size and ramps of the next block (T1, T3, T4)
            const double I_E = s_tot[it & 1][0], Q_E = s_tot[it & 1][1], I_L = s_tot[it & 1][4], Q_L = s_tot[it & 1][5];
            g0 = (coh && j > 0) ? g0 + I_E : I_E;
            g1 = (coh && j > 0) ? g1 + Q_E : Q_E;
            g2 = (coh && j > 0) ? g2 + I_L : I_L;
            g3 = (coh && j > 0) ? g3 + Q_L : Q_L;
            const long long pos_after = s_st.pos;
            const double rem_next = s_st.remCode;
            if (update) {
                n0 = rn = trk_dll_update(g0, g1, g2, g3, n0, e0, coh ? C.k_code_a : K.k_code_a, coh ? C.k_code_b : K.k_code_b, re);
                e0 = re;
                if (!coh && lane == 0) s_ring[1][it % H] = rn;
                if (hand) {
                    n0 = coh_ring_mean(s_ring[1], it, nh, H, rn);
                    e0 = 0.0;
                }
                f = K.code_basis - n0;
            }
            if (lane == 0) {
                s_out[it & 1][4] = (double)(pos_after + K.file_off);
                s_out[it & 1][5] = f;
                s_out[it & 1][6] = re;
                s_out[it & 1][7] = rn;
            }
            if (more) prep_code(K, f, rem_next, pos_after, s_st, s_blk, lane == 0);
        } else if (wave == 2) {
            // record (T9) of the PREVIOUS block: staged in LDS by the filter waves, visible since the last barrier
            if (it > 0) trk_store_row(o, m, it - 1, s_tot[(it - 1) & 1], s_out[(it - 1) & 1], lane);
        }
        done = it + 1;
        __syncthreads();   // next block's parameters visible
    }
    if (wave == 2 && done > 0) trk_store_row(o, m, done - 1, s_tot[(done - 1) & 1], s_out[(done - 1) & 1], lane);
    if (wave == 3 && lane < 20) C.energy[ch * 20 + lane] = a_en;
    if (tid == 0) {
        C.ms_done[ch] = done;
        C.edge_out[ch] = s_edge;
        C.k0_out[ch] = s_k0 == COH_K0_NONE ? -1 : s_k0;
    }
}

// ---- the host side -------------------------------------------------------------------------------------------------------

static int coh_check(const sgx_ctx* c, const sgx_chan_init* ch, int n_ch, int ms, const sgx_coh_params* p, const int32_t* edge) {
    const int T = p->coherent_ms;
    if (!(T == 1 || T == 2 || T == 4 || T == 5 || T == 10 || T == 20)) {
        sgx_set_error("sgx_track_coherent: coherent_ms %d is not one of 1, 2, 4, 5, 10, 20", T);
        return SGX_E_ARG;
    }
    bool find = false;
    for (int i = 0; i < n_ch; ++i) {
        if (edge[i] < -1 || edge[i] > 19) {
            sgx_set_error("sgx_track_coherent: bit edge %d of channel %d outside -1 .. 19", (int)edge[i], i);
            return SGX_E_ARG;
        }
        find = find || (edge[i] == -1 && ch[i].prn != 0);
    }
    if (p->pull_in_ms < 40 || (find && p->pull_in_ms < 220) || p->pull_in_ms > ms) {
        sgx_set_error("sgx_track_coherent: pull_in_ms %d outside %d .. ms = %d (40 blocks settle the 1 ms loops; finding a bit "
                      "edge takes 220)", (int)p->pull_in_ms, find ? 220 : 40, ms);
        return SGX_E_ARG;
    }
    if (p->handover_ms < 1 || p->handover_ms > COH_MAX_H) {
        sgx_set_error("sgx_track_coherent: handover_ms %d outside 1 .. %d", (int)p->handover_ms, COH_MAX_H);
        return SGX_E_ARG;
    }
    if (!(p->tau1_pll > 0.0 && p->tau2_pll > 0.0 && p->tau1_dll > 0.0 && p->tau2_dll > 0.0)) {
        sgx_set_error("sgx_track_coherent: the coherent loops' coefficients must be positive (sgx_calc_loop_coef)");
        return SGX_E_ARG;
    }
    if (!(c->s.dllCorrelatorSpacing > 0.0 && c->s.dllCorrelatorSpacing < 1.0)) {
        sgx_set_error("dllCorrelatorSpacing %g outside (0, 1) chips", c->s.dllCorrelatorSpacing);
        return SGX_E_ARG;
    }
    return SGX_OK;
}

// The stages of sgx_track's call (sgx_trk.hip, declared in sgx_trk_common.h) for an int8 record and one workgroup per
// channel; this call's own: the coherent loops' constants, the results beside the series, and one launch that is never repeated
extern "C" int sgx_track_coherent(sgx_ctx* c, const sgx_if* r, int64_t rec_file_offset, const sgx_chan_init* ch, int32_t n_ch,
                                  int32_t ms, const sgx_coh_params* p, const int32_t* bit_edge_in, double* out,
                                  int32_t* ms_done, int32_t* bit_edge, int32_t* coh_start, double* edge_energy) {
    SGX_CHECK_ARG(c && r && ch && p && bit_edge_in && out && ms_done && bit_edge && coh_start && edge_energy);
    SGX_CHECK_ARG(n_ch >= 1 && n_ch <= 65535 && ms >= 1);
    int rc = coh_check(c, ch, n_ch, ms, p, bit_edge_in);
    if (rc != SGX_OK) return rc;
    TrkConst K;
    sgx_trk_const(K, c->s, (long long)c->n_code, (long long)r->n, SGX_DT_INT8, (long long)rec_file_offset, ms, n_ch, sgx_trk_multi(c->s));
    K.split = 1;
    K.n_units = sgx_trk_units((long long)c->n_code);
    CohConst C;
    const double pdi = (double)p->coherent_ms * 0.001;
    C.k_code_a = p->tau2_dll / p->tau1_dll;
    C.k_code_b = pdi / p->tau1_dll;
    C.k_carr_a = p->tau2_pll / p->tau1_pll;
    C.k_carr_b = pdi / p->tau1_pll;
    C.T = p->coherent_ms;
    C.P = p->pull_in_ms;
    C.H = p->handover_ms;
    rc = sgx_trk_units_check((long long)c->n_code, K.n_units);
    if (rc != SGX_OK) return rc;
    std::vector<TrkChan> hc;
    rc = sgx_trk_channels(hc, ch, n_ch, (long long)c->s.skipNumberOfBytes, (long long)rec_file_offset, 1);
    if (rc != SGX_OK) return rc;
    SGX_HIP(hipSetDevice(c->device));
    rc = sgx_if_require(r, r->n);   // the kernel follows no watermark
    if (rc != SGX_OK) return rc;
    // device state of the call: the series (staged), then [channels | done | err | edge in | edge | k0 | energies]
    const size_t elems = (size_t)n_ch * SGX_NUM_SERIES * (size_t)ms;
    rc = c->d_trk_out.ensure(elems * sizeof(double));
    if (rc != SGX_OK) return rc;
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t sz_ch = up(sizeof(TrkChan) * (size_t)n_ch), sz_i = up(sizeof(int) * (size_t)n_ch);
    const size_t sz_en = up(sizeof(double) * 20 * (size_t)n_ch);
    rc = c->d_trk_aux.ensure(sz_ch + 4 * sz_i + 256 + sz_en);
    if (rc != SGX_OK) return rc;
    char* aux = c->d_trk_aux;
    TrkChan* d_ch = (TrkChan*)aux;
    int* d_done = (int*)(aux + sz_ch);
    int* d_err = (int*)(aux + sz_ch + sz_i);
    int* d_edge_in = (int*)(aux + sz_ch + sz_i + 256);
    int* d_edge = (int*)(aux + sz_ch + 2 * sz_i + 256);
    int* d_k0 = (int*)(aux + sz_ch + 3 * sz_i + 256);
    double* d_en = (double*)(aux + sz_ch + 4 * sz_i + 256);
    double* d_out = c->d_trk_out;
    hipStream_t st = c->stream;
    SGX_HIP(hipMemcpyAsync(d_ch, hc.data(), sizeof(TrkChan) * (size_t)n_ch, hipMemcpyHostToDevice, st));
    SGX_HIP(hipMemsetAsync(d_done, 0, sz_i + 256, st));   // done, err
    SGX_HIP(hipMemcpyAsync(d_edge_in, bit_edge_in, sizeof(int) * (size_t)n_ch, hipMemcpyHostToDevice, st));
    sgx_trk_fill(d_out, ms, elems, st);
    hipEventRecord(c->ev[3], st);
    C.edge_in = d_edge_in;
    C.edge_out = d_edge;
    C.k0_out = d_k0;
    C.ms_done = d_done;
    C.err = d_err;
    C.energy = d_en;
    trk_kernel_coh<<<n_ch, TRK_THREADS, 0, st>>>(r->d, c->d_codes, d_ch, d_out, K, C);
    hipEventRecord(c->ev[4], st);
    hipError_t e = hipGetLastError();
    int h_err = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, elems * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(ms_done, d_done, sizeof(int) * (size_t)n_ch, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(bit_edge, d_edge, sizeof(int) * (size_t)n_ch, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(coh_start, d_k0, sizeof(int) * (size_t)n_ch, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(edge_energy, d_en, sizeof(double) * 20 * (size_t)n_ch, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&h_err, d_err, sizeof(int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        sgx_set_error("coherent tracking kernel failed: %s", hipGetErrorString(e));
        return SGX_E_HIP;
    }
    hipEventElapsedTime(&c->timing.track_ms, c->ev[3], c->ev[4]);
    c->timing.track_kernel = 7.f;
    c->timing.track_members = 1.f;
    c->timing.track_streamed = 0.f;
    // why a channel ended early (a silent one: NaN rates behind an update whose sums - a group's, from k0 on - are exactly zero)
    const int range_ch1 = (h_err & TRK_ERR_RANGE) ? (h_err & 0xFFFF) : 0;   // (the kernel's word: the flag | 1 + channel)
    return sgx_trk_diagnose(ch, nullptr, n_ch, ms, out, ms_done, "the update behind its block", range_ch1, K.n_units,
                            c->s.dllNoiseBandwidth);
}
