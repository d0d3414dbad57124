// Body of the per-sample cooperative tracking kernel (the round-1 kernel body: map / reduce / exchange / filter with two
// barriers per block).  Every sample looks its replicas up (tracking.py:166-188).  Two instances:
//   sgx_trk_multi.hip  <false> int8 records at low sampling rates (fewer than ~15.4 samples per chip), 16-byte groups;
//   sgx_trk_any.hip    <true>  any sample type numpy reads (K.kind), each sample fetched where it lies: float32 /
//                      float64 records of arbitrary values, the wider integers, and int16 / uint8 at low rates.
// The pieces that work on one workgroup's view of a block - code table, maps, fold, filters, record - are those of
// sgx_trk_block.h, shared with the coherent kernel; what is this body's own is the members of a channel: placement check,
// granule exchange, abort, and the profile and its probes.
#pragma once
#include "sgx_trk_block.h"

// (static: an instance's LDS variables then have internal linkage, like those a kernel declares itself)
template <bool ANY>
static __device__ __forceinline__ void trk_persample_body(const int8_t* __restrict__ rec, const int8_t* __restrict__ codes,
                                                          const TrkChan* __restrict__ chans, double* __restrict__ out,
                                                          int* __restrict__ ms_done, const TrkConst& K,
                                                          long long* __restrict__ prof, unsigned long long* __restrict__ xch,
                                                          int* __restrict__ err) {
    __shared__ unsigned s_code_hi[1028];   // hi dword of +-1.0 for [c1022, c0..c1022, c0] (tracking.py:111)
    __shared__ TrkBlock s_blk;
    __shared__ double s_red[6][TRK_THREADS];
    __shared__ double s_tot[2][6];         // block sums by block parity, order I_E Q_E I_P Q_P I_L Q_L
    __shared__ TrkState s_st;
    __shared__ double s_rc;                // carrier phase at the end of the current block (wave 3 -> wave 0)
    __shared__ double s_out[2][8];         // scalar outputs of a block, staged for wave 2 to store one block later
    __shared__ int s_abort;                // a cooperating workgroup of this launch timed out: leave the block loop

    // optional phase profile (SGX_TRK_PROFILE=1): shader cycles of lane 0 in map / wait / reduce / filter
    long long pf_map = 0, pf_wait = 0, pf_red = 0, pf_flt = 0;
#ifdef TRK_FINEPROF
    long long fp[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    long long fp_last = 0;
#endif

    // block -> (channel, member): members of a channel share blockIdx % 8, i.e. (observed) one XCD / one L2;
    // placement only affects speed, the exchange below is agent-scope and placement independent
    const int P = K.split;
    const int bq = blockIdx.x >> 3, br = blockIdx.x & 7;
    const int ch = br + 8 * (bq / P);
    const int member = bq % P;
    if (ch >= K.n_ch) return;
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const TrkChan cc = chans[ch];
    if (cc.prn == 0) {
        if (tid == 0 && member == 0) ms_done[ch] = 0;
        return;
    }
    // ANY: K.rec_len is in bytes: this channel's sample grid starts at byte cc.pad of the record (tracking.py:107 seeks bytes)
    const int any_sb = ANY ? sgx_dt_bytes(K.kind) : 1;
    const int8_t* __restrict__ const recc = rec + (ANY ? cc.pad : 0);
    const long long rec_len = ANY ? (K.rec_len - cc.pad) / any_sb : -1;   // in samples (-1: K.rec_len, see prep_code)
    if (tid == 0) s_abort = 0;
    __syncthreads();
    // exchange area of the channel: [2 epoch parities][TRK_MAX_SPLIT members][12 granules], then one
    // placement granule per member
    unsigned long long* __restrict__ xbase = xch + (long long)ch * (2 * TRK_MAX_SPLIT * 12 + 16);
    bool fast = false;
    if (P > 1) {
        // placement check through the placement-independent path: all members on one XCD?
        unsigned long long* pl = xbase + 2 * TRK_MAX_SPLIT * 12;
        const unsigned me = xcc_id();
        if (tid == 0) __hip_atomic_store(pl + member, 0xC0DE000000000000ull | me, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        bool same = true;
        if (wave == 0) {
            unsigned long long x = 0;
            int budget = 1 << 20;
            for (;;) {
                if (lane < P) x = __hip_atomic_load(pl + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const bool ok = lane >= P || (x >> 48) == 0xC0DE;
                if (__all(ok)) break;
                if (--budget == 0) {   // a member is not resident: give the launch up (see the gather below)
                    if (lane == 0) {
                        atomicCAS(err, 0, 1 + ch);
                        s_abort = 1;
                    }
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
            same = __all(lane >= P || (unsigned)(x & 0xF) == me);
            if (lane == 0) s_tot[0][0] = same ? 1.0 : 0.0;
        }
        __syncthreads();
        fast = (s_tot[0][0] != 0.0) && (K.fast_xcd != 0);
        __syncthreads();
    }
    trk_code_table(s_code_hi, codes, cc.prn, tid, TRK_THREADS);
    if (tid == 0) trk_state_start(s_st, K, cc);
    __syncthreads();
    if (wave == 0) prep_carr(K, s_st.w, s_st.remCarr, (int)(cc.pos0 & 15), s_blk, lane);
    if (wave == 1) prep_code(K, s_st.codeFreq, s_st.remCode, s_st.pos, s_st, s_blk, lane == 0, rec_len);
    __syncthreads();

    const long long limit = K.rec_alloc - 16;
    const long long lane_off = (long long)(tid + member * TRK_THREADS) * 16;   // byte offset of the lane's first unit
    uint4 cur = make_uint4(0u, 0u, 0u, 0u);                                    // (16-byte groups: the int8 instance only)
    if constexpr (!ANY) cur = load_group(rec, (s_blk.pos & ~15ll) + lane_off, limit);
    double* __restrict__ o = out + (long long)ch * SGX_NUM_SERIES * K.ms;
    int done = 0;
    for (int it = 0; it < K.ms; ++it) {
        const long long tk0 = prof ? (long long)__builtin_amdgcn_s_memtime() : 0;
#ifdef TRK_FINEPROF
        fp_last = (long long)__builtin_amdgcn_s_memtime();
#endif
        const long long pos = s_blk.pos;
        const int blk = s_blk.blk;
        if (s_blk.stop) break;   // short read: tracking.py:159-163
        if (s_abort) {           // a cooperating workgroup timed out somewhere in this launch: the last block's sums are void
            done = done > 0 ? done - 1 : 0;
            break;
        }
        if ((int)(pos & 15) + blk > K.n_units * TRK_UNIT) {
            // the code NCO drove the block past the units of the launch: samples would be dropped silently
            if (tid == 0) atomicExch(err, TRK_ERR_RANGE | (1 + ch));
            break;
        }
        const TrkRamps R = trk_ramps(s_blk);
        double2 B[16];
#pragma unroll
        for (int b = 0; b < 16; ++b) B[b] = s_blk.B[b];

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
        for (int u = member; u < K.n_units; u += P) {
            // issue the load of the lane's next unit (this block's, or the first one of the next block)
            const int un = u + P;
            const uint4 nxt = ANY ? cur
                            : (un < K.n_units) ? load_group(rec, abase + (long long)(tid + un * TRK_THREADS) * 16, limit)
                                               : load_group(rec, abase_next + lane_off, limit);
            const int g = tid + u * TRK_THREADS;
            PROBE(0);   // block parameters, B table, lane phasor, next-unit load issued, current unit landed
            if (g < n_groups) {
                const int i0 = g * 16 - head;             // sample index of byte 0 of this group
                unsigned wd[4] = {cur.x, cur.y, cur.z, cur.w};
                if constexpr (!ANY) trk_mask_group(wd, i0, blk);
                // group-start phasor G = (lane part) * W3[u]
                const double2 w3 = s_blk.W3[u];
                const double gc = __builtin_fma(lc, w3.x, -(ls * w3.y));
                const double gs = __builtin_fma(lc, w3.y, ls * w3.x);
                if (ANY && !K.multi) {
                    // (trk_kernel_any above ~15.4 samples per chip; the carrier table from its register copy)
                    double xd[16];
                    any_group(recc + (pos + i0) * any_sb, K.kind, i0, blk, xd);
                    trk_map_one_switch<16>(sum, xd, B, s_code_hi, R, i0, gc, gs);
                } else {
                    // (low sampling rates: trk_kernel_multi always, its own kernel for them, and trk_kernel_any below the bound)
                    trk_map_by_sample(sum, s_blk.B, s_code_hi, R, i0, blk, gc, gs, [&](int b, int i) {
                        return ANY ? any_sample(recc + (pos + i) * any_sb, K.kind) : trk_byte(wd, b);
                    });
                }
            }
            cur = nxt;
            PROBE(4);   // group finalisation
        }
        const long long tk1 = prof ? (long long)__builtin_amdgcn_s_memtime() : 0;
        sum.publish(s_red, tid);
        // carrier phase at the end of this block (T5) does not need the sums: the otherwise idle wave 3
        // computes it.  remCarrPhase = trigarg[blk] % (2 pi), trigarg = w*(blk/fs) + rem; exact remainder by FMA
        if (wave == 3) {
            const double rc = trk_end_phase(K, s_st.w, s_st.remCarr, blk);
            if (lane == 0) s_rc = rc;
        }
        PROBE(5);   // partials to LDS, end-of-block carrier phase
        __syncthreads();
        PROBE(6);   // barrier 1 (waits for the slowest wave)
        const long long tk2 = prof ? (long long)__builtin_amdgcn_s_memtime() : 0;
        if (wave < 3) {
            // wave w folds values 2w (lanes 0..31) and 2w+1 (lanes 32..63)
            const int v = 2 * wave + (lane >> 5), l = lane & 31;
            const double acc = trk_fold(s_red, wave, lane);
            PROBE(7);   // local fold
            if (P == 1) {
                if (l == 0) s_tot[it & 1][v] = acc;
            } else if (l == 0) {
                // publish this member's partial as two {epoch, 32-bit payload} granules: ONE aligned 8-byte
                // store each, so a reader never sees a torn granule (Guideline 16, R2)
                const unsigned long long tag = (unsigned long long)(unsigned)(it + 1) << 32;
                unsigned long long* gp = xbase + ((it & 1) * TRK_MAX_SPLIT + member) * 12 + 2 * v;
                granule_store(gp, tag | (unsigned)__double2loint(acc), fast);
                granule_store(gp + 1, tag | (unsigned)__double2hiint(acc), fast);
            }
        }
        // totals of the six sums, uniform in the wave that needs them:
        //   wave 0 (PLL): tA = I_P, tB = Q_P;  wave 1 (DLL): tA = I_E, tB = Q_E, tC = I_L, tD = Q_L
        double tA = 0.0, tB = 0.0, tC = 0.0, tD = 0.0;
        if (P > 1 && wave < 2) {
            // each filter wave gathers exactly the values it needs from every member's granules (relaxed,
            // L1-bypassing polls, bounded) and goes straight into its filter: no LDS round trip, no barrier.
            // lane = 16*row + c reads member c's value val(row); same layout and order in every member.
            const unsigned epoch = (unsigned)(it + 1);
            const int row = lane >> 4, c = lane & 15;
            const int val = (wave == 0) ? 2 + row : (row < 2 ? row : row + 2);
            const bool mine = c < P && (wave == 1 || row < 2);
            const unsigned long long* gp = xbase + ((it & 1) * TRK_MAX_SPLIT + c) * 12 + 2 * val;
            unsigned long long a0 = 0, a1 = 0;
            // A member that does not show up within the budget flags the launch in `err`; every workgroup of the launch
            // looks at that word every 64 polls and leaves its block loop at the next barrier, so the whole launch is over
            // within one budget and the host repeats it with one workgroup per channel (sgx_trk.hip) - nobody spins
            // through the remaining blocks on sums that will never arrive.
            int budget = 1 << 20;
            for (;;) {
                if (mine) {
                    a0 = __hip_atomic_load(gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    a1 = __hip_atomic_load(gp + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                const bool ok = !mine || ((unsigned)(a0 >> 32) == epoch && (unsigned)(a1 >> 32) == epoch);
                if (__all(ok)) break;
                if ((--budget & 63) == 0) {
                    const int seen = __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & ~TRK_ERR_STREAM;
                    if (budget == 0 || seen != 0) {
                        if (lane == 0) {
                            if (seen == 0) atomicCAS(err, 0, 1 + ch);
                            s_abort = 1;
                        }
                        break;
                    }
                }
                __builtin_amdgcn_s_sleep(1);
            }
            PROBE(8);   // gather (includes waiting for the slowest member)
            const double d = mine ? __hiloint2double((int)(unsigned)a1, (int)(unsigned)a0) : 0.0;
            const double sr = row_sum(d);   // every lane of a row holds the row's total
            const int lo = __double2loint(sr), hi = __double2hiint(sr);
            tA = __hiloint2double(__builtin_amdgcn_readlane(hi, 0), __builtin_amdgcn_readlane(lo, 0));
            tB = __hiloint2double(__builtin_amdgcn_readlane(hi, 16), __builtin_amdgcn_readlane(lo, 16));
            tC = __hiloint2double(__builtin_amdgcn_readlane(hi, 32), __builtin_amdgcn_readlane(lo, 32));
            tD = __hiloint2double(__builtin_amdgcn_readlane(hi, 48), __builtin_amdgcn_readlane(lo, 48));
            if (c == 0 && mine && member == 0) s_tot[it & 1][val] = sr;   // for the record stores (wave 2, next block)
        }
        PROBE(9);   // totals
        if (P == 1) {
            __syncthreads();
            if (wave == 0) {
                tA = s_tot[it & 1][2];
                tB = s_tot[it & 1][3];
            } else if (wave == 1) {
                tA = s_tot[it & 1][0];
                tB = s_tot[it & 1][1];
                tC = s_tot[it & 1][4];
                tD = s_tot[it & 1][5];
            }
        }
        PROBE(10);  // barrier 2 (single-member mode only)
        const long long tk3 = prof ? (long long)__builtin_amdgcn_s_memtime() : 0;
        const bool more = (it + 1 < K.ms);
        if (wave == 0) {
            // T7 PLL (tracking.py:223-235); carrier parameters of the next block
            double carrError;
            const double carrNco = trk_pll_update(tA, tB, s_st.oldCarrNco, s_st.oldCarrErr, K.k_carr_a, K.k_carr_b, K.inv_pi, carrError);
            const double carrFreq = s_st.carrBasis + carrNco;
            const double w_new = (carrFreq * 2.0) * M_PI;
            const double rc = s_rc;
            if (more) prep_carr(K, w_new, rc, (int)((pos + blk) & 15), s_blk, lane);
            if (lane == 0) {
                s_st.w = w_new;
                s_st.remCarr = rc;
                s_st.oldCarrNco = carrNco;
                s_st.oldCarrErr = carrError;
                s_st.carrFreq = carrFreq;
            }
            if (lane == 0 && member == 0) {
                s_out[it & 1][0] = carrFreq;       // T9 record (tracking.py:255-275), stored by wave 2
                s_out[it & 1][1] = carrError;
                s_out[it & 1][2] = carrNco;
            }
        } else if (wave == 1) {
            // T8 DLL (tracking.py:238-251), then block size and ramps of the next block (T1, T3, T4)
            const long long pos_after = s_st.pos;
            const double rem_next = s_st.remCode;
            double codeError;
            const double codeNco = trk_dll_update(tA, tB, tC, tD, s_st.oldCodeNco, s_st.oldCodeErr, K.k_code_a, K.k_code_b, codeError);
            const double codeFreq = K.code_basis - codeNco;
            if (lane == 0) {
                s_st.oldCodeNco = codeNco;
                s_st.oldCodeErr = codeError;
                s_st.codeFreq = codeFreq;
            }
            if (lane == 0 && member == 0) {
                if constexpr (ANY) s_out[it & 1][4] = (double)(pos_after * any_sb + cc.pad + K.file_off);   // fid.tell(): bytes (tracking.py:255)
                else s_out[it & 1][4] = (double)(pos_after + K.file_off);
                s_out[it & 1][5] = codeFreq;
                s_out[it & 1][6] = codeError;
                s_out[it & 1][7] = codeNco;
            }
            if (more) prep_code(K, codeFreq, rem_next, pos_after, s_st, s_blk, lane == 0, rec_len);
        }
        else if (wave == 2 && member == 0) {
            // record (T9) of the PREVIOUS block: its six sums and scalar series were staged in LDS by the
            // filter waves and are visible since the last barrier - off the critical path
            if (it > 0) trk_store_row(o, K.ms, it - 1, s_tot[(it - 1) & 1], s_out[(it - 1) & 1], lane);
        }
        done = it + 1;
        PROBE(11);  // loop filter (this wave's side) + next block's parameters
        __syncthreads();   // next block's parameters visible
        PROBE(12);  // barrier 3 (waits for the other filter wave)
        if (prof && tid == 0) {
            const long long tk4 = (long long)__builtin_amdgcn_s_memtime();
            pf_map += tk1 - tk0;
            pf_wait += tk2 - tk1;
            pf_red += tk3 - tk2;
            pf_flt += tk4 - tk3;
        }
    }
    if (tid == 0 && prof && member == 0) {
        prof[ch * 64 + 0] = pf_map;
        prof[ch * 64 + 1] = pf_wait;
        prof[ch * 64 + 2] = pf_red;
        prof[ch * 64 + 3] = pf_flt;
    }
    if (wave == 2 && member == 0 && done > 0) trk_store_row(o, K.ms, done - 1, s_tot[(done - 1) & 1], s_out[(done - 1) & 1], lane);
#ifdef TRK_FINEPROF
    if (tid == 0 && prof && member == 0 && ch == 0) {
        for (int k = 0; k < 13; ++k) printf("[fineprof] probe %2d: %8.1f cycles/block\n", k, (double)fp[k] / K.ms);
    }
#endif
    if (tid == 0 && member == 0) ms_done[ch] = done;
}
