// Bit-aligned coherent tracking of weak signals (include/sgx.h: sgx_track_coherent; the contract in numpy is
// tests/coh_track_spec.py): the kernel and its host side.
//
// Every block is the reference's block (tracking.py:148-219), mapped, reduced and recorded as the per-sample body does
// (sgx_trk_persample.h with one member per channel); only WHEN the two loop filters run changes.  Blocks k < k0 are updated
// one by one (the reference); at the end of block k0 - 1 both filters restart from the mean of their last H NCO values; from
// k0 on the sums of T blocks are added and the filters run once per group with PDI = T ms, the rates held in between.
// k0 sits on a navigation-bit edge, given or found by the 20 hypotheses of the bit synchronisation during the pull-in.
//
// ONE workgroup per channel and no exchange between workgroups: nothing in this kernel polls memory another workgroup
// writes, so no wait can fail to end and no launch is repeated.  Four waves:
//   every lane   maps the block's groups of 16 samples (sample by sample below ~15.4 samples per chip, one chip switch per
//                ramp and group above), six partial sums -> s_red
//   wave 0       folds I_E / Q_E; PLL side: group sums of I_P / Q_P, discriminator, filter, hand-over, next block's phasors
//   wave 1       folds I_P / Q_P; DLL side: group sums of the early and late arms, discriminator, filter, hand-over, next ramps
//   wave 2       folds I_L / Q_L; stores the previous block's row
//   wave 3       the carrier phase at the block's end; lanes 0..19 the 20 bit-synchronisation hypotheses
#include "sgx_trk_common.h"

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

__global__ __launch_bounds__(256) void coh_fill_kernel(double* __restrict__ out, long long ms, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int series = (int)((i / ms) % SGX_NUM_SERIES);
    const bool zero = (series == 0) || (series >= 3 && series <= 8);   // tracking.py:65-94
    out[i] = zero ? 0.0 : __longlong_as_double(0x7FF0000000000000ll);
}

__global__ __launch_bounds__(TRK_THREADS, 1) void trk_kernel_coh(const int8_t* __restrict__ rec, const int8_t* __restrict__ codes,
    const TrkChan* __restrict__ chans, double* __restrict__ out, const TrkConst Kin, const CohConst Cin) {
    // The call's constants live in LDS, not in scalar registers: the filter waves read a field when they need it (a
    // broadcast read), and nothing is held across the map - with them as kernel arguments 54 scalars were kept in vector lanes
    __shared__ TrkConst s_K;
    __shared__ CohConst s_C;
    __shared__ unsigned s_code_hi[1028];   // hi dword of +-1.0 for [c1022, c0..c1022, c0] (tracking.py:111)
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
    for (int i = tid; i < 1028; i += TRK_THREADS) {
        int j = i - 1;
        if (j < 0) j = 1022;
        if (j >= 1023) j -= 1023;
        if (j >= 1023) j -= 1023;
        s_code_hi[i] = (codes[(cc.prn - 1) * 1023 + j] > 0) ? 0x3FF00000u : 0xBFF00000u;
    }
    if (tid == 0) {   // tracking.py:114-130
        s_st.codeFreq = K.code_basis;
        s_st.remCode = 0.0;
        s_st.oldCodeNco = s_st.oldCodeErr = 0.0;
        s_st.pos = cc.pos0;
        s_st.carrFreq = cc.acquiredFreq;
        s_st.carrBasis = cc.acquiredFreq;
        s_st.remCarr = 0.0;
        s_st.w = (cc.acquiredFreq * 2.0) * M_PI;
        s_st.oldCarrNco = s_st.oldCarrErr = 0.0;
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
    const double two_pi = 2 * M_PI;
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
        const double startE = s_blk.startE, stepE = s_blk.stepE;
        const double startP = s_blk.startP, stepP = s_blk.stepP;
        const double startL = s_blk.startL, stepL = s_blk.stepL;
        const double inv_step = s_blk.inv_step;
        const long long abase = pos & ~15ll;
        const long long abase_next = (pos + blk) & ~15ll;
        const int head = (int)(pos - abase);              // bytes of the first group before the block
        const int n_groups = (head + blk + 15) >> 4;
        double aIE = 0.0, aQE = 0.0, aIP = 0.0, aQP = 0.0, aIL = 0.0, aQL = 0.0;
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
                if (i0 < 0 || i0 + 16 > blk) {
                    // zero the bytes outside [0, blk): they then add nothing to the sums
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                        int lo = -(i0 + 4 * d);
                        lo = lo < 0 ? 0 : (lo > 4 ? 4 : lo);
                        int hi = i0 + 4 * d + 4 - blk;
                        hi = hi < 0 ? 0 : (hi > 4 ? 4 : hi);
                        unsigned mk = (lo >= 4) ? 0u : (0xFFFFFFFFu << (8 * lo));
                        mk &= (hi >= 4) ? 0u : (0xFFFFFFFFu >> (8 * hi));
                        wd[d] &= mk;
                    }
                }
                // group-start phasor G = (lane part) * W3[u]
                const double2 w3 = s_blk.W3[u];
                const double gc = __builtin_fma(lc, w3.x, -(ls * w3.y));
                const double gs = __builtin_fma(lc, w3.y, ls * w3.x);
                if (!K.multi) {
                    // 16 samples span less than a chip, so a group meets at most one switch of a ramp: each ramp's index and
                    // switch sample at the group's first sample by the exact reference arithmetic (ramp_setup), then the
                    // group as a sum over all its samples plus a sum over those behind the switch - where the ramps that
                    // switch inside the group do so at ONE sample (always, at >= 16 samples per half chip and spacing 1/2);
                    // the samples one by one with the switches as compares otherwise (sgx_trk_persample.h shows the route)
                    double xd[16];
#pragma unroll
                    for (int b = 0; b < 16; ++b) xd[b] = (double)(int)(signed char)((wd[b >> 2] >> (8 * (b & 3))) & 0xFF);
                    const int ilo = i0 < 0 ? 0 : i0;
                    int kE, swE, kP, swP, kL, swL;
                    ramp_setup(startE, stepE, inv_step, ilo, kE, swE);
                    ramp_setup(startP, stepP, inv_step, ilo, kP, swP);
                    ramp_setup(startL, stepL, inv_step, ilo, kL, swL);
                    const double cE1 = __hiloint2double((int)s_code_hi[kE], 0), cE2 = __hiloint2double((int)s_code_hi[kE + 1], 0);
                    const double cP1 = __hiloint2double((int)s_code_hi[kP], 0), cP2 = __hiloint2double((int)s_code_hi[kP + 1], 0);
                    const double cL1 = __hiloint2double((int)s_code_hi[kL], 0), cL2 = __hiloint2double((int)s_code_hi[kL + 1], 0);
                    const int iend = i0 + 16;
                    int swmin = swE < swP ? swE : swP;
                    swmin = swL < swmin ? swL : swmin;
                    const bool eS = (swE == swmin), pS = (swP == swmin), lS = (swL == swmin);
                    const bool odd = (swE < iend && !eS) || (swP < iend && !pS) || (swL < iend && !lS);
                    if (__any(odd)) {
#pragma unroll 4
                        for (int b = 0; b < 16; ++b) {
                            const int i = i0 + b;
                            const double2 Bb = s_blk.B[b];
                            const double c = __builtin_fma(gc, Bb.x, -(gs * Bb.y));
                            const double sn = __builtin_fma(gs, Bb.x, gc * Bb.y);
                            const double xs = sn * xd[b], xc = c * xd[b];
                            const double cE = i >= swE ? cE2 : cE1;
                            const double cP = i >= swP ? cP2 : cP1;
                            const double cL = i >= swL ? cL2 : cL1;
                            aIE = __builtin_fma(cE, xs, aIE);
                            aQE = __builtin_fma(cE, xc, aQE);
                            aIP = __builtin_fma(cP, xs, aIP);
                            aQP = __builtin_fma(cP, xc, aQP);
                            aIL = __builtin_fma(cL, xs, aIL);
                            aQL = __builtin_fma(cL, xc, aQL);
                        }
                    } else {
                        const int bsw = swmin - i0;           // samples b >= bsw come after the switch
                        double Ac = 0.0, As = 0.0, Tc = 0.0, Ts = 0.0;
#pragma unroll
                        for (int b = 0; b < 16; ++b) {
                            const double2 Bb = s_blk.B[b];
                            Ac = __builtin_fma(xd[b], Bb.x, Ac);
                            As = __builtin_fma(xd[b], Bb.y, As);
                            const double xt = (b >= bsw) ? xd[b] : 0.0;
                            Tc = __builtin_fma(xt, Bb.x, Tc);
                            Ts = __builtin_fma(xt, Bb.y, Ts);
                        }
                        // rotate by the group phasor: cos part -> Q, sin part -> I (tracking.py:205-207)
                        const double allQ = __builtin_fma(gc, Ac, -(gs * As));
                        const double allI = __builtin_fma(gs, Ac, gc * As);
                        const double tlQ = __builtin_fma(gc, Tc, -(gs * Ts));
                        const double tlI = __builtin_fma(gs, Tc, gc * Ts);
                        const double dE = eS ? (cE2 - cE1) : 0.0;
                        const double dP = pS ? (cP2 - cP1) : 0.0;
                        const double dL = lS ? (cL2 - cL1) : 0.0;
                        aIE = __builtin_fma(dE, tlI, __builtin_fma(cE1, allI, aIE));
                        aQE = __builtin_fma(dE, tlQ, __builtin_fma(cE1, allQ, aQE));
                        aIP = __builtin_fma(dP, tlI, __builtin_fma(cP1, allI, aIP));
                        aQP = __builtin_fma(dP, tlQ, __builtin_fma(cP1, allQ, aQP));
                        aIL = __builtin_fma(dL, tlI, __builtin_fma(cL1, allI, aIL));
                        aQL = __builtin_fma(dL, tlQ, __builtin_fma(cL1, allQ, aQL));
                    }
                } else {
                    // under ~15.4 samples per chip a group can hold several chip switches of a ramp: the replicas are
                    // indexed sample by sample as the reference does, code[ceil(linspace(...))] (tracking.py:166-188)
#pragma unroll 1
                    for (int b = 0; b < 16; ++b) {
                        const int i = i0 + b;
                        if (i < 0 || i >= blk) continue;
                        const double xd = (double)(int)(signed char)((wd[b >> 2] >> (8 * (b & 3))) & 0xFF);
                        const double2 Bb = s_blk.B[b];
                        const double c = __builtin_fma(gc, Bb.x, -(gs * Bb.y));
                        const double sn = __builtin_fma(gs, Bb.x, gc * Bb.y);
                        const double xs = sn * xd, xc = c * xd;
                        const double cE = __hiloint2double((int)s_code_hi[(int)ceil(ramp_at(i, stepE, startE))], 0);
                        const double cP = __hiloint2double((int)s_code_hi[(int)ceil(ramp_at(i, stepP, startP))], 0);
                        const double cL = __hiloint2double((int)s_code_hi[(int)ceil(ramp_at(i, stepL, startL))], 0);
                        aIE = __builtin_fma(cE, xs, aIE);
                        aQE = __builtin_fma(cE, xc, aQE);
                        aIP = __builtin_fma(cP, xs, aIP);
                        aQP = __builtin_fma(cP, xc, aQP);
                        aIL = __builtin_fma(cL, xs, aIL);
                        aQL = __builtin_fma(cL, xc, aQL);
                    }
                }
            }
            cur = nxt;
        }
        s_red[0][tid] = aIE;
        s_red[1][tid] = aQE;
        s_red[2][tid] = aIP;
        s_red[3][tid] = aQP;
        s_red[4][tid] = aIL;
        s_red[5][tid] = aQL;
        // carrier phase at the end of this block (T5) does not need the sums: remCarrPhase = trigarg[blk] % (2 pi)
        if (wave == 3) {
            const double arg_end = s_st.w * ((double)blk / K.fs) + s_st.remCarr;
            const double kq = floor(arg_end * K.inv_2pi);
            double rc = __builtin_fma(-kq, two_pi, arg_end);
            if (rc < 0.0) rc += two_pi;
            if (rc >= two_pi) rc -= two_pi;
            if (lane == 0) s_rc = rc;
        }
        __syncthreads();
        if (wave < 3) {
            // wave w folds values 2w (lanes 0..31) and 2w+1 (lanes 32..63): 8 partials per lane (consecutive lanes read
            // consecutive 8-byte words: no bank conflict), then DPP
            const int v = 2 * wave + (lane >> 5), l = lane & 31;
            double acc = s_red[v][l];
#pragma unroll
            for (int k = 1; k < TRK_THREADS / 32; ++k) acc += s_red[v][l + 32 * k];
            acc = half_wave_sum(acc, lane);
            if (l == 0) s_tot[it & 1][v] = acc;
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
            // T7 PLL (tracking.py:223-235) of the block's sums, or of the group's; carrier parameters of the next block
            const double I_P = s_tot[it & 1][2], Q_P = s_tot[it & 1][3];
            g0 = (coh && j > 0) ? g0 + I_P : I_P;
            g1 = (coh && j > 0) ? g1 + Q_P : Q_P;
            if (update) {
                const double ka = coh ? C.k_carr_a : K.k_carr_a, kb = coh ? C.k_carr_b : K.k_carr_b;
                const double carrError = div_rn(atan(g1 / g0) / 2.0, M_PI, K.inv_pi);   // atan(Q/I) / 2 / pi
                const double carrNco = n0 + ka * (carrError - e0) + carrError * kb;
                n0 = rn = carrNco;
                e0 = re = carrError;
                if (!coh && lane == 0) s_ring[0][it % H] = carrNco;
                if (hand) {
                    double acc = 0.0;
                    for (int q = it + 1 - nh; q < it; ++q) acc += s_ring[0][q % H];
                    acc += carrNco;
                    n0 = acc / (double)nh;
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
            // T8 DLL (tracking.py:238-251), then block size and ramps of the next block (T1, T3, T4)
            const double I_E = s_tot[it & 1][0], Q_E = s_tot[it & 1][1], I_L = s_tot[it & 1][4], Q_L = s_tot[it & 1][5];
            g0 = (coh && j > 0) ? g0 + I_E : I_E;
            g1 = (coh && j > 0) ? g1 + Q_E : Q_E;
            g2 = (coh && j > 0) ? g2 + I_L : I_L;
            g3 = (coh && j > 0) ? g3 + Q_L : Q_L;
            const long long pos_after = s_st.pos;
            const double rem_next = s_st.remCode;
            if (update) {
                const double ka = coh ? C.k_code_a : K.k_code_a, kb = coh ? C.k_code_b : K.k_code_b;
                const double eE = sqrt(g0 * g0 + g1 * g1);
                const double eL = sqrt(g2 * g2 + g3 * g3);
                const double codeError = (eE - eL) / (eE + eL);
                const double codeNco = n0 + ka * (codeError - e0) + codeError * kb;
                n0 = rn = codeNco;
                e0 = re = codeError;
                if (!coh && lane == 0) s_ring[1][it % H] = codeNco;
                if (hand) {
                    double acc = 0.0;
                    for (int q = it + 1 - nh; q < it; ++q) acc += s_ring[1][q % H];
                    acc += codeNco;
                    n0 = acc / (double)nh;
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
            if (it > 0 && lane < 6) {
                const int series = (lane == 0) ? 4 : (lane == 1) ? 6 : (lane == 2) ? 3 : (lane == 3) ? 7 : (lane == 4) ? 5 : 8;
                o[series * m + (it - 1)] = s_tot[(it - 1) & 1][lane];
            }
            if (it > 0 && lane >= 8 && lane < 16 && lane != 11) {
                const int k = lane - 8;
                const int series = (k == 0) ? 2 : (k == 1) ? 11 : (k == 2) ? 12 : (k == 4) ? 0 : (k == 5) ? 1 : (k == 6) ? 9 : 10;
                o[series * m + (it - 1)] = s_out[(it - 1) & 1][k];
            }
        }
        done = it + 1;
        __syncthreads();   // next block's parameters visible
    }
    if (wave == 2 && done > 0 && lane < 6) {
        const int series = (lane == 0) ? 4 : (lane == 1) ? 6 : (lane == 2) ? 3 : (lane == 3) ? 7 : (lane == 4) ? 5 : 8;
        o[series * m + (done - 1)] = s_tot[(done - 1) & 1][lane];
    }
    if (wave == 2 && done > 0 && lane >= 8 && lane < 16 && lane != 11) {
        const int k = lane - 8;
        const int series = (k == 0) ? 2 : (k == 1) ? 11 : (k == 2) ? 12 : (k == 4) ? 0 : (k == 5) ? 1 : (k == 6) ? 9 : 10;
        o[series * m + (done - 1)] = s_out[(done - 1) & 1][k];
    }
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

extern "C" int sgx_track_coherent(sgx_ctx* c, const sgx_if* r, int64_t rec_file_offset, const sgx_chan_init* ch, int32_t n_ch,
                                  int32_t ms, const sgx_coh_params* p, const int32_t* bit_edge_in, double* out,
                                  int32_t* ms_done, int32_t* bit_edge, int32_t* coh_start, double* edge_energy) {
    SGX_CHECK_ARG(c && r && ch && p && bit_edge_in && out && ms_done && bit_edge && coh_start && edge_energy);
    SGX_CHECK_ARG(n_ch >= 1 && n_ch <= 65535 && ms >= 1);
    int rc = coh_check(c, ch, n_ch, ms, p, bit_edge_in);
    if (rc != SGX_OK) return rc;
    const sgx_settings& S = c->s;
    // the constants every tracking kernel reads (tracking.py:13-64), for one workgroup per channel
    TrkConst K;
    memset(&K, 0, sizeof(K));
    K.fs = S.samplingFreq;
    K.code_basis = S.codeFreqBasis;
    K.code_len = (double)S.codeLength;
    K.spacing = S.dllCorrelatorSpacing;
    double t1c, t2c, t1p, t2p;
    sgx_calc_loop_coef(S.dllNoiseBandwidth, S.dllDampingRatio, 1.0, &t1c, &t2c);     // tracking.py:45
    sgx_calc_loop_coef(S.pllNoiseBandwidth, S.pllDampingRatio, 0.25, &t1p, &t2p);    // tracking.py:52
    K.k_code_a = t2c / t1c;
    K.k_code_b = 0.001 / t1c;
    K.k_carr_a = t2p / t1p;
    K.k_carr_b = 0.001 / t1p;
    CohConst C;
    const double pdi = (double)p->coherent_ms * 0.001;
    C.k_code_a = p->tau2_dll / p->tau1_dll;
    C.k_code_b = pdi / p->tau1_dll;
    C.k_carr_a = p->tau2_pll / p->tau1_pll;
    C.k_carr_b = pdi / p->tau1_pll;
    C.T = p->coherent_ms;
    C.P = p->pull_in_ms;
    C.H = p->handover_ms;
    const long double two_pi = 2.0L * (long double)M_PI;   // the reference's 2*np.pi (a double)
    const long double inv = 1.0L / (two_pi * (long double)S.samplingFreq);
    K.inv_2pifs_hi = (double)inv;
    K.inv_2pifs_lo = (double)(inv - (long double)K.inv_2pifs_hi);
    K.inv_2pi = (double)(1.0L / two_pi);
    K.rec_len = (long long)r->n;
    K.rec_alloc = (long long)r->n + SGX_IF_PAD;
    K.multi = (15.0 * 1.001 * S.codeFreqBasis / S.samplingFreq >= 1.0) ? 1 : 0;   // (the rule of sgx_track's plan)
    K.kind = SGX_DT_INT8;
    K.file_off = (long long)rec_file_offset;
    K.ms = ms;
    K.n_ch = n_ch;
    K.split = 1;
    // units needed by the longest plausible block at the worst alignment (samplesPerCode + 64, as sgx_track allows)
    K.n_units = (int)(((long long)c->n_code + 64 + 15 + 15) / 16 + TRK_THREADS - 1) / TRK_THREADS;
    if (K.n_units > 16) {
        sgx_set_error("samplesPerCode %lld needs %d units, the tracking kernel holds 16", (long long)c->n_code, K.n_units);
        return SGX_E_ARG;
    }
    K.nb_base = (int)c->n_code - 3;
    for (int k = 0; k < 8; ++k) K.inv_nb[k] = 1.0 / (double)(K.nb_base + k);
    K.inv_fs = 1.0 / S.samplingFreq;
    K.inv_pi = 1.0 / M_PI;
    K.fscale = 1.0;
    std::vector<TrkChan> hc((size_t)n_ch);
    for (int i = 0; i < n_ch; ++i) {
        SGX_CHECK_ARG(ch[i].prn >= 0 && ch[i].prn <= 32);
        const long long p0 = (long long)S.skipNumberOfBytes + (long long)ch[i].codePhase - (long long)rec_file_offset;
        if (ch[i].prn != 0 && p0 < 0) {
            sgx_set_error("channel %d starts at file byte %lld, before the record (offset %lld)", i,
                          (long long)S.skipNumberOfBytes + (long long)ch[i].codePhase, (long long)rec_file_offset);
            return SGX_E_RANGE;
        }
        hc[(size_t)i] = TrkChan{ch[i].acquiredFreq, p0, ch[i].prn, 0};
    }
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
    coh_fill_kernel<<<(unsigned)((elems + 255) / 256), 256, 0, st>>>(d_out, ms, (long long)elems);
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
    // why a channel ended early, from the series (as sgx_track decides it): NaN rates behind an update of exactly zero sums
    for (int i = 0; i < n_ch; ++i) {
        if (ch[i].prn == 0) continue;
        const int dn = ms_done[i];
        if (dn < 1 || dn >= ms) continue;
        const double* row = out + (size_t)i * SGX_NUM_SERIES * (size_t)ms + (size_t)(dn - 1);
        const double codeFreq = row[(size_t)ms];
        if (codeFreq != codeFreq) {
            sgx_set_error("ValueError: cannot convert float NaN to integer: channel %d went silent - the six sums of the update "
                          "behind its block %d are exactly zero (a zero-filled stretch of the record) or its filters diverged, "
                          "the rates are NaN, and block %d has no length", i, dn - 1, dn);
            return SGX_E_SILENT;
        }
    }
    if (h_err & TRK_ERR_RANGE) {
        sgx_set_error("tracking: channel %d reached a block longer than the %d units of %d samples the kernel provides (the "
                      "code NCO left its plausible range)", (h_err & 0xFFFF) - 1, K.n_units, TRK_UNIT);
        return SGX_E_RANGE;
    }
    return SGX_OK;
}
