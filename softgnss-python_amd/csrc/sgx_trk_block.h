// One workgroup's view of a tracking block (tracking.py:148-275), piece by piece: what the per-channel kernels that map a
// block in groups of 16 samples have in common.  Used by
//   sgx_trk_persample.h  trk_kernel_multi / trk_kernel_any: every piece, around the members' exchange;
//   sgx_trk_coh.hip      trk_kernel_coh: every piece, around its own schedule of the two loop filters;
//   sgx_trk_tp.hip       trk_kernel_tp: the code table and the loop state's start (its map is by chip, not by group).
// Each piece is the arithmetic whose rounding the tests hold to the bit (tests/test_trk_math_gpu.py, the tie-follow tests):
// it is written here once.  Where the kernels differ on purpose - the carrier table of a group in registers or in LDS, how
// far the rare sample-by-sample route of a one-switch group is unrolled, how a sample is fetched - the difference is an
// argument.
#pragma once
#include "sgx_trk_common.h"

// hi dword of +-1.0 for [c1022, c0..c1022, c0] (tracking.py:111)
static __device__ __forceinline__ void trk_code_table(unsigned (&code_hi)[1028], const int8_t* __restrict__ codes, int prn, int tid,
                                                      int n_threads) {
    for (int i = tid; i < 1028; i += n_threads) {
        int j = i - 1;
        if (j < 0) j = 1022;
        if (j >= 1023) j -= 1023;
        if (j >= 1023) j -= 1023;
        code_hi[i] = (codes[(prn - 1) * 1023 + j] > 0) ? 0x3FF00000u : 0xBFF00000u;
    }
}

// tracking.py:114-130: the loop state in front of block 0 (one thread)
static __device__ __forceinline__ void trk_state_start(TrkState& s, const TrkConst& K, const TrkChan& cc) {
    s.codeFreq = K.code_basis;
    s.remCode = 0.0;
    s.oldCodeNco = s.oldCodeErr = 0.0;
    s.pos = cc.pos0;
    s.carrFreq = cc.acquiredFreq;
    s.carrBasis = cc.acquiredFreq;
    s.remCarr = 0.0;
    s.w = (cc.acquiredFreq * 2.0) * M_PI;
    s.oldCarrNco = s.oldCarrErr = 0.0;
}

// A 16-byte group of an int8 record whose byte 0 is sample i0 of a block of blk samples: the bytes outside [0, blk) zeroed
// (they then add nothing to the sums), and one byte as the reference's float64 arithmetic sees it
static __device__ __forceinline__ void trk_mask_group(unsigned (&wd)[4], int i0, int blk) {
    if (i0 >= 0 && i0 + 16 <= blk) return;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        int lo = -(i0 + 4 * d);
        lo = lo < 0 ? 0 : (lo > 4 ? 4 : lo);
        int hi = i0 + 4 * d + 4 - blk;
        hi = hi < 0 ? 0 : (hi > 4 ? 4 : hi);
        unsigned m = (lo >= 4) ? 0u : (0xFFFFFFFFu << (8 * lo));
        m &= (hi >= 4) ? 0u : (0xFFFFFFFFu >> (8 * hi));
        wd[d] &= m;
    }
}
static __device__ __forceinline__ double trk_byte(const unsigned (&wd)[4], int b) {
    return (double)(int)(signed char)((wd[b >> 2] >> (8 * (b & 3))) & 0xFF);
}

// The three code ramps of a block (TrkBlock's, held in registers across the map)
struct TrkRamps {
    double startE, stepE, startP, stepP, startL, stepL, inv_step;
};
static __device__ __forceinline__ TrkRamps trk_ramps(const TrkBlock& b) {
    return TrkRamps{b.startE, b.stepE, b.startP, b.stepP, b.startL, b.stepL, b.inv_step};
}

// A lane's six partial sums of a block
struct TrkSums {
    double IE, QE, IP, QP, IL, QL;
    // one sample: xs / xc its products with the carrier's sine / cosine, cE / cP / cL the three replicas' chips
    __device__ __forceinline__ void add(double xs, double xc, double cE, double cP, double cL) {
        IE = __builtin_fma(cE, xs, IE);
        QE = __builtin_fma(cE, xc, QE);
        IP = __builtin_fma(cP, xs, IP);
        QP = __builtin_fma(cP, xc, QP);
        IL = __builtin_fma(cL, xs, IL);
        QL = __builtin_fma(cL, xc, QL);
    }
    __device__ __forceinline__ void publish(double (&red)[6][TRK_THREADS], int tid) const {
        red[0][tid] = IE;
        red[1][tid] = QE;
        red[2][tid] = IP;
        red[3][tid] = QP;
        red[4][tid] = IL;
        red[5][tid] = QL;
    }
};

// THE ONE-SWITCH MAP of a group (16 samples span less than a chip, so a group meets at most one switch of a ramp): the
// three ramps' index and switch sample at the group's first sample by the exact reference arithmetic (ramp_setup), then the
// group as a sum over all its samples plus a sum over those behind the switch - when the ramps that switch inside the group
// do so at ONE sample (always, at >= 16 samples per half chip and dllCorrelatorSpacing 1/2); the samples one by one with the
// switches as compares otherwise (ODD_UNROLL: how far that rare loop is unrolled).
// xd: the group's samples, those outside the block zero; B: the block's carrier table of a group, in registers or in LDS;
// (gc, gs): the group-start phasor.
template <int ODD_UNROLL>
static __device__ __forceinline__ void trk_map_one_switch(TrkSums& a, const double (&xd)[16], const double2 (&B)[16],
                                                          const unsigned (&code_hi)[1028], const TrkRamps& R, int i0, double gc,
                                                          double gs) {
    const int ilo = i0 < 0 ? 0 : i0;
    int kE, swE, kP, swP, kL, swL;
    ramp_setup(R.startE, R.stepE, R.inv_step, ilo, kE, swE);
    ramp_setup(R.startP, R.stepP, R.inv_step, ilo, kP, swP);
    ramp_setup(R.startL, R.stepL, R.inv_step, ilo, kL, swL);
    const double cE1 = __hiloint2double((int)code_hi[kE], 0), cE2 = __hiloint2double((int)code_hi[kE + 1], 0);
    const double cP1 = __hiloint2double((int)code_hi[kP], 0), cP2 = __hiloint2double((int)code_hi[kP + 1], 0);
    const double cL1 = __hiloint2double((int)code_hi[kL], 0), cL2 = __hiloint2double((int)code_hi[kL + 1], 0);
    const int iend = i0 + 16;
    int swmin = swE < swP ? swE : swP;
    swmin = swL < swmin ? swL : swmin;
    const bool eS = (swE == swmin), pS = (swP == swmin), lS = (swL == swmin);
    const bool odd = (swE < iend && !eS) || (swP < iend && !pS) || (swL < iend && !lS);
    if (__any(odd)) {
#pragma unroll ODD_UNROLL
        for (int b = 0; b < 16; ++b) {
            const int i = i0 + b;
            const double2 Bb = B[b];
            const double c = __builtin_fma(gc, Bb.x, -(gs * Bb.y));
            const double sn = __builtin_fma(gs, Bb.x, gc * Bb.y);
            a.add(sn * xd[b], c * xd[b], i >= swE ? cE2 : cE1, i >= swP ? cP2 : cP1, i >= swL ? cL2 : cL1);
        }
    } else {
        const int bsw = swmin - i0;           // samples b >= bsw come after the switch
        double Ac = 0.0, As = 0.0, Tc = 0.0, Ts = 0.0;
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            const double2 Bb = B[b];
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
        a.IE = __builtin_fma(dE, tlI, __builtin_fma(cE1, allI, a.IE));
        a.QE = __builtin_fma(dE, tlQ, __builtin_fma(cE1, allQ, a.QE));
        a.IP = __builtin_fma(dP, tlI, __builtin_fma(cP1, allI, a.IP));
        a.QP = __builtin_fma(dP, tlQ, __builtin_fma(cP1, allQ, a.QP));
        a.IL = __builtin_fma(dL, tlI, __builtin_fma(cL1, allI, a.IL));
        a.QL = __builtin_fma(dL, tlQ, __builtin_fma(cL1, allQ, a.QL));
    }
}

// THE SAMPLE-BY-SAMPLE MAP of a group, for low sampling rates (under ~15.4 samples per chip a group can hold several chip
// switches of a ramp): the replicas are indexed sample by sample exactly as the reference does, code[ceil(linspace(...))]
// (tracking.py:166-188).  Correctness over speed.  sample(b, i): byte b of the group = sample i of the block, asked for
// samples inside the block only (a functor, not sixteen values: a sample outside the block is not read, and nothing is
// indexed by the loop's counter but what the caller indexes so).
template <class Sample>
static __device__ __forceinline__ void trk_map_by_sample(TrkSums& a, const double2 (&B)[16], const unsigned (&code_hi)[1028],
                                                         const TrkRamps& R, int i0, int blk, double gc, double gs, Sample sample) {
#pragma unroll 1
    for (int b = 0; b < 16; ++b) {
        const int i = i0 + b;
        if (i < 0 || i >= blk) continue;
        const double2 Bb = B[b];
        const double xd = sample(b, i);
        const double c = __builtin_fma(gc, Bb.x, -(gs * Bb.y));
        const double sn = __builtin_fma(gs, Bb.x, gc * Bb.y);
        const double xs = sn * xd, xc = c * xd;
        const double cE = __hiloint2double((int)code_hi[(int)ceil(ramp_at(i, R.stepE, R.startE))], 0);
        const double cP = __hiloint2double((int)code_hi[(int)ceil(ramp_at(i, R.stepP, R.startP))], 0);
        const double cL = __hiloint2double((int)code_hi[(int)ceil(ramp_at(i, R.stepL, R.startL))], 0);
        a.add(xs, xc, cE, cP, cL);
    }
}

// Carrier phase at the end of a block of blk samples (T5): remCarrPhase = trigarg[blk] % (2 pi), trigarg = w * (blk / fs) +
// rem; the exact remainder by FMA.  It does not need the block's sums.
static __device__ __forceinline__ double trk_end_phase(const TrkConst& K, double w, double remCarr, int blk) {
    const double two_pi = 2 * M_PI;
    const double arg_end = w * ((double)blk / K.fs) + remCarr;
    const double kq = floor(arg_end * K.inv_2pi);
    double rc = __builtin_fma(-kq, two_pi, arg_end);
    if (rc < 0.0) rc += two_pi;
    if (rc >= two_pi) rc -= two_pi;
    return rc;
}

// The fold of the lanes' partials (TrkSums::publish, a barrier behind it): wave w < 3 folds values 2w (lanes 0..31) and 2w + 1
// (lanes 32..63) - 8 partials per lane (consecutive lanes read consecutive 8-byte words: no bank conflict), then DPP; every
// lane of a half wave returns its value's total.  Fixed order: deterministic.
static __device__ __forceinline__ double trk_fold(const double (&red)[6][TRK_THREADS], int wave, int lane) {
    const int v = 2 * wave + (lane >> 5), l = lane & 31;
    double acc = red[v][l];
#pragma unroll
    for (int k = 1; k < TRK_THREADS / 32; ++k) acc += red[v][l + 32 * k];
    return half_wave_sum(acc, lane);
}

// T7 PLL (tracking.py:223-235) and T8 DLL (tracking.py:238-251): discriminator and loop filter of a pair / two pairs of sums,
// from the filter's memory (oldNco, oldErr) and its two coefficients (tau2 / tau1, PDI / tau1) -> the NCO command; err: the
// discriminator's value
static __device__ __forceinline__ double trk_pll_update(double I_P, double Q_P, double oldNco, double oldErr, double ka, double kb,
                                                        double inv_pi, double& err) {
    const double carrError = div_rn(atan(Q_P / I_P) / 2.0, M_PI, inv_pi);   // atan(Q/I) / 2 / pi
    err = carrError;
    return oldNco + ka * (carrError - oldErr) + carrError * kb;
}
static __device__ __forceinline__ double trk_dll_update(double I_E, double Q_E, double I_L, double Q_L, double oldNco, double oldErr,
                                                        double ka, double kb, double& err) {
    const double eE = sqrt(I_E * I_E + Q_E * Q_E);
    const double eL = sqrt(I_L * I_L + Q_L * Q_L);
    const double codeError = (eE - eL) / (eE + eL);
    err = codeError;
    return oldNco + ka * (codeError - oldErr) + codeError * kb;
}

// T9 record (tracking.py:255-275) of block `row`, by lanes 0..15 of one wave: its six sums (tot: I_E Q_E I_P Q_P I_L Q_L) and
// the scalars the filter waves staged (outs: [0] carrFreq [1] carrError [2] carrNco, [4] absoluteSample [5] codeFreq
// [6] codeError [7] codeNco) to their series of the channel's output o, m entries each
static __device__ __forceinline__ void trk_store_row(double* __restrict__ o, long long m, int row, const double (&tot)[6],
                                                     const double (&outs)[8], int lane) {
    if (lane < 6) {
        const int series = (lane == 0) ? 4 : (lane == 1) ? 6 : (lane == 2) ? 3 : (lane == 3) ? 7 : (lane == 4) ? 5 : 8;
        o[series * m + row] = tot[lane];
    }
    if (lane >= 8 && lane < 16 && lane != 11) {
        const int k = lane - 8;
        const int series = (k == 0) ? 2 : (k == 1) ? 11 : (k == 2) ? 12 : (k == 4) ? 0 : (k == 5) ? 1 : (k == 6) ? 9 : 10;
        o[series * m + row] = outs[k];
    }
}
