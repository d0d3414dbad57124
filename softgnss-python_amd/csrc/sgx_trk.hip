// TrackingResult.track on gfx950 (reference tracking.py:13-295): the host side.
//
// A channel is a chain of `ms` dependent 1-ms steps: every block's length, code ramps and NCO rates depend on the
// previous block's six correlator sums.  Channels are independent.  Every kernel is persistent: one launch walks all
// code periods of all channels.  A block (~38 192 samples) is cut into UNITS of 256 groups x 16 samples (4 KiB of IF).
//
// Which kernel runs, with how many workgroups per channel: the table in front of trk_plan below; what a repeated launch
// runs: trk_launch_step.  The launchers and the layout the host sizes are declared in sgx_trk_common.h.
// fp64 everywhere: 1e-7 errors in the sums move the code NCO enough to flip a chip-boundary sample somewhere in a 37 s
// run, which is a 1e-3 relative blip.
#include <algorithm>
#include <chrono>
#include "sgx_trk_common.h"

// tracking.py:65-94: series start as zeros (absoluteSample, I/Q) or +Inf (the others)
__global__ __launch_bounds__(256) void trk_fill_kernel(double* __restrict__ out, long long ms, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int series = (int)((i / ms) % SGX_NUM_SERIES);
    const bool zero = (series == 0) || (series >= 3 && series <= 8);
    out[i] = zero ? 0.0 : __longlong_as_double(0x7FF0000000000000ll);
}
void sgx_trk_fill(double* d_out, int ms, size_t elems, hipStream_t st) {
    trk_fill_kernel<<<(unsigned)((elems + 255) / 256), 256, 0, st>>>(d_out, ms, (long long)elems);
}

// What a tracking launch leaves for the host: the result page's TrkLook (sgx_internal.h), then the word the host spins on
__global__ __launch_bounds__(SGX_TRK_LOOK_CH) void trk_finish_kernel(const int* __restrict__ d_err, const int* __restrict__ d_done,
                                                                     int n_ch, TrkLook* __restrict__ look, unsigned long long seq) {
    const int t = threadIdx.x;
    if (t < 2) look->err[t] = d_err[t];
    if (t < n_ch) look->done[t] = d_done[t];
    __threadfence_system();
    __syncthreads();
    if (t == 0) __hip_atomic_store(&look->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// THE SPECULATIVE KERNEL'S SCALE GUARD for int8 records read resident (sgx_trk3.hip: a unit's total must stay below 2^17, and no
// arm's total can exceed the sum of the unit's magnitudes).  One pass over the record, once per record (cached in the
// handle): the largest sum of |x| over 17 consecutive 128-byte blocks - any 2 048-byte window of the kernel lies inside
// such a run - by workgroups of 256 blocks with a halo of 16.  1.4 GB in ~0.4 ms; a streaming record that is not resident
// yet is guarded inside the kernel instead (its record wave adds up the magnitudes of every block's window).
__global__ __launch_bounds__(256) void if_mag_kernel(const int8_t* __restrict__ x, long long n_bytes, int* __restrict__ out_max) {
    __shared__ int s_m[256 + 16];
    const long long blk0 = (long long)blockIdx.x * 256;
    auto block_mag = [&](long long j) -> int {
        const long long a = j * 128;
        if (a >= n_bytes) return 0;                      // (the allocation is padded with zero bytes: SGX_IF_PAD)
        int m = 0;
        const uint4* p = reinterpret_cast<const uint4*>(x + a);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint4 w = p[k];
            const unsigned b = 0x80808080u;
            m = (int)__builtin_amdgcn_sad_u8(w.x ^ b, b, (unsigned)m);
            m = (int)__builtin_amdgcn_sad_u8(w.y ^ b, b, (unsigned)m);
            m = (int)__builtin_amdgcn_sad_u8(w.z ^ b, b, (unsigned)m);
            m = (int)__builtin_amdgcn_sad_u8(w.w ^ b, b, (unsigned)m);
        }
        return m;
    };
    s_m[threadIdx.x] = block_mag(blk0 + threadIdx.x);
    if (threadIdx.x < 16) s_m[256 + threadIdx.x] = block_mag(blk0 + 256 + threadIdx.x);
    __syncthreads();
    int w = 0;
#pragma unroll
    for (int k = 0; k < 17; ++k) w += s_m[threadIdx.x + k];
    for (int o = 32; o > 0; o >>= 1) {
        const int v = __shfl_down(w, o);
        w = v > w ? v : w;
    }
    if ((threadIdx.x & 63) == 0) atomicMax(out_max, w);
}

// -> the bound (cached in the handle), or -1 when the record is not fully resident yet / on an error
// (resident: every copy has completed - host_mark reaches the end a moment before the loader thread sets load_done)
// (a buffer of the call's own, S.rec null, is resident and has no handle to cache the bound in)
static long long if_mag_bound(sgx_ctx* c, const TrkSource& S) {
    const sgx_if* r = S.rec;
    if (r) {
        long long known = r->mag_max.load();
        if (known >= 0) return known;
        if (r->loader && !r->load_done.load() && r->host_mark.load() < r->n) return -1;
    }
    int* d_max = &c->d_small->trk_mag;
    if (hipMemsetAsync(d_max, 0, sizeof(int), c->stream) != hipSuccess) return -1;
    const long long n_blocks128 = (S.n + 127) / 128;
    const unsigned grid = (unsigned)((n_blocks128 + 255) / 256);
    if_mag_kernel<<<grid ? grid : 1u, 256, 0, c->stream>>>(S.d, S.n + SGX_IF_PAD - 128, d_max);
    int h = 0;
    if (hipMemcpyAsync(&h, d_max, sizeof(int), hipMemcpyDeviceToHost, c->stream) != hipSuccess) return -1;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return -1;
    if (r) const_cast<sgx_if*>(r)->mag_max.store((long long)h);
    return (long long)h;
}

// (struct TrkEnv: sgx_trk_common.h - the float front reads its two switches from it)
TrkEnv sgx_trk_env() {
    auto first = [](const char* name) -> char {   // (0 when unset)
        const char* v = getenv(name);
        return v ? v[0] : 0;
    };
    const char* split = getenv("SGX_TRK_SPLIT");
    const char* arms = getenv("SGX_TRK_ARMS");
    const char* lds = getenv("SGX_TRK_LDSPAD");
    TrkEnv E;
    E.trace = first("SGX_STEP_TRACE") == '1';              // host-side time stamps of the call on stderr, us since its entry
    E.float_typed = first("SGX_TRK_FLOAT_TYPED") != '0';   // '0': float records always on the per-sample kernel
    E.f32_narrow = first("SGX_TRK_F32_NARROW") != '0';     // '0': no narrowing - every float32 record as floats
    E.split = (split && atoi(split) >= 1) ? atoi(split) : 0;
    E.arms = arms ? (arms[0] == '3' ? 3 : 1) : 0;
    E.v3_off = first("SGX_TRK_V3") == '0';
    E.v3_generic = first("SGX_TRK3_GENERIC") == '1';       // the speculative kernel's generic text for every case (tests, A/B)
    E.fast_xcd = first("SGX_TRK_FASTX") != '0';            // '0': no same-XCD exchange path
    E.profile = first("SGX_TRK_PROFILE") == '1';           // the kernels' phase cycles on stderr
    E.lds_pad = lds ? atoi(lds) : 90112;                   // dynamic LDS per cooperative workgroup; default: one per CU
    E.stream = first("SGX_TRK_STREAM") != '0';             // '0': never follow a record that is still streaming in
    E.withhold = first("SGX_TRK_TEST_WITHHOLD") == '1';    // test hooks: launch without each channel's last member; ...
    E.timeout = first("SGX_TRK_TEST_TIMEOUT");             // ... '1' the first launch times out, '2' the one after a stall;
    E.stall = first("SGX_TRK_TEST_STALL") == '1';          // ... the first launch's stream stalls
    E.scatter = first("SGX_TRK_TEST_SCATTER") == '1';      // ... the speculative kernel's headline text finds its members scattered
    return E;
}

// ---- The stages every per-channel tracking call runs (sgx_trk_common.h declares them: sgx_track_coherent, sgx_trk_coh.hip, is
// the other caller).  Fewer than ~15.4 samples per chip: a 16-sample group can hold several chip switches of a ramp
int sgx_trk_multi(const sgx_settings& S) {
    return (15.0 * 1.001 * S.codeFreqBasis / S.samplingFreq >= 1.0) ? 1 : 0;
}

// Units needed by the longest possible block, worst alignment.  A block is samplesPerCode +- 1 samples long while the
// code NCO stays near its basis; the allowance of 64 samples corresponds to a code-rate error of 0.17 % (1.7 kHz at
// 1.023 MHz), three orders of magnitude beyond what the DLL's filter can command.
int sgx_trk_units(long long n_code) {
    return (int)((n_code + 64 + 15 + 15) / 16 + TRK_THREADS - 1) / TRK_THREADS;
}
int sgx_trk_units_check(long long n_code, int n_units) {
    if (n_units <= 16) return SGX_OK;
    sgx_set_error("samplesPerCode %lld needs %d units, the tracking kernel holds 16", n_code, n_units);
    return SGX_E_ARG;
}

// tracking.py:13-64: the constants every kernel reads, for a record of rec_len bytes of `kind` samples that starts at byte
// file_off of its file (each launch sets split, n_units and mark; fast_xcd and fscale are the caller's)
void sgx_trk_const(TrkConst& K, const sgx_settings& S, long long n_code, long long rec_len, int kind, long long file_off, int ms,
                   int n_ch, int multi) {
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
    const long double two_pi = 2.0L * (long double)M_PI;   // the reference's 2*np.pi (a double)
    const long double inv = 1.0L / (two_pi * (long double)S.samplingFreq);
    K.inv_2pifs_hi = (double)inv;
    K.inv_2pifs_lo = (double)(inv - (long double)K.inv_2pifs_hi);
    K.inv_2pi = (double)(1.0L / two_pi);
    K.rec_len = rec_len;                                 // bytes; wider samples: the kernel divides (per-channel shift)
    K.rec_alloc = rec_len + SGX_IF_PAD - (sgx_dt_bytes(kind) - 1);   // bytes, less the largest per-channel shift
    K.multi = multi;
    K.uns = kind == SGX_DT_UINT8 ? 1 : 0;
    K.kind = kind;
    K.file_off = file_off;
    K.ms = ms;
    K.n_ch = n_ch;
    K.nb_base = (int)n_code - 3;
    for (int k = 0; k < 8; ++k) K.inv_nb[k] = 1.0 / (double)(K.nb_base + k);
    K.inv_fs = 1.0 / S.samplingFreq;
    K.inv_pi = 1.0 / M_PI;
    K.fscale = 1.0;
}

// The channel table the kernels read, from channels that start skip_bytes + codePhase bytes into the file
int sgx_trk_channels(std::vector<TrkChan>& hc, const sgx_chan_init* ch, int n_ch, long long skip_bytes, long long file_off,
                     int sample_bytes) {
    hc.resize((size_t)n_ch);
    for (int i = 0; i < n_ch; ++i) {
        TrkChan& h = hc[(size_t)i];
        h.acquiredFreq = ch[i].acquiredFreq;
        h.prn = ch[i].prn;
        SGX_CHECK_ARG(ch[i].prn >= 0 && ch[i].prn <= 32);
        const long long p0 = skip_bytes + (long long)ch[i].codePhase - file_off;
        if (ch[i].prn != 0 && p0 < 0) {
            sgx_set_error("channel %d starts at file byte %lld, before the record (offset %lld)", i,
                          skip_bytes + (long long)ch[i].codePhase, file_off);
            return SGX_E_RANGE;
        }
        // wider samples: the channel's own sample grid starts at byte p0 % sample_bytes of the record
        h.pos0 = p0 / sample_bytes;
        h.pad = (int)(p0 % sample_bytes);
    }
    return SGX_OK;
}

int sgx_trk_source(TrkSource& S, const sgx_settings& st, const sgx_if* r, long long file_off, const sgx_chan_init* ch, int n_ch, int kind) {
    S.d = r->d;
    S.n = (long long)r->n;
    S.rec = r;
    S.kind = kind;
    S.file_off = file_off;
    return ch ? sgx_trk_channels(S.hc, ch, n_ch, (long long)st.skipNumberOfBytes, file_off, sgx_dt_bytes(kind)) : SGX_OK;
}

// ---- WHICH KERNEL, HOW MANY MEMBERS: the one rule (include/sgx.h: sgx_track_plan; tests/test_cabi_and_host.py holds the table)
//
//   sample type                      channels   samples / chip      spacing   -> kernel                        members per channel
//   any but int8/uint8/int16/float*  any        any                 any          6 trk_kernel_any              min(units, CUs / ch8, 10)
//   float32 / float64 out of range   any        any                 any          6 trk_kernel_any              (as above)
//   uint8 / int16 / float            any        < ~15.4 (multi)     any          6 trk_kernel_any              (as above)
//   int8                             any        < ~15.4 (multi)     any          4 trk_kernel_multi            min(units, CUs / ch8, 10)
//   int8 / uint8 / int16             > 128 and CUs / ch8 < 2        any          3 trk_kernel_tp               1
//   int8 / uint8                     ch8 x 2 units <= CUs, 18 samples < 1/2 chip, spacing 1/2
//                                                                                5 trk3_kernel                 2 x units (128-group units)
//   everything else                                                              2 trk2_kernel                 3 x units (one per unit and arm)
//                                                                                                              while 3 ch8 units <= CUs and not float,
//                                                                                                              else min(units, CUs / ch8)
//   (ch8 = channels rounded up to 8; units = ceil((samplesPerCode + 94) / 16 / 256); the members are trk_launch_step's for
//   the first launch with every CU free - a launch whose CUs are taken, or a repeated one, may run fewer)
struct TrkPlan {
    int kernel;          // of the first launch: 2, 3, 4, 5 or 6 (sgx_timing.track_kernel)
    int ch8, multi, arm_split, split, n_units, n_units3;
};

// (split_env: SGX_TRK_SPLIT or 0; arms_env: 0 unset, 3 SGX_TRK_ARMS=3, 1 any other value; v3_off: SGX_TRK_V3=0 - diagnostics)
static TrkPlan trk_plan(const sgx_settings& S, int kind, int n_ch, long long n_code, int cus_total, bool floaty,
                        int split_env = 0, int arms_env = 0, bool v3_off = false) {
    TrkPlan P;
    P.multi = sgx_trk_multi(S);
    if (P.multi) floaty = false;
    const bool typed = kind == SGX_DT_INT8 || kind == SGX_DT_UINT8 || kind == SGX_DT_INT16 || floaty;
    const bool use_any = !typed || (P.multi && kind != SGX_DT_INT8);
    const int ch8 = P.ch8 = ((n_ch + 7) / 8) * 8;
    P.n_units = sgx_trk_units(n_code);
    int split = cus_total / ch8;
    if (split > P.n_units) split = P.n_units;
    if ((P.multi || use_any) && split > TRK_MAX_SPLIT) split = TRK_MAX_SPLIT;
    if (split < 1) split = 1;
    if (split_env >= 1 && split_env <= split) split = split_env;
    P.split = split;
    const bool use_tp = !use_any && !floaty && !P.multi && split == 1 && n_ch > 128;
    const bool use_v2 = !use_any && !P.multi && !use_tp;
    P.arm_split = (use_v2 && !floaty && split == P.n_units && P.n_units >= 2 && 3 * ch8 * P.n_units <= cus_total &&
                   split_env == 0 && arms_env != 3) ? 1 : 0;
    // The speculative kernel (sgx_trk3.hip) serves all three arms from one lane, which rests on a 16-sample group (and one
    // sample on either side of it) meeting at most ONE chip boundary of ANY arm: the arms' boundaries lie at code phases
    // 0, d and 1 - d (mod 1 chip; d = dllCorrelatorSpacing), so the smallest gap between two DIFFERENT ones must exceed 18
    // samples of code phase (1 % margin for the code NCO) - and its fused half-chip ramp puts the early / late boundaries
    // on the ODD half chips: spacing 1/2 exactly.  int8 / uint8 records, one workgroup per unit of 128 groups, while
    // 8-padded channels x units fit the CUs.
    P.n_units3 = 2 * P.n_units;
    const double d = S.dllCorrelatorSpacing, e = 1.0 - d;
    double pts[3] = {0.0, d < e ? d : e, d < e ? e : d};
    double gap = 2.0;
    for (int i = 0; i < 3; ++i) {
        const double g = (i < 2 ? pts[i + 1] : pts[0] + 1.0) - pts[i];
        if (g > 1e-9 && g < gap) gap = g;
    }
    const double stepn = S.codeFreqBasis / S.samplingFreq;
    const bool use_v3 = use_v2 && sgx_dt_bytes(kind) == 1 && P.n_units3 >= 2 && P.n_units3 <= T3_MAXP && ch8 * P.n_units3 <= cus_total &&
                        fabs(d - 0.5) < 1e-12 && 18.0 * stepn * 1.01 <= gap && split_env == 0 && arms_env == 0 && !v3_off;
    P.kernel = use_any ? 6 : use_tp ? 3 : use_v3 ? 5 : use_v2 ? 2 : 4;
    return P;
}

// What the launches of a call have established: each cause of a repeated launch (at most five launches in all)
struct TrkRepeat {
    bool stream_stalled = false;   // a streaming record's watermark stalled: the launch was repeated on the resident record
    bool one_member = false;       // a member of a cooperative layout timed out: one workgroup per channel from then on
    bool v3_off = false;           // too strong for the speculative kernel's fixed point: the round-3 kernel from then on
    bool scattered = false;        // a channel's members do not share an XCD: the speculative kernel's generic text from then on
};

// One launch: the kernel that runs (2, 3, 4, 5 or 6), its layout, and the CUs reserved for it
struct TrkLaunch {
    int kernel, split, n_units, arms, members, n_blocks, cus;   // (arms, trk2_kernel: 1 a workgroup per unit and arm, 3 per unit)
};

// THE PER-LAUNCH STEP: the plan's kernel under the repeats so far and the CUs that `reserve(want)` grants (want, or 0).
// Cooperating workgroups wait for each other, so all of a launch must be resident at once, one workgroup per CU (of a budget
// all contexts share): trk3 whose CUs are taken runs trk2; one per unit and arm tries one per unit, then one per channel.
template <class Reserve>
static TrkLaunch trk_launch_step(const TrkPlan& P, const TrkRepeat& R, Reserve reserve) {
    TrkLaunch L{P.kernel, R.one_member ? 1 : P.split, P.n_units, 3, 0, 0, 0};
    if (L.kernel == 5) {
        if (!R.one_member && !R.v3_off) L.cus = reserve(P.ch8 * P.n_units3);
        if (L.cus) L.split = L.n_units = P.n_units3;   // (units of half the size: the same room for a code NCO that left its basis)
        else L.kernel = 2;
    }
    if (L.kernel != 5 && L.split > 1) {
        if (L.kernel == 2 && P.arm_split) {
            L.cus = reserve(P.ch8 * L.split * 3);
            L.arms = L.cus ? 1 : 3;
        }
        if (!L.cus) L.cus = reserve(P.ch8 * L.split);
        if (!L.cus) L.split = 1;
    }
    L.members = L.arms == 1 ? 3 * L.split : L.split;
    L.n_blocks = P.ch8 * L.members;
    return L;
}

extern "C" int sgx_track_plan(const sgx_settings* s, int32_t data_type, int32_t n_ch, int32_t n_cus, int32_t float_in_range,
                              int32_t* kernel, int32_t* members) {
    SGX_CHECK_ARG(s && kernel && members && n_ch >= 1 && n_cus >= 1);
    if (sgx_dt_bytes(data_type) == 0) {
        sgx_set_error("sgx_track_plan: data_type %d is not one of SGX_DT_* (include/sgx.h)", (int)data_type);
        return SGX_E_ARG;
    }
    int64_t n_code = 0;
    const int rc = sgx_samples_per_code(s, &n_code);
    if (rc != SGX_OK) return rc;
    const bool fl = (data_type == SGX_DT_FLOAT32 || data_type == SGX_DT_FLOAT64) && float_in_range != 0;
    const TrkPlan P = trk_plan(*s, data_type, n_ch, (long long)n_code, n_cus, fl);
    const TrkLaunch L = trk_launch_step(P, TrkRepeat{}, [&](int want) { return want <= n_cus ? want : 0; });
    *kernel = L.kernel;
    *members = L.members;
    return SGX_OK;
}

// One tracking call: its arguments, and what the stages below make of them
struct TrkCall {
    sgx_ctx* c;
    const TrkSource& S;          // what it runs on, and how its results are undone (sgx_trk_common.h)
    const sgx_chan_init* ch;     // null when chained
    int n_ch, ms;
    double* out;
    int32_t* ms_done;
    bool chained;
    TrkEnv E;
    std::chrono::steady_clock::time_point t0;
    int cus_total;
    TrkPlan P;
    TrkConst K;
    size_t elems;                // n_ch x SGX_NUM_SERIES x ms
    double* d_out;               // the series: the caller's pinned buffer itself (direct), or the context's staging buffer
    bool direct;
    TrkChan* d_ch;               // the rest is one cached allocation: [channels | done | exchange | err | profile]
    int* d_done;
    unsigned long long* d_xch;
    int* d_err;
    long long* d_prof;           // SGX_TRK_PROFILE=1 only
    size_t sz_clear, sz_prof;    // bytes from d_done to the profile (cleared in front of every launch); of the profile
    bool fast_look;              // error words and ms_done through the pinned page: direct, and the channels fit the page
    TrkRepeat rep;
    TrkLaunch L;                 // the last launch ...
    hipError_t e;                // ... its status (hipSuccess before the first) ...
    int h_err;                   // ... and its error word: 0, or 1 + the channel that timed out
    int range_ch1;               // 1 + the channel that reached a block beyond the launch's units (0: none); sgx_trk_diagnose
    void stamp(const char* what) const {
        if (E.trace) fprintf(stderr, "[sgx step trace] %-28s %8.1f us\n", what,
                             std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    }
};

// If the caller's result buffer is pinned host memory (sgx_host_alloc; the Python binding's is), the kernel's record
// stores - 104 bytes per channel per millisecond, issued by an otherwise idle wave - go straight to it over PCIe: no device
// staging buffer, no D2H copy and no prefill pass after the kernel.  The call state is one cached device allocation.
static int trk_buffers(TrkCall& T) {
    sgx_ctx* c = T.c;
    T.elems = (size_t)T.n_ch * SGX_NUM_SERIES * (size_t)T.ms;
    hipPointerAttribute_t pa;
    T.direct = hipPointerGetAttributes(&pa, T.out) == hipSuccess && pa.type == hipMemoryTypeHost && pa.devicePointer;
    if (T.direct) {
        T.d_out = (double*)pa.devicePointer;
    } else {
        (void)hipGetLastError();   // a pageable pointer is not an error
        const int rc = c->d_trk_out.ensure(T.elems * sizeof(double));
        if (rc != SGX_OK) return rc;
        T.d_out = c->d_trk_out;
    }
    const size_t sz_ch = ((sizeof(TrkChan) * (size_t)T.n_ch + 255) / 256) * 256;
    const size_t sz_done = ((sizeof(int) * (size_t)T.n_ch + 255) / 256) * 256;
    const size_t xch_words = std::max({2 * TRK_MAX_SPLIT * 12 + 16, T2_XCH_STRIDE, T3_XCH_STRIDE});
    const size_t xch_bytes = sizeof(unsigned long long) * (size_t)T.n_ch * xch_words;
    const size_t sz_xch = ((xch_bytes + 255) / 256) * 256;
    T.sz_clear = sz_done + sz_xch + 256;
    T.sz_prof = sizeof(long long) * T2_PROF_STRIDE * (size_t)T.n_ch;
    const int rc = c->d_trk_aux.ensure(sz_ch + T.sz_clear + T.sz_prof);
    if (rc != SGX_OK) return rc;
    char* aux = c->d_trk_aux;
    T.d_ch = (TrkChan*)aux;
    T.d_done = (int*)(aux + sz_ch);
    T.d_xch = (unsigned long long*)(aux + sz_ch + sz_done);
    T.d_err = (int*)(aux + sz_ch + sz_done + sz_xch);
    T.d_prof = T.E.profile ? (long long*)(aux + sz_ch + T.sz_clear) : nullptr;
    T.fast_look = T.direct && T.n_ch <= SGX_TRK_LOOK_CH && !T.E.profile;
    return SGX_OK;
}

// The launch's error words ([0] flags | 1 + channel of a timeout; [1] 1 + channel of a block beyond the units): from the
// pinned page trk_finish_kernel fills (the host spins, then sleeps in the stream synchronisation), or copied and synchronised
static int trk_collect(TrkCall& T, int words[2]) {
    sgx_ctx* c = T.c;
    hipStream_t st = c->stream;
    hipError_t& e = T.e;
    if (!T.fast_look) {
        if (e == hipSuccess) e = hipMemcpyAsync(words, T.d_err, 2 * sizeof(int), hipMemcpyDeviceToHost, st);
        T.stamp("error word copy queued");
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        T.stamp("stream synchronised");
        return SGX_OK;
    }
    const unsigned long long seq = ++c->trk_seq;
    if (e == hipSuccess) {
        trk_finish_kernel<<<1, SGX_TRK_LOOK_CH, 0, st>>>(T.d_err, T.d_done, T.n_ch, &c->d_look->trk, seq);
        e = hipGetLastError();
    }
    T.stamp("finish kernel queued");
    if (e == hipSuccess) {
        const TrkLook* look = &c->h_look->trk;
        const int rc = sgx_look_wait(st, &look->seq, seq, true, 0.25, 4096, "tracking: the launch's result words were not written", &e);
        if (rc != SGX_OK) return rc;
        words[0] = look->err[0];
        words[1] = look->err[1];
    }
    T.stamp("result words seen");
    return SGX_OK;
}

// What follows a launch whose error words are in: `again` when it is repeated (the cause recorded in T.rep, said on
// stderr), or the error.  Test hooks first: a timed-out launch (SGX_TRK_TEST_TIMEOUT), a stalled stream (..._STALL).
static int trk_repeat(TrkCall& T, int launch, const int words[2], bool& again) {
    const TrkLaunch& L = T.L;
    TrkRepeat& R = T.rep;
    int& h_err = T.h_err;
    again = false;
    h_err = words[0];
    if (T.e != hipSuccess) return SGX_OK;   // (trk_finish reports it)
    if (T.E.timeout && L.split > 1 && !R.one_member &&
        ((T.E.timeout == '1' && launch == 0) || (T.E.timeout == '2' && R.stream_stalled)))
        h_err = 1;
    if (T.E.stall && launch == 0) h_err = TRK_ERR_STREAM;
    if ((h_err & TRK_ERR_STREAM) && !R.stream_stalled && !R.one_member) {
        // the streaming record's watermark stalled (the copy stream could not run beside the kernel): repeat
        // with the same decomposition once the whole record is resident
        fprintf(stderr, "[sgx] tracking: the record did not stream in beside the kernel; repeating the launch "
                        "on the resident record\n");
        R.stream_stalled = again = true;
        return SGX_OK;
    }
    h_err &= ~TRK_ERR_STREAM;
    if ((h_err & TRK_ERR_SCALE) && !R.v3_off) {
        // samples beyond what the speculative kernel's 2^30 fixed point holds in 48 bits (a record that clips all the
        // time): the round-3 kernel, whose 2^28 holds full-scale samples that all line up, tracks it
        fprintf(stderr, "[sgx] tracking: samples too strong for the speculative kernel's fixed point (2 048 samples add up "
                        "to 131 072 or more in magnitude); repeating the launch with the round-3 kernel\n");
        R.v3_off = again = true;
        return SGX_OK;
    }
    h_err &= ~TRK_ERR_SCALE;
    if ((h_err & TRK_ERR_PLACE) && !R.scattered) {
        // the speculative kernel's headline text takes every member of a channel to sit on one XCD (its exchange stays in
        // that L2); the placement check at the kernel's start found otherwise: the generic text asks at run time
        fprintf(stderr, "[sgx] tracking: a channel's workgroups do not share an XCD; repeating the launch with the "
                        "speculative kernel's generic text\n");
        R.scattered = again = true;
        return SGX_OK;
    }
    h_err &= ~TRK_ERR_PLACE;
    if ((h_err & TRK_ERR_RANGE) == 0) h_err &= 0xFFFF;
    if (h_err & TRK_ERR_RANGE) {
        // (every workgroup has retired: the series and ms_done are collected first, sgx_trk_diagnose then says what happened)
        T.range_ch1 = words[1] ? words[1] : (h_err & 0xFFFF);
        if (T.range_ch1 < 1) T.range_ch1 = 1;
        h_err = 0;
        return SGX_OK;
    }
    if (h_err == 0 || L.split == 1) return SGX_OK;
    // a member timed out (bounded spins) waiting for the others - something else occupies the CUs: one workgroup per channel
    fprintf(stderr, "[sgx] tracking: channel %d timed out waiting for a cooperating workgroup (%d workgroups per "
                    "channel, are the CUs shared?); repeating the launch with one workgroup per channel\n", h_err - 1,
            L.members);
    R.one_member = again = true;
    return SGX_OK;
}

// CUs claimed by a cooperative launch; given back on EVERY way out of the call
struct CuGuard {
    int device, n;
    ~CuGuard() { drop(); }
    void drop() {
        if (n) sgx_cu_release(device, n);
        n = 0;
    }
};

// One launch, in stream order: the scale scan, the channel table, the cleared state, the fill kernel, the CUs, the record,
// the profile, the kernel between ev[3] and ev[4], its result words; -> what trk_repeat makes of them
static int trk_launch_once(TrkCall& T, int launch, CuGuard& reserved, bool& again) {
    sgx_ctx* c = T.c;
    const TrkSource& S = T.S;
    const sgx_if* r = S.rec;
    hipStream_t st = c->stream;
    // a record that is still streaming in is followed by the latency-mode kernel (its record wave watches the
    // device watermark); the other kernels, and a launch repeated on the resident record, first wait for all of it
    const bool streaming = r && r->loader && !r->load_done.load() && launch == 0 && T.E.stream && (T.P.kernel == 2 || T.P.kernel == 5);
    if (T.P.kernel == 5 && S.kind == SGX_DT_INT8 && !T.rep.one_member && !T.rep.v3_off && !streaming) {
        // THE SCALE GUARD of every speculative launch that does not stream (sgx_trk3.hip says why 2^17; a streaming launch
        // has its record wave's): a bound computed once per record, before the kernel is chosen and its CUs reserved,
        // whatever the record was when the call began - still loading (SGX_TRK_STREAM=0, a stalled stream) or resident
        const int rq = r ? sgx_if_require(r, r->n) : SGX_OK;
        if (rq != SGX_OK) return rq;
        const long long mag = if_mag_bound(c, S);
        if (mag < 0) {
            sgx_set_error("tracking: the magnitude scan of the record failed");
            return SGX_E_HIP;
        }
        if (mag >= 131072) {
            fprintf(stderr, "[sgx] tracking: samples too strong for the speculative kernel's fixed point (2 048 samples add "
                            "up to 131 072 or more in magnitude); the round-3 kernel tracks this record\n");
            T.rep.v3_off = true;
        }
    }
    if (!T.chained) {
        SGX_HIP(hipMemcpyAsync(T.d_ch, S.hc.data(), sizeof(TrkChan) * (size_t)T.n_ch, hipMemcpyHostToDevice, st));
    } else if (launch == 0) {
        // preRun on the device: the table lands in d_ch (a repeated launch finds it there)
        const int rp = sgx_prerun_enqueue(c, T.d_ch, T.n_ch, (long long)c->s.skipNumberOfBytes, S.file_off, sgx_dt_bytes(S.kind));
        if (rp != SGX_OK) return rp;
    }
    T.stamp("channel table queued");
    SGX_HIP(hipMemsetAsync(T.d_done, 0, T.sz_clear, st));   // done, every polled word, err
    T.stamp("memset queued");
    if (!T.direct) sgx_trk_fill(T.d_out, T.ms, T.elems, st);
    const TrkLaunch& L = T.L = trk_launch_step(T.P, T.rep, [&](int want) { return sgx_cu_reserve(c->device, T.cus_total, want); });
    reserved.n = L.cus;
    T.K.split = L.split;
    T.K.n_units = L.n_units;
    if (r && !streaming) {
        const int rq = sgx_if_require(r, r->n);
        if (rq != SGX_OK) return rq;
    }
    T.K.mark = streaming ? r->d_mark : nullptr;
    if (T.d_prof) SGX_HIP(hipMemsetAsync(T.d_prof, 0, T.sz_prof, st));
    hipEventRecord(c->ev[3], st);
    // THE LAUNCH.  Test hook (SGX_TRK_TEST_WITHHOLD=1): launch without each channel's last member - the speculative kernel
    // always, the other cooperative kernels while their members wait for each other, trk_kernel_tp never
    const bool withhold = T.E.withhold && (L.kernel == 5 || (L.kernel != 3 && L.split > 1));
    const int nb = withhold ? L.n_blocks - 8 : L.n_blocks;
    const int8_t* codes = c->d_codes;
    switch (L.kernel) {
    case 2:   // (one workgroup per CU only matters while members wait for each other)
        sgx_trk2_launch(nb, st, S.d, codes, T.d_ch, T.d_out, T.d_done, T.K, T.d_prof, T.d_xch, T.d_err, sgx_dt_bytes(S.kind),
                        L.arms, L.split > 1 ? T.E.lds_pad : 0);
        break;
    case 3: sgx_trk_tp_launch(nb, st, S.d, codes, T.d_ch, T.d_out, T.d_done, T.K, T.d_prof, T.d_xch, T.d_err); break;
    case 4: sgx_trk_multi_launch(nb, st, S.d, codes, T.d_ch, T.d_out, T.d_done, T.K, T.d_prof, T.d_xch, T.d_err); break;
    case 5:
        sgx_trk3_launch(nb, st, S.d, codes, T.d_ch, T.d_out, T.d_done, T.K, T.d_prof, T.d_xch, T.d_err, T.E.lds_pad,
                        T.E.v3_generic || T.rep.scattered, T.E.scatter);
        break;
    case 6: sgx_trk_any_launch(nb, st, S.d, codes, T.d_ch, T.d_out, T.d_done, T.K, T.d_prof, T.d_xch, T.d_err); break;
    }
    hipEventRecord(c->ev[4], st);
    T.stamp("kernel queued");
    c->timing.track_kernel = (float)L.kernel;
    c->timing.track_members = (float)L.members;
    c->timing.track_streamed = streaming ? 1.f : 0.f;
    T.e = hipGetLastError();
    int words[2] = {0, 0};
    const int rc = trk_collect(T, words);
    if (rc != SGX_OK) return rc;
    reserved.drop();
    return trk_repeat(T, launch, words, again);
}

// After the last launch: ms_done (and the series out of the staging buffer), the profile, the entries no channel reached,
// the errors, the kernel time, the description's undo
static int trk_finish(TrkCall& T) {
    sgx_ctx* c = T.c;
    const int n_ch = T.n_ch, ms = T.ms;
    hipError_t e = T.e;
    if (T.fast_look && e == hipSuccess) {
        for (int i = 0; i < n_ch; ++i) T.ms_done[i] = c->h_look->trk.done[i];
        e = hipEventSynchronize(c->ev[4]);   // (the word is stored a moment before the kernels retire: the times need the event)
    } else {
        if (e == hipSuccess && !T.direct) e = hipMemcpyAsync(T.out, T.d_out, T.elems * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(T.ms_done, T.d_done, sizeof(int) * (size_t)n_ch, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    }
    T.stamp("ms_done copied");
    if (T.d_prof && e == hipSuccess) {
        // SGX_TRK_PROFILE=1: cycles per block of the kernel's phases (tools/r5_harvest.py and r6_harvest.py read these lines)
        std::vector<long long> hp(T2_PROF_STRIDE * (size_t)n_ch);
        hipMemcpy(hp.data(), T.d_prof, sizeof(long long) * hp.size(), hipMemcpyDeviceToHost);
        if (T.L.kernel == 2 || T.L.kernel == 5) {
            for (int i = 0; i < n_ch && i < 8; ++i)
                for (int mm = 0; mm < T.L.members; mm += (i == 0 ? 1 : T.L.members - 1))
                    fprintf(stderr, "[sgx trk2 profile] ch %d member %2d cycles/block: release->publish %.0f  publish->sums %.0f  "
                                    "sums->release %.0f\n", i, mm, (double)hp[T2_PROF_STRIDE * i + mm] / ms,
                            (double)hp[T2_PROF_STRIDE * i + 64 + mm] / ms, (double)hp[T2_PROF_STRIDE * i + 128 + mm] / ms);
        } else
        for (int i = 0; i < n_ch && i < 4; ++i)
            fprintf(stderr, "[sgx trk profile] ch %d cycles/block: map %.0f wait %.0f reduce %.0f filter %.0f\n", i,
                    (double)hp[64 * i] / ms, (double)hp[64 * i + 1] / ms, (double)hp[64 * i + 2] / ms,
                    (double)hp[64 * i + 3] / ms);
    }
    if (e != hipSuccess) {
        sgx_set_error("tracking kernel failed: %s", hipGetErrorString(e));
        return SGX_E_HIP;
    }
    if (T.direct) {
        // entries never reached keep the reference's initial values (tracking.py:65-94): zeros or +Inf
        const StepLook* slook = &c->h_look->step;   // (chained: preRun's table)
        for (int i = 0; i < n_ch; ++i) {
            if (T.chained && slook->prn[i] == 0) continue;      // (a channel that is off: the caller gets the first n_active rows)
            const int dn = T.chained ? T.ms_done[i] : ((T.ch[i].prn == 0) ? 0 : T.ms_done[i]);
            if (dn >= ms) continue;
            for (int sidx = 0; sidx < SGX_NUM_SERIES; ++sidx) {
                const bool zero = (sidx == 0) || (sidx >= 3 && sidx <= 8);
                double* row = T.out + ((size_t)i * SGX_NUM_SERIES + (size_t)sidx) * (size_t)ms;
                for (int t = dn; t < ms; ++t) row[t] = zero ? 0.0 : INFINITY;
            }
        }
    }
    if (T.h_err != 0) {
        sgx_set_error("tracking kernel: channel %d reported a timeout with split %d", T.h_err - 1, T.K.split);
        return SGX_E_HIP;
    }
    const sgx_if* r = T.S.rec;
    if (r && r->loader && r->load_rc.load() != SGX_OK) return sgx_if_require(r, r->n);   // the loader failed while the kernel ran
    hipEventElapsedTime(&c->timing.track_ms, c->ev[3], c->ev[4]);
    T.stamp("done");
    // THE UNDO.  The kernel tracked a power of two times the caller's samples (scaled on conversion, or narrowed to integers):
    // the six correlator series carry the factor (exact), everything the discriminators made of them (ratios) does not.  It
    // reported absoluteSample, fid.tell() in the reference (tracking.py:255), in bytes of what it read: those of a narrowed
    // window map back to bytes of the caller's file.  Only rows that were written: a silent channel's are, an off channel has none.
    const TrkSource& S = T.S;
    const bool moved = S.pos_a != 1.0 || S.pos_b != 0.0;
    for (int i = 0; i < n_ch && !T.chained && (moved || S.sums != 1.0); ++i) {
        if (T.ch[i].prn == 0) continue;
        double* o = T.out + (size_t)i * SGX_NUM_SERIES * (size_t)ms;
        const int dn = T.ms_done[i] < ms ? T.ms_done[i] : ms;
        for (int t = 0; t < dn && moved; ++t) o[t] = o[t] * S.pos_a + S.pos_b;
        for (int sidx = 3; sidx <= 8 && S.sums != 1.0; ++sidx)
            for (int t = 0; t < dn; ++t) o[(size_t)sidx * ms + t] *= S.sums;
    }
    return SGX_OK;
}

// Why a launch that completed ended a channel early, from what the kernels write anyway (nothing is added to a block chain).
// A block whose six sums are exactly zero - a zero-filled stretch of the record - makes both discriminators 0 / 0: that
// block is recorded with NaN rates, and no kernel starts the next one (a NaN step fails every kernel's test of the block
// length: prep_code's stop, the latency kernels' (unsigned)(blk - 1) >= lim).  The reference dies there in
// int(np.ceil(nan)) (tracking.py:148-151): one report for every kernel, SGX_E_SILENT.  A channel whose last row is finite
// ran out of record (ms_done says so, SGX_OK) or reached a block beyond the launch's units (SGX_E_RANGE).
// Why no kernel reads another block behind the NaN one, per kernel:
//   trk3_kernel, trk2_kernel  the next block's length is (int)ceil(q) of a NaN quotient - 0 on the device, which the evaluator
//       test of sgx_block_length holds (tests/test_trk_math_gpu.py) - so (unsigned)(blk - 1) >= lim posts stop 1 with the
//       parameters; every role tests stop before it touches the block (the speculative pass of trk3 ran on block k's finite
//       rates, and every load address is an integer position clamped to the allocation).  Their per-block chains are left as
//       they are: unlike prep_code they have no test of the step itself.
//   trk_kernel_tp, _multi, _any (per-sample), the float instances  prep_code posts stop = 1 for a step that is not > 0 (tested on
//       the step, not on what (int) makes of NaN), and the loops test stop first, before a ramp or an address is formed.
// ch, or (chained: ch is null) look_prn, preRun's table: which channels are off.  zero_sums: what was exactly zero when the
// rates became NaN, in front of the block's number - "its block", or the coherent call's "the update behind its block" (the
// sums of a group of blocks; all zero, the group's last block is).  range_ch1: 1 + the channel that reached a block beyond
// the launch's n_units (0: none).
int sgx_trk_diagnose(const sgx_chan_init* ch, const int32_t* look_prn, int n_ch, int ms, const double* out, const int32_t* ms_done,
                     const char* zero_sums, int range_ch1, int n_units, double dll_bw) {
    for (int i = 0; i < n_ch; ++i) {
        if (ch ? ch[i].prn == 0 : look_prn[i] == 0) continue;
        const int dn = ms_done[i];
        if (dn < 1 || dn >= ms) continue;
        const double* row = out + (size_t)i * SGX_NUM_SERIES * (size_t)ms + (size_t)(dn - 1);
        const double codeFreq = row[(size_t)ms];
        if (codeFreq != codeFreq) {
            bool zero = true;   // (the six sums of the block, series 3 .. 8)
            for (int sidx = 3; sidx <= 8; ++sidx) zero = zero && row[(size_t)sidx * (size_t)ms] == 0.0;
            if (zero)
                sgx_set_error("ValueError: cannot convert float NaN to integer: channel %d went silent - the six sums of %s "
                              "%d are exactly zero (a zero-filled stretch of the record), the loop filters' rates are "
                              "NaN, and block %d has no length", i, zero_sums, dn - 1, dn);
            else   // (NaN some other way - a loop filter that left the finite numbers: the reference dies at the same place)
                sgx_set_error("ValueError: cannot convert float NaN to integer: channel %d - the loop filters' rates are NaN "
                              "after block %d (its sums are not zero: the filters diverged), and block %d has no length",
                              i, dn - 1, dn);
            return SGX_E_SILENT;
        }
    }
    if (range_ch1) {
        sgx_set_error("tracking: channel %d reached a block longer than the %d units of %d samples the kernel "
                      "provides (the code NCO left its plausible range; dllNoiseBandwidth %g)",
                      range_ch1 - 1, n_units, TRK_UNIT, dll_bw);
        return SGX_E_RANGE;
    }
    return SGX_OK;
}

// sample_bytes: 1 (int8 record) or 2 (little-endian int16 record; the record handle holds the file's BYTES).  The
// reference seeks skipNumberOfBytes + codePhase BYTES whatever the sample type and reports fid.tell(), also bytes
// (tracking.py:107, 255); so a two-byte channel may start on an odd byte - its samples then straddle the file's - and
// the kernel follows it there (per-channel byte shift of the record pointer, unaligned 16-byte loads).
// What the call runs on - the record as it lies, or what the float front made of it - and how its results are undone: S
// (TrkSource, sgx_trk_common.h).
// chained (round 6, sgx_track_chained): `ch` is null - the channel table is made ON THE DEVICE by the preRun kernel queued
// in front of the first launch (sgx_prerun_enqueue, sgx_acq.hip) from the acquisition that is pending on this context.
int sgx_track_source(sgx_ctx* c, const TrkSource& S, const TrkEnv& E, const sgx_chan_init* ch, int n_ch, int ms, double* out,
                     int32_t* ms_done) {
    const bool chained = !ch;
    SGX_CHECK_ARG(n_ch >= 1 && n_ch <= 65535 && ms >= 1);
    if (!(c->s.dllCorrelatorSpacing > 0.0 && c->s.dllCorrelatorSpacing < 1.0)) {
        // beyond one chip the reference's replica index ceil(t) leaves its 1025-entry code table (or wraps)
        sgx_set_error("dllCorrelatorSpacing %g outside (0, 1) chips", c->s.dllCorrelatorSpacing);
        return SGX_E_ARG;
    }
    SGX_HIP(hipSetDevice(c->device));
    TrkCall T{c, S, ch, n_ch, ms, out, ms_done, chained, E, std::chrono::steady_clock::now()};
    SGX_HIP(hipDeviceGetAttribute(&T.cus_total, hipDeviceAttributeMultiprocessorCount, c->device));
    // THE RULE (trk_plan above), with the diagnostic overrides of this process's environment
    T.P = trk_plan(c->s, S.kind, n_ch, (long long)c->n_code, T.cus_total, S.float_typed, E.split, E.arms, E.v3_off);
    sgx_trk_const(T.K, c->s, (long long)c->n_code, S.n, S.kind, S.file_off, ms, n_ch, T.P.multi);
    T.K.fast_xcd = E.fast_xcd ? 1 : 0;
    T.K.fscale = S.fscale;
    int rc = sgx_trk_units_check((long long)c->n_code, T.P.n_units);
    if (rc == SGX_OK) rc = trk_buffers(T);
    if (rc != SGX_OK) return rc;
    if (chained && S.rec->loader && !S.rec->load_done.load()) return SGX_E_DEFER;   // (a record that is still streaming in)
    CuGuard reserved{c->device, 0};
    bool again = true;
    // at most five launches: a repeat has a cause in T.rep (trk_repeat), said on stderr
    for (int launch = 0; launch < 5 && again; ++launch) {
        rc = trk_launch_once(T, launch, reserved, again);
        if (rc != SGX_OK) return rc;
    }
    rc = trk_finish(T);
    if (rc != SGX_OK) return rc;
    return sgx_trk_diagnose(ch, c->h_look->step.prn, n_ch, ms, out, ms_done, "its block", T.range_ch1, T.L.n_units, c->s.dllNoiseBandwidth);
}

// A record of `kind` samples tracked as it lies; float32 / float64 records enter through the float front, which may describe
// them otherwise (sgx_trk_f32.hip)
int sgx_track_kind(sgx_ctx* c, const sgx_if* r, int64_t rec_file_offset, const sgx_chan_init* ch, int32_t n_ch,
                   int32_t ms, double* out, int32_t* ms_done, int kind) {
    SGX_CHECK_ARG(c && r && ch && out && ms_done && n_ch >= 1 && ms >= 1 && sgx_dt_bytes(kind) >= 1);
    if (kind == SGX_DT_FLOAT32 || kind == SGX_DT_FLOAT64) return sgx_track_float(c, r, rec_file_offset, ch, n_ch, ms, out, ms_done, kind);
    TrkSource S;
    const int rc = sgx_trk_source(S, c->s, r, (long long)rec_file_offset, ch, n_ch, kind);
    return rc == SGX_OK ? sgx_track_source(c, S, sgx_trk_env(), ch, n_ch, ms, out, ms_done) : rc;
}

// include/sgx.h: preRun on the device behind the pending acquisition, the tracking kernel behind it, ONE wait.
extern "C" int sgx_track_chained(sgx_ctx* c, const sgx_if* r, int64_t rec_file_offset, int32_t n_ch, int32_t ms, double* out,
                                 int32_t* ms_done, int32_t data_type, int32_t* prn, double* acquiredFreq, double* codePhase,
                                 int32_t* n_active) {
    SGX_CHECK_ARG(c && r && out && ms_done && prn && acquiredFreq && codePhase && n_active);
    // (n_ch <= 8: the eager sequence launches the ACTIVE channels only, and which kernel runs depends on their number
    // rounded up to 8 - with at most 8 configured channels that is the same launch whatever preRun finds)
    if (c->acq_pending.mode != 1 || n_ch < 1 || n_ch > 8) return SGX_E_DEFER;
    if (data_type != SGX_DT_INT8 && data_type != SGX_DT_UINT8) return SGX_E_DEFER;
    TrkSource S;   // (no host table: preRun makes it on the device; tracked as it lies, nothing to undo)
    (void)sgx_trk_source(S, c->s, r, (long long)rec_file_offset, nullptr, n_ch, data_type);
    const int rc = sgx_track_source(c, S, sgx_trk_env(), nullptr, n_ch, ms, out, ms_done);
    if (rc != SGX_OK && rc != SGX_E_SILENT) return rc;
    // (the stream has been synchronised: the page is complete - also for a silent channel, whose rows the caller reads with
    // the table below)
    const StepLook* look = &c->h_look->step;
    if (look->n_ch != n_ch || look->flags != 0) return SGX_E_DEFER;   // a NaN metric, a failed search, a channel in front of
                                                                       // the record: nothing was tracked, the eager calls report it
    *n_active = look->n_active;
    for (int i = 0; i < n_ch; ++i) {
        prn[i] = look->prn[i];
        acquiredFreq[i] = look->acquiredFreq[i];
        codePhase[i] = look->codePhase[i];
    }
    return rc;
}

extern "C" int sgx_track(sgx_ctx* c, const sgx_if* r, int64_t rec_file_offset, const sgx_chan_init* ch,
                         int32_t n_ch, int32_t ms, double* out, int32_t* ms_done) {
    return sgx_track_kind(c, r, rec_file_offset, ch, n_ch, ms, out, ms_done, SGX_DT_INT8);
}

extern "C" int sgx_track_ex(sgx_ctx* c, const sgx_if* r, int64_t rec_file_offset, const sgx_chan_init* ch,
                            int32_t n_ch, int32_t ms, double* out, int32_t* ms_done, int32_t data_type) {
    if (sgx_dt_bytes(data_type) == 0) {
        sgx_set_error("sgx_track_ex: data_type %d is not one of SGX_DT_* (include/sgx.h)", (int)data_type);
        return SGX_E_ARG;
    }
    return sgx_track_kind(c, r, rec_file_offset, ch, n_ch, ms, out, ms_done, data_type);
}
