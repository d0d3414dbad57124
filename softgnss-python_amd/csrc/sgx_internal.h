// Internal declarations shared by the translation units of libsgx.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

#include "sgx.h"
#include "sgx_check.h"   // sgx_set_error, SGX_CHECK_ARG, SGX_VERSION_STR: all that the HIP-free host files need
#include "sgx_count.h"   // SGX_COUNT_SLOTS, SGX_COUNT_STRIDE: the layout of SgxSmall::stage_count

#define SGX_HIP(call)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) {                                                                \
            sgx_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__,    \
                          __LINE__);                                                           \
            return SGX_E_HIP;                                                                  \
        }                                                                                      \
    } while (0)

typedef double2 cplx;   // complex128 as (re, im)

// A device allocation and its size: the context's grow-only scratch as members, a call's temporaries as locals.  Frees
// itself; not copyable.  Reads as the pointer it holds.
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;   // bytes
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    // Room for `bytes`: the allocation is kept where it is large enough, else freed and made anew (the contents are lost).
    // On failure the buffer is empty.
    int ensure(size_t bytes) {
        if (p && cap >= bytes) return SGX_OK;
        release();
        const hipError_t e = hipMalloc((void**)&p, bytes);
        if (e != hipSuccess) {
            p = nullptr;
            sgx_set_error("hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
            return SGX_E_NOMEM;
        }
        cap = bytes;
        return SGX_OK;
    }
    void release() {
        if (p) hipFree(p);
        p = nullptr;
        cap = 0;
    }
    T* get() const { return p; }
    operator T*() const { return p; }
};

// The samples an acquisition reads: the int8 record (Settings.dataType 'int8'), or - acquire() handed any other real
// array (acquisition.py:55-59 works on whatever numpy dtype it gets) - an fp64 copy of it.
struct SgxSig {
    const int8_t* i8;
    const double* f64;
#ifdef __HIPCC__
    __device__ __forceinline__ double at(long long i) const { return f64 ? f64[i] : (double)i8[i]; }
#endif
};

// One FFT length and every table the kernels launched with this plan read, W_N^t = hi[t >> lo_bits] * lo[t & lo_mask] among
// them.  sgx_fft_plan_create uploads them as ONE device allocation (`tables`), which sgx_fft_plan_destroy frees; the other
// pointers are carved from it.  A plan without tables (n set by hand) serves host arithmetic only.
struct FftPlan {
    int64_t n = 0;
    int lo_bits = 0;
    std::vector<int> radices;
    void* tables = nullptr;             // device
    cplx* tw_hi = nullptr;
    cplx* tw_lo = nullptr;
    cplx* wr[32] = {};                  // wr[R][m] = W_R^m, m < R, for every radix R of the plan
    cplx* f4_sub[2] = {};               // four-step length only: W_217^t | W_176^t
    cplx* fine[3] = {};                 // fine-search length only: W_1024^t | W_4096^(64 h) | W_4096^l
    int cus = 0;                        // fine-search length only: compute units of the plan's device
};

// The tables of one segment length of a short-time-transform stage (sgx_seg_fft.h), in ONE device allocation the plan owns
// and kept with the context until another length is asked for: tw[t] = W_n^t, t < n / 2 (seg_twiddles), then what the stage
// adds - the excision its root-Hann window win[n] (ex_tables), the monitor nothing on the device (the sum of its squared
// window, which the table implies, stays beside its plan in the context).
struct SegPlan {
    int n = 0;
    DevBuf<double> tables;
    bool holds(int n_seg) const { return n == n_seg && tables.get(); }
    // The tables of length n_seg as the stage computed them on the host: `count` doubles
    int upload(int n_seg, const double* h, size_t count) {
        n = 0;
        const int rc = tables.ensure(sizeof(double) * count);
        if (rc != SGX_OK) return rc;
        SGX_HIP(hipMemcpy(tables.get(), h, sizeof(double) * count, hipMemcpyHostToDevice));
        n = n_seg;
        return SGX_OK;
    }
    const cplx* tw() const { return reinterpret_cast<const cplx*>(tables.get()); }
    const double* extra() const { return tables.get() + n; }     // behind the n / 2 complex twiddles
};
void ex_tables(int n_seg, cplx* tw, double* win);

// sgx_iq.hip: the padded length of one polyphase branch of the longest filter (cp = 64, d up to 64, rounded up to 8)
#define SGX_IQ_LP_MAX 136

// sgx_requant.hip: the fixed grid of the statistics pass (the float sums are reproducible because it is fixed) and its loads
// in flight per lane
#define RQ_STATS_BLOCKS 2048
#define RQ_STATS_UNROLL 4

// sgx_array.hip: the copies of rho the statistics kernel spreads its per-workgroup sums over, each of AR_SUM_VALUES int64
// values (A^2 K lanes <= 8 x 64 x 2 of them used)
#define AR_SUM_SLOTS 8
#define AR_SUM_VALUES 1024

// The record front-end stages, one per entry point that runs through sgx_stage_run (sgx_stage.h): sgx_if_filter,
// sgx_if_from_iq, sgx_requant_stats_of, sgx_if_requantize, sgx_cond_block_stats, sgx_if_condition, sgx_if_unpack, sgx_if_decimate,
// sgx_if_resample, sgx_array_stats, sgx_if_combine, sgx_array_block_stats, sgx_if_combine_blocks, sgx_if_excise, sgx_if_cancel
enum SgxStageSlot { SGX_STAGE_FILTER, SGX_STAGE_IQ, SGX_STAGE_REQUANT_STATS, SGX_STAGE_REQUANT, SGX_STAGE_COND_STATS,
                    SGX_STAGE_COND_APPLY, SGX_STAGE_UNPACK, SGX_STAGE_DECIM, SGX_STAGE_RESAMP, SGX_STAGE_ARRAY_STATS,
                    SGX_STAGE_COMBINE, SGX_STAGE_ARRAY_BLOCK_STATS, SGX_STAGE_COMBINE_BLOCKS, SGX_STAGE_EXCISE, SGX_STAGE_CANCEL,
                    SGX_STAGE_SLOTS };

struct sgx_if {
    int8_t* d = nullptr;   // device pointer; allocation is padded by SGX_IF_PAD zero bytes
    size_t n = 0;
    size_t cap = 0;        // bytes of the allocation behind d (>= n + SGX_IF_PAD)
    int device = 0;
    // background file -> HBM streaming (sgx_if_open_file): samples [0, host_mark) are resident
    std::thread* loader = nullptr;
    std::atomic<size_t> host_mark{0};        // bytes whose copy has completed, as the host knows it
    std::atomic<int> load_rc{0};             // SGX_OK while running / after success, an error code otherwise
    std::atomic<bool> load_done{false};
    std::atomic<long long> mag_max{-1};      // largest sum of magnitudes (bytes read as int8) over 17 consecutive 128-byte
                                             // blocks = a bound for every 2 048-byte window; -1: not scanned yet (sgx_trk.hip)
    unsigned long long* d_mark = nullptr;    // the same watermark in device memory, advanced in copy-stream order
    hipStream_t copy_stream = nullptr;
    char load_err[256] = {0};
};
// sgx_record.cpp
// Block until samples [0, end) of a (possibly still streaming) record are resident; returns the loader's status.
int sgx_if_require(const sgx_if* r, size_t end);
// A new record of n samples on the context's device, for the stages that write one.  sgx_if_free is the one way out of it.
int sgx_if_alloc_internal(sgx_ctx* c, size_t n, sgx_if** out);
// One record allocation, streaming watermark and copy stream kept from the last sgx_if_free: a caller that opens a
// record file per step (the reference's, initialize.py:466-506) would otherwise pay hipMalloc + hipFree of 1.4 GB and
// a stream creation every time (milliseconds against a 50 ms step).  Every method locks; release() is the teardown.
#define SGX_IF_PAD 256
struct RecordSpare {
    // The parked allocation where it fits a record of n samples (large enough and not absurdly larger), else null
    int8_t* take(size_t n, size_t* cap_out) {
        std::lock_guard<std::mutex> g(mu);
        if (!d || cap < n + SGX_IF_PAD || cap > 2 * (n + SGX_IF_PAD) + (1u << 20)) return nullptr;
        *cap_out = std::exchange(cap, 0);
        return std::exchange(d, nullptr);
    }
    // Gives the parked allocation back to the device (it may be what is in the way of a hipMalloc); false: none was parked
    bool drop() {
        std::lock_guard<std::mutex> g(mu);
        if (!d) return false;
        hipFree(std::exchange(d, nullptr));
        cap = 0;
        return true;
    }
    unsigned long long* take_mark() {
        std::lock_guard<std::mutex> g(mu);
        return std::exchange(mark, nullptr);
    }
    hipStream_t take_stream() {
        std::lock_guard<std::mutex> g(mu);
        return std::exchange(stream, nullptr);
    }
    // What a freed record leaves: the larger allocation wins, the first watermark and the first stream are kept.  What is
    // parked is taken out of *r.  SGX_IF_SPARE=0 parks no allocation, SGX_STREAM_PRIO (set) no stream.
    void park(sgx_if* r) {
        std::lock_guard<std::mutex> g(mu);
        const char* sp = getenv("SGX_IF_SPARE");   // '0': nothing is parked, a freed record's memory goes back at once
        if (r->d && r->cap > cap && !(sp && sp[0] == '0')) {
            if (d) hipFree(d);
            d = std::exchange(r->d, nullptr);
            cap = r->cap;
        }
        if (r->d_mark && !mark) mark = std::exchange(r->d_mark, nullptr);
        if (r->copy_stream && !stream && !getenv("SGX_STREAM_PRIO")) stream = std::exchange(r->copy_stream, nullptr);
    }
    // Device memory first, then the stream
    void release() {
        drop();
        if (unsigned long long* m = take_mark()) hipFree(m);
        if (hipStream_t s = take_stream()) hipStreamDestroy(s);
    }
    RecordSpare() = default;
    RecordSpare(const RecordSpare&) = delete;
    RecordSpare& operator=(const RecordSpare&) = delete;
    ~RecordSpare() { release(); }

private:
    std::mutex mu;
    int8_t* d = nullptr;
    size_t cap = 0;
    unsigned long long* mark = nullptr;
    hipStream_t stream = nullptr;
};
// Tracking (sgx_trk.hip).  kind: SGX_DT_*.  int8 / uint8 / int16 run the typed kernels (sgx_trk2 / sgx_trk3 / sgx_trk_tp);
// every other type - and int16 / uint8 at sampling rates below 16 x the chip rate - the per-sample kernel of sgx_trk_any.hip.
// The one entry of every eager tracking call.  It describes what the call runs on (TrkSource, sgx_trk_common.h: the bytes, the
// sample kind, every channel's start, the undo) and runs that description; the chained call makes its own, without a host table.
int sgx_track_kind(sgx_ctx* c, const sgx_if* r, int64_t rec_file_offset, const sgx_chan_init* ch, int32_t n_ch,
                   int32_t ms, double* out, int32_t* ms_done, int kind);
// The float front (sgx_trk_f32.hip), sgx_track_kind's way for float32 / float64: one scan of the window the channels can reach
// picks the route - the per-sample kernel, the latency-mode kernel on samples scaled by a power of two, or (float32) an exact
// int8 / int16 copy of the window with the map back to the caller's file - and the description says which.
int sgx_track_float(sgx_ctx* c, const sgx_if* r, int64_t rec_file_offset, const sgx_chan_init* ch, int32_t n_ch, int32_t ms,
                    double* out, int32_t* ms_done, int kind);

// ---- acquisition (sgx_acq.hip): the limits and the small structs its kernels hand to each other and to the host ----
#define ACQ_MAX_BINS 128          // Doppler bins of the 1-ms search
#define ACQ_MAX_ROWS 2048         // correlation rows of one batch
#define ACQ_COH_MAX_BINS 1024     // Doppler bins of the coherent search
#define SGX_FINE_PARTIALS 512     // per-detection partial maxima of the fine search (sgx_fft_fine_partials())

struct SecondArgs {
    int row[32];          // power row to search, -1 = skip
    int lo0[32], hi0[32]; // first index range [lo0, hi0)
    int lo1[32], hi1[32]; // second index range
};

// The peak logic's outcome for every PRN of a call (acquisition.py:129-162)
struct PeakOut {
    double peak[32];
    int cph[32], fbi[32];
    int index_error[32];
};
// The coarse search's outcome, written by one small kernel straight into a coherent pinned page: the host spins on
// `seq` instead of sleeping in hipStreamSynchronize behind two device-to-host copies (~55 us -> ~10 us between the last
// coarse kernel and the first fine one).
struct CoarseLook {
    PeakOut po;
    double second[32];
    unsigned long long seq;
    // device-led fine search (round 4): the detections the publish kernel found (in PRN order, as the reference's loop
    // finds them), and what the fine search made of them - the host looks ONCE, at seq2
    int n_det;
    int range_error;          // a detection's fine window (code phase + 10 ms) leaves the record: 1 + its slot
    int det_slot[32];         // position in the call's PRN list
    int det_phase[32];
    long long fine_bi[32];    // arg-max of the 2^22-point magnitude spectrum over [4, uniq - 5)
    unsigned long long seq2;
};

// The detection list in device memory: the coarse search's publish step (sgx_acq.hip) writes it, the device-led fine
// kernels (sgx_fft.hip) read it, so that they are queued right behind the coarse ones without the host looking in between
struct AcqDet {
    int n_det;                // (0 on a range error: the fine kernels have nothing to do)
    int prn[32];              // PRN index of detection d, in ascending position of the call's PRN list
    int phase[32];            // its code phase
    int pad[15];
    unsigned fine_done;       // fine_rows_kernel's arrival counter (zero between calls)
};

// Where an acquisition call leaves its results: the caller's five arrays, one entry per PRN of the call's list
struct AcqOut {
    double *carrFreq, *codePhase, *peakMetric;
    int32_t *freqBin, *fineIdx;
};
// ... and the same results kept by the library for up to 32 PRNs
struct AcqResults {
    double carrFreq[32], codePhase[32], peakMetric[32];
    int32_t freqBin[32], fineIdx[32];
    AcqOut out() { return AcqOut{carrFreq, codePhase, peakMetric, freqBin, fineIdx}; }
};

struct PeakRec {      // a rank's peak in the sharded search = shard.PEAK_DTYPE, 40 bytes
    int prn0, freqBin;
    double carrFreq, codePhase, peakMetric;
    int fineIdx, valid;   // valid 1; 0 unused slot; -1 the reference's IndexError at this PRN; -2 its fine window leaves the record
};
static_assert(sizeof(PeakRec) == 40, "shard.PEAK_DTYPE");
// Entry i of a call's results as the valid record of PRN prn0, and a record into entry q.prn0 of the merged results
inline PeakRec peak_rec_pack(int prn0, const AcqOut& o, int i) {
    return PeakRec{prn0, o.freqBin[i], o.carrFreq[i], o.codePhase[i], o.peakMetric[i], o.fineIdx[i], 1};
}
inline void peak_rec_merge(const PeakRec& q, const AcqOut& o) {
    o.carrFreq[q.prn0] = q.carrFreq;
    o.codePhase[q.prn0] = q.codePhase;
    o.peakMetric[q.prn0] = q.peakMetric;
    o.freqBin[q.prn0] = q.freqBin;
    o.fineIdx[q.prn0] = q.fineIdx;
}

// The context's small device area (d_small) and its pinned mirror (h_small): one layout for both.  Every slot reaches the
// kernels as a pointer argument.  A slot is used through the device area, the mirror or both as its comment says.  (alignas:
// what hipMemsetAsync clears - a fill of an unaligned range takes the runtime several launches instead of one)
struct SgxSmall {
    long long sum;                          // record sum (mean for acquisition.py:59) of the paths that clear it themselves
    alignas(16) long long sum2[2];          // acq_front_kernel's two alternating slots (sgx_ctx::acq_sum_phase)
    int prn[32];                            // the call's PRN list
    int2 bin_map[ACQ_COH_MAX_BINS];         // (phi index, circular shift) per Doppler bin (four-step, coherent shift path)
    double rowmax[ACQ_MAX_ROWS];            // round-1 passes: row maxima of a chunk; both
    int rowarg[ACQ_MAX_ROWS];
    alignas(256) double second[32];         // second peaks; both
    int det_prn[32], det_phase[32];         // host-led fine search on the pass-per-launch transform
    alignas(256) int arrived[64];           // [32] rows finished per PRN, [32] PRNs finished
    double fine_pv[32 * SGX_FINE_PARTIALS]; // fine search: per-detection partial maxima and their indices; both
    long long fine_pi[32 * SGX_FINE_PARTIALS];
    int2 row_map[32 * 64];                  // rows the second-peak search transforms again (PRNs x blocks); both
    SecondArgs second_args;
    PeakOut peak_out;
    AcqDet det;
    CoarseLook stage;                       // device-side copy of the result page (device-led search)
    PeakRec shard[32];                      // sgx_acquire_sharded without a communicator: the packed records
    double frq[ACQ_COH_MAX_BINS];           // coherent search, direct path: the frequency table; both
    long long fine_win[64];                 // coherent search: arg-max range per detection; both
    int stage_prn[32];                      // mirror only: staging of the PRN list and the bin map (coherent shift path)
    int2 stage_bin_map[ACQ_COH_MAX_BINS];
    int trk_mag;                            // sgx_trk.hip: the record's magnitude bound
    uint8_t nav_bits[SGX_MAX_SATS][256];    // sgx_synth.hip: the scene's navigation bits
    // The record front-end stages: what sgx_stage_run (sgx_stage.h) copies up in front of a stage's kernel or down behind
    // it.  Every stage waits before it returns, so one call owns a slot at a time; both.
    // sgx_fir_dot4.h: (hi, lo) tap dwords of one sgx_if_filter, sgx_if_from_iq, sgx_if_decimate, sgx_if_resample or
    // sgx_if_combine call
    alignas(16) unsigned fir_taps[2 * ((SGX_FILTER_MAX_TAPS + 30) / 16) * 4];
    // sgx_requant.hip: one partial (sum, sum of squares, non-finite count, max) per workgroup of the statistics pass
    alignas(256) unsigned long long requant_part[RQ_STATS_BLOCKS * 4];
    // sgx_count.h: the counters of the stage that runs - outputs on the rails, blanked frames, codes, cut bins
    alignas(256) unsigned long long stage_count[SGX_COUNT_SLOTS * SGX_COUNT_STRIDE];
    // sgx_array.hip: the statistics kernel's copies of rho (int64 values, added modulo 2^64)
    alignas(256) unsigned long long array_sum[AR_SUM_SLOTS * AR_SUM_VALUES];
};
static_assert(2 * 2 * (SGX_IQ_LP_MAX / 4) <= sizeof(SgxSmall::fir_taps) / sizeof(unsigned),
              "the two branches of sgx_iq.hip fit the tap staging too");
#define SGX_SMALL_BYTES (1 << 20)
static_assert(sizeof(SgxSmall) <= SGX_SMALL_BYTES, "the small areas hold the layout");

// A DEFERRED acquisition (sgx_acquire_begin, round 6): every kernel of the search is queued, the host has not looked.
// mode 1: the device-led sequence is in flight (the result page's seq2 will equal `seq`); mode 2: the path could not be
// deferred, the search ran eagerly and its outputs wait in `res` for sgx_acquire_end.
struct AcqPending {
    int mode = 0;
    unsigned long long seq = 0;
    int n_prn = 0;
    int prn0[32];
    long long npts = 0, fine_len = 0;
    size_t n_samples = 0;
    bool split_event = false, spin = true;   // SGX_ACQ_SPLIT_EVENT / SGX_ACQ_SPIN as the queued call read them
    int rc = 0;                // mode 2: the eager search's return code
    AcqResults res;
};

// What the device-side preRun + a chained tracking launch leave in the result page
struct StepLook {
    int n_ch, n_active;         // channels of the table, channels that are on (acquisition.py:289)
    int flags;                  // 1 a NaN among the metrics (the host sorts); 2 IndexError / range error of the search (no
                                // channel is on); 4 a channel starts before the record
    int pad;
    int prn[32];
    double acquiredFreq[32], codePhase[32];
};
// The gathered peak records of sgx_acquire_sharded behind the word the host spins on: as many as the part has room for
struct GatherLook {
    unsigned long long seq;
    unsigned long long pad;
    PeakRec rec[(2048 - 16) / sizeof(PeakRec)];
};
// What a tracking launch leaves for the host's look (sgx_trk.hip: trk_finish_kernel, round 6): the word the host spins on,
// the two error words and ms_done of up to SGX_TRK_LOOK_CH channels, copied here by ONE small kernel behind the tracking
// kernel - instead of two copies to pageable memory with a stream synchronisation each (~80 us behind every launch)
#define SGX_TRK_LOOK_CH 256
struct TrkLook {
    unsigned long long seq;
    int err[2];
    int done[SGX_TRK_LOOK_CH];
};
// The result "page" (two pages of coherent pinned memory): every part a kernel publishes to and the host looks at, each
// at a fixed offset that no neighbour can grow into
struct LookPage {
    alignas(2048) CoarseLook coarse;
    alignas(2048) StepLook step;
    alignas(2048) GatherLook gather;
    alignas(2048) TrkLook trk;
};
static_assert(offsetof(LookPage, coarse) == 0 && offsetof(LookPage, step) == 2048 && offsetof(LookPage, gather) == 4096 &&
                  offsetof(LookPage, trk) == 6144 && sizeof(LookPage) == 8192,
              "every part of the result page where it has always been");
static_assert(offsetof(GatherLook, rec) == 16, "the gathered records start 16 bytes behind their word");

struct sgx_ctx {
    sgx_settings s;
    AcqPending acq_pending;
    int device = 0;
    int priority = 0;            // stream priority class of the context: -1 high, 0 normal, +1 low
    hipStream_t stream = nullptr;
    hipStream_t acq_stream2 = nullptr;        // second queue of the correlation batch (created on first use)
    hipEvent_t acq_ev2[2] = {nullptr, nullptr};
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    sgx_timing timing;
    int64_t n_code = 0;          // samplesPerCode
    int8_t* d_codes = nullptr;   // [32][1023] +-1
    // acquisition scratch (lazily sized)
    FftPlan plan_code;           // length samplesPerCode
    FftPlan plan_fine;           // length 8 * 2^ceil(log2(10 N))
    DevBuf<cplx> d_fwd;          // [n_blocks][n_bins][N] mixed-signal spectra
    DevBuf<cplx> d_codefd;       // [32][N] code spectra
    DevBuf<cplx> d_work[2];      // ping-pong [rows][N]
    DevBuf<double> d_pow;        // [rows][N] correlation power
    DevBuf<cplx> d_fine[2];
    DevBuf<double> d_sig64;      // fp64 copy of a non-int8 signal handed to sgx_acquire_f64
    SgxSmall* d_small = nullptr; // small device area
    int acq_sum_phase = 0;       // acq_front_kernel: which of the two record-sum slots this call adds into ...
    bool acq_sum_clean[2] = {false, false};   // ... and whether a slot is known to hold zero (the other call's set-up zeroed it)
    SgxSmall* h_small = nullptr; // pinned mirror
    LookPage* h_look = nullptr;  // coherent pinned page the kernels publish their outcomes to (the host spins on its words)
    LookPage* d_look = nullptr;  // its device address
    unsigned long long look_seq = 0;
    unsigned long long trk_seq = 0;
    // tracking
    DevBuf<double> d_trk_out;    // the series of a call whose result buffer is pageable
    DevBuf<char> d_trk_aux;      // per-call device state of sgx_track (channels, done, exchange, err, profile)
    RecordSpare spare;           // what the last freed record left for the next one
    // pinned staging buffers of the file streamer, kept between calls (pinning 64 MiB costs ~15 ms)
    void* stage[2] = {nullptr, nullptr};
    std::atomic<bool> stage_busy{false};
    // HIP-event times of the last sgx_track_replay (sgx_replay.hip): the kernel, and upload + kernel + result copy
    float replay_kernel_ms = 0.0f, replay_device_ms = 0.0f;
    // HIP-event time of the kernel of the last call of each record front-end stage, 0 where that call had no work
    // (sgx_stage.h: sgx_stage_run writes them, the four sgx_*_timing getters read them)
    float stage_ms[SGX_STAGE_SLOTS] = {};
    // front-end conditioning (sgx_cond.hip): the per-block statistics and the plan as the kernels write and read them
    // (grow-only)
    DevBuf<sgx_cond_stats> d_cond_stats;
    DevBuf<sgx_cond_entry> d_cond_plan;
    // the record monitor (sgx_waterfall.hip; sgx_probe_stats runs it too): its plan and the sum of the squared window of
    // the plan's length, the scratch rows of the segments in flight, the results on the device (grow-only) and the
    // HIP-event time of the kernels of the last sgx_probe_waterfall
    SegPlan plan_waterfall;
    double waterfall_w2 = 0.0;
    DevBuf<double> d_wf_rows;
    DevBuf<char> d_wf_out;
    float waterfall_ms = 0.0f;
    // block-adaptive antenna combining (sgx_array.hip): the statistics of every block as the kernel adds them up, int64
    // [n_blocks][A][A][K][lanes], and the tap images of every block as the combiner reads them (grow-only)
    DevBuf<unsigned long long> d_array_blocks;
    DevBuf<uint2> d_array_taps;
    // swept-interference excision (sgx_excise.hip): its plan and the cut bins of every segment as the kernel leaves them
    // (grow-only)
    SegPlan plan_excise;
    DevBuf<uint16_t> d_excise_cut;
    // strong-signal cancellation (sgx_cancel.hip): the block table and the channels as the kernel reads them (grow-only)
    DevBuf<char> d_cancel;
    // Everything above that the context owns goes here and nowhere else (sgx_host.cpp); safe on a partly built context
    ~sgx_ctx();
};

// sgx_host.cpp
// The host's wait for a word of the result page: spins on it (where `spin`; the clock is read every `stride` looks) for
// up to budget_s seconds, then sleeps in the stream synchronisation, after which the page is complete in any case, and
// looks once more; `unwritten` is the error text if the word still differs from seq.  A synchronisation that fails is an
// error here where sync_err is null; else it is handed back in *sync_err for the caller to report, with SGX_OK.
int sgx_look_wait(hipStream_t st, const unsigned long long* word, unsigned long long seq, bool spin, double budget_s,
                  unsigned stride, const char* unwritten, hipError_t* sync_err);
// Compute units claimed by this process's cooperative tracking launches (all contexts of a device): `want` CUs are
// granted (returned) only if they fit next to what is already running, else 0.
int sgx_cu_reserve(int device, int cus_total, int want);
void sgx_cu_release(int device, int n);
// sgx_core.cpp
int sgx_host_ca_code(int prn0, int8_t* out /*1023*/);
int64_t sgx_host_samples_per_code(const sgx_settings* s);

// sgx_fft.hip
int sgx_fft_plan_create(FftPlan* p, int64_t n);
// The length a circular correlation of n points runs on: n where it factors into 2..31, else a padded length >= 2 n - 1
// that does (sgx_fft.hip states the rule); 0 where n is out of range.  Host arithmetic only.
int64_t sgx_fft_corr_length(int64_t n);
void sgx_fft_plan_destroy(FftPlan* p);
// Forward DFT of `rows` contiguous rows of length p->n. Result lands in *result (a or b).
int sgx_fft_forward(const FftPlan* p, cplx* a, cplx* b, int64_t rows, hipStream_t st, cplx** result,
                    int64_t nonzero_len);

// Optional fusion of the acquisition's pointwise kernels into the first / last radix pass.
struct FftFuse {
    const cplx* mul_x = nullptr;   // first pass input = conj(mul_x[bk]) * mul_f[prn]
    const cplx* mul_f = nullptr;
    const int2* row_map = nullptr; // device (bk, prn) per row, or null for the regular batch layout
    int rows_per_prn = 1;
    int prn_base = 0;
    double* pmax = nullptr;        // last pass: per-workgroup (max, first index) of |.|^2 * inv_n^2
    int* parg = nullptr;
    double inv_n = 0.0;
    int64_t n_valid = 0;           // last pass: only outputs k < n_valid count (0: all of them)
};
int sgx_fft_forward_fused(const FftPlan* p, cplx* a, cplx* b, int64_t rows, hipStream_t st, cplx** result,
                          int64_t nonzero_len, const FftFuse* fuse);
int sgx_fft_last_pass_blocks(const FftPlan* p);
// The radix passes sgx_fft_plan_create would set up for length n, in the order they run, and each pass's workgroup width;
// false where n does not factor into 2..31.  Host arithmetic only.
bool sgx_fft_pass_list(int64_t n, std::vector<int>* radices, std::vector<int>* tpb);

// Four-step transform with LDS-resident sub-transforms (sgx_fft.hip), for the lengths it is instantiated for.
struct Fft4Fuse {
    const cplx* mul_x = nullptr;   // columns kernel input = conj(mul_x[b * n_phi + phi][(i + shift) mod n]) * mul_f[prn][i]
    const cplx* mul_f = nullptr;
    const int2* bin_map = nullptr; // device, per Doppler bin: (phi index, circular shift)
    const int2* row_map = nullptr; // device (block * n_bins + bin, prn) per row, or null for the regular batch layout
    int n_bins = 1, n_phi = 1, rows_per_prn = 1, prn_base = 0;
    int n_blocks = 1, blocks_fast = 0;   // regular batch rows ordered (prn, bin, block) instead of (prn, block, bin)
    double* pmax = nullptr;        // rows kernel: per-workgroup (max, first index) of |.|^2 * inv_n^2 ...
    int* parg = nullptr;
    double* pout = nullptr;        // ... or the powers themselves, [rows / sum_blocks][n]
    double inv_n = 0.0;
    int sum_blocks = 1;            // powers of this many consecutive rows are added before the reduction / store
    // ... or, per output row p, the maximum power over the index ranges [sec[32 + p], sec[64 + p]) and [sec[96 + p],
    // sec[128 + p]) folded into second_out[p] (integer atomic max on the bit pattern; rows with sec[p] < 0 are skipped):
    // the second-peak search (acquisition.py:162) without a stored row
    const int* sec = nullptr;
    double* second_out = nullptr;
    // ... or, per output row and residue k mod sgx_fft4_residues(): the maximum power, the maximum of the residue's other
    // powers and the maximum's first index ([rows / sum_blocks][residues] each): peak AND second peak from one pass
    double* t2_b1 = nullptr;
    double* t2_b2 = nullptr;
    int* t2_i1 = nullptr;
};
bool sgx_fft_fine_supported(int64_t npts);
int sgx_fft_fine_partials(void);
// One fine search on the two-kernel 2^22-point transform (sgx_fft.hip): n_det detections, two per complex row.
struct FineSearch {
    // the signal and the codes
    SgxSig x = {nullptr, nullptr};
    const int8_t* codes = nullptr;          // device [32][1023]
    long long len = 0;                      // 10 N samples of signal, zeros beyond
    const long long* d_sum = nullptr;       // device: sum of the record window; mean = sum / n_mean
    double n_mean = 0.0, ts = 0.0, tc1 = 0.0;
    cplx* work = nullptr;                   // [(n_det + 1) / 2][2^22] intermediate
    // the detections, host-led: the list (host memory, <= 32) and the arg-max range [lo, hi), or per detection the device
    // ranges win[2 d], win[2 d + 1] inside it
    int n_det = 0;                          // (device-led: the most the list can hold)
    const int* det_prn = nullptr;
    const int* det_phase = nullptr;
    long long lo = 0, hi = 0;
    const long long* win = nullptr;
    // ... or device-led: the list in device memory; the last workgroup copies stage_words dwords from stage_src (device) to
    // stage_dst (the pinned page), folds the partial maxima into out_bi[32] (the page) and then stores seq to *out_seq
    const AcqDet* d_det = nullptr;
    const int* stage_src = nullptr;
    int* stage_dst = nullptr;
    int stage_words = 0;
    long long* out_bi = nullptr;
    unsigned long long* out_seq = nullptr;
    unsigned long long seq = 0;
    // the outputs: per-detection partial maxima and their indices, [n_det][sgx_fft_fine_partials()] each (device)
    double* pv = nullptr;
    long long* pi = nullptr;
};
int sgx_fft_fine_search(const FftPlan* plan, const FineSearch& f, hipStream_t st);
bool sgx_fft4_supported(int64_t n);
int sgx_fft4_row_blocks(void);
int sgx_fft4_residues(void);
int sgx_fft4_forward(const FftPlan* p, const cplx* in, cplx* work, cplx* out, int64_t rows, hipStream_t st,
                     const Fft4Fuse* fuse);

// sgx_acq.hip: preRun (acquisition.py:259-306) on the device, behind a deferred acquisition: channel table -> d_ch (what the
// tracking kernels read) and the result page's StepLook.  d_ch: TrkChan[n_ch] in device memory.
struct TrkChan {      // one channel as the tracking kernels read it
    double acquiredFreq;
    long long pos0;   // record index of the channel's first sample
    int prn;          // 1-based, 0 = off
    int pad;          // two-byte samples: byte shift (0 / 1) of the channel's sample grid in the record; else 0
};
int sgx_prerun_enqueue(sgx_ctx* c, TrkChan* d_ch, int n_ch, long long skip_bytes, long long rec_file_offset, int sample_bytes);
// Wait for a deferred acquisition and decode it (the tail of the eager call); clears c->acq_pending.
int sgx_acquire_finish(sgx_ctx* c, const AcqOut& out);

// sgx_comm.cpp: the RCCL communicator of a context (librccl.so by dlopen)
struct sgx_comm {
    sgx_ctx* ctx;
    void* comm;
    int n_ranks, rank;
    DevBuf<char> d_send;   // cap bytes
    DevBuf<char> d_recv;   // cap bytes per rank
    size_t cap;
};
int sgx_comm_allgather_device(sgx_comm* m, size_t bytes);

// sgx_synth.hip / sgx_acq.hip / sgx_trk.hip provide the C-ABI entry points directly.
