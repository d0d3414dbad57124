/* sgx.h - C-ABI of libsgx.so: MI355X (gfx950) GPS L1 C/A acquisition + tracking engine.
 *
 * The reference (perrysou/SoftGNSS-python) has no FFI; its boundary is the Python object API
 *   Settings                              reference initialize.py:80-185
 *   AcquisitionResult.acquire(longSignal) reference acquisition.py:27-204
 *   AcquisitionResult.preRun()            reference acquisition.py:259-306  (host glue, stays in Python)
 *   TrackingResult.track(fid)             reference tracking.py:13-295
 * The entry points below sit directly under those methods: the drop-in Python modules in
 * softgnss-python_amd/ bind them with ctypes (INTEGRATION.md shows the stub).  Further down: the stages either
 * side of that path - Settings.probeData statistics, the navigation chain of
 * postNavigation.py / ephemeris.py / geoFunctions - each citing the reference lines it replaces.
 *
 * Conventions: plain C, int status return (0 = SGX_OK, <0 = error; text via sgx_last_error),
 * no exceptions/callbacks across the boundary, the CALLER owns every host buffer (the library
 * copies and never keeps a host pointer after return), opaque handles for the device context
 * and for IF records resident in HBM.  One context per device; a context is not thread-safe,
 * different contexts are.  No torch / framework types anywhere in the signatures.
 */
#ifndef SGX_H
#define SGX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SGX_OK          0
#define SGX_E_ARG      -1   /* bad argument */
#define SGX_E_HIP      -2   /* HIP runtime error (no device, launch failure, ...) */
#define SGX_E_NOMEM    -3   /* allocation failed */
#define SGX_E_INDEX    -4   /* the reference's IndexError: coarse code phase == samples-per-chip
                               (acquisition.py:152-153 builds index N) */
#define SGX_E_RCCL     -5   /* RCCL error / library not loadable */
#define SGX_E_RANGE    -6   /* record too short for the request; also where the reference's numpy code raises on
                               out-of-range data (the error text then starts with the exception's name) */
#define SGX_E_DEFER    -7   /* sgx_track_chained: the queued (deferred) sequence does not apply to this call - no
                               acquisition pending, a kernel other than the cooperative int8 / uint8 ones, a streaming
                               record, a table preRun could not make (a NaN metric, a failed search, a channel in front
                               of the record); the caller runs sgx_acquire_end, preRun and sgx_track_ex instead (nothing
                               has been lost: the search's results are still pending).  A launch that has to be repeated
                               is repeated on the table the device made, inside the call */
#define SGX_E_SILENT   -8   /* tracking: a channel went silent - the six sums of one block are exactly zero (a zero-filled
                               stretch of the record), both discriminators are 0 / 0 and the next block has no length: the
                               reference's ValueError "cannot convert float NaN to integer" (tracking.py:148-151).  out and
                               ms_done are complete as for SGX_OK: the silent block is the channel's last row.  (Rates that are
                               NaN behind a block whose sums are not zero - diverged loop filters - end the same way;
                               the text says which.) */

#define SGX_NUM_SERIES 13   /* per-ms tracking series, in this order (tracking.py:255-275):
                               absoluteSample codeFreq carrFreq I_P I_E I_L Q_E Q_P Q_L
                               dllDiscr dllDiscrFilt pllDiscr pllDiscrFilt */
#define SGX_MAX_SATS   16

typedef struct sgx_ctx sgx_ctx;     /* device context: one per GPU */
typedef struct sgx_if sgx_if;       /* int8 IF record resident in HBM */
typedef struct sgx_comm sgx_comm;   /* RCCL communicator for the acquisition peak gather */

/* POD mirror of the reference's Settings attributes used on the path (initialize.py:85-173). */
typedef struct sgx_settings {
    double samplingFreq;          /* initialize.py:107 */
    double IF;                    /* initialize.py:105 */
    double codeFreqBasis;         /* initialize.py:109 */
    double acqSearchBand;         /* kHz, initialize.py:123 */
    double acqThreshold;          /* initialize.py:126 */
    double dllDampingRatio;       /* initialize.py:130 */
    double dllNoiseBandwidth;     /* initialize.py:132 */
    double dllCorrelatorSpacing;  /* initialize.py:134 */
    double pllDampingRatio;       /* initialize.py:137 */
    double pllNoiseBandwidth;     /* initialize.py:139 */
    int64_t skipNumberOfBytes;    /* initialize.py:94 */
    int32_t codeLength;           /* initialize.py:112 */
    int32_t numberOfChannels;     /* initialize.py:88 */
} sgx_settings;

/* One tracking channel as preRun() hands it over (acquisition.py:285-303). */
typedef struct sgx_chan_init {
    double acquiredFreq;
    double codePhase;   /* samples; tracking seeks to skipNumberOfBytes + codePhase (tracking.py:107) */
    int32_t prn;        /* 1-based; 0 = channel off */
    int32_t reserved;
} sgx_chan_init;

/* Integer-only synthetic scene (softgnss-python_amd/synth.py); host and device generators are
 * bit-identical. */
typedef struct sgx_sat {
    uint64_t code_fcw;  /* 32.32 chips per sample */
    uint64_t code_c0;   /* 32.32 code phase at sample 0 (whole code periods shift the navigation bit edges) */
    uint64_t nav_seed;
    uint32_t car_fcw;   /* carrier NCO word, cycles per sample * 2^32 */
    uint32_t car_ph0;
    int32_t prn;        /* 1-based */
    int32_t amp;
} sgx_sat;

typedef struct sgx_scene {
    uint64_t seed;
    int32_t n_sats;
    int32_t nav_mode;                      /* 0: hash navigation bits; 1: nav_bits tables (2048 bits per satellite) */
    sgx_sat sats[SGX_MAX_SATS];
    int16_t cos_lut[256];
    uint8_t nav_bits[SGX_MAX_SATS][256];   /* bit b of satellite s = (nav_bits[s][b >> 3] >> (b & 7)) & 1 */
} sgx_scene;

/* Timings of the last call, measured with HIP events on the context's stream. */
typedef struct sgx_timing {
    float acquire_ms;        /* whole sgx_acquire device time */
    float acq_coarse_ms;     /* mix + FFTs + correlation + peak search; the split is measured with SGX_ACQ_SPLIT_EVENT=1 */
    float acq_fine_ms;       /* fine-frequency FFTs                     (else: coarse = the whole call, fine = 0)          */
    float track_ms;          /* the tracking kernel */
    float synth_ms;          /* the generator kernel */
    float track_kernel;      /* which tracking kernel the last sgx_track ran: 2 latency-mode (sgx_trk2.hip), 3 throughput-mode
                                (sgx_trk_tp.hip), 4 low-rate (sgx_trk_multi.hip), 5 speculative latency-mode (sgx_trk3.hip),
                                6 per-sample, any sample type (sgx_trk_any.hip); 7: sgx_track_coherent ran (sgx_trk_coh.hip) */
    float track_members;     /* workgroups per channel of that launch */
    float track_streamed;    /* 1: the kernel followed the watermark of a record that was still streaming in */
} sgx_timing;

/* ---- library ------------------------------------------------------------------------------ */
const char* sgx_version(void);
int sgx_last_error(char* buf, size_t n);         /* copies the calling thread's last error text */

/* ---- host-side exact helpers (no GPU needed) ---------------------------------------------- */
/* samplesPerCode property, initialize.py:183-185 */
int sgx_samples_per_code(const sgx_settings* s, int64_t* n);
/* Settings.generateCAcode(prn0), initialize.py:234-302: out[1023] of +-1.0, prn0 in 0..31 */
int sgx_generate_ca_code(int32_t prn0, double* out);
/* Settings.makeCaTable(), initialize.py:188-231: out[32 * samplesPerCode] of +-1.0 */
int sgx_make_ca_table(const sgx_settings* s, double* out);
/* Settings.calcLoopCoef(LBW, zeta, k), initialize.py:304-328 */
int sgx_calc_loop_coef(double lbw, double zeta, double k, double* tau1, double* tau2);
/* Host evaluation of the short-chain arithmetic the tracking kernel's loop-filter waves use (csrc/sgx_trk_math.h; on the
 * host the hardware reciprocal seeds are replaced by float-precision ones).  Diagnostics for the parity tests:
 * fn 0: 1/a   1: a/b   2: sqrt(a)   3: atan(a/b)   4: out[0..1] = sin, cos of 2 pi a   5: ceil(a/b)
 * 6: sgx_div1   7: sgx_sqrt1   8: sgx_atan_ratio_k   9: sgx_rot_small -> sin, cos
 * 10: sgx_block_length(a = 1023 - rem, b = codeFreq) at fs = 38.192 MHz -> block length, step_a */
int sgx_trk_math_eval(int32_t fn, double a, double b, double* out);
/* The same for n elements with up to four operands each (host arrays; an unused operand may be null) and two results per
 * element: fn 0 .. 9 as above, and
 *   10: sgx_block_length(a = 1023 - rem, b = codeFreq, c = fs, d = RN(1 / fs)) -> block length, step_a
 *   11: sgx_sqrt1_pos(a)   12: sgx_div_rn(a, b, c = RN(1 / b))   13: as 10 -> block length, ~1 / step_a
 * Both entries run the ONE fn -> call table of csrc/sgx_trk_math_eval.h. */
int sgx_trk_math_eval_batch(int32_t fn, int64_t n, const double* a, const double* b, const double* c, const double* d,
                            double* out0, double* out1);

/* ---- device context and IF records --------------------------------------------------------- */
int sgx_device_count(int* n);
int sgx_ctx_create(const sgx_settings* s, int device, sgx_ctx** out);
/* The same with a stream priority class (-1 high, 0 normal, +1 low).  HIP multiplexes the streams of one priority
 * onto a few hardware queues, where two persistent tracking kernels would run one after the other; contexts that
 * are meant to run AT THE SAME TIME on one GPU (independent records) therefore take different classes. */
int sgx_ctx_create_prio(const sgx_settings* s, int device, int priority, sgx_ctx** out);
int sgx_ctx_destroy(sgx_ctx* c);
int sgx_ctx_sync(sgx_ctx* c);                     /* hipStreamSynchronize on the context stream */
int sgx_get_timing(sgx_ctx* c, sgx_timing* out);
/* sgx_trk_math_eval_batch on the device (csrc/sgx_trk_math_dev.hip; 1 <= n <= 2^20): the same table as the device
 * compiles it, and the __device__ helpers of csrc/sgx_trk_common.h:
 *   16: div_rn(a, b, c = RN(1 / b))   17: sincos_turns(a) -> sin, cos
 *   18: ramp_setup(start a, ramp step b, ilo = (int)d), its reciprocal estimate formed from the code step c as prep_code
 *       forms it -> k1, isw
 *   20 .. 24: prep_code(codeFreq a, rem b) with the kernels' constants for fs = c[0] and correlator spacing = d[0] (c and d
 *       hold that one value in every element) -> 20: blk, remCode   21: stepE, startE   22: stepP, startP
 *       23: stepL, startL   24: the reciprocal estimate, stop
 * Test support: nothing on the processing path calls it. */
int sgx_trk_math_eval_device(sgx_ctx* ctx, int32_t fn, int64_t n, const double* a, const double* b, const double* c,
                             const double* d, double* out0, double* out1);

/* Optional pinned host memory for the big result buffer of sgx_track (a plain pageable buffer works too,
 * it only copies slower). */
int sgx_host_alloc(size_t bytes, void** out);
int sgx_host_free(void* p);

/* np.fromfile(fid, 'int8', n) replacement: copy n host samples into a new HBM record
 * (initialize.py:481, tracking.py:154). */
int sgx_if_upload(sgx_ctx* c, const int8_t* host, size_t n, sgx_if** out);
/* The same straight from the record file (the reference's fid, initialize.py:466-481 / tracking.py:107,154):
 * bytes [file_offset, file_offset + n) of `path` (raw headerless int8 samples) are streamed through two
 * pinned staging buffers, the next pread overlapping the previous chunk's H2D copy.  A file shorter than
 * requested yields a shorter record (tracking then reports the reference's short-read exit). */
int sgx_if_upload_file(sgx_ctx* c, const char* path, uint64_t file_offset, size_t n, sgx_if** out);
/* The same record, but the call returns at once: a background thread streams the file into HBM in file order and
 * sgx_acquire / sgx_track / sgx_if_download / sgx_probe_stats wait for exactly the samples they need - sgx_track's
 * cooperative kernel follows a device-side watermark block by block, so tracking overlaps the transfer.
 * sgx_if_wait blocks until the first n samples (0 = all) are resident and reports a read error if there was one;
 * sgx_if_free joins the thread. */
int sgx_if_open_file(sgx_ctx* c, const char* path, uint64_t file_offset, size_t n, sgx_if** out);
int sgx_if_wait(sgx_ctx* c, sgx_if* r, size_t n);
/* Generate samples [offset, offset+n) of a synthetic scene directly in HBM. */
int sgx_if_synth(sgx_ctx* c, const sgx_scene* scene, uint64_t offset, size_t n, sgx_if** out);
int sgx_if_download(sgx_ctx* c, const sgx_if* r, size_t offset, size_t n, int8_t* host);
int sgx_if_length(const sgx_if* r, size_t* n);
int sgx_if_free(sgx_ctx* c, sgx_if* r);

/* ---- AcquisitionResult.acquire (acquisition.py:27-204) -------------------------------------
 * Searches PRN indices prn0[0..n_prn) (0-based) on samples [offset, offset+n_samples) of the
 * record.  n_blocks 1-ms blocks feed the coarse search (reference: 2); noncoh = 0 keeps the
 * reference rule (block with the larger maximum, acquisition.py:129-133), noncoh = 1 sums
 * |corr|^2 over the blocks (extension, BASELINE.json config 4).  n_samples is the length of the
 * reference's longSignal: its mean is the DC removed before the fine search (acquisition.py:59)
 * and codePhase + 10 ms must fit in it (acquisition.py:177).
 * Outputs, each [n_prn]: the three reference fields (acquisition.py:201-203) and, for parity
 * checks, frequencyBinIndex and fftMaxIndex (-1 where the PRN is not detected).
 * Returns SGX_E_INDEX where the reference raises IndexError (outputs up to that PRN are valid).
 */
int sgx_acquire(sgx_ctx* c, const sgx_if* r, size_t offset, size_t n_samples,
                const int32_t* prn0, int32_t n_prn, int32_t n_blocks, int32_t noncoh,
                double* carrFreq, double* codePhase, double* peakMetric,
                int32_t* freqBin, int32_t* fineIdx);

/* The same for a signal that is not int8: acquisition.py:55-59 works on whatever real dtype numpy hands it (float
 * samples, int16 values, a record rescaled on the host).  `signal` = n_samples fp64 samples on the host; they are copied to
 * HBM and the kernels read them in place of the int8 record (same fp64 arithmetic, same outputs as sgx_acquire). */
int sgx_acquire_f64(sgx_ctx* c, const double* signal, size_t n_samples, const int32_t* prn0, int32_t n_prn,
                    int32_t n_blocks, int32_t noncoh, double* carrFreq, double* codePhase, double* peakMetric,
                    int32_t* freqBin, int32_t* fineIdx);

/* ---- coherent multi-millisecond acquisition (extends acquisition.py:62-133) --------------------
 * The reference correlates 1-ms blocks on a 500 Hz grid, which leaves signals below about 40 dB-Hz under acqThreshold.
 * Here window w of coherent_ms = T_c blocks (1..20) is folded with a carrier that runs on across the window and restarts
 * at each window start, as the reference restarts it at each block (acquisition.py:103-105):
 *   F[w][k][n] = sum_{m < T_c} x[(w T_c + m) N + n] (sin + j cos)(f_k (((n + m N) 2) pi ts)),   n < N = samplesPerCode
 * on the grid f_k = IF - acqSearchBand/2 * 1000 + bin_step_hz * k, k < round(acqSearchBand * 1000 / bin_step_hz) + 1
 * (<= 1024 bins; bin_step_hz > 0, the Python layer's default is 500 / T_c).  Each folded window then goes through the
 * reference's correlation (acquisition.py:120-126) and the n_windows = M windows (1..64, T_c M <= 400) take the place of
 * the 1-ms blocks: noncoh = 0 keeps the window with the larger maximum (acquisition.py:129-133), noncoh = 1 sums them.
 * Peak, second peak, peakMetric, codePhase and freqBin follow acquisition.py:135-166 on this grid.  The fine search is
 * the reference's (acquisition.py:167-193); for T_c > 1 each detection's arg-max is limited to the spectrum indices i
 * (frequency i fs / npts) within bin_step_hz of its coarse bin's frequency.  carrFreq / fineIdx keep the reference's
 * slice index (acquisition.py:187-191).
 * tests/coherent_acq_spec.py states the contract in numpy.  T_c = 1 with bin_step_hz = 500 is sgx_acquire itself.
 * Errors, before anything is launched: SGX_E_ARG for parameters out of range, SGX_E_RANGE for a window shorter than
 * T_c M N samples (and, as sgx_acquire, for a detection whose fine window leaves it), SGX_E_INDEX as sgx_acquire. */
typedef struct sgx_acq_params {
    int32_t coherent_ms;          /* T_c, 1..20 */
    int32_t n_windows;            /* M, 1..64 */
    int32_t noncoh;               /* 0 reference rule, 1 non-coherent sum over the windows */
    int32_t reserved;             /* 0 */
    double bin_step_hz;           /* Doppler step in Hz, > 0 (SGX_E_ARG otherwise) */
} sgx_acq_params;
int sgx_acquire_coherent(sgx_ctx* c, const sgx_if* r, size_t offset, size_t n_samples, const int32_t* prn0, int32_t n_prn,
                         const sgx_acq_params* p, double* carrFreq, double* codePhase, double* peakMetric,
                         int32_t* freqBin, int32_t* fineIdx);
int sgx_acquire_coherent_f64(sgx_ctx* c, const double* signal, size_t n_samples, const int32_t* prn0, int32_t n_prn,
                             const sgx_acq_params* p, double* carrFreq, double* codePhase, double* peakMetric,
                             int32_t* freqBin, int32_t* fineIdx);
/* The search sgx_acquire_coherent runs for these settings, for 32 PRNs; needs no GPU.  n_bins Doppler bins; n_phi distinct
 * fractions phi of f_k N / fs = shift + phi; path 1: the shift path (the forward transforms are n_windows x n_phi folded
 * rows, each bin reads its phi's spectrum with a circular shift; needs the four-step transform's length and n_phi <= 64),
 * 0: the direct path (every (window, bin) row folded and transformed; n_windows x n_bins <= 2048).  prn_chunk PRNs per
 * correlation batch; bin_runs > 1: one PRN per batch, cut into that many runs (of bins for noncoh = 1, of windows for
 * noncoh = 0). */
int sgx_acquire_coherent_plan(const sgx_settings* s, const sgx_acq_params* p, int32_t* n_bins, int32_t* n_phi,
                              int32_t* path, int32_t* prn_chunk, int32_t* bin_runs);

/* ---- the same path without host round trips between its stages (round 6) --------------------
 * The reference's caller looks at every stage's result before it starts the next (initialize.py:484-506: acquire, preRun,
 * TrackingResult.track).  A caller that wants the tracking results can queue all three and wait once:
 *   sgx_acquire_begin    sgx_acquire's arguments without the outputs: the search is queued (acquisition.py:27-204), the
 *                        call returns without looking at it.  One acquisition may be pending per context: any other
 *                        sgx_acquire* call on the context (this one, sgx_acquire, _f64, _coherent, _coherent_f64,
 *                        _sharded) drops a pending search, whether or not it succeeds - sgx_track_chained then returns
 *                        SGX_E_DEFER and sgx_acquire_end SGX_E_ARG ("no acquisition is pending").
 *   sgx_track_chained    preRun (acquisition.py:259-306: stable descending sort of the 32 peak metrics, the first
 *                        min(n_ch, #detected) become channels) runs ON THE DEVICE behind the pending search and the tracking
 *                        kernel (tracking.py:13-295) behind it, reading the channel table where preRun left it; the call
 *                        waits once, for everything.  out = [n_ch][13][ms] (pinned memory from sgx_host_alloc), ms_done =
 *                        [n_ch]; the channel table as preRun made it comes back in prn / acquiredFreq / codePhase [n_ch]
 *                        (prn 0 = off; the first *n_active channels are on, in order of descending metric).  Returns
 *                        SGX_E_SILENT as sgx_track: out, ms_done AND the table (prn, acquiredFreq, codePhase, n_active) are
 *                        complete, the rows of out in the table's order.
 *                        SGX_E_DEFER when the queued sequence does not apply (see the code's comment; n_ch > 8) - then nothing has
 *                        been tracked and the eager calls do the work; SGX_E_INDEX / SGX_E_RANGE where the SEARCH failed
 *                        the way the reference's acquire() raises (no channel was tracked).
 *   sgx_acquire_end      the pending search's outputs (sgx_acquire's), without waiting if sgx_track_chained has run.
 * Results are those of sgx_acquire + preRun + sgx_track_ex, bit for bit: the same kernels in the same order, and the
 * device-side preRun repeats the host's arithmetic (tests/test_gpu_parity.py). */
int sgx_acquire_begin(sgx_ctx* c, const sgx_if* r, size_t offset, size_t n_samples,
                      const int32_t* prn0, int32_t n_prn, int32_t n_blocks, int32_t noncoh);
int sgx_acquire_end(sgx_ctx* c, double* carrFreq, double* codePhase, double* peakMetric,
                    int32_t* freqBin, int32_t* fineIdx);
int sgx_track_chained(sgx_ctx* c, const sgx_if* r, int64_t rec_file_offset, int32_t n_ch, int32_t ms,
                      double* out, int32_t* ms_done, int32_t data_type,
                      int32_t* prn, double* acquiredFreq, double* codePhase, int32_t* n_active);

/* ---- TrackingResult.track (tracking.py:13-295) ----------------------------------------------
 * Tracks n_ch channels for `ms` code periods on the record.  rec_file_offset is the byte offset
 * in the reference's file of the record's first sample (0 when the whole file was uploaded):
 * a channel starts at file byte skipNumberOfBytes + codePhase (tracking.py:107) and
 * absoluteSample is reported as a file position (tracking.py:255).
 * out is [n_ch][SGX_NUM_SERIES][ms] float64, pre-filled exactly like tracking.py:65-94 (0 or
 * +Inf) for entries never reached; ms_done[ch] = blocks completed (== ms unless the record ran
 * out, the reference's short-read exit tracking.py:159-163; channels with prn == 0 report 0).
 * SGX_E_SILENT, whichever kernel ran: a channel stopped because block ms_done[ch] - 1 summed to exactly zero and left its
 * rates NaN (the text names the lowest such channel and the block that could not start).  Decided on the host from the
 * series; a launch that ended early for another reason keeps its own report.
 */
int sgx_track(sgx_ctx* c, const sgx_if* r, int64_t rec_file_offset,
              const sgx_chan_init* ch, int32_t n_ch, int32_t ms,
              double* out, int32_t* ms_done);

/* The same for a record of Settings.dataType samples (settings.dataType, initialize.py:60; read with
 * np.fromfile(fid, dataType, blksize) at tracking.py:154).  data_type SGX_DT_INT8 is sgx_track; otherwise the record
 * handle holds the file's BYTES as they are (little endian) and rec_file_offset, skipNumberOfBytes + codePhase and
 * absoluteSample stay BYTE positions, exactly as the reference's fid.seek / fid.tell treat them (tracking.py:107, 255) -
 * so a channel whose start byte lies inside a sample reads samples that straddle the file's, as it does there.
 * int8, uint8 and int16 have typed kernels (int16 and uint8 at samplingFreq >= 16 x codeFreqBasis).  SGX_DT_FLOAT32 is
 * tracked through them EXACTLY when every sample of the window is m 2^-k for one k and 16-bit integers m (floats written
 * from ADC samples, or normalised by a power of two) and the channels start on samples: the integers go through the int8
 * / int16 kernels and the correlator series are scaled back, which no rounding of the reference's float64 arithmetic can
 * tell from the real thing.  Other float32 records, and SGX_DT_FLOAT64, run the latency-mode kernel on samples scaled by a
 * power of two (the window is scanned once for its largest |x|; exact both ways).  Everything else - float16, the wider
 * integers, int16 / uint8 at low sampling rates, float records with NaN / infinite samples or channels that start inside
 * a sample - is read sample by sample where it lies and promoted to float64 as numpy promotes it (the per-sample kernel,
 * sgx_trk_any.hip: slower, same contract).  Complex types are not tracked (the reference's
 * discriminators fail on them). */
#define SGX_DT_INT8  0
#define SGX_DT_INT16 1
#define SGX_DT_UINT8 2   /* offset-binary bytes as the reference reads them with dataType 'uint8': no offset is removed */
#define SGX_DT_FLOAT32 3 /* IEEE binary32 */
#define SGX_DT_FLOAT64 4
#define SGX_DT_UINT16  5
#define SGX_DT_INT32   6
#define SGX_DT_UINT32  7
#define SGX_DT_INT64   8
#define SGX_DT_UINT64  9
#define SGX_DT_FLOAT16 10
int sgx_track_ex(sgx_ctx* c, const sgx_if* r, int64_t rec_file_offset,
                 const sgx_chan_init* ch, int32_t n_ch, int32_t ms,
                 double* out, int32_t* ms_done, int32_t data_type);

/* Which tracking kernel sgx_track_ex runs, and with how many cooperating workgroups (members) per channel - the one rule
 * the host applies (csrc/sgx_trk.hip: sgx_track_plan), without the diagnostic SGX_TRK_* overrides.  No reference
 * counterpart (tracking.py:59 is one serial loop); needs no GPU.  n_cus: compute units of the device (256 on an MI355X);
 * float_in_range != 0: a float32 / float64 record whose window was scanned and can run the typed kernel.
 *   kernel  2 trk2_kernel (latency mode, any member layout)   3 trk_kernel_tp (throughput mode, > 128 channels)
 *           4 trk_kernel_multi (< ~15.4 samples per chip)      5 trk3_kernel (speculative latency mode, the headline)
 *           6 trk_kernel_any (any sample type, sample by sample)
 *   members workgroups per channel (trk2_kernel with one workgroup per unit AND correlator arm: 3 x units) */
int sgx_track_plan(const sgx_settings* s, int32_t data_type, int32_t n_ch, int32_t n_cus, int32_t float_in_range,
                   int32_t* kernel, int32_t* members);

/* ---- Bit-aligned coherent tracking of weak signals (no reference counterpart; the contract in numpy is
 * tests/coh_track_spec.py, the kernel csrc/sgx_trk_coh.hip) -------------------------------------------------------------
 * Every block is sgx_track's block - its own length from remCodePhase and codeFreq, the reference's three ramps, a carrier
 * that runs on through remCarrPhase, the six sums (tracking.py:148-219).  Only WHEN the loops are updated changes:
 *   blocks k < k0    the reference's update after every block (tracking.py:223-251, PDI 0.001, the settings' loops).
 *   bit sync         where bit_edge_in[ch] == -1, over the pull-in blocks k < pull_in_ms: with z = I_P + j Q_P, every
 *                    hypothesis h in 0..19 adds z to a[h] from block h on and, at (k - h) % 20 == 19, adds |a[h]|^2 to
 *                    E[h] and clears a[h]; behind block pull_in_ms - 1 the edge is the lowest h with the largest E[h].
 *   k0               the smallest k >= pull_in_ms with (k - edge) % 20 == 0.  coherent_ms == 1: never.
 *   hand-over        at the end of block k0 - 1 (if k0 < ms), behind its own update: oldCarrNco = the mean of carrNco over
 *                    the last min(handover_ms, k0) blocks (added in ascending block order), oldCarrError = 0, carrFreq =
 *                    carrFreqBasis + oldCarrNco; the same for the code loop (codeFreq = codeFreqBasis - oldCodeNco).
 *   blocks k >= k0   groups of coherent_ms blocks: both NCO rates are held inside a group, the six sums of its blocks are
 *                    added in block order, and behind its last block the reference's two discriminators are taken of the
 *                    group sums and both filters run with PDI = coherent_ms x 0.001 and the coefficients of the
 *                    parameters, in the reference's expressions.  A group that ms cuts short is never updated.
 * out row k: absoluteSample and the six sums are block k's alone (bits, preambles, sgx_track_quality, sgx_replay_state and
 * sgx_if_cancel read them as they read sgx_track's); codeFreq / carrFreq are the rates block k + 1 runs with (row k0 - 1:
 * the handed-over ones); the four discriminator series hold the values of the latest update - they repeat inside a group.
 * out (pre-fill, file positions) and ms_done as sgx_track; SGX_E_RANGE as there; SGX_E_SILENT where the six sums of an
 * UPDATE (a block's before k0, a group's after) are exactly zero: that block is the channel's last row.
 * bit_edge[ch]: the edge used or found (-1: the channel ended before it was found); coh_start[ch]: k0, or -1 where there
 * is none (coherent_ms 1, no edge, a channel that is off); edge_energy[ch][20]: E (zeros where the edge was given).
 * int8 records, resident before the launch (the call waits for the whole record; the kernel follows no watermark); one
 * workgroup per channel at any sampling rate.  SGX_E_ARG before anything is launched: coherent_ms outside {1, 2, 4, 5, 10,
 * 20}; pull_in_ms < 40, < 220 where an edge is to be found, or > ms; handover_ms outside 1..1000; an edge outside -1..19.
 * sgx_get_timing: track_ms, track_kernel 7, track_members 1. */
typedef struct sgx_coh_params {          /* 64 bytes */
    double tau1_pll, tau2_pll;           /* the coherent loops: sgx_calc_loop_coef(cohPllBW, pllDampingRatio, 0.25) */
    double tau1_dll, tau2_dll;           /* ... and sgx_calc_loop_coef(cohDllBW, dllDampingRatio, 1.0) */
    int32_t coherent_ms;                 /* T: blocks per group */
    int32_t pull_in_ms;                  /* P: blocks updated one by one in front of the first group */
    int32_t handover_ms;                 /* H: blocks whose NCO values are averaged at the hand-over */
    int32_t reserved;
    double reserved2[2];
} sgx_coh_params;
int sgx_track_coherent(sgx_ctx* c, const sgx_if* r, int64_t rec_file_offset, const sgx_chan_init* ch, int32_t n_ch,
                       int32_t ms, const sgx_coh_params* p, const int32_t* bit_edge_in, double* out, int32_t* ms_done,
                       int32_t* bit_edge, int32_t* coh_start, double* edge_energy);

/* How sgx_acquire cuts the correlation batch of a call into chunks over its (one or two) queues - the host's one rule
 * (csrc/sgx_acq.hip: acq_plan), without the SGX_ACQ_* overrides; no reference counterpart (acquisition.py:93-133 is one
 * loop over PRNs and bins); needs no GPU.  chunk_rows <= 0: the default (348).  A chunk is prn_chunk whole PRNs
 * (bin_runs == 1) or one PRN's rows of bins_per_run Doppler bins (bin_runs > 1, non-coherent sums only). */
int sgx_acquire_plan(int32_t n_prn, int32_t n_bins, int32_t n_blocks, int32_t noncoh, int32_t chunk_rows,
                     int32_t max_queues, int32_t* prn_chunk, int32_t* bin_runs, int32_t* bins_per_run, int32_t* queues);
/* The two constants behind that rule: the default chunk size (rows; SGX_ACQ_CHUNK_ROWS overrides it) and the largest batch
 * of rows one launch takes. */
int sgx_acquire_plan_limits(int32_t* default_chunk_rows, int32_t* max_rows);
/* The transform length the search of sgx_acquire runs on for n_code = samplesPerCode; needs no GPU.  n_code itself where
 * it factors into 2..31 (every radix the library has).  Any other n_code - the reference takes np.fft.fft of any length
 * (acquisition.py:120-124) - has its circular correlation computed inside a longer one: *length >= 2 n_code - 1, factors
 * into 2..31, is at most the next power of two, and is the cheapest such length by the rule csrc/sgx_fft.hip states
 * (sgx_fft_corr_length).  Results are the reference's either way; a padded search moves about twice the bytes. */
int sgx_acquire_fft_length(int64_t n_code, int64_t* length);
/* The radix passes that transform runs as (csrc/sgx_fft.hip), for the tests of the pass kernels; needs no GPU.
 * *length as sgx_acquire_fft_length gives it; radices_out[i] and tpb_out[i], i < *n_passes <= SGX_FFT_MAX_PASSES: the
 * radix and the workgroup width of pass i in the order the passes run; *last_pass_blocks: workgroups per row of the last
 * pass, each leaving one partial maximum where that pass is fused with the peak search. */
#define SGX_FFT_MAX_PASSES 32
int sgx_acquire_fft_passes(int64_t n_code, int32_t* radices_out, int32_t* n_passes, int64_t* length,
                           int32_t* last_pass_blocks, int32_t* tpb_out);
/* Diagnostics for the transform tests: the radix-pass kernels of the search on the caller's rows, through the plan and the
 * pass loop sgx_acquire uses (a length that does not factor into 2..31 is refused as there).  Host pointers, complex128 as
 * (re, im) pairs, rows of n elements; rows <= 4096, n <= 2^24.
 *   plain (mul_x null): out_rows[rows][n] = DFT of in[rows][n], the input taken as zero from element nonzero_len on
 *     (1 <= nonzero_len <= n);
 *   fused (mul_x[n_x][n], mul_f[n_f][n], in null): row r is the DFT of conj(mul_x[b]) * mul_f[p], formed in the first
 *     pass, with (b, p) = (row_map[2 r], row_map[2 r + 1]) or, row_map null, (r % rows_per_prn, prn_base + r / rows_per_prn).
 *     out_max / out_arg given: the last pass squares, scales by 1 / n^2 and max-reduces; out_max[r] is the largest power
 *     among the outputs k < n_valid (0 or n: all of them) and out_arg[r] its first index.  out_rows given instead: the
 *     rows themselves (the route the second-peak search takes).  A one-pass length cannot fuse both ends. */
int sgx_fft_run_passes(sgx_ctx* c, int64_t n, int32_t rows, const double* in, int64_t nonzero_len, const double* mul_x,
                       int32_t n_x, const double* mul_f, int32_t n_f, int32_t rows_per_prn, int32_t prn_base,
                       const int32_t* row_map, int64_t n_valid, double* out_rows, double* out_max, int32_t* out_arg);

/* Measured HBM rates of this device for the roofline report (no reference counterpart): a read-only stream and a
 * copy (read + write bytes counted) over `bytes` of device memory, `reps` timed launches each, GB/s. */
int sgx_stream_rates(sgx_ctx* c, size_t bytes, int reps, double* read_gbs, double* copy_gbs);

/* ---- next row: raw-data statistics of Settings.probeData (initialize.py:330-417) ------------------------------
 * Window [offset, offset+n) of a resident record (the reference reads 10 * samplesPerCode samples,
 * initialize.py:369-371).  f[8193] (MHz) and pxx[8193] = welch(data - mean(data), fs_mhz, hamming(16384, False),
 * 16384, 1024, 16384) (initialize.py:389-394); hist[255] = np.histogram(data, arange(-128, 128))[0]
 * (initialize.py:400, last bin closed); *n_segments = Welch segments averaged.  SGX_E_RANGE ("ValueError") for
 * fewer than 16384 samples.  The call is the record monitor below at nperseg 16384, noverlap 1024 and one slice of n
 * samples, so a window longer than the monitor's longest slice, 2^32 samples, is refused as the monitor refuses it
 * (SGX_E_ARG, the monitor's message).  It leaves sgx_waterfall_timing as it was. */
#define SGX_PROBE_BINS 8193
#define SGX_PROBE_HIST 255
int sgx_probe_stats(sgx_ctx* c, const sgx_if* rec, size_t offset, size_t n, double fs_mhz, double* f, double* pxx,
                    int64_t* hist, int32_t* n_segments);

/* ---- the record monitor (no reference counterpart: probeData looks at the first 10 code periods only) -----------
 * Window [offset, offset+n) of an int8 record cut into slices of slice_len samples; slice j covers [offset + j slice_len,
 * offset + min((j+1) slice_len, n)) and is kept while it holds one whole segment - a trailing piece shorter than nperseg
 * is dropped.  Segments never cross a slice boundary: slice j has (len_j - noverlap) / (nperseg - noverlap) of them.
 * Per slice: pxx = the Welch density of sgx_probe_stats at this segment length (exact constant detrend per segment,
 * periodic Hamming window, one-sided, mean over the segments in segment order; a constant segment gives exactly 0);
 * moments = count, sum x, sum x^2, sum x^4 and hist = the 256-bin histogram (-128 in bin 0) of ALL samples of the slice,
 * exact.  hold[k] = max over the slices of pxx[.][k]; f[nperseg/2+1] (MHz) as sgx_probe_stats.  A segment goes from its
 * int8 samples to its powers inside one compute unit; the sums have one order, so two calls give the same bits.
 * sgx_waterfall_plan: the number of slices kept, to size the arrays; host code, needs no GPU.
 * SGX_E_ARG: nperseg not a power of two in 256 .. 16384, noverlap outside [0, nperseg), slice_len below nperseg or above
 * 2^32 (a slice's sum of x^4 then fits int64), a NULL pointer, a record on another device; SGX_E_RANGE: a window outside
 * the record, or ("ValueError") shorter than one segment.
 * sgx_waterfall_host: pxx[n_slices][nperseg/2+1] and n_segments[n_slices] of the window x[n] by the kernels' own work
 * items and order of additions in a host loop - what the kernels are tested against, bit for bit; needs no GPU.
 * sgx_waterfall_timing: HIP-event time of the last sgx_probe_waterfall's kernels on this context. */
int sgx_probe_waterfall(sgx_ctx* c, const sgx_if* rec, size_t offset, size_t n, double fs_mhz, int32_t nperseg,
                        int32_t noverlap, size_t slice_len, double* f, double* pxx, double* hold, int64_t* moments,
                        int64_t* hist, int64_t* n_segments, int64_t* n_slices);
int sgx_waterfall_plan(size_t n, int32_t nperseg, int32_t noverlap, size_t slice_len, int64_t* n_slices);
int sgx_waterfall_host(const int8_t* x, size_t n, double fs_mhz, int32_t nperseg, int32_t noverlap, size_t slice_len,
                       double* pxx, int64_t* n_segments);
int sgx_waterfall_timing(sgx_ctx* c, float* kernel_ms);

/* ---- swept (chirp) interference excision (no reference counterpart; behind every preparing stage, in front of
 * sgx_if_filter) --------------------------------------------------------------------------------------------------
 * A real int8 record of n >= 1 samples through a short-time Fourier transform and back.  Segment j = 0 .. J - 1,
 * J = ceil(n / H) + 1, H = N / 2, covers samples [(j - 1) H, (j + 1) H), zero outside the record, under the periodic
 * root-Hann window w[i] = sin(pi i / N).  Of its bins k = 1 .. N/2 - 1 (DC and Nyquist are never cut) those are zeroed that
 * stand above threshold x m, m the mean power of the kept bins, found in `passes` rounds that start from all of them; the
 * segment goes back through the inverse transform and the same window into an overlap-add, and
 * y = clip(floor(o + 1/2), -127, 127).  fp64 throughout.  A NEW record of the same length (sgx_if_free); sample n lines up
 * with sample n of the input.  info: the segments J, the bins cut, the segments with a cut bin, and the outputs that lay
 * outside [-127, 127] in front of the clip; cut_per_segment (may be NULL): the bins cut in each of the J segments.  No sum
 * crosses a workgroup and every sum has one order: two calls give the same bytes.
 * SGX_E_ARG, before anything is launched, with a text that names the argument: N not a power of two in 64 .. 1024, a
 * threshold below 1 or not finite, passes outside 1 .. 8, an empty record, a record beyond one launch, a NULL pointer, a
 * record on another device.
 * sgx_excise_plan: J and the segments one workgroup holds, 8192 / N (a tile owns the hops between them; its last segment is
 * the next tile's first); host code, needs no GPU.
 * sgx_excise_host: the same arithmetic, item by item, in a host loop - what the kernel is tested against; needs no GPU.
 * sgx_excise_host_spectra: the J x (N/2 + 1) complex bins (re, im) of the windowed segments as that loop computes them.
 * sgx_excise_timing: HIP-event time of the last sgx_if_excise's kernel on this context, 0 where it had no work. */
typedef struct { int64_t segments, bins_cut, segments_cut, clipped; } sgx_excise_info;
int sgx_excise_plan(size_t n, int32_t N, int64_t* n_segments, int32_t* tile_segments);
int sgx_if_excise(sgx_ctx* c, const sgx_if* rec, int32_t N, double threshold, int32_t passes, sgx_if** out,
                  sgx_excise_info* info, uint16_t* cut_per_segment);
int sgx_excise_host(const int8_t* x, size_t n, int32_t N, double threshold, int32_t passes, int8_t* y,
                    sgx_excise_info* info, uint16_t* cut_per_segment);
int sgx_excise_host_spectra(const int8_t* x, size_t n, int32_t N, double* spectra);
int sgx_excise_timing(sgx_ctx* c, float* kernel_ms);

/* ---- next row: bit sync + preamble search on the tracking output (postNavigation.py:443-631) ----------------
 * NavigationResult.findPreambles: I_P is [n_ch][ms] float64 (row i = i-th record of the tracking results);
 * firstSubFrame[ch] = ms index of the first verified TLM preamble, 0 = none (then the reference drops the
 * channel from its active list).  The sign correlation against the 160-ms preamble runs on the device, the
 * 6000-ms spacing test and the TLM/HOW parity checks (navPartyChk) on the host.  SGX_E_RANGE where the
 * reference's numpy code raises on a slice cut short by the record ends (candidate within 40 ms of the start
 * or 1200 ms of the end); sgx_last_error() then starts with "ValueError" or "IndexError" accordingly. */
int sgx_find_preambles(sgx_ctx* c, const double* I_P, int32_t n_ch, int32_t ms, int32_t search_start,
                       int32_t* firstSubFrame);
/* NavigationResult.navPartyChk (postNavigation.py:443-521): ndat32 = D29* D30* d1..d24 D25..D30 as +-1;
 * flips d1..d24 in place when D30* != 1 like the reference; status +1 / -1 (parity ok) or 0. */
int sgx_nav_parity_check(double* ndat32, int32_t* status);

/* ---- C/N0 estimate and lock detector on the tracking output (the reference's hook at tracking.py:276-278) ----------
 * Channel c's prompt series are I_P[c*row_stride + k], Q_P[c*row_stride + k] for k < ms_done[c] (ms_done NULL: ms).
 * Over non-overlapping windows of W = p->window ms (window j covers k = jW .. jW+W-1, j < n_c = ms_done[c] / W; a
 * trailing partial window is dropped), in fp64:
 *   R = sum(I^2 - Q^2), X = sum(2 I Q), P = sum(I^2 + Q^2), phi = atan2(X, R) / 2, A = sum |I cos phi + Q sin phi|
 *   cno[c][j] = 10 log10(Psig / ((Ptot - Psig) T)) dB-Hz with Psig = (A/W)^2, Ptot = P/W   (NaN for P = 0, -inf for
 *               Psig = 0 < P, +inf for Ptot - Psig <= 0 < Psig)
 *   carr_lock[c][j] = R / sqrt(R^2 + X^2) = cos 2 phi   (NaN for R = X = 0)
 *   pass[c][j] = cno >= cno_min and carr_lock >= carr_lock_min (a NaN fails)
 * lost[c] = the first j at which the counter f (0; fail: f + 1, pass: max(f - 1, 0)) reaches max_fail, else -1.
 * Windows j >= n_c hold NaN, NaN, 0 and are not counted.  cno, carr_lock, pass are [n_ch][ms / W]; the inputs are any
 * host memory (the [n][13][ms] series of sgx_track_ex: row_stride = 13 ms, pointers to rows 3 and 7).
 * SGX_E_ARG for window < 2 or > ms, max_fail < 1, T not finite or <= 0, row_stride < ms, an ms_done entry outside
 * [0, ms] or a NULL pointer; nothing is launched then.  tests/lock_spec.py restates all of it in numpy. */
typedef struct sgx_lock_params {
    double T;               /* s per ms-rate sample: codeLength / codeFreqBasis */
    double cno_min;         /* dB-Hz */
    double carr_lock_min;
    int32_t window;         /* W, ms */
    int32_t max_fail;
} sgx_lock_params;          /* 32 bytes */
int sgx_track_quality(sgx_ctx* c, const double* I_P, const double* Q_P, int64_t row_stride, int32_t n_ch, int32_t ms,
                      const int32_t* ms_done, const sgx_lock_params* p, double* cno, double* carr_lock, uint8_t* pass,
                      int32_t* lost);

/* ---- multi-correlator replay of tracked channels (no reference counterpart: tracking.py:166-219 forms three arms) ----
 * Once a channel has been tracked, every block's code rate, carrier rate, start and length are on record, so the
 * correlation at ANY code offset can be formed afterwards, all blocks at once.  Block k of a channel is rebuilt exactly as
 * tracking.py:148-251 forms it, from the rows absoluteSample, codeFreq, carrFreq (rows 0, 1, 2 of the channel's series):
 *   code_freq_k = codeFreq[k-1] (k = 0: codeFreqBasis), carr_freq_k = carrFreq[k-1] (k = 0: acquiredFreq),
 *   step = code_freq_k / fs, blk = ceil((codeLength - rem_code) / step), start byte pos_k = absoluteSample[k-1]
 *   (k = 0: skipNumberOfBytes + codePhase), arg_n = carr_freq_k 2.0 pi (n / fs) + rem_carr, and after the block
 *   rem_code = tp[blk-1] + step - 1023.0 with tp = linspace(rem_code, blk step + rem_code, blk, endpoint=False),
 *   rem_carr = arg_blk mod 2 pi (both start at 0).
 * For tap offset d_j (chips) and block k < ms_done[c]:
 *   t = linspace(rem_code + d_j, blk step + rem_code + d_j, blk, endpoint=False), chip_n = code[(ceil(t_n) - 1) mod 1023],
 *   I[j][k] = sum_n chip_n sin(arg_n) x_n,  Q[j][k] = sum_n chip_n cos(arg_n) x_n
 * so d = -dllCorrelatorSpacing, 0, +dllCorrelatorSpacing are the reference's early, prompt and late arms.  Blocks
 * k >= ms_done[c] and channels with prn == 0 hold 0.  tests/replay_spec.py restates all of it in numpy.
 *
 * sgx_replay_state: the per-block state, state[c * ms + k], from the series ([n_ch][SGX_NUM_SERIES][ms], any host memory);
 * exact host code, needs no GPU.  rec_bytes: bytes of the record behind rec_file_offset (< 0: not checked).  Entries
 * k >= ms_done[c] (ms_done NULL: ms) and channels that are off are zeroed.  SGX_E_ARG when a rebuilt block end disagrees
 * with absoluteSample[k] - the series is not a tracking result of these channels - or a rate is not finite; SGX_E_RANGE
 * when a block starts before the record or ends beyond it; sgx_last_error names the channel and the block.  data_type:
 * SGX_DT_INT8, SGX_DT_UINT8 or SGX_DT_INT16 (BYTE positions, as sgx_track_ex: an int16 channel may start on an odd byte);
 * every other SGX_DT_* is SGX_E_ARG (float, wide-integer and complex records are not replayed).
 *
 * sgx_track_replay: I and Q of n_taps taps on the resident record (a streaming record is waited for, as sgx_if_wait):
 * out is [n_ch][n_taps][2][ms] float64, I then Q.  One launch covers every (channel, block); two calls give identical
 * bytes.  SGX_E_ARG, before anything is launched or written, for n_taps outside [1, SGX_REPLAY_MAX_TAPS], a tap that is
 * not finite, a NULL pointer, an ms_done entry outside [0, ms], a data_type other than the three above, and whatever
 * sgx_replay_state refuses (with its code).  sgx_replay_timing: HIP-event times of the last replay on this context - the
 * kernel alone, and the whole device side (state upload, kernel, result copy). */
#define SGX_REPLAY_MAX_TAPS 64
typedef struct sgx_replay_block {
    int64_t start;      /* file byte position of the block's first sample */
    double rem_code;    /* chips */
    double rem_carr;    /* rad */
    double step;        /* chips per sample */
    double carr_freq;   /* Hz */
    int32_t blk;        /* samples */
    int32_t reserved;
} sgx_replay_block;     /* 48 bytes */
int sgx_replay_state(const sgx_settings* s, int32_t data_type, const sgx_chan_init* ch, int32_t n_ch, int32_t ms,
                     const int32_t* ms_done, const double* series, int64_t rec_file_offset, int64_t rec_bytes,
                     sgx_replay_block* state);
int sgx_track_replay(sgx_ctx* c, const sgx_if* rec, int64_t rec_file_offset, const sgx_chan_init* ch, int32_t n_ch,
                     int32_t ms, const int32_t* ms_done, const double* series, int32_t data_type, const double* taps,
                     int32_t n_taps, double* out);
int sgx_replay_timing(sgx_ctx* c, float* kernel_ms, float* device_ms);

/* ---- strong-signal cancellation: tracked channels subtracted from a record (no reference counterpart) ---------------
 * A C/A code lies only about 24 dB under another one, so a strong satellite's cross-correlation peaks stand above a weak
 * satellite's own peak however long the search integrates.  Once the strong channels are tracked, their blocks are on
 * record (sgx_replay_state) and the prompt sums give each block's amplitude and phase: the signals are rebuilt and
 * subtracted, and the new record is searched and tracked like any other.  For sample i < blk of block k < ms_done[c] of
 * channel c, with the block's state (start, blk, rem_code, rem_carr, step, carr_freq) and its amplitude pair (aI, aQ):
 *   arg_i = carr_freq 2.0 pi (i / fs) + rem_carr,  t_i = linspace(rem_code, blk step + rem_code, blk, endpoint=False)[i],
 *   chip_i = code[(ceil(t_i) - 1) mod 1023],  s_c = chip_i (aI sin(arg_i) + aQ cos(arg_i))
 * v[n] = x[n] - sum_c s_c[n] at file position n = start + i, channels in channel order; y[n] = clip(rint(v[n]), -127, 127),
 * round half to even, where at least one block covers n, and y[n] = x[n] elsewhere (so -128 stays -128 there).  clipped:
 * the covered samples whose rint(v) lay outside [-127, 127].  tests/cancel_spec.py restates all of it in numpy.
 *
 * sgx_cancel_design: the amplitude pairs amp[n_ch][ms][2] from the series and the state; exact host code, needs no GPU.
 * p_j = 2 (I_P, Q_P)[j] / blk_j; (aI, aQ)_k is the mean, added in ascending j, of d p_j over the blocks j < ms_done[c] with
 * |j - k| <= (smooth - 1) / 2, d = sign(pI_j pI_k + pQ_j pQ_k) with 0 counting as +1 (the data-bit sign of block j against
 * block k).  smooth is odd, 1 .. 41; blocks k >= ms_done[c] and channels that are off hold 0.
 *
 * sgx_if_cancel: a resident int8 record (a streaming record is waited for, as sgx_track_replay) -> a NEW record of the same
 * length (sgx_if_free); the input is not written.  It runs sgx_replay_state itself and hands its codes back unchanged.  Every
 * output byte is written once by one lane and the channels are subtracted in channel order: two calls give the same bytes.
 * SGX_E_ARG, before anything is launched or written, for a NULL pointer, n_ch outside 1 .. 32, a data_type other than
 * SGX_DT_INT8, an amplitude that is not finite (all n_ch x ms pairs are looked at), an ms_done entry outside [0, ms], an empty
 * record, a record on another device.
 * sgx_cancel_host: the same work sample by sample with libm on the host, into the caller's y[n]; x is the record, the
 * bytes from rec_file_offset on.  Needs no GPU.  sgx_cancel_timing: HIP-event time of the last sgx_if_cancel's kernel. */
int sgx_cancel_design(const double* series, const sgx_replay_block* state, int32_t n_ch, int32_t ms, const int32_t* ms_done,
                      int32_t smooth, double* amp);
int sgx_if_cancel(sgx_ctx* c, const sgx_if* rec, int64_t rec_file_offset, const sgx_chan_init* ch, int32_t n_ch, int32_t ms,
                  const int32_t* ms_done, const double* series, int32_t data_type, const double* amp, sgx_if** out,
                  int64_t* clipped);
int sgx_cancel_host(const sgx_settings* s, const int8_t* x, size_t n, int64_t rec_file_offset, const sgx_chan_init* ch,
                    int32_t n_ch, int32_t ms, const int32_t* ms_done, const double* series, int32_t data_type,
                    const double* amp, int8_t* y, int64_t* clipped);
int sgx_cancel_timing(sgx_ctx* c, float* kernel_ms);

/* ---- narrowband interference excision ahead of acquisition (no reference counterpart: initialize.py:330-417 only plots
 * the spectrum a continuous-wave line shows up in) ----------------------------------------------------------------------
 * Opt-in.  A resident int8 record goes through a zero-phase integer FIR and comes out as a NEW int8 record of the same
 * length: sample n of the output lines up with sample n of the input, so code phases, absoluteSample and byte seeks mean
 * what they did, and acquisition, tracking, replay, quality and navigation run on the new record unchanged.
 * tests/notch_spec.py restates all of it in numpy.
 *
 * sgx_if_filter: taps h[n_taps] (n_taps = L odd, 1 .. SGX_FILTER_MAX_TAPS), c = (L - 1) / 2, x = 0 outside the record:
 *   y[n] = clip((sum_k h[k] x[n + c - k] + (shift ? 2^(shift-1) : 0)) >> shift, -127, 127)
 * with an arithmetic (floor) shift and a sum that is exact in int32 - pure integer, so the output is the contract's byte
 * for byte.  The whole record is filtered on the context's stream (a record that is still streaming in is waited for,
 * as sgx_if_wait to its full length); *out is an ordinary record (its own magnitude-bound cache; sgx_if_free).
 * SGX_E_ARG, before anything is launched: n_taps even or out of range, shift outside 0 .. 30, a |h[k]| > 32 512 (a tap must
 * split into two signed bytes, h = 256 hi + lo), 128 sum|h| >= 2^31, a NULL pointer, a record that lies on another device
 * than the context's (as the requantiser and the conditioning stage refuse it).  The record's bytes are read as int8:
 * records of other sample types (uint8, int16, ...) are not filtered.
 * sgx_filter_timing: HIP-event time of the last sgx_if_filter's kernel on this context.
 *
 * sgx_notch_design: the lines of a one-sided PSD (f_mhz, pxx of n_bins >= 2 bins, as sgx_probe_stats gives them) and the
 * notch that removes them; exact host code, needs no GPU.
 *   detect  baseline b[i] = median(pxx[max(0, i-128) : min(n, i+129)]); bin i is flagged when pxx[i] > 10^(threshold_db/10)
 *           b[i]; flagged bins with at most 2 unflagged bins between them form one line; centre = frequency of its largest
 *           bin, width = max(width_hz, the run's extent + 2 bin widths); at most SGX_NOTCH_MAX_LINES lines are kept, the
 *           strongest by peak / baseline, reported in ascending frequency in line_hz / line_width_hz (8 entries each).
 *   design  with m = k - c: h_ideal[k] = delta[m] - sum_i 2 (w_i / fs) sinc(w_i m / fs) cos(2 pi f_i m / fs), fs =
 *           s->samplingFreq, times a symmetric Hann window of n_taps points, times 2^SGX_NOTCH_SHIFT, rounded half to even
 *           into taps[n_taps]; *shift = SGX_NOTCH_SHIFT.  *n_lines == 0 is not an error: the taps are then the identity.
 * SGX_E_ARG for n_taps even or outside 1 .. SGX_FILTER_MAX_TAPS, n_bins < 2, a threshold or width that is not finite, a
 * width <= 0, a PSD entry that is negative or not finite, a NULL pointer, and for lines so wide that the taps leave what
 * sgx_if_filter takes. */
#define SGX_FILTER_MAX_TAPS 4095
#define SGX_NOTCH_MAX_LINES 8
#define SGX_NOTCH_SHIFT 14
int sgx_notch_design(const sgx_settings* s, const double* f_mhz, const double* pxx, int32_t n_bins, double threshold_db,
                     double width_hz, int32_t n_taps, int16_t* taps, int32_t* shift, double* line_hz,
                     double* line_width_hz, int32_t* n_lines);
int sgx_if_filter(sgx_ctx* c, const sgx_if* in, const int16_t* taps, int32_t n_taps, int32_t shift, sgx_if** out);
int sgx_filter_timing(sgx_ctx* c, float* kernel_ms);

/* ---- interleaved I/Q baseband records (no reference counterpart: every stage of the reference reads a real IF record) ----
 * Opt-in.  A resident record holding the raw BYTES of an interleaved 8-bit I/Q file (I0 Q0 I1 Q1 ...) at complex rate fs_c
 * comes out as a NEW int8 record of the same length: the equivalent REAL record at 2 fs_c whose IF is IF_bb + fs_c / 2.
 * z = I + jQ is interpolated by 2, shifted up by a quarter of the new rate and its real part kept; the spectrum of the
 * result lies in (0, fs_c) clear of its mirror image.  Acquisition, tracking, replay, quality, the notch and navigation run
 * on the new record unchanged, with samplingFreq = 2 fs_c and IF = IF_bb + fs_c / 2.  tests/iq_spec.py restates all of it
 * in numpy.
 *
 * sgx_if_from_iq: N bytes b (N even), pairs m = 0 .. N/2 - 1: I[m] = b[2m], Q[m] = b[2m+1]; SGX_IQ_Q_FIRST swaps the two
 * roles; SGX_IQ_OFFSET_BINARY first turns every byte into byte - 128 (uint8 files: XOR 0x80 read as int8), without it
 * the bytes are int8 as they stand and -128 is a legal value.  Taps h[n_taps] (n_taps = L odd, 1 .. SGX_IQ_MAX_TAPS),
 * c = (L - 1) / 2:
 *   u[2m] = I[m] + j Q[m], u[odd] = 0, u = 0 outside [0, N);   w[n] = sum_k h[k] u[n + c - k]
 *   a[n] = Re w[n], -Im w[n], -Re w[n], Im w[n]  for n mod 4 = 0, 1, 2, 3
 *   y[n] = clip((a[n] + (shift ? 2^(shift-1) : 0)) >> shift, -127, 127)
 * with an arithmetic (floor) shift and a sum that is exact in int32 - pure integer, so the output is the contract's byte
 * for byte.  Output sample n is the instant of byte n's pair (half an input period later for odd n): a byte offset into
 * the file is a sample offset into the new record, so skipNumberOfBytes (even), code phases and absoluteSample keep their
 * meaning.  The whole record is converted on the context's stream (a record that is still streaming in is waited for, as
 * sgx_if_wait to its full length); the input is left alone; *out is an ordinary record (its own magnitude-bound cache;
 * sgx_if_free).  SGX_E_ARG, before anything is launched: n_taps even or out of range, shift outside 0 .. 30, a
 * |h[k]| > 32 512 (a tap must split into two signed bytes, h = 256 hi + lo), 128 sum|h| >= 2^31, an unknown flag bit, a
 * NULL pointer, a record that lies on another device than the context's, N odd.
 * sgx_iq_timing: HIP-event time of the last sgx_if_from_iq's kernel on this context.
 * sgx_iq_tile: the output bytes one workgroup of the kernel makes (the lengths at which its tile seams lie).
 *
 * sgx_iq_design: the default interpolation filter, exact host code, needs no GPU.  With m = k - c:
 *   h[k] = rint(2^SGX_IQ_SHIFT sinc(m / 2) hann_L[k]),  sinc(t) = sin(pi t) / (pi t), rounded half to even,
 * hann_L the symmetric Hann window of L points (1 for L = 1): a half-band low-pass at the input's Nyquist frequency with
 * the gain of 2 that zero-stuffing needs.  sinc(m / 2) is taken in closed form - 1 at m = 0, (-1)^((m-1)/2) 2 / (pi m) at
 * odd m - so the centre tap is 2^SGX_IQ_SHIFT and every other even-m tap exactly 0.  *shift = SGX_IQ_SHIFT.  SGX_E_ARG
 * for n_taps even or outside 1 .. SGX_IQ_MAX_TAPS, a NULL pointer. */
#define SGX_IQ_MAX_TAPS 255
#define SGX_IQ_SHIFT 14
#define SGX_IQ_Q_FIRST 1
#define SGX_IQ_OFFSET_BINARY 2
int sgx_iq_design(int32_t n_taps, int16_t* taps, int32_t* shift);
int sgx_if_from_iq(sgx_ctx* c, const sgx_if* iq_bytes, const int16_t* taps, int32_t n_taps, int32_t shift, int32_t flags,
                   sgx_if** out);
int sgx_iq_timing(sgx_ctx* c, float* kernel_ms);
int sgx_iq_tile(int32_t* tile_bytes);

/* ---- int16 / float32 records through a fixed-gain requantiser (no reference counterpart; the stage in front of
 * sgx_if_from_iq for sc16 and fc32 captures) -----------------------------------------------------------------------------
 * Opt-in.  A resident record holding the raw BYTES of a file of little-endian int16 (w = 2) or IEEE float32 (w = 4)
 * elements, N bytes = n = N / w elements x[i], comes out as a NEW int8 record of n bytes, element i -> byte i, through one
 * fixed gain (a digital AGC that does not vary in time).  I and Q of an interleaved file share the gain, so the stage is
 * elementwise and knows nothing of pairs; it reads real records of these types just as well.  data_type is SGX_DT_INT16 or
 * SGX_DT_FLOAT32.  tests/requant_spec.py restates all of it in numpy.
 *
 * sgx_requant_stats_of: elements [offset, offset + count) of the record.  NaN and +-inf elements are counted in n_nonfinite
 * and left out of everything else; n_finite + n_nonfinite = count; max_abs = max |x| (0 for an empty window); the counts and
 * max_abs are exact.
 *   int16    sum and sum_sq are accumulated exactly in integers and converted to double once: float(int(...)).
 *   float32  each element is promoted to double and squared there (exact) and the doubles are summed in a FIXED order: two
 *            calls on the same bytes and window give the same bits.  Against the correctly rounded sums the results differ
 *            by at most count 2^-52 sum|x| (sum) and count 2^-52 sum_sq (sum_sq), the worst case of recursive summation in
 *            any order.  Denormal elements count with their value.
 * The window is read on the context's stream (a record that is still streaming in is waited for up to the window's end).
 *
 * sgx_requant_gain: the gain that brings a record with these statistics to target_rms, in (0, 127]; exact host code, needs
 * no GPU.  rms = sqrt(sum_sq / n_finite), g = target_rms / rms; g = 1 for n_finite <= 0 or an rms that is not > 0.
 *   *shift = the largest S in 0 .. 30 with rint(g 2^S) <= 32767 (half to even), *mult = max(1, rint(g 2^S)); if even S = 0
 *            gives more than 32767: *mult = 32767, *shift = 0.  |x mult| + 2^(shift-1) < 2^31 then holds for every int16 x.
 *   *scale = (float)g, clamped to [SGX_REQUANT_SCALE_MIN, SGX_REQUANT_SCALE_MAX] = [2^-100, 2^100].
 * All three are filled for either data_type; sgx_if_requantize reads the pair or the scale by its own data_type.
 *
 * sgx_if_requantize:
 *   int16    y = clip((x mult + ((1 << shift) >> 1)) >> shift, -127, 127), arithmetic (floor) shift, exact in int32.
 *   float32  y = clip(rint(x * scale), -127, 127): ONE float32 multiply, round to nearest even; NaN -> 0, +-inf -> +-127.
 *            With scale <= 2^100 a denormal element (below 2^-126) times scale lies below 2^-26 and rounds to 0, as does a
 *            denormal product: the output does not depend on whether the hardware flushes denormals.
 * The whole record is requantised on the context's stream (a record that is still streaming in is waited for, as
 * sgx_if_wait to its full length); the input is left alone; *out is an ordinary record (sgx_if_free); N = 0 gives an empty
 * record.  *n_clipped (may be NULL): the outputs that are +-127.
 * sgx_requant_timing: HIP-event times of the last sgx_requant_stats_of's and the last sgx_if_requantize's kernel on this
 * context.  sgx_requant_tile: the output bytes one workgroup of the quantiser makes (where its tile seams lie).
 * SGX_E_ARG, before anything is launched, with a text that names the argument: a data_type other than the two, N not a
 * multiple of w, a window that leaves the record, mult outside 1 .. 32767 or shift outside 0 .. 30 (int16), a scale that is
 * not finite or outside [2^-100, 2^100] (float32), target_rms outside (0, 127], a NULL pointer. */
#define SGX_REQUANT_SCALE_MIN 0x1p-100f
#define SGX_REQUANT_SCALE_MAX 0x1p+100f
typedef struct sgx_requant_stats {
    int64_t n_finite, n_nonfinite;
    double max_abs, sum, sum_sq;
} sgx_requant_stats;        /* 40 bytes */
int sgx_requant_stats_of(sgx_ctx* c, const sgx_if* rec, int32_t data_type, size_t offset, size_t count,
                         sgx_requant_stats* out);
int sgx_requant_gain(const sgx_requant_stats* st, int32_t data_type, double target_rms, int32_t* mult, int32_t* shift,
                     float* scale);
int sgx_if_requantize(sgx_ctx* c, const sgx_if* rec, int32_t data_type, int32_t mult, int32_t shift, float scale,
                      sgx_if** out, int64_t* n_clipped);
int sgx_requant_timing(sgx_ctx* c, float* stats_ms, float* kernel_ms);
int sgx_requant_tile(int32_t* tile_bytes);

/* ---- block-wise front-end conditioning: DC removal, AGC and pulse blanking (no reference counterpart; the stage in front
 * of sgx_if_from_iq, where the fixed-gain requantiser sits otherwise) ------------------------------------------------------
 * Opt-in.  A resident record holding the raw BYTES of a file of int8 (w = 1) or little-endian int16 (w = 2) elements,
 * n = N / w of them, comes out as a NEW int8 record of n bytes, element i -> byte i.  data_type is SGX_DT_INT8 or
 * SGX_DT_INT16; with SGX_COND_OFFSET_BINARY (w = 1 only) an element is byte - 128.  lanes L is 1 or 2: frame f holds
 * elements x[f L + l], L = 2 is interleaved I/Q; n must be a multiple of L, F = n / L frames.  float32 is out of scope: its
 * sums are not order-free, so there is no byte-exact contract.  Blocks of `block` = B frames, 256 <= B <= 16384, a multiple
 * of 16: block k holds frames [k B, min(F, (k + 1) B)), n_k >= 1 of them, K = ceil(F / B); F = 0 gives K = 0 and an empty
 * output.  tests/cond_spec.py restates all of it in numpy.
 *
 * sgx_cond_block_stats (device): per block, in exact integers, with S_l the sum of lane l over the block:
 *   dc_l = (16 S_l + (n_k >> 1)) // n_k   (floor division; the DC in 1/16 LSB)
 *   d_l[f] = 16 x - dc_l, |d| < 2^21;  e[f] = sum_l d_l[f]^2 < 2^43;  P_0 = sum_f e[f] < 2^57, m_0 = n_k, e_max = max e[f]
 * and two clipping rounds r = 1, 2 with blank_q4 = 16 c^2, an integer that is 0 or 16 .. 4096:
 *   theta_r = ((P_{r-1} // m_{r-1}) blank_q4) >> 4;  the frames with e[f] <= theta_r are kept: m_r of them, P_r their sum
 * (blank_q4 >= 16 keeps every frame at or below the mean, so m_r >= 1; blank_q4 = 0 skips the rounds: m_2 = n_k, P_2 = P_0).
 * out[k] = {n_k, m_2, dc_0, dc_1 (0 for L = 1), P_2, P_0, e_max, 0}.  out must hold out_cap >= K entries; *n_blocks = K.
 * The record is read on the context's stream (a record that is still streaming in is waited for).
 *
 * sgx_cond_plan: DC, gain and blanking threshold per block; exact host code in doubles, in this order, needs no GPU.
 *   v_k = p_kept / (kept L 256.0);  D_lk = (double)dc_l;  alpha = 1 / agc_blocks (agc_blocks real, >= 1)
 *   a_0 = v_0, a_k = a_{k-1} + alpha (v_k - a_{k-1});  A_lk from D_lk by the same recursion
 *   g_k = target_rms / sqrt(a_k), 1 where a_k is not > 0;  (mult, shift) from g_k by sgx_requant_gain's rule: the largest
 *   shift in 0 .. 30 with rint(g 2^shift) <= 32767, mult = max(1, that);  dc_l = (int)rint(A_lk)
 *   theta = (int64)floor(a_k (16 L blank_q4)), INT64_MAX for blank_q4 = 0.   target_rms lies in (0, 127].
 *
 * sgx_if_condition (device): with k the block of frame f and plan[k] = {dc0, dc1, mult, shift, theta}:
 *   d_l = 16 x - dc_l;  hit[f] = sum_l d_l^2 > theta;  frame f is BLANKED if any frame within `guard` G (0 .. 64) of it is
 *   hit - the dilation crosses block boundaries and the kernel's tile seams and is cut only by the ends of the record.
 *   A blanked element gives 0, any other y = clip((d mult + (1 << (shift + 3))) >> (shift + 4), -127, 127), a floor shift
 *   of a 64-bit intermediate.  *blanked_frames and *clipped (elements on +-127; either may be NULL) are exact.
 * n_plan must be K; a plan entry has mult 1 .. 32767, shift 0 .. 30, |dc| <= 2^20, theta >= 0.  The input is left alone;
 * *out is an ordinary record (sgx_if_free).
 * sgx_cond_timing: HIP-event times of the last sgx_cond_block_stats' and the last sgx_if_condition's kernel on this context.
 * sgx_cond_tile: the frames one workgroup of the apply kernel makes (where its tile seams lie).
 * SGX_E_ARG, before anything is launched: a data_type other than the two, an unknown flag, offset binary with int16, lanes
 * other than 1 or 2, a block outside 256 .. 16384 or no multiple of 16, blank_q4 other than 0 or 16 .. 4096, N that does not
 * hold whole frames, guard outside 0 .. 64, out_cap or n_plan that is not K, a plan entry out of range, kept < 1,
 * target_rms outside (0, 127], agc_blocks that is not finite or below 1, a NULL pointer. */
#define SGX_COND_OFFSET_BINARY 1
typedef struct sgx_cond_stats {
    int64_t n, kept, dc0, dc1, p_kept, p_all, e_max, reserved;
} sgx_cond_stats;           /* 64 bytes */
typedef struct sgx_cond_entry {
    int32_t dc0, dc1, mult, shift;
    int64_t theta;
} sgx_cond_entry;           /* 24 bytes */
int sgx_cond_block_stats(sgx_ctx* c, const sgx_if* rec, int32_t data_type, int32_t lanes, int32_t block, int32_t blank_q4,
                         int32_t flags, sgx_cond_stats* out, size_t out_cap, size_t* n_blocks);
int sgx_cond_plan(const sgx_cond_stats* stats, size_t n_blocks, int32_t lanes, int32_t blank_q4, double target_rms,
                  double agc_blocks, sgx_cond_entry* plan);
int sgx_if_condition(sgx_ctx* c, const sgx_if* rec, int32_t data_type, int32_t lanes, int32_t block, int32_t flags,
                     const sgx_cond_entry* plan, size_t n_plan, int32_t guard, sgx_if** out, int64_t* blanked_frames,
                     int64_t* clipped);
int sgx_cond_timing(sgx_ctx* c, float* stats_ms, float* apply_ms);
int sgx_cond_tile(int32_t* tile_frames);

/* ---- 1-, 2- and 4-bit packed records through an unpacker (no reference counterpart; first of all front-end stages, ahead
 * of sgx_if_from_iq and sgx_if_filter) ----------------------------------------------------------------------------------------
 * Opt-in.  A resident record holding the raw BYTES of a packed file, N bytes B[0 .. N) of b-bit fields, b = bits in
 * {1, 2, 4}, comes out as a NEW int8 record, one byte per selected field.  tests/unpack_spec.py restates all of it in numpy.
 *
 * Field j, j = 0 .. 8N/b - 1, lies in byte j b / 8 at position p = j mod (8 / b); its code is
 *   (B >> (8 - b (p + 1))) & (2^b - 1)   first field in the high bits, or with SGX_UNPACK_LSB_FIRST
 *   (B >> (b p)) & (2^b - 1)             first field in the low bits.
 * A frame is `frame` = F consecutive fields, F in {1, 2, 4, 8, 16} (a frame never straddles a byte partially); 8N/b must be a
 * multiple of F.  Of every frame the stage takes `take` fields from field `first` on, take >= 1, first >= 0,
 * first + take <= F:
 *   n_out = (8N / b / F) take,   out[q take + t] = table[code(q F + first + t)]
 * A real or an interleaved I/Q file is F = 1 (the converter sorts I and Q out); one of four interleaved streams is F = 4,
 * first = s, take = 1; the second antenna of a two-antenna I/Q file F = 4, first = 2, take = 2.  table holds 2^b int8
 * values, any mapping.  code_counts (16 int64; may be NULL) receives the exact count of each code among the selected fields,
 * entries 2^b and above 0: the histogram of the ADC's levels.
 * The whole record is unpacked on the context's stream (a record that is still streaming in is waited for, as sgx_if_wait
 * to its full length); the input is left alone; *out is an ordinary record (sgx_if_free); N = 0 gives an empty record and
 * launches nothing.
 *
 * sgx_unpack_table: the table of the three usual encodings as symmetric odd levels times one integer scale,
 * table[c] = level(c) (peak / (2^b - 1)) with an integer (floor) division, peak in 2^b - 1 .. 127; exact host code, needs
 * no GPU.
 *   SGX_UNPACK_SIGN_MAGNITUDE   s = c >> (b - 1), mu = c & (2^(b-1) - 1): level (1 - 2 s)(2 mu + 1)
 *   SGX_UNPACK_OFFSET_BINARY    level 2 c - (2^b - 1)
 *   SGX_UNPACK_TWOS_COMPLEMENT  k = c, or c - 2^b for c >= 2^(b-1): level 2 k + 1
 * 2 bits, sign/magnitude, peak 48: {16, 48, -16, -48}.  A peak of 63 or below keeps the sum of magnitudes of every
 * 2 048-sample window below the bound at which tracking leaves its fastest kernel.
 * sgx_unpack_timing: HIP-event time of the last sgx_if_unpack's kernel on this context.
 * sgx_unpack_tile: the output bytes one workgroup of the kernel makes (where its tile seams lie).
 * SGX_E_ARG, before anything is launched, with a text that names the argument: bits other than 1, 2 or 4, an unknown flag
 * or encoding, frame outside the five values, take < 1, first < 0 or first + take > frame, fields that do not fill whole
 * frames, peak out of range, a NULL record, table or out, a record that lies on another device than the context's, a record
 * beyond one launch. */
#define SGX_UNPACK_LSB_FIRST 1
#define SGX_UNPACK_SIGN_MAGNITUDE 0
#define SGX_UNPACK_OFFSET_BINARY 1
#define SGX_UNPACK_TWOS_COMPLEMENT 2
int sgx_unpack_table(int32_t bits, int32_t encoding, int32_t peak, int8_t* table);
int sgx_if_unpack(sgx_ctx* c, const sgx_if* rec, int32_t bits, int32_t flags, int32_t frame, int32_t first, int32_t take,
                  const int8_t* table, sgx_if** out, int64_t* code_counts);
int sgx_unpack_timing(sgx_ctx* c, float* kernel_ms);
int sgx_unpack_tile(int32_t* tile_bytes);

/* ---- band selection and integer decimation ahead of acquisition (no reference counterpart; behind the unpacker, the
 * conditioning stage and the requantiser, in front of sgx_if_from_iq and sgx_if_filter) -----------------------------------
 * Opt-in.  A resident int8 record of N bytes goes through an integer FIR that selects a band and comes out as a NEW int8
 * record at 1 / D of the rate, D = 2 .. 16.  Every later stage then runs at the lower rate.  tests/decim_spec.py restates
 * all of it in numpy.
 *
 * sgx_if_decimate: n_taps = L odd, 1 .. SGX_DECIM_MAX_TAPS, c = (L - 1) / 2, x = 0 outside the record, rnd = shift ?
 * 2^(shift-1) : 0, q(a) = clip((a + rnd) >> shift, -127, 127) with an arithmetic (floor) shift.
 *   lanes = 1  a real record x[0 .. N); taps int16 h[L]:
 *                y[m] = q(sum_k h[k] x[m D + c - k]),  m = 0 .. ceil(N / D) - 1
 *   lanes = 2  interleaved I/Q, N even, z[n] = b[2n] + j b[2n+1]; taps COMPLEX, int16 h[2 L], re and im interleaved:
 *                w[m] = sum_k h[k] z[m D + c - k],  output bytes q(Re w[m]), q(Im w[m]),  m = 0 .. ceil(N/2 / D) - 1
 *              Complex taps select a band that is not centred on zero.
 * SGX_DECIM_OFFSET_BINARY first turns every input byte into byte - 128 (XOR 0x80 read as int8).  There is no Q-first flag:
 * for a Q-first file the caller conjugates the taps and the output is Q-first again (filtering Q + jI with conj(h) gives
 * Im w + j Re w).  Output frame m is the instant of input frame m D (zero phase): a frame offset into the input that is a
 * multiple of D is a frame offset into the output.  *clipped (may be NULL): the exact count of output bytes whose value
 * before the clip lay outside [-127, 127].  The sums are exact in int32 - pure integer, so the output is the contract's
 * byte for byte.  The whole record is read on the context's stream (a record that is still streaming in is waited for, as
 * sgx_if_wait to its full length); the input is left alone; *out is an ordinary record (sgx_if_free); N = 0 gives an empty
 * record and launches nothing.
 * SGX_E_ARG, before anything is launched, with a text that names the argument: L even or out of range, D outside 2 .. 16,
 * lanes not 1 or 2, shift outside 0 .. 30, a tap component beyond 32 512 in magnitude, 128 sum|h| >= 2^31 (lanes = 2: the
 * sum of |re| + |im|, so that both output sums stay in int32), an unknown flag bit, a NULL pointer, N odd with lanes = 2, a
 * record that lies on another device than the context's, a record beyond one launch.
 * sgx_decim_timing: HIP-event time of the last sgx_if_decimate's kernel on this context.
 * sgx_decim_tile: the output bytes one workgroup of the kernel makes (where its tile seams lie).
 *
 * sgx_decim_design: the band-pass that selects f0 +- bandwidth_hz / 2 of a record at rate fs (lanes = 2: the complex rate,
 * f0 the offset from the centre, either sign); exact host code, needs no GPU.  With m = k - c, in doubles, in this order:
 *   t = bandwidth_hz m / fs;  sinc = sin(pi t) / (pi t), 1 at m = 0;  hann = 0.5 - 0.5 cos(2 pi k / (L - 1)), 1 for L = 1
 *   lp = (bandwidth_hz / fs) sinc hann;  ph = 2 pi f0 m / fs;  a = 2^SGX_DECIM_SHIFT g lp
 *   lanes = 1: h[k] = rint(a (2 cos ph));   lanes = 2: h[2k] = rint(a cos ph), h[2k+1] = rint(a sin ph)   (half to even)
 * g = gain, or for gain <= 0 the gain that keeps a white input's rms: sqrt((fs / l) / bandwidth_hz), l = 2 for a real
 * record and 1 for I/Q.  *shift = SGX_DECIM_SHIFT, *fs_out = fs / D, and where the band lands:
 *   lanes = 2: *f_out = ((f0 + fs_out / 2) mod fs_out) - fs_out / 2 (mod as floor), *inverted = 0
 *   lanes = 1: z = floor(f0 / (fs_out / 2)), *inverted = z & 1, *f_out = f0 - z fs_out / 2 where upright, else
 *              (z + 1) fs_out / 2 - f0.  An inverted band acquires and tracks like any other; the sign of the Doppler it
 *              reports is flipped.
 * SGX_E_ARG: fs or bandwidth_hz not finite or not > 0, f0 or gain not finite, lanes not 1 or 2, D outside 2 .. 16, n_taps
 * even or out of range, a NULL pointer, a tap that leaves what sgx_if_decimate takes, and a band that aliases onto itself:
 * lanes = 1, f0 +- bandwidth_hz / 2 does not lie strictly inside one Nyquist zone [z, z + 1) fs_out / 2, 0 <= z < D (the
 * default record, 38.192 Msps with the IF at 9.548 MHz, at D = 2 or 4: the IF sits on a zone edge); lanes = 2,
 * bandwidth_hz >= fs_out. */
#define SGX_DECIM_MAX_TAPS 511
#define SGX_DECIM_SHIFT 14
#define SGX_DECIM_OFFSET_BINARY 1
int sgx_decim_design(double fs, double f0, double bandwidth_hz, int32_t lanes, int32_t D, int32_t n_taps, double gain,
                     int16_t* taps, int32_t* shift, double* fs_out, double* f_out, int32_t* inverted);
int sgx_if_decimate(sgx_ctx* c, const sgx_if* rec, int32_t lanes, const int16_t* taps, int32_t n_taps, int32_t shift,
                    int32_t D, int32_t flags, sgx_if** out, int64_t* clipped);
int sgx_decim_timing(sgx_ctx* c, float* kernel_ms);
int sgx_decim_tile(int32_t* tile_bytes);

/* ---- rational resampling by L / M ahead of acquisition (no reference counterpart; behind the unpacker, the conditioning
 * stage or requantiser, the decimator and sgx_if_from_iq, in front of sgx_if_filter) ---------------------------------------
 * Opt-in.  A resident REAL int8 record of N bytes is brought to L / M of its rate, 1 <= M <= 3, M < L <= 16, gcd(L, M) = 1
 * (31 pairs), as a NEW int8 record: a capture below the 15.4 samples per chip the fast tracking kernels need reaches them
 * (4.096 Msps x 10, 16.368 Msps x 7/3, 2.048 Msps x 8).  tests/resamp_spec.py restates all of it in numpy.
 *
 * sgx_if_resample: n_taps = Lh odd, 1 .. SGX_RESAMP_MAX_TAPS, c = (Lh - 1) / 2, taps int16 h[Lh], rnd = shift ?
 * 2^(shift-1) : 0, q(a) = clip((a + rnd) >> shift, -127, 127) with an arithmetic (floor) shift.  With the zero-stuffed
 * record u[i] = x[i / L] where L divides i and 0 <= i / L < N, else 0:
 *   y[m] = q(sum_k h[k] u[m M + c - k]),  m = 0 .. ceil(N L / M) - 1
 * Output sample m is the instant of input position m M / L (zero phase): a sample offset into the input that is a multiple
 * of M is the output offset (offset L / M).  *clipped (may be NULL): the exact count of outputs whose value before the clip
 * lay outside [-127, 127].  The sums are exact in int32 - pure integer, so the output is the contract's byte for byte.  No
 * multiply-accumulate is spent on a stuffed zero: the kernel runs the L sub-filters h[phi + j L] on the input.  The whole
 * record is read on the context's stream (a record that is still streaming in is waited for, as sgx_if_wait to its full
 * length); the input is left alone; *out is an ordinary record (sgx_if_free); N = 0 gives an empty record and launches
 * nothing.  SGX_E_NOMEM when the output cannot be allocated.
 * SGX_E_ARG, before anything is launched, with a text that names the argument: a pair L / M outside the 31, n_taps even or
 * out of range, shift outside 0 .. 30, a tap beyond 32 512 in magnitude, 128 sum|h| >= 2^31, a NULL pointer, a record that
 * lies on another device than the context's, an output beyond one launch.
 * sgx_resamp_timing: HIP-event time of the last sgx_if_resample's kernel on this context.
 * sgx_resamp_tile: the output bytes one workgroup of the kernel makes at L = 16, the largest; at a pair L / M a workgroup
 * makes tile_bytes L / 16 (where its tile seams lie).
 *
 * sgx_resamp_design: the low-pass at the stuffed rate fu = fs L; exact host code, needs no GPU.  fc = cutoff_hz, or for
 * cutoff_hz = 0 min(fs, fs L / M) / 2.  With m = k - c, in doubles, in this order:
 *   fu = fs L;  t = 2 fc m / fu;  sinc = sin(pi t) / (pi t), 1 at m = 0;  hann = 0.5 - 0.5 cos(2 pi k / (Lh - 1)), 1 for
 *   Lh = 1;  lp = (2 fc / fu) sinc hann;  h[k] = rint((2^SGX_RESAMP_SHIFT g L) lp)   (half to even; g = gain)
 * *shift = SGX_RESAMP_SHIFT, *fs_out = fs L / M.  The usual length is 24 L + 1: beyond fc + 2 fu / (Lh - 1) the taps are
 * 44 dB down; with M = 1 and the default cutoff phase 0 is the single tap 2^14, y[m L] = x[m].
 * SGX_E_ARG: fs, gain not finite or not > 0, cutoff_hz not finite, negative or above min(fs, fs_out) / 2, a pair outside
 * the 31, n_taps even or out of range, a NULL pointer, a tap that leaves what sgx_if_resample takes. */
#define SGX_RESAMP_MAX_TAPS 1023
#define SGX_RESAMP_SHIFT 14
int sgx_resamp_design(double fs, int32_t L, int32_t M, int32_t n_taps, double cutoff_hz, double gain, int16_t* taps,
                      int32_t* shift, double* fs_out);
int sgx_if_resample(sgx_ctx* c, const sgx_if* rec, const int16_t* taps, int32_t n_taps, int32_t shift, int32_t L, int32_t M,
                    sgx_if** out, int64_t* clipped);
int sgx_resamp_timing(sgx_ctx* c, float* kernel_ms);
int sgx_resamp_tile(int32_t* tile_bytes);

/* ---- multi-antenna records: a space-time combiner with power-inversion weights (no reference counterpart; directly behind
 * the unpacker, in front of every other stage) ---------------------------------------------------------------------------
 * Opt-in.  A resident int8 record of N bytes holds F = N / (A lanes) frames of A antennas: byte (f A + a) lanes + l is
 * component l of antenna a at frame f; lanes = 1 a real record x_a[f], lanes = 2 interleaved I/Q, z_a[f] = I + j Q.
 * SGX_ARRAY_OFFSET_BINARY first turns every byte into byte - 128 (XOR 0x80 read as int8).  A = 2 .. SGX_ARRAY_MAX_ANTENNAS,
 * K odd, 1 .. SGX_ARRAY_MAX_TAPS, A K <= SGX_ARRAY_MAX_WEIGHTS, N a multiple of A lanes; x = 0 outside the record.  The
 * exact integer statistics of the streams are taken on the GPU (sgx_array_stats), weights that minimise the output power
 * while one tap of one antenna is held at 1 are designed from them on the host (sgx_array_design: power inversion, which
 * needs no array geometry, calibration or satellite direction - the GNSS signals lie below the noise, so only what stands
 * above it is cancelled), and the A streams go through one integer FIR each and are summed into ONE int8 record
 * (sgx_if_combine) that every later stage reads as before.  tests/array_spec.py restates all of it in numpy.
 *
 * sgx_array_stats: the lag statistics of the whole record, int64 rho[A][A][K][lanes]:
 *   lanes = 1   rho[a][b][d]    = sum_{f = 0}^{F-1-d} x_a[f + d] x_b[f]
 *   lanes = 2   rho[a][b][d][.] = sum_{f = 0}^{F-1-d} z_a[f + d] conj(z_b[f]),  the real part, then the imaginary part
 * Exact integers: a workgroup sums a tile of sgx_array_stats_tile frames in 32 bits (at most 2^27 in magnitude) and adds
 * the tile's sums into 64 bits, so no partial sum wraps; the result does not depend on the order and two calls are
 * bit-identical.  A record that is still streaming in is waited for; N = 0 gives zeros and launches nothing.
 * SGX_E_ARG, before anything is launched, with a text that names the argument: lanes not 1 or 2, A or K outside the limits
 * above, an unknown flag bit, a NULL pointer, N no multiple of A lanes, a record on another device than the context's.
 *
 * sgx_array_design: exact host code, needs no GPU.  frames = F.  n = A K, c = (K - 1) / 2, the stacked index (a, k) = a K + k
 * stands for x_a[f + c - k].  In doubles, in this order (every sum from its first index up, starting from the first term):
 *   1. R[(a,k)][(b,l)] = rho_ab[l - k] / frames, rho_ab[-d] = conj(rho_ba[d]) (int64 -> double, then the division)
 *   2. tr = sum_i R[i][i];  ld = (loading tr) / n;  RL = R with ld added to every diagonal entry
 *   3. M = RL (lanes = 1, m = n) or the real symmetric embedding [[P, -Q], [Q, P]] of RL = P + j Q (lanes = 2, m = 2 n);
 *      Cholesky M = L L^T, for j = 0 .. m-1, for i = j .. m-1:  s = M[i][j] - L[i][0] L[j][0] - .. - L[i][j-1] L[j][j-1]
 *      (one subtraction after the other); i = j: s > 0 or the matrix is refused, L[j][j] = sqrt(s); else L[i][j] = s / L[j][j].
 *      b = unit vector at (ref, c).  Forward: y[i] = (b[i] - L[i][0] y[0] - .. - L[i][i-1] y[i-1]) / L[i][i], i upwards;
 *      back: g[i] = (y[i] - L[i+1][i] g[i+1] - .. - L[m-1][i] g[m-1]) / L[i][i], i downwards.  lanes = 2: g = g[0..n) + j g[n..2n)
 *   4. g <- g / Re g[(ref,c)] (each component divided);  h = conj(g)
 *   5. p_out = g^H R g with the UNLOADED R: t_i = sum_j R[i][j] g[j] (lanes = 2: re = P gr - Q gi, im = P gi + Q gr, each
 *      product added or subtracted in this order per j), p_out = sum_i (gr_i tr_i [+ gi_i ti_i])
 *   6. *gain = target_rms / sqrt(p_out / lanes)
 *   7. taps[(a K + k) lanes + l] = rint((2^SGX_ARRAY_SHIFT gain) h) (half to even), re then im;  *shift = SGX_ARRAY_SHIFT
 *   8. *suppression_db = 10 log10(R[(ref,c)][(ref,c)] / p_out)
 *   9. weights[(a K + k) lanes + l] = h before the gain
 * The output w[f] = sum_a sum_k h_a[k] z_a[f + c - k] = g^H u[f] then has the least power among all weights with
 * h_ref[c] = 1, and power target_rms^2 per component behind the gain.
 * SGX_E_ARG with a text that names the cause: a matrix that is not positive definite (an all-zero record), a tap beyond
 * 32 512 in magnitude, 128 sum(|re| + |im|) >= 2^31, ref outside 0 .. A - 1, loading < 0 or not finite, target_rms outside
 * (0, 127], frames < 1, the limits above, a NULL pointer (weights, gain and suppression_db may be NULL).
 *
 * sgx_if_combine: a NEW int8 record of F lanes bytes; taps int16 [A][K] (lanes = 2: COMPLEX, [A][K][2], re and im
 * interleaved), c = (K - 1) / 2, rnd = shift ? 2^(shift-1) : 0, q(a) = clip((a + rnd) >> shift, -127, 127) with an
 * arithmetic (floor) shift, exactly as sgx_if_decimate:
 *   lanes = 1   y[f] = q(sum_a sum_k h_a[k] x_a[f + c - k])
 *   lanes = 2   w[f] = sum_a sum_k h_a[k] z_a[f + c - k],  output bytes q(Re w[f]), q(Im w[f])
 * Output frame f is the instant of input frame f.  The sums are exact in int32 under the bound on sum|h|, so the output is
 * the contract's byte for byte.  *clipped (may be NULL): the exact count of output bytes whose value before the clip lay
 * outside [-127, 127].  The input is left alone; a record that is still streaming in is waited for; *out is an ordinary
 * record (sgx_if_free); N = 0 gives an empty record and launches nothing.
 * SGX_E_ARG, before anything is launched, with a text that names the argument: lanes not 1 or 2, A or K outside the limits
 * above, shift outside 0 .. 30, a tap component beyond 32 512 in magnitude, 128 sum(|re| + |im|) over all antennas >= 2^31,
 * an unknown flag bit, a NULL pointer, N no multiple of A lanes, a record on another device than the context's, a record
 * beyond one launch.
 * sgx_array_stats_timing, sgx_combine_timing: HIP-event time of the last call's kernel on this context.
 * sgx_array_stats_tile: the frames one workgroup sums at a time; sgx_combine_tile: the output bytes one workgroup makes. */
#define SGX_ARRAY_MAX_ANTENNAS 8
#define SGX_ARRAY_MAX_TAPS 15
#define SGX_ARRAY_MAX_WEIGHTS 64
#define SGX_ARRAY_SHIFT 12
#define SGX_ARRAY_OFFSET_BINARY 1
int sgx_array_stats(sgx_ctx* c, const sgx_if* rec, int32_t lanes, int32_t A, int32_t K, int32_t flags, int64_t* rho);
int sgx_array_stats_timing(sgx_ctx* c, float* kernel_ms);
int sgx_array_stats_tile(int32_t* tile_frames);
int sgx_array_design(const int64_t* rho, int64_t frames, int32_t lanes, int32_t A, int32_t K, int32_t ref, double loading,
                     double target_rms, int16_t* taps, int32_t* shift, double* weights, double* gain,
                     double* suppression_db);
int sgx_if_combine(sgx_ctx* c, const sgx_if* rec, int32_t lanes, int32_t A, const int16_t* taps, int32_t K, int32_t shift,
                   int32_t flags, sgx_if** out, int64_t* clipped);
int sgx_combine_timing(sgx_ctx* c, float* kernel_ms);
int sgx_combine_tile(int32_t* tile_bytes);

/* ---- weights that change along the record: the same three steps block by block (opt-in; tests/array_block_spec.py) -------
 * The record layout, lanes, A, K, flags, c = (K - 1) / 2 and q() are those above.  A block is B frames, B a positive multiple
 * of SGX_ARRAY_BLOCK_UNIT = 4096: the combiner's tile of a real record, two of its tiles for I/Q and two tiles of the
 * statistics kernel, so that no workgroup of either kernel straddles a seam.  n_blocks = ceil(F / B), the last block may be
 * short; n_blocks <= SGX_ARRAY_MAX_BLOCKS = 2^20 (the statistics launch one workgroup or more per block, the table of
 * statistics holds A A K lanes int64 per block and the tap table up to 768 bytes per block; 2^20 blocks of 4096 frames are
 * 17 minutes at 4.092 Msps).
 *
 * sgx_array_block_stats: int64 rho_blocks[n_blocks][A][A][K][lanes].  Block j holds the terms of the sums above whose x_b
 * frame f lies in [j B, min((j + 1) B, F)); the x_a[f + d] factor may lie in the next block, frames beyond F are zero.  Exact
 * integers that do not depend on the order, two calls are bit-identical, and sum_j rho_blocks[j] is what sgx_array_stats
 * gives.  F = 0 launches nothing and writes nothing.  SGX_E_ARG as sgx_array_stats, and for a B that is no positive multiple
 * of the unit, more than SGX_ARRAY_MAX_BLOCKS blocks, a NULL pointer.
 *
 * sgx_array_design_blocks: exact host code, needs no GPU.  W odd, 1 .. SGX_ARRAY_MAX_WINDOW, h = (W - 1) / 2.  Block j is
 * designed from the window lo = max(0, j - h) .. hi = min(n_blocks, j + h + 1): rho = the exact int64 sum of the window's
 * blocks, frames = min(hi B, F) - lo B, then steps 1 to 9 of sgx_array_design on that pair - the same code.  Per block:
 * taps int16 [n_blocks][A][K][lanes], gain, suppression_db, weights (doubles, [n_blocks][A][K][lanes]) and status; the last
 * four may be NULL.  A window whose matrix the design refuses as not positive definite (an all-zero stretch) does not fail
 * the call: the block takes taps, weights, gain and suppression of the nearest designed block before it, a leading block
 * those of the first designed block, and status[j] = 1 (else 0).  If no block can be designed: SGX_E_ARG with
 * sgx_array_design's text.  A tap beyond 32 512 or 128 sum(|re| + |im|) >= 2^31 in any block: SGX_E_ARG, the text names the
 * block.  Otherwise the refusals of sgx_array_design, and: B no positive multiple of the unit, W not odd or outside its
 * range, F < 1, n_blocks not ceil(F / B) or beyond the limit.
 *
 * sgx_if_combine_blocks: taps int16 [n_blocks][A][K][lanes].  OUTPUT frame f is made with tap set j = f / B and is otherwise
 * exactly sgx_if_combine's formula: the inputs f + c - k of a frame next to a seam come from the neighbouring block, the
 * taps are block j's.  The same kind and length of record, *clipped the exact count; a record that is still streaming in,
 * N = 0 (n_blocks = 0 then), another device and a record beyond one launch as sgx_if_combine.  The bounds on the taps are
 * checked for every block before anything is launched; the text names the block.  SGX_E_ARG also for a B off the unit and
 * an n_blocks that is not ceil(F / B) or beyond the limit.
 * sgx_array_block_stats_timing, sgx_combine_blocks_timing: HIP-event time of the last call's kernel on this context. */
#define SGX_ARRAY_BLOCK_UNIT 4096
#define SGX_ARRAY_MAX_BLOCKS (1 << 20)
#define SGX_ARRAY_MAX_WINDOW 63
int sgx_array_block_stats(sgx_ctx* c, const sgx_if* rec, int32_t lanes, int32_t A, int32_t K, int32_t flags, int64_t B,
                          int64_t* rho_blocks);
int sgx_array_block_stats_timing(sgx_ctx* c, float* kernel_ms);
int sgx_array_design_blocks(const int64_t* rho_blocks, int64_t n_blocks, int64_t F, int64_t B, int32_t W, int32_t lanes,
                            int32_t A, int32_t K, int32_t ref, double loading, double target_rms, int16_t* taps,
                            int32_t* shift, double* weights, double* gain, double* suppression_db, uint8_t* status);
int sgx_if_combine_blocks(sgx_ctx* c, const sgx_if* rec, int32_t lanes, int32_t A, const int16_t* taps, int64_t n_blocks,
                          int64_t B, int32_t K, int32_t shift, int32_t flags, sgx_if** out, int64_t* clipped);
int sgx_combine_blocks_timing(sgx_ctx* c, float* kernel_ms);

/* The bit integration at the head of postNavigate (postNavigation.py:125-138): I_P[start-20 : start+30000] of one
 * channel summed in 20-ms columns (numpy's summation order), bit = sum > 0.  bits must hold 1501 entries;
 * *n_bits = 1501 for a full slice, fewer where Python's slice is clipped; SGX_E_RANGE ("ValueError") when the
 * clipped slice is not a multiple of 20 ms.  Host code: 30 020 additions per channel. */
int sgx_nav_bits(const double* I_P_row, int32_t ms, int32_t subFrameStart, uint8_t* bits, int32_t* n_bits);

/* ephemeris.ephemeris (ephemeris.py:60-195): bits = n_bits >= 1500 values 0/1 starting at the first bit of a
 * subframe, d30star = last bit of the word before; eph[27] in the reference's field order (weekNumber, accuracy,
 * health, T_GD, IODC, t_oc, a_f2, a_f1, a_f0, IODE_sf2, C_rs, deltan, M_0, C_uc, e, C_us, sqrtA, t_oe, C_ic,
 * omega_0, C_is, i_0, C_rc, omega, omegaDot, IODE_sf3, iDot), *tow in seconds.  Like the reference, parity is not
 * checked here.  SGX_E_ARG ("TypeError") for fewer than 1500 bits, SGX_E_RANGE ("UnboundLocalError") when
 * subframe 1, 2 or 3 is not among the five.  Host code. */
#define SGX_EPH_FIELDS 27
int sgx_ephemeris(const uint8_t* bits, int32_t n_bits, uint8_t d30star, double* eph, int64_t* tow);

/* NavigationResult.calculatePseudoranges (postNavigation.py:27-72): absoluteSample is [n_rows][ms] (row i = i-th
 * record of the tracking results), msOfTheSignal[numberOfChannels] the measurement point per channel, channelList
 * the channels to use; pseudoranges[numberOfChannels] in metres, +inf for channels not listed (NaN everywhere if
 * the list is empty, as in the reference).  SGX_E_RANGE ("IndexError") for a point outside the series.  Host code. */
int sgx_pseudoranges(const double* absoluteSample, int32_t n_rows, int32_t ms, const double* msOfTheSignal,
                     const int32_t* channelList, int32_t n_list, int32_t numberOfChannels, int64_t samplesPerCode,
                     double startOffset, double c_mps, double* pseudoranges);

/* ---- next row: satellite positions and the least-squares fix (geoFunctions/__init__.py); scalar host code -------
 * eph is [32][SGX_EPH_FIELDS] in sgx_ephemeris order, row PRN-1.  Angles in degrees where the reference's are. */
int sgx_check_t(double time, double* corrTime);                                  /* geoFunctions/__init__.py:745-771 */
int sgx_e_r_corr(double traveltime, const double* X_sat, double* X_sat_rot);     /* :491-523, 3-vectors */
int sgx_togeod(double a, double finv, double X, double Y, double Z, double* dphi, double* dlambda, double* h); /* :892-996 */
int sgx_topocent(const double* X, const double* dx, double* Az, double* El, double* D);                      /* :1003-1064 */
int sgx_tropo(double sinel, double hsta, double p, double tkel, double hum, double hp, double htkel, double hhum,
              double* ddr);                                                                                 /* :1071-1186 */
/* satpos (:779-885): satPositions [3][n] (row-major, one column per entry of prnList), satClkCorr [n] seconds */
int sgx_satpos(double transmitTime, const int32_t* prnList, int32_t n, const double* eph, double* satPositions,
               double* satClkCorr);
/* leastSquarePos (:636-739): satpos [3][n], obs [n] metres; pos[4] = X Y Z dt, el / az [n], dop[5] = G P H V T.
 * *rank_deficient = 1 where the reference gives up (matrix_rank(A) != 4) and returns a zero position. */
int sgx_least_square_pos(const double* satpos, const double* obs, int32_t n, double c_mps, int32_t useTropCorr,
                         double* pos, double* el, double* az, double* dop, int32_t* rank_deficient);
int sgx_cart2geo(double X, double Y, double Z, int32_t i, double* phi, double* lambda_, double* h);   /* :7-77 */
int sgx_find_utm_zone(double latitude, double longitude, int32_t* utmZone);                          /* :529-571 */
int sgx_cart2utm(double X, double Y, double Z, int32_t zone, double* E, double* N, double* U);      /* :176-372 */

/* The measurement-epoch loop of NavigationResult.postNavigate (postNavigation.py:150-290): for epoch m = 0 .. n_meas-1
 * the channels in use are those of `ready` whose elevation at the previous solved epoch was >= elevationMask (all of
 * `ready` at first); pseudoranges at millisecond subFrameStart[ch] + navSolPeriod m (sgx_pseudoranges), satellite
 * positions at transmitTime = tow + m navSolPeriod / 1000 (sgx_satpos), and with more than three channels the
 * least-squares fix, geodetic and UTM coordinates (sgx_least_square_pos, sgx_cart2geo, sgx_find_utm_zone,
 * sgx_cart2utm); otherwise the epoch is flagged in not_enough[m] and its fix is NaN, as the reference leaves it.
 * absoluteSample is [n_rows][ms] and prn_of_row [n_rows] (results row k serves channel k, as in the reference).
 * Outputs, prefilled here as the reference prefills them: chan_PRN (zeros) and chan_el / chan_az / chan_rawP /
 * chan_correctedP (NaN) are [numberOfChannels][64]; DOP [5][64] zeros; X Y Z dt latitude longitude height E N U
 * [64] NaN each, in this order in `sol` ([10][64]); *utmZone the zone of the last solved epoch.  n_meas > 64 is the
 * reference's IndexError (SGX_E_RANGE).  Host code. */
int sgx_post_navigate(const double* absoluteSample, int32_t n_rows, int32_t ms, const int32_t* prn_of_row,
                      const double* subFrameStart, const int32_t* ready, int32_t n_ready, int32_t numberOfChannels,
                      const double* eph, int64_t tow, int64_t samplesPerCode, double startOffset, double c_mps,
                      double navSolPeriod, double elevationMask, int32_t useTropCorr, int32_t n_meas,
                      double* chan_PRN, double* chan_el, double* chan_az, double* chan_rawP, double* chan_correctedP,
                      double* DOP, double* sol, int32_t* utmZone, int32_t* not_enough);

/* ---- RCCL peak gather (multi-GPU acquisition shard) ------------------
 * (SURVEY.md section 8(b) sketched single-process sgx_group_* entry points - one host thread driving every device
 * through ncclCommInitAll.  The build runs ONE PROCESS PER GPU instead, as the bench contract launches it, so the
 * collective side of the boundary is a per-rank communicator; sharding itself is a loop over PRN / channel index
 * ranges on the caller's side: softgnss-python_amd/shard.py.)
 * One process per GPU.  Rank 0 calls sgx_comm_unique_id and ships the 128 bytes to the other
 * ranks by any host channel; every rank then calls sgx_comm_create.  sgx_comm_allgather
 * all-gathers `bytes` bytes per rank (host buffers, staged through HBM, ncclAllGather on the
 * context stream over xGMI). */
int sgx_comm_unique_id(uint8_t id[128]);
int sgx_comm_create(sgx_ctx* c, int32_t n_ranks, int32_t rank, const uint8_t id[128], sgx_comm** out);
int sgx_comm_allgather(sgx_comm* m, const void* send, void* recv, size_t bytes);

/* The sharded search as ONE call (round 6; BASELINE configs[3]: acquisition.py:92 is the loop that shards, :135-193 do not
 * shrink).  Rank `rank` of `world` searches its contiguous, balanced share of PRN indices 0 .. n_prn_total-1 (the partition
 * of softgnss-python_amd/shard.py: plan_shards); its peaks are packed into 40-byte records on the device behind the search,
 * ONE ncclAllGather on the context's stream gathers every rank's, a small kernel copies them to a pinned page and the host
 * looks once.  Outputs: the merged 32-entry arrays of acquisition.py:201-203 plus frequencyBinIndex / fftMaxIndex (-1 where
 * not detected), identical on every rank.  comm NULL: no collective - world 1, or one rank's shard run alone (what one
 * rank of an N-GPU run executes, for timing; only its own PRNs are filled in).  A rank whose search fails the way the
 * reference's acquire() raises (SGX_E_INDEX / SGX_E_RANGE) marks its record and EVERY rank returns that error. */
int sgx_acquire_sharded(sgx_ctx* c, sgx_comm* comm, int32_t rank, int32_t world, const sgx_if* r, size_t offset,
                        size_t n_samples, int32_t n_prn_total, int32_t n_blocks, int32_t noncoh,
                        double* carrFreq, double* codePhase, double* peakMetric, int32_t* freqBin, int32_t* fineIdx);
int sgx_comm_destroy(sgx_comm* m);

#ifdef __cplusplus
}
#endif
#endif /* SGX_H */
