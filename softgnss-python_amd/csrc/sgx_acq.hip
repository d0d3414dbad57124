// AcquisitionResult.acquire on gfx950 (reference acquisition.py:27-204).
//
// Data flow per call (everything fp64 / complex128, int8 IF read once):
//   mix      x[n]*(sin,cos)(f_k * phasePoints[n])        -> [blocks][bins][N]      (PRN independent,
//   FFT_N                                                 -> spectra X[b][k]         computed ONCE; the
//                                                                                    reference redoes it
//                                                                                    per PRN, Q6)
//   code     table[p][n] = ca[p][ceil((ts*k)/tc)-1]      -> FFT_N -> F[p]
//   corr     conj(X[b][k]) * F[p]  -> FFT_N  (= conj(N * ifft(X conj F)))  -> |.|^2 / N^2
//   peaks    per row max / first argmax (device), block choice + exclusion list (host, tiny),
//            second peak over the exclusion list (device)
//   fine     (x - mean) * code(floor((ts*k)/tc) mod 1023), zero-padded 2^22-point FFT, argmax of |X|
// HBM-resident scratch replaces the reference's per-PRN numpy temporaries.
// A samplesPerCode with a prime factor above 31 has no transform of its own length here: its circular correlation runs
// inside a longer one (acquire_passes, "padded length").
#include <cmath>
#include <math.h>
#include <chrono>

#include "sgx_internal.h"

// ================================ limits and structs ================================
// (ACQ_MAX_BINS, ACQ_MAX_ROWS, ACQ_COH_MAX_BINS and the structs the small areas hold: sgx_internal.h)
#define ACQ_DEFAULT_CHUNK_ROWS 348   // correlation rows per chunk (the intermediate then stays in the Infinity Cache)

// the kernels, their argument structs and the coherent search's limits (this file is their only includer)
#include "sgx_acq_kernels.h"

// How the correlation batch of a call is cut (round 5).  Rows are ordered (PRN, block, bin) - reference rule - or (PRN, bin,
// block) - non-coherent sums; a batch is whole PRNs (prn_chunk of them, runs == 1) or ONE PRN's rows of a run (runs per
// PRN, per_run each) of Doppler bins - non-coherent sums: a run's output rows are whole bins - or of blocks - reference
// rule: whole blocks (the coherent search's windows).  Two rules fill it: acq_plan (the reference's grid) and coh_plan (a
// coherent grid); acq_corr_queue walks it.
// The batches alternate between `queues` HIP streams, each with its own intermediate of chunk_rows / queues rows: the columns
// kernel is bound by its stores and the rows kernel by its loads, and with two chunks in flight the one's stores overlap
// the other's loads (0.85 -> 0.77 ms for config 2, 3.21 -> 2.89 ms for config 4; both kernels move their bytes at 3-5 TB/s
// over the same fabric - the intermediate lives in the Infinity Cache - so a producer / consumer fusion has no more to win).
struct AcqCut {
    int prn_chunk = 1, runs = 1, per_run = 1, queues = 1;
};

// The grid of a coherent multi-millisecond search (sgx_acquire_coherent; coh_grid fills it)
struct CohGrid {
    int T = 1, M = 1, noncoh = 0;       // coherent_ms, n_windows, rule
    double step = 500.0, f0 = 0.0;      // f_k = f0 + step k
    int n_bins = 0, n_phi = 0, path = 0;
    std::vector<int2> bin_map;          // shift path: (phi index, circular shift) per bin
    std::vector<double> phi;
    AcqCut cut;                         // correlation batches (coh_plan)
};

// ================================ environment and plans ================================
// The environment an acquisition call reads, once at its entry: diagnosis switches, and the cross-references of
// test_acquire_variants_agree.  Each of the older paths is also the only one for some input.
struct AcqEnv {
    bool v1;              // SGX_ACQ_V1=1: the round-1 passes (else: lengths the four-step transform does not take)
    bool one_queue;       // SGX_ACQ_STREAMS=1: the correlation batches on one queue (else: where the plan says so)
    bool top2_off;        // SGX_ACQ_TOP2=0: the round-4 second-peak search (else: sampling rates above 111 MHz)
    bool front_off;       // SGX_ACQ_FRONT=0: the four-launch front (else: fp64 signals)
    bool fine_v1;         // SGX_ACQ_FINE_V1=1: the fine search on the pass-per-launch transform
    bool device_led_off;  // SGX_ACQ_DEVICE_LED=0: the host looks between the coarse and the fine search
    bool split_event;     // SGX_ACQ_SPLIT_EVENT=1: an event between them, so that the split is measured
    bool spin;            // SGX_ACQ_SPIN=0 clears it: the look goes straight to the stream synchronisation
    int chunk_rows;       // SGX_ACQ_CHUNK_ROWS: correlation rows per chunk
};
static AcqEnv acq_env() {
    auto is = [](const char* name, char v) {
        const char* e = getenv(name);
        return e && e[0] == v;
    };
    AcqEnv e;
    e.v1 = is("SGX_ACQ_V1", '1');
    e.one_queue = is("SGX_ACQ_STREAMS", '1');
    e.top2_off = is("SGX_ACQ_TOP2", '0');
    e.front_off = is("SGX_ACQ_FRONT", '0');
    e.fine_v1 = is("SGX_ACQ_FINE_V1", '1');
    e.device_led_off = is("SGX_ACQ_DEVICE_LED", '0');
    e.split_event = is("SGX_ACQ_SPLIT_EVENT", '1');
    e.spin = !is("SGX_ACQ_SPIN", '0');
    e.chunk_rows = ACQ_DEFAULT_CHUNK_ROWS;
    const char* ce = getenv("SGX_ACQ_CHUNK_ROWS");
    if (ce && atoi(ce) > 0) e.chunk_rows = atoi(ce);
    return e;
}

// The cut on the reference's grid: PRN chunks on two queues; non-coherent sums whose PRN does not fit half a chunk go in
// runs of bins (a run is a batch of its own with fewer bins).  per_run is the bins of a run, all of them where runs == 1.
static AcqCut acq_plan(int n_prn, int n_bins, int n_blocks, bool noncoh, int chunk_rows, int max_queues) {
    if (chunk_rows > ACQ_MAX_ROWS) chunk_rows = ACQ_MAX_ROWS;
    if (chunk_rows < 1) chunk_rows = 1;
    const int rows_per_prn = n_bins * n_blocks;
    AcqCut p;
    p.runs = 1;
    p.queues = (max_queues >= 2 && n_prn >= 2 && chunk_rows / 2 >= rows_per_prn) ? 2 : 1;
    if (max_queues >= 2 && p.queues == 1 && noncoh && rows_per_prn > chunk_rows / 2 && rows_per_prn <= chunk_rows && n_bins >= 2) {
        int runs = (rows_per_prn + chunk_rows / 2 - 1) / (chunk_rows / 2);
        if (runs > n_bins) runs = n_bins;
        if (runs >= 2) {
            p.runs = runs;
            p.queues = 2;
        }
    }
    if (p.queues == 2 && p.runs == 1) chunk_rows /= 2;
    p.prn_chunk = p.runs > 1 ? 1 : chunk_rows / rows_per_prn;   // (a run of bins belongs to ONE PRN)
    if (p.prn_chunk < 1) p.prn_chunk = 1;
    if (p.prn_chunk > n_prn) p.prn_chunk = n_prn;
    if (p.queues == 2 && p.runs == 1 && p.prn_chunk > (n_prn + 1) / 2) p.prn_chunk = (n_prn + 1) / 2;   // (both queues get work)
    p.per_run = (n_bins + p.runs - 1) / p.runs;
    return p;
}
extern "C" int sgx_acquire_plan(int32_t n_prn, int32_t n_bins, int32_t n_blocks, int32_t noncoh, int32_t chunk_rows,
                                int32_t max_queues, int32_t* prn_chunk, int32_t* bin_runs, int32_t* bins_per_run,
                                int32_t* queues) {
    SGX_CHECK_ARG(n_prn >= 1 && n_bins >= 1 && n_blocks >= 1 && prn_chunk && bin_runs && bins_per_run && queues);
    const AcqCut p = acq_plan(n_prn, n_bins, n_blocks, noncoh != 0, chunk_rows > 0 ? chunk_rows : ACQ_DEFAULT_CHUNK_ROWS, max_queues);
    *prn_chunk = p.prn_chunk;
    *bin_runs = p.runs;
    *bins_per_run = p.per_run;
    *queues = p.queues;
    return SGX_OK;
}

// PRNs per correlation batch of acquire_passes: whole PRNs, ACQ_MAX_ROWS rows at most - and, on a padded length len > n, no
// more rows than keep a batch's intermediate at the bytes ACQ_MAX_ROWS rows of the code's own length take (padding at
// least doubles a row; the batch shrinks instead of the context's two intermediates growing).  A batch is never less than
// one PRN: where one PRN's rows alone exceed that share (more than about 1 000 blocks x bins, a large coherent grid on
// the direct path), its intermediate is rows_per_prn padded rows, up to twice those bytes.
static int acq_passes_chunk(long long n, long long len, int rows_per_prn, int n_prn) {
    const long long max_rows = len > n ? (long long)ACQ_MAX_ROWS * n / len : ACQ_MAX_ROWS;
    int chunk = (int)(max_rows / rows_per_prn);
    if (chunk < 1) chunk = 1;
    if (chunk > n_prn) chunk = n_prn;
    return chunk;
}

extern "C" int sgx_acquire_fft_length(int64_t n_code, int64_t* length) {
    SGX_CHECK_ARG(length);
    const int64_t len = sgx_fft_corr_length(n_code);
    if (len == 0) {
        sgx_set_error("bad argument: %lld samples per code (2 .. 2^29)", (long long)n_code);
        return SGX_E_ARG;
    }
    *length = len;
    return SGX_OK;
}

extern "C" int sgx_acquire_fft_passes(int64_t n_code, int32_t* radices_out, int32_t* n_passes, int64_t* length,
                                      int32_t* last_pass_blocks, int32_t* tpb_out) {
    SGX_CHECK_ARG(radices_out && n_passes && length && last_pass_blocks && tpb_out);
    const int64_t len = sgx_fft_corr_length(n_code);
    if (len == 0) {
        sgx_set_error("bad argument: %lld samples per code (2 .. 2^29)", (long long)n_code);
        return SGX_E_ARG;
    }
    FftPlan p;   // (host fields only: no tables, nothing to destroy)
    std::vector<int> tpb;
    if (!sgx_fft_pass_list(len, &p.radices, &tpb) || p.radices.size() > SGX_FFT_MAX_PASSES) {
        sgx_set_error("no pass list for length %lld", (long long)len);
        return SGX_E_ARG;
    }
    p.n = len;
    for (size_t i = 0; i < p.radices.size(); ++i) {
        radices_out[i] = p.radices[i];
        tpb_out[i] = tpb[i];
    }
    *n_passes = (int32_t)p.radices.size();
    *length = len;
    *last_pass_blocks = sgx_fft_last_pass_blocks(&p);
    return SGX_OK;
}

// The radix passes on caller data (include/sgx.h): the tests' way to the kernels behind sgx_fft_forward_fused, through the
// plan and the pass loop the search uses.  Everything is allocated and freed here; the context lends device and stream.
namespace {
struct ProbeBufs {
    static constexpr int kMax = 12;   // (the fused form with a row map and maxima takes nine)
    void* p[kMax] = {nullptr};
    int n = 0;
    ~ProbeBufs() {
        for (int i = 0; i < n; ++i) hipFree(p[i]);
    }
    int get(void** out, size_t bytes) {
        *out = nullptr;
        if (n >= kMax) {
            sgx_set_error("sgx_fft_run_passes: more than %d buffers", kMax);
            return SGX_E_NOMEM;
        }
        hipError_t e = hipMalloc(out, bytes);
        if (e != hipSuccess) {
            sgx_set_error("hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
            return SGX_E_NOMEM;
        }
        p[n++] = *out;
        return SGX_OK;
    }
};
struct ProbePlan {
    FftPlan plan;
    ~ProbePlan() { sgx_fft_plan_destroy(&plan); }
};
}   // namespace

extern "C" int sgx_fft_run_passes(sgx_ctx* c, int64_t n, int32_t rows, const double* in, int64_t nonzero_len,
                                  const double* mul_x, int32_t n_x, const double* mul_f, int32_t n_f, int32_t rows_per_prn,
                                  int32_t prn_base, const int32_t* row_map, int64_t n_valid, double* out_rows,
                                  double* out_max, int32_t* out_arg) {
    SGX_CHECK_ARG(c && n >= 2 && n <= (1ll << 24) && rows >= 1 && rows <= 4096);
    const bool fused = mul_x != nullptr;
    if (fused) {
        SGX_CHECK_ARG(mul_f && !in && n_x >= 1 && n_x <= 4096 && n_f >= 1 && n_f <= 4096 && n_valid >= 0 && n_valid <= n);
        SGX_CHECK_ARG((out_max != nullptr) == (out_arg != nullptr) && (out_max != nullptr) != (out_rows != nullptr));
        if (row_map) {
            for (int r = 0; r < rows; ++r)
                SGX_CHECK_ARG(row_map[2 * r] >= 0 && row_map[2 * r] < n_x && row_map[2 * r + 1] >= 0 && row_map[2 * r + 1] < n_f);
        } else {
            SGX_CHECK_ARG(rows_per_prn >= 1 && rows_per_prn <= n_x && prn_base >= 0 &&
                          prn_base + (rows - 1) / rows_per_prn < n_f);
        }
    } else {
        SGX_CHECK_ARG(in && out_rows && !mul_f && !out_max && !out_arg && nonzero_len >= 1 && nonzero_len <= n);
    }
    SGX_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    ProbePlan pp;
    int rc = sgx_fft_plan_create(&pp.plan, n);   // (refuses what the search's plan refuses)
    if (rc != SGX_OK) return rc;
    const size_t row_bytes = sizeof(cplx) * (size_t)n;
    ProbeBufs bufs;
    cplx *wa = nullptr, *wb = nullptr, *res = nullptr;
    if ((rc = bufs.get((void**)&wa, (size_t)rows * row_bytes)) != SGX_OK) return rc;
    if ((rc = bufs.get((void**)&wb, (size_t)rows * row_bytes)) != SGX_OK) return rc;
    if (!fused) {
        SGX_HIP(hipMemcpyAsync(wa, in, (size_t)rows * row_bytes, hipMemcpyHostToDevice, st));
        rc = sgx_fft_forward(&pp.plan, wa, wb, rows, st, &res, nonzero_len);
        if (rc != SGX_OK) return rc;
        SGX_HIP(hipMemcpyAsync(out_rows, res, (size_t)rows * row_bytes, hipMemcpyDeviceToHost, st));
        SGX_HIP(hipStreamSynchronize(st));
        return SGX_OK;
    }
    cplx *dx = nullptr, *df = nullptr;
    if ((rc = bufs.get((void**)&dx, (size_t)n_x * row_bytes)) != SGX_OK) return rc;
    if ((rc = bufs.get((void**)&df, (size_t)n_f * row_bytes)) != SGX_OK) return rc;
    SGX_HIP(hipMemcpyAsync(dx, mul_x, (size_t)n_x * row_bytes, hipMemcpyHostToDevice, st));
    SGX_HIP(hipMemcpyAsync(df, mul_f, (size_t)n_f * row_bytes, hipMemcpyHostToDevice, st));
    FftFuse fu;
    fu.mul_x = dx;
    fu.mul_f = df;
    fu.rows_per_prn = row_map ? 1 : rows_per_prn;
    fu.prn_base = row_map ? 0 : prn_base;
    if (row_map) {
        int2* dm = nullptr;
        if ((rc = bufs.get((void**)&dm, sizeof(int2) * (size_t)rows)) != SGX_OK) return rc;
        SGX_HIP(hipMemcpyAsync(dm, row_map, sizeof(int2) * (size_t)rows, hipMemcpyHostToDevice, st));
        fu.row_map = dm;
    }
    if (out_rows) {
        rc = sgx_fft_forward_fused(&pp.plan, wa, wb, rows, st, &res, n, &fu);
        if (rc != SGX_OK) return rc;
        SGX_HIP(hipMemcpyAsync(out_rows, res, (size_t)rows * row_bytes, hipMemcpyDeviceToHost, st));
        SGX_HIP(hipStreamSynchronize(st));
        return SGX_OK;
    }
    const int nblk = sgx_fft_last_pass_blocks(&pp.plan);
    double *d_pmax = nullptr, *d_max = nullptr;
    int *d_parg = nullptr, *d_arg = nullptr;
    if ((rc = bufs.get((void**)&d_pmax, sizeof(double) * (size_t)rows * (size_t)nblk)) != SGX_OK) return rc;
    if ((rc = bufs.get((void**)&d_parg, sizeof(int) * (size_t)rows * (size_t)nblk)) != SGX_OK) return rc;
    if ((rc = bufs.get((void**)&d_max, sizeof(double) * (size_t)rows)) != SGX_OK) return rc;
    if ((rc = bufs.get((void**)&d_arg, sizeof(int) * (size_t)rows)) != SGX_OK) return rc;
    fu.pmax = d_pmax;
    fu.parg = d_parg;
    fu.inv_n = 1.0 / (double)n;
    fu.n_valid = n_valid;
    rc = sgx_fft_forward_fused(&pp.plan, wa, wb, rows, st, &res, n, &fu);
    if (rc != SGX_OK) return rc;
    acq_rowmax_finish_kernel<<<rows, 64, 0, st>>>(d_pmax, d_parg, nblk, d_max, d_arg);
    SGX_HIP(hipGetLastError());
    SGX_HIP(hipMemcpyAsync(out_max, d_max, sizeof(double) * (size_t)rows, hipMemcpyDeviceToHost, st));
    SGX_HIP(hipMemcpyAsync(out_arg, d_arg, sizeof(int) * (size_t)rows, hipMemcpyDeviceToHost, st));
    SGX_HIP(hipStreamSynchronize(st));
    return SGX_OK;
}

extern "C" int sgx_acquire_plan_limits(int32_t* default_chunk_rows, int32_t* max_rows) {
    SGX_CHECK_ARG(default_chunk_rows && max_rows);
    *default_chunk_rows = ACQ_DEFAULT_CHUNK_ROWS;
    *max_rows = ACQ_MAX_ROWS;
    return SGX_OK;
}
// How the correlation batch is cut: whole PRNs while one PRN's rows fit a chunk (ACQ_DEFAULT_CHUNK_ROWS), else one PRN
// per batch in runs - of bins for non-coherent sums (rows (bin, window): a run's output rows are whole bins), of windows
// for the reference rule (rows (window, bin): a run's output rows are whole windows).
static void coh_plan(CohGrid* g, int n_prn, long long N) {
    const int chunk = ACQ_DEFAULT_CHUNK_ROWS;
    const int rows_per_prn = g->M * g->n_bins;
    AcqCut& cut = g->cut;   // (one queue)
    const int total = g->noncoh ? g->n_bins : g->M;
    cut.runs = 1;
    cut.per_run = total;
    if (g->path == 0) {   // (acquire_passes: its own chunks of whole PRNs)
        cut.prn_chunk = acq_passes_chunk(N, sgx_fft_corr_length(N), rows_per_prn, n_prn);
    } else if (rows_per_prn <= chunk) {
        cut.prn_chunk = chunk / rows_per_prn;
    } else {
        cut.prn_chunk = 1;
        const int other = g->noncoh ? g->M : g->n_bins;
        cut.per_run = chunk / other < 1 ? 1 : chunk / other;
        cut.runs = (total + cut.per_run - 1) / cut.per_run;
    }
    if (cut.prn_chunk < 1) cut.prn_chunk = 1;
    if (cut.prn_chunk > n_prn) cut.prn_chunk = n_prn;
}

// f N / fs = shift + phi (shift integer, 0 <= phi < 1) for every bin f0 + step k of a grid: the distinct fractions to
// *phi, (phi index, circular shift) per bin to *bin_map.  Returns the number of distinct fractions; a path that shares
// forward spectra takes the grid if they are few enough for it.
static int acq_phi_split(double f0, double step, int n_bins, long long N, double fs, std::vector<double>* phi,
                         std::vector<int2>* bin_map) {
    phi->clear();
    bin_map->assign((size_t)n_bins, make_int2(0, 0));
    for (int k = 0; k < n_bins; ++k) {
        const double f = f0 + step * k;
        const double ratio = f * (double)N / fs;
        const double sh = floor(ratio + 1e-9);
        double ph = ratio - sh;
        if (ph < 1e-9) ph = 0.0;
        int j = -1;
        for (size_t q = 0; q < phi->size() && j < 0; ++q)
            if (fabs((*phi)[q] - ph) < 1e-9) j = (int)q;
        if (j < 0) {
            j = (int)phi->size();
            phi->push_back(ph);
        }
        long long shm = (long long)sh % N;
        if (shm < 0) shm += N;
        (*bin_map)[(size_t)k] = make_int2(j, (int)shm);
    }
    return (int)phi->size();
}

// Parameters -> grid, phi decomposition, path and batches.  SGX_E_ARG (with the reason) for anything out of range.
static int coh_grid(const sgx_settings& S, long long N, const sgx_acq_params* p, int n_prn, CohGrid* g) {
    if (!p) {
        sgx_set_error("bad argument: no sgx_acq_params");
        return SGX_E_ARG;
    }
    const int T = p->coherent_ms, M = p->n_windows;
    const double step = p->bin_step_hz;
    if (T < 1 || T > ACQ_COH_MAX_MS || M < 1 || M > ACQ_COH_MAX_WINDOWS || (long long)T * M > ACQ_COH_MAX_SPAN_MS) {
        sgx_set_error("bad argument: coherent_ms %d x n_windows %d (coherent_ms 1..%d, n_windows 1..%d, product <= %d ms)",
                      T, M, ACQ_COH_MAX_MS, ACQ_COH_MAX_WINDOWS, ACQ_COH_MAX_SPAN_MS);
        return SGX_E_ARG;
    }
    if ((p->noncoh != 0 && p->noncoh != 1) || p->reserved != 0) {
        sgx_set_error("bad argument: noncoh %d (0 or 1), reserved %d (0)", p->noncoh, p->reserved);
        return SGX_E_ARG;
    }
    if (!(step > 0.0) || !std::isfinite(step)) {
        sgx_set_error("bad argument: bin_step_hz %g (must be > 0)", step);
        return SGX_E_ARG;
    }
    const double nb = nearbyint(S.acqSearchBand * 1000.0 / step) + 1;
    if (!(nb >= 1.0 && nb <= (double)ACQ_COH_MAX_BINS)) {
        sgx_set_error("bad argument: a %g kHz band at %g Hz steps is %.0f Doppler bins (at most %d)", S.acqSearchBand, step,
                      nb, ACQ_COH_MAX_BINS);
        return SGX_E_ARG;
    }
    if (sgx_fft_corr_length(N) == 0) {
        sgx_set_error("bad argument: %lld samples per code", N);
        return SGX_E_ARG;
    }
    g->T = T;
    g->M = M;
    g->noncoh = p->noncoh;
    g->step = step;
    g->f0 = S.IF - S.acqSearchBand / 2 * 1000;
    g->n_bins = (int)nb;
    g->n_phi = acq_phi_split(g->f0, step, g->n_bins, N, S.samplingFreq, &g->phi, &g->bin_map);
    g->path = (sgx_fft4_supported(N) && g->n_phi <= ACQ_COH_MAX_PHI) ? 1 : 0;
    if (g->path == 0 && (long long)M * g->n_bins > ACQ_MAX_ROWS) {
        sgx_set_error("bad argument: the direct path (%d distinct Doppler fractions, %lld samples per code) takes at most "
                      "%d windows x bins, asked for %d x %d", g->n_phi, N, ACQ_MAX_ROWS, M, g->n_bins);
        return SGX_E_ARG;
    }
    coh_plan(g, n_prn, N);
    return SGX_OK;
}

// The fine search's lengths (acquisition.py:167-187): 10 ms of signal, the padded transform, its one-sided spectrum
struct FineGeom {
    long long len, npts, uniq;
};
static FineGeom acq_fine_geom(long long N) {
    FineGeom f;
    f.len = 10 * N;
    f.npts = 8ll << (long long)ceil(log2((double)f.len));
    f.uniq = (long long)ceil((double)(f.npts + 1) / 2.0);
    return f;
}

// Detection d's fine-search range for T > 1: the spectrum indices i of the 2^k-point transform (frequency i fs / npts)
// within one bin step of its coarse bin, inside the reference's [4, uniq - 5).
static std::vector<long long> coh_fine_windows(const CohGrid& g, const sgx_settings& S, long long N,
                                               const std::vector<int>& det_bin) {
    const FineGeom fg = acq_fine_geom(N);
    const long long npts = fg.npts, uniq = fg.uniq;
    std::vector<long long> win;
    for (int k : det_bin) {
        const double fk = g.f0 + g.step * k;
        long long lo = (long long)ceil(((fk - g.step) * (double)npts) / S.samplingFreq);
        long long hi = (long long)floor(((fk + g.step) * (double)npts) / S.samplingFreq) + 1;
        if (lo < 4) lo = 4;
        if (hi > uniq - 5) hi = uniq - 5;
        if (hi <= lo) hi = lo + 1;
        win.push_back(lo);
        win.push_back(hi);
    }
    return win;
}

// ================================ stages ================================
// One call as every stage and path sees it
struct AcqCall {
    sgx_ctx* c;
    SgxSig x;
    size_t n_samples;
    const int32_t* prn0;
    int n_prn;
    AcqOut out;   // [n_prn]
    AcqEnv env;
    // the context's constants: samples per code, sample and chip periods, samples per chip (acquisition.py:145)
    long long N;
    double ts, tc;
    int spc;
    // bit b: block b of the coarse search (window b of a coherent one) holds a sample that is not finite - an fp64 signal
    // only; acq_peak_bin takes that block's rows as the reference's NaN maxima
    unsigned long long bad_rows;
};
static AcqCall acq_call(sgx_ctx* c, SgxSig x, size_t n_samples, const int32_t* prn0, int32_t n_prn, const AcqOut& out,
                        const AcqEnv& env) {
    AcqCall a;
    a.c = c;
    a.x = x;
    a.n_samples = n_samples;
    a.prn0 = prn0;
    a.n_prn = n_prn;
    a.out = out;
    a.env = env;
    a.N = c->n_code;
    a.ts = 1.0 / c->s.samplingFreq;
    a.tc = 1.0 / c->s.codeFreqBasis;
    a.spc = (int)llround(c->s.samplingFreq / c->s.codeFreqBasis);
    a.bad_rows = 0ull;
    return a;
}
// The reference's Doppler grid (acquisition.py:68,99-101): bin k at IF - band / 2 + 500 k
static int acq_ref_bins(const sgx_settings& S) { return (int)(nearbyint(S.acqSearchBand * 2) + 1); }
static double acq_ref_f0(const sgx_settings& S) { return S.IF - S.acqSearchBand / 2 * 1000; }
// The detections of a call (acquisition.py:164-166) in ascending position of its PRN list
struct AcqDets {
    std::vector<int> prn, phase, slot;
};

static int acq_check_prns(const int32_t* prn0, int32_t n_prn) {
    SGX_CHECK_ARG(n_prn >= 1 && n_prn <= 32);
    for (int i = 0; i < n_prn; ++i) SGX_CHECK_ARG(prn0[i] >= 0 && prn0[i] < 32);
    return SGX_OK;
}

// The record's window as the kernels read it, once it is resident
static int acq_record_sig(sgx_ctx* c, const sgx_if* r, size_t offset, size_t n_samples, SgxSig* x) {
    const int rq = sgx_if_require(r, offset + n_samples);   // a record that is still streaming in
    if (rq != SGX_OK) return rq;
    SGX_HIP(hipSetDevice(c->device));
    x->i8 = r->d + offset;
    x->f64 = nullptr;
    return SGX_OK;
}

// acquire() on a signal that is not int8 (acquisition.py:55-59 takes whatever real dtype numpy hands it): the caller's
// fp64 samples are copied to HBM and every kernel reads them instead of the int8 record; the arithmetic is the same
// fp64 arithmetic either way.
static int acq_upload_f64(sgx_ctx* c, const double* signal, size_t n_samples, SgxSig* x) {
    SGX_HIP(hipSetDevice(c->device));
    const int rc = c->d_sig64.ensure(sizeof(double) * (n_samples + 64));
    if (rc != SGX_OK) return rc;
    SGX_HIP(hipMemcpyAsync(c->d_sig64, signal, sizeof(double) * n_samples, hipMemcpyHostToDevice, c->stream));
    SGX_HIP(hipStreamSynchronize(c->stream));   // the caller may free `signal` on return
    x->i8 = nullptr;
    x->f64 = c->d_sig64;
    return SGX_OK;
}

// Where a search's samples come from: n_samples at `offset` of a resident record, or (r null) of the caller's fp64 signal
struct AcqSource {
    const sgx_if* r;
    size_t offset;
    const double* signal;
    size_t n_samples;
};
// Bit w: window w of the search - ms_per_row code periods each, `rows` of them (at most 64) - holds a sample that is not
// finite.  A record's samples are integers; the caller's fp64 signal is looked at on the host, where it lies.  (64 bits hold
// every search: n_blocks <= 64, acq_open_source, and ACQ_COH_MAX_WINDOWS = 64.)
static unsigned long long acq_bad_rows(const AcqSource& src, long long N, int ms_per_row, int rows) {
    if (src.r) return 0ull;
    unsigned long long bad = 0ull;
    const size_t len = (size_t)N * (size_t)ms_per_row;
    for (int w = 0; w < rows && w < 64; ++w) {
        const size_t lo = (size_t)w * len, hi = lo + len < src.n_samples ? lo + len : src.n_samples;
        for (size_t i = lo; i < hi; ++i)
            if (!std::isfinite(src.signal[i])) {
                bad |= 1ull << w;
                break;
            }
    }
    return bad;
}
static int acq_source_sig(sgx_ctx* c, const AcqSource& src, SgxSig* x) {
    return src.r ? acq_record_sig(c, src.r, src.offset, src.n_samples, x) : acq_upload_f64(c, src.signal, src.n_samples, x);
}

// What the searches on the reference's grid check before they touch the device: PRN list, blocks, the source's length
static int acq_open_source(sgx_ctx* c, const AcqSource& src, const int32_t* prn0, int32_t n_prn, int32_t n_blocks, SgxSig* x) {
    SGX_CHECK_ARG(c && (src.r || src.signal) && prn0);
    SGX_CHECK_ARG(n_blocks >= 1 && n_blocks <= 64);
    const int rc = acq_check_prns(prn0, n_prn);
    if (rc != SGX_OK) return rc;
    const long long need = (long long)n_blocks * c->n_code;
    const bool outside = src.r && (src.offset > src.r->n || src.n_samples > src.r->n - src.offset);
    if (outside || (long long)src.n_samples < need) {
        if (src.r)
            sgx_set_error("record window too short: %zu samples at offset %zu, %lld needed for the coarse search",
                          src.n_samples, src.offset, need);
        else
            sgx_set_error("signal too short: %zu samples, %lld needed for the coarse search", src.n_samples, need);
        return SGX_E_RANGE;
    }
    return acq_source_sig(c, src, x);
}

static bool acq_out_non_null(const AcqOut& o) {
    return o.carrFreq && o.codePhase && o.peakMetric && o.freqBin && o.fineIdx;
}
static void acq_reset_outputs(const AcqOut& o, int n) {
    for (int i = 0; i < n; ++i) {
        o.carrFreq[i] = 0.0;
        o.codePhase[i] = 0.0;
        o.peakMetric[i] = 0.0;
        o.freqBin[i] = -1;
        o.fineIdx[i] = -1;
    }
}
static void acq_copy_results(const AcqOut& dst, const AcqOut& src, int n) {
    for (int i = 0; i < n; ++i) {
        dst.carrFreq[i] = src.carrFreq[i];
        dst.codePhase[i] = src.codePhase[i];
        dst.peakMetric[i] = src.peakMetric[i];
        dst.freqBin[i] = src.freqBin[i];
        dst.fineIdx[i] = src.fineIdx[i];
    }
}

// Device times of a call from its events ev[0] (start), ev[1] (between coarse and fine search), ev[2] (end).  An event
// between the coarse and the fine kernels holds the fine search back by 6-8 us, so the device-led sequence records it on
// request only (SGX_ACQ_SPLIT_EVENT=1); without it the split is NOT measured: NaN, not total / 0
static void acq_event_times(sgx_ctx* c, bool split_measured) {
    hipEventElapsedTime(&c->timing.acquire_ms, c->ev[0], c->ev[2]);
    if (split_measured) {
        hipEventElapsedTime(&c->timing.acq_coarse_ms, c->ev[0], c->ev[1]);
        hipEventElapsedTime(&c->timing.acq_fine_ms, c->ev[1], c->ev[2]);
    } else {
        c->timing.acq_coarse_ms = __builtin_nanf("");
        c->timing.acq_fine_ms = __builtin_nanf("");
    }
}

// The reference's IndexError (Q5; acquisition.py:152-162) and its failure to broadcast (acquisition.py:177) as errors
static int acq_index_error(long long N, int prn, int code_phase) {
    sgx_set_error("IndexError: index %lld is out of bounds for axis 1 with size %lld "
                  "(PRN index %d, codePhase %d; reference acquisition.py:152-162)", N, N, prn, code_phase);
    return SGX_E_INDEX;
}
static int acq_fine_range_error(long long end, size_t n_samples) {
    sgx_set_error("fine search needs codePhase + 10 ms = %lld samples, record window has %zu "
                  "(reference acquisition.py:177 would fail to broadcast)", end, n_samples);
    return SGX_E_RANGE;
}

// The first of PRNs [first, first + n) of the call at which the reference raises (po: entry i = PRN first + i)
static int acq_look_index_error(const AcqCall& a, const PeakOut& po, int first, int n) {
    for (int i = 0; i < n; ++i)
        if (po.index_error[i]) return acq_index_error(a.c->n_code, a.prn0[first + i], po.cph[i]);
    return SGX_OK;
}

// The look decoded: peaks and second peaks of PRNs [first, first + n) -> peakMetric, freqBin and the detections
// (acquisition.py:164-166), or the reference's IndexError
static int acq_look_decode(const AcqCall& a, const PeakOut& po, const double* second, int first, int n, AcqDets* det) {
    const int rc = acq_look_index_error(a, po, first, n);
    if (rc != SGX_OK) return rc;
    for (int i = 0; i < n; ++i) {
        const int o = first + i;
        const double ratio = po.peak[i] / second[i];
        a.out.peakMetric[o] = ratio;
        a.out.freqBin[o] = po.fbi[i];
        if (ratio > a.c->s.acqThreshold) {
            det->prn.push_back(a.prn0[o]);
            det->phase.push_back(po.cph[i]);
            det->slot.push_back(o);
        }
    }
    return SGX_OK;
}

// Waits for a result word in the pinned page (acq_publish_kernel's `seq`, the fine search's `seq2`, the gathered peaks' word)
static int acq_look_wait(sgx_ctx* c, const unsigned long long* word, unsigned long long seq, bool spin) {
    return sgx_look_wait(c->stream, word, seq, spin, 0.05, 1024, "acquisition: the search's result page was not written", nullptr);
}

// The second queue of the correlation batches and its two events, created on first use
static int acq_second_queue(sgx_ctx* c, hipStream_t* st2) {
    if (!c->acq_stream2) {
        // (into locals; the context gets them only when ALL exist - a half-made second queue would fail every later call)
        int least = 0, greatest = 0;
        SGX_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
        hipStream_t ns = nullptr;
        hipEvent_t ne[2] = {nullptr, nullptr};
        hipError_t ce = (c->priority == 0) ? hipStreamCreateWithFlags(&ns, hipStreamNonBlocking)
                                           : hipStreamCreateWithPriority(&ns, hipStreamNonBlocking, c->priority < 0 ? greatest : least);
        for (int i = 0; i < 2 && ce == hipSuccess; ++i) ce = hipEventCreateWithFlags(&ne[i], hipEventDisableTiming);
        if (ce != hipSuccess) {
            for (int i = 0; i < 2; ++i)
                if (ne[i]) hipEventDestroy(ne[i]);
            if (ns) hipStreamDestroy(ns);
            sgx_set_error("acquisition: the second queue could not be created: %s", hipGetErrorString(ce));
            return SGX_E_HIP;
        }
        c->acq_stream2 = ns;
        c->acq_ev2[0] = ne[0];
        c->acq_ev2[1] = ne[1];
    }
    *st2 = c->acq_stream2;
    return SGX_OK;
}

// The correlation of the paths that read shifted forward spectra (four-step, coherent shift): its geometry, and where in
// the reduction buffer (c->d_pow) its kernels leave their results
struct AcqCorr {
    int n_bins, n_phi, n_blocks, noncoh;   // (blocks: 1-ms blocks, or the coherent search's windows)
    int out_per_prn, rows_out_all;
    bool top2;                             // peak and second peak from one pass (acq_rowtop2_peak_kernel)
    int nblk, nres;
    const cplx* d_codefd;                  // code spectra, behind the forward spectra in c->d_fwd
    // [per-workgroup maxima | their indices] or [per-residue maxima | second maxima | indices], [row maxima | row indices],
    // then (non-coherent, round-4 sequence) the second-peak power rows
    double* pmax;
    int* parg;
    double *t2b1, *t2b2;
    int* t2i1;
    double* rowmax;
    int* rowarg;
    double* power;
};
static int acq_corr_carve(sgx_ctx* c, AcqCorr* k, size_t pow_need) {
    const size_t rows = (size_t)k->rows_out_all;
    const size_t part_bytes = ((rows * (k->top2 ? (size_t)k->nres * 20 : (size_t)k->nblk * 12)) + 255) / 256 * 256;
    const size_t red_bytes = (part_bytes + rows * 12 + 1023) / 256 * 256;
    const int rc = c->d_pow.ensure(red_bytes + pow_need);
    if (rc != SGX_OK) return rc;
    char* red = (char*)c->d_pow.get();
    k->pmax = (double*)red;
    k->parg = (int*)(red + rows * k->nblk * 8);
    k->t2b1 = (double*)red;
    k->t2b2 = k->t2b1 + rows * k->nres;
    k->t2i1 = (int*)(k->t2b2 + rows * k->nres);
    k->rowmax = (double*)(red + part_bytes);
    k->rowarg = (int*)(red + part_bytes + rows * 8);
    k->power = (double*)(red + red_bytes);
    return SGX_OK;
}
// The scratch of such a correlation - two intermediates of work_rows rows (the forward batch's rows at least) and d_fwd =
// [forward | code] spectra - and its AcqCorr.  power_rows: room behind the reductions for the round-4 sequence's second-peak
// power rows.
static int acq_corr_setup(sgx_ctx* c, AcqCorr* k, int n_prn, int n_bins, int n_phi, int n_blocks, int noncoh, bool top2,
                          size_t work_rows, bool power_rows) {
    const size_t N = (size_t)c->n_code, row_bytes = sizeof(cplx) * N;
    const size_t rows_fwd = (size_t)n_blocks * n_phi;
    if (work_rows < rows_fwd + n_prn) work_rows = rows_fwd + n_prn;
    int rc;
    if ((rc = c->d_work[0].ensure(work_rows * row_bytes)) != SGX_OK) return rc;
    if ((rc = c->d_work[1].ensure(work_rows * row_bytes)) != SGX_OK) return rc;
    if ((rc = c->d_fwd.ensure((rows_fwd + n_prn) * row_bytes)) != SGX_OK) return rc;
    k->n_bins = n_bins;
    k->n_phi = n_phi;
    k->n_blocks = n_blocks;
    k->noncoh = noncoh;
    k->out_per_prn = noncoh ? n_bins : n_blocks * n_bins;
    k->rows_out_all = n_prn * k->out_per_prn;
    k->nblk = sgx_fft4_row_blocks();
    k->nres = sgx_fft4_residues();
    k->top2 = top2;
    k->d_codefd = c->d_fwd + rows_fwd * N;
    size_t pow_need = 0;
    if (power_rows) {
        pow_need = (size_t)k->rows_out_all * k->nblk * 12 + 4096;
        if (noncoh && pow_need < (size_t)n_prn * sizeof(double) * N) pow_need = (size_t)n_prn * sizeof(double) * N;
    }
    return acq_corr_carve(c, k, pow_need);
}

// One correlation batch: PRNs [p0, p0 + np) x bins [bin0, bin0 + nb) x blocks [blk0, blk0 + nblocks) -> its Fft4Fuse (a
// run of bins is a batch of its own with fewer bins; a run of blocks reads its blocks' forward rows) and the transform,
// through intermediate `work` on queue `st`.  Rows are ordered (PRN, block, bin), or (PRN, bin, block) for non-coherent
// sums, which take all blocks of a bin in one batch.
static int acq_corr_batch(sgx_ctx* c, const AcqCorr& k, int p0, int np, int bin0, int nb, int blk0, int nblocks, cplx* work,
                          hipStream_t st) {
    Fft4Fuse fu;
    fu.mul_x = c->d_fwd + (size_t)blk0 * k.n_phi * (size_t)c->n_code;
    fu.mul_f = k.d_codefd;
    fu.bin_map = c->d_small->bin_map + bin0;
    fu.n_bins = nb;
    fu.n_phi = k.n_phi;
    fu.rows_per_prn = nb * nblocks;
    fu.prn_base = p0;
    fu.n_blocks = nblocks;
    fu.blocks_fast = k.noncoh ? 1 : 0;
    const size_t out0 = (size_t)p0 * k.out_per_prn + (k.noncoh ? (size_t)bin0 : (size_t)blk0 * k.n_bins + (size_t)bin0);
    if (k.top2) {
        fu.t2_b1 = k.t2b1 + out0 * k.nres;
        fu.t2_b2 = k.t2b2 + out0 * k.nres;
        fu.t2_i1 = k.t2i1 + out0 * k.nres;
    } else {
        fu.pmax = k.pmax + out0 * k.nblk;
        fu.parg = k.parg + out0 * k.nblk;
    }
    fu.inv_n = 1.0 / (double)c->n_code;
    fu.sum_blocks = k.noncoh ? nblocks : 1;
    return sgx_fft4_forward(&c->plan_code, nullptr, work, nullptr, (int64_t)np * fu.rows_per_prn, st, &fu);
}

// The correlation batches of a cut, queued back to back: PRN chunks x runs - of bins (non-coherent sums) or of blocks
// (reference rule) - on the call's queue, or alternating between it and a second one, each with its own intermediate.
static int acq_corr_queue(const AcqCall& a, const AcqCorr& k, const AcqCut& cut) {
    sgx_ctx* c = a.c;
    hipStream_t st = c->stream, st2 = st;
    const bool two_q = cut.queues == 2;
    int rc;
    if (two_q) {
        if ((rc = acq_second_queue(c, &st2)) != SGX_OK) return rc;
        // (the second queue's intermediate is the buffer the forward transforms read: they are queued in front)
        SGX_HIP(hipEventRecord(c->acq_ev2[0], st));
        SGX_HIP(hipStreamWaitEvent(st2, c->acq_ev2[0], 0));
    }
    const int total = k.noncoh ? k.n_bins : k.n_blocks;
    const int step = cut.runs == 1 ? total : cut.per_run;
    int batch_no = 0;
    for (int p0 = 0; p0 < a.n_prn; p0 += cut.prn_chunk)
        for (int r0 = 0; r0 < total; r0 += step, ++batch_no) {
            const int np = (p0 + cut.prn_chunk <= a.n_prn) ? cut.prn_chunk : (a.n_prn - p0);
            const int nr = r0 + step <= total ? step : total - r0;
            const int q = two_q ? (batch_no & 1) : 0;
            rc = k.noncoh ? acq_corr_batch(c, k, p0, np, r0, nr, 0, k.n_blocks, c->d_work[q], q ? st2 : st)
                          : acq_corr_batch(c, k, p0, np, 0, k.n_bins, r0, nr, c->d_work[q], q ? st2 : st);
            if (rc != SGX_OK) {
                // (the second queue may still hold batches that write d_work[1]: nothing of the next call may overtake them)
                if (two_q) hipStreamSynchronize(st2);
                return rc;
            }
        }
    if (two_q) {
        SGX_HIP(hipEventRecord(c->acq_ev2[1], st2));
        SGX_HIP(hipStreamWaitEvent(st, c->acq_ev2[1], 0));
    }
    return SGX_OK;
}

// The front of the two paths that read shifted forward spectra: call set-up (PRN list and bin map to their device tables,
// accumulators zeroed), the record sum (to *d_sum), the forward rows (blocks x phi) and the code rows (PRNs) behind them
// in d_work[1], then the spectra of all of them as ONE batch straight into d_fwd = [forward | code].  Three row sources:
// the reference's 1-ms blocks mixed by phi, in one launch with everything else (acq_front_kernel: int8 records) or in
// four launches, and g's coherent windows folded (acq_fold_phi_kernel; its grid has more bins than a set-up by value holds).
static int acq_front(const AcqCall& a, const AcqCorr& k, const std::vector<int2>& bin_map, const std::vector<double>& phi,
                     const CohGrid* g, long long** d_sum) {
    sgx_ctx* c = a.c;
    hipStream_t st = c->stream;
    SgxSmall* dsm = c->d_small;
    SgxSmall* hsm = c->h_small;
    const long long N = a.N;
    const int n_prn = a.n_prn, rows_fwd = k.n_blocks * k.n_phi;
    const unsigned gx = (unsigned)((N + 255) / 256);
    cplx* rows = c->d_work[1];
    AcqSetup su;
    PhiArgs pa;
    if (g) {
        // (host staging in the pinned small buffer: the copies are queued, the buffer is not touched again before the look)
        for (int i = 0; i < n_prn; ++i) hsm->stage_prn[i] = a.prn0[i];
        for (int b = 0; b < k.n_bins; ++b) hsm->stage_bin_map[b] = bin_map[(size_t)b];
    } else {
        memset(&su, 0, sizeof(su));
        su.n_prn = n_prn;
        su.n_bins = k.n_bins;
        for (int i = 0; i < n_prn; ++i) su.prn[i] = a.prn0[i];
        for (int b = 0; b < k.n_bins; ++b) su.bin[b] = bin_map[(size_t)b];
        static_assert(ACQ_MAX_BINS <= 256, "the set-up workgroup has 256 threads");
        pa.n_phi = k.n_phi;
        for (int j = 0; j < k.n_phi; ++j) pa.phi[j] = phi[(size_t)j];
    }
    *d_sum = &dsm->sum;
    hipEventRecord(c->ev[0], st);
    if (!g && !a.x.f64 && !a.env.front_off) {
        // the record sum goes to the slot the PREVIOUS call's set-up zeroed; this one zeroes the other
        const int ph = c->acq_sum_phase & 1;
        long long* sum_now = dsm->sum2 + ph;
        long long* sum_next = dsm->sum2 + (ph ^ 1);
        if (!c->acq_sum_clean[ph]) SGX_HIP(hipMemsetAsync(sum_now, 0, 8, st));
        acq_front_kernel<<<(unsigned)(rows_fwd + n_prn) * gx + ACQ_SUM_WGS + 1, 256, 0, st>>>(
            su, a.x, pa, c->d_codes, rows, N, rows_fwd, a.ts, a.tc, (long long)a.n_samples, dsm->prn, dsm->bin_map, sum_now,
            sum_next, dsm->second, dsm->arrived);
        c->acq_sum_clean[ph] = false;
        c->acq_sum_clean[ph ^ 1] = true;
        c->acq_sum_phase = ph ^ 1;
        *d_sum = sum_now;
    } else {
        if (g) {
            SGX_HIP(hipMemcpyAsync(dsm->prn, hsm->stage_prn, sizeof(int) * (size_t)n_prn, hipMemcpyHostToDevice, st));
            SGX_HIP(hipMemcpyAsync(dsm->bin_map, hsm->stage_bin_map, sizeof(int2) * (size_t)k.n_bins, hipMemcpyHostToDevice, st));
            SGX_HIP(hipMemsetAsync(&dsm->sum, 0, 8, st));
            SGX_HIP(hipMemsetAsync(dsm->second, 0, sizeof(double) * 32, st));
            SGX_HIP(hipMemsetAsync(dsm->arrived, 0, sizeof(int) * 64, st));
        } else {
            acq_setup_kernel<<<1, 128, 0, st>>>(su, dsm->prn, dsm->bin_map, &dsm->sum, dsm->second, dsm->arrived);
        }
        if (a.x.f64) acq_sum_f64_kernel<<<1, 1024, 0, st>>>(a.x.f64, (long long)a.n_samples, &dsm->sum);
        else acq_sum_kernel<<<64, 256, 0, st>>>(a.x.i8, (long long)a.n_samples, &dsm->sum);
        if (g) {
            FoldArgs fa;
            memset(&fa, 0, sizeof(fa));
            fa.n_phi = k.n_phi;
            fa.T = g->T;
            for (int j = 0; j < k.n_phi; ++j) fa.phi[j] = phi[(size_t)j];
            acq_fold_phi_kernel<<<dim3(gx, (unsigned)k.n_blocks), 256, 0, st>>>(a.x, rows, N, fa);
        } else {
            acq_mixphi_kernel<<<dim3(gx, (unsigned)rows_fwd), 256, 0, st>>>(a.x, rows, N, pa);
        }
        acq_code_kernel<<<dim3(gx, (unsigned)n_prn), 256, 0, st>>>(c->d_codes, dsm->prn, rows + (size_t)rows_fwd * (size_t)N, N,
                                                                   a.ts, a.tc);
    }
    return sgx_fft4_forward(&c->plan_code, rows, c->d_work[0], c->d_fwd, rows_fwd + n_prn, st, nullptr);
}

// Row maxima, then per PRN block choice, global peak, exclusion list and second peak - one launch from the one pass's
// (maximum, maximum of the others) pairs (k.top2), or the round-4 sequence, which transforms each PRN's winning row(s) again
// - and the outcome published with `seq`: to the pinned page, or (device_led) with the detection list to the device-side
// copy of the page, which the fine search hands on.  Then the event between the coarse and the fine search.
static int acq_peaks_publish(const AcqCall& a, const AcqCorr& k, unsigned long long seq, bool device_led) {
    sgx_ctx* c = a.c;
    hipStream_t st = c->stream;
    SgxSmall* dsm = c->d_small;
    const long long fine_len = acq_fine_geom(a.N).len;
    // (device-led: into a device-side copy of the page - a kernel that writes host memory ends with a flush the next one
    // waits for, 5 us in front of the fine search)
    CoarseLook* const page = device_led ? &dsm->stage : &c->d_look->coarse;
    if (k.top2) {
        PublishArgs pub;   // (with a stage the kernel publishes itself, the detections too; else a publish kernel follows)
        pub.stage = device_led ? page : nullptr;
        pub.prn_list = dsm->prn;
        pub.threshold = c->s.acqThreshold;
        pub.fine_len = fine_len;
        pub.n_samples = (long long)a.n_samples;
        pub.det = &dsm->det;
        acq_rowtop2_peak_kernel<<<k.rows_out_all, 64, 0, st>>>(k.t2b1, k.t2b2, k.t2i1, k.nres, k.rowmax, k.rowarg, dsm->arrived,
                                                               a.n_prn, k.out_per_prn, k.n_bins, k.n_blocks, k.noncoh, a.N, a.spc,
                                                               &dsm->peak_out, dsm->second, pub, a.bad_rows);
    } else {
        acq_rowmax_peak_kernel<<<k.rows_out_all, 64, 0, st>>>(k.pmax, k.parg, k.nblk, k.rowmax, k.rowarg, dsm->arrived, a.n_prn,
                                                              k.out_per_prn, k.n_bins, k.n_blocks, k.noncoh, a.N, a.spc,
                                                              &dsm->peak_out, &dsm->second_args, dsm->row_map, a.bad_rows);
        // the rows the second-peak search reads, transformed again
        Fft4Fuse fu;
        fu.mul_x = c->d_fwd;
        fu.mul_f = k.d_codefd;
        fu.bin_map = dsm->bin_map;
        fu.row_map = dsm->row_map;
        fu.n_bins = k.n_bins;
        fu.n_phi = k.n_phi;
        fu.n_blocks = k.n_blocks;
        // the rows kernel folds each row's maximum over the exclusion list into d_second itself (the same powers, formed
        // by the same arithmetic, as the first pass: peak / second peak is a ratio of consistently rounded values);
        // neither the rows nor their powers are stored
        static_assert(sizeof(SecondArgs) == 5 * 32 * sizeof(int), "row / lo0 / hi0 / lo1 / hi1, 32 each");
        fu.sec = reinterpret_cast<const int*>(&dsm->second_args);
        fu.second_out = dsm->second;
        fu.inv_n = 1.0 / (double)a.N;
        fu.sum_blocks = k.noncoh ? k.n_blocks : 1;
        const int rows2 = a.n_prn * (k.noncoh ? k.n_blocks : 1);
        const int rc = sgx_fft4_forward(&c->plan_code, nullptr, c->d_work[0], nullptr, rows2, st, &fu);
        if (rc != SGX_OK) return rc;
    }
    if (!k.top2 || !device_led)
        acq_publish_kernel<<<1, 64, 0, st>>>(&dsm->peak_out, dsm->second, a.n_prn, page, seq, dsm->prn, c->s.acqThreshold, fine_len,
                                             (long long)a.n_samples, reinterpret_cast<int*>(device_led ? &dsm->det : nullptr));
    // (an event between the coarse and the fine kernels holds the fine search back by 6-8 us: device-led, on request only)
    if (a.env.split_event || !device_led) hipEventRecord(c->ev[1], st);
    SGX_HIP(hipGetLastError());
    return SGX_OK;
}

// ---- fine frequency search (acquisition.py:167-193) ----
// Its plan and its scratch: `rows` complex rows (two real signals each), and the pass-per-launch transform's second buffer
static int acq_fine_reserve(sgx_ctx* c, const FineGeom& fg, int rows, bool second) {
    int rc = sgx_fft_plan_create(&c->plan_fine, fg.npts);
    if (rc != SGX_OK) return rc;
    const size_t bytes = (size_t)rows * sizeof(cplx) * (size_t)fg.npts;
    if ((rc = c->d_fine[0].ensure(bytes)) != SGX_OK) return rc;
    return second ? c->d_fine[1].ensure(bytes) : SGX_OK;
}
// What every fused fine search is told: signal, codes, the mean's parts, periods, scratch and where the partial maxima go
// (two kernels with LDS-resident sub-transforms, input built on the fly - the mean comes from the device-side sum: no
// host look - arg-max fused: sgx_fft.hip).  The caller adds its detections: a host list and ranges, or the device's list.
static FineSearch acq_fine_args(const AcqCall& a, const FineGeom& fg, long long* d_sum) {
    FineSearch f;
    f.x = a.x;
    f.codes = a.c->d_codes;
    f.len = fg.len;
    f.d_sum = d_sum;
    f.n_mean = (double)a.n_samples;
    f.ts = a.ts;
    f.tc1 = a.tc;
    f.work = a.c->d_fine[0];
    f.pv = a.c->d_small->fine_pv;
    f.pi = a.c->d_small->fine_pi;
    return f;
}
// Arg-max `bi` of a detection's spectrum -> the outputs of its PRN, entry o (acquisition.py:187-191, Q3)
static void acq_fine_result(const AcqOut& out, int o, long long bi, int phase, double fs, long long npts) {
    const long long m = bi - 4;   // index inside the [4:uniq-5] slice
    out.carrFreq[o] = ((double)m * fs) / (double)npts;
    out.codePhase[o] = (double)phase;
    out.fineIdx[o] = (int)m;
}

// The device-led fine search, queued right behind the coarse one: the detections were decided on the device
// (acquisition.py:164-166) and the fine kernels read their list, so the host looks ONCE, at the very end.  Its plan and
// scratch are reserved BEFORE the last coarse kernels are queued (acq_fine_reserve: nothing of the host's between them and
// the fine kernels).  Leaves what the look needs to be decoded later in c->acq_pending; not deferred: looks at once.
static int acq_fine_device_led(const AcqCall& a, long long* d_sum, unsigned long long seq, bool defer) {
    sgx_ctx* c = a.c;
    SgxSmall* dsm = c->d_small;
    CoarseLook* const d_look = &c->d_look->coarse;
    const FineGeom fg = acq_fine_geom(a.N);
    FineSearch f = acq_fine_args(a, fg, d_sum);
    f.n_det = a.n_prn;
    f.lo = 4;
    f.hi = fg.uniq - 5;
    f.d_det = &dsm->det;
    f.stage_src = reinterpret_cast<const int*>(&dsm->stage);
    f.stage_dst = reinterpret_cast<int*>(d_look);
    f.stage_words = (int)(offsetof(CoarseLook, fine_bi) / sizeof(int));
    f.out_bi = d_look->fine_bi;
    f.out_seq = &d_look->seq2;
    f.seq = seq;
    const int rc = sgx_fft_fine_search(&c->plan_fine, f, c->stream);
    if (rc != SGX_OK) return rc;
    hipEventRecord(c->ev[2], c->stream);
    SGX_HIP(hipGetLastError());
    AcqPending& P = c->acq_pending;
    P.mode = 1;
    P.seq = seq;
    P.n_prn = a.n_prn;
    for (int i = 0; i < a.n_prn; ++i) P.prn0[i] = a.prn0[i];
    P.npts = fg.npts;
    P.fine_len = fg.len;
    P.n_samples = a.n_samples;
    P.split_event = a.env.split_event;
    P.spin = a.env.spin;
    if (defer) return SGX_OK;
    return sgx_acquire_finish(c, a.out);
}

// The pass-per-launch fine search (SGX_ACQ_FINE_V1=1, or a length the fused one does not take): the host fetches the mean,
// then input rows, transform and arg-max as launches of their own.  Partial maxima where the fused search leaves them.
static int acq_fine_mean(const AcqCall& a, long long* d_sum, double* mean) {
    long long h_sum = 0;
    SGX_HIP(hipMemcpyAsync(&h_sum, d_sum, 8, hipMemcpyDeviceToHost, a.c->stream));
    SGX_HIP(hipStreamSynchronize(a.c->stream));
    double h_sumd;
    memcpy(&h_sumd, &h_sum, 8);
    *mean = (a.x.f64 ? h_sumd : (double)h_sum) / (double)a.n_samples;   // longSignal.mean(), acquisition.py:59
    return SGX_OK;
}
static int acq_fine_passes(const AcqCall& a, const AcqDets& det, const FineGeom& fg, double mean, const long long* d_win,
                           int nblk) {
    sgx_ctx* c = a.c;
    hipStream_t st = c->stream;
    SgxSmall* dsm = c->d_small;
    const int n_det = (int)det.prn.size(), n_rows = (n_det + 1) / 2;
    SGX_HIP(hipMemcpyAsync(dsm->det_prn, det.prn.data(), sizeof(int) * (size_t)n_det, hipMemcpyHostToDevice, st));
    SGX_HIP(hipMemcpyAsync(dsm->det_phase, det.phase.data(), sizeof(int) * (size_t)n_det, hipMemcpyHostToDevice, st));
    dim3 grid((unsigned)((fg.len + 255) / 256), (unsigned)n_rows);
    acq_fine_prep_kernel<<<grid, 256, 0, st>>>(a.x, c->d_codes, c->d_fine[0], fg.len, fg.npts, mean, a.ts, a.tc, dsm->det_prn,
                                               dsm->det_phase, n_det);
    cplx* res = nullptr;
    const int rc = sgx_fft_forward(&c->plan_fine, c->d_fine[0], c->d_fine[1], n_rows, st, &res, fg.len);
    if (rc != SGX_OK) return rc;
    dim3 g2((unsigned)nblk, (unsigned)n_det);
    acq_fine_argmax_kernel<<<g2, 256, 0, st>>>(res, fg.npts, 4, fg.uniq - 5, dsm->fine_pv, dsm->fine_pi, d_win);
    return SGX_OK;
}

// The host-led fine search for the detected PRNs; records event ev[2] and synchronises.
// win (coherent search, else null): [2 d], [2 d + 1] = detection d's own arg-max range in place of [4, uniq - 5)
static int acquire_fine(const AcqCall& a, const AcqDets& det, long long* d_sum, const std::vector<long long>* win) {
    sgx_ctx* c = a.c;
    hipStream_t st = c->stream;
    SgxSmall* dsm = c->d_small;
    SgxSmall* hsm = c->h_small;
    int rc = SGX_OK;
    const int n_det = (int)det.prn.size();
    if (n_det == 0) {
        hipEventRecord(c->ev[2], st);
        SGX_HIP(hipStreamSynchronize(st));
        return SGX_OK;
    }
    const FineGeom fg = acq_fine_geom(a.N);
    for (int d = 0; d < n_det; ++d)
        if ((long long)det.phase[d] + fg.len > (long long)a.n_samples)
            return acq_fine_range_error((long long)det.phase[d] + fg.len, a.n_samples);
    if ((rc = acq_fine_reserve(c, fg, (n_det + 1) / 2, true)) != SGX_OK) return rc;
    const bool fused = sgx_fft_fine_supported(fg.npts) && !a.env.fine_v1;
    double mean = 0.0;
    if (!fused && (rc = acq_fine_mean(a, d_sum, &mean)) != SGX_OK) return rc;
    // per-detection ranges (coherent search): to device memory, and their union as the common range
    long long* d_win = nullptr;
    long long win_lo = 4, win_hi = fg.uniq - 5;
    if (win) {
        d_win = dsm->fine_win;
        memcpy(hsm->fine_win, win->data(), sizeof(long long) * 2 * (size_t)n_det);
        SGX_HIP(hipMemcpyAsync(d_win, hsm->fine_win, sizeof(long long) * 2 * (size_t)n_det, hipMemcpyHostToDevice, st));
        win_lo = (*win)[0];
        win_hi = (*win)[1];
        for (int d = 1; d < n_det; ++d) {
            win_lo = (*win)[2 * (size_t)d] < win_lo ? (*win)[2 * (size_t)d] : win_lo;
            win_hi = (*win)[2 * (size_t)d + 1] > win_hi ? (*win)[2 * (size_t)d + 1] : win_hi;
        }
    }
    const int nblk = fused ? sgx_fft_fine_partials() : 256;
    if (fused) {
        FineSearch f = acq_fine_args(a, fg, d_sum);
        f.n_det = n_det;
        f.det_prn = det.prn.data();
        f.det_phase = det.phase.data();
        f.lo = win_lo;
        f.hi = win_hi;
        f.win = d_win;
        rc = sgx_fft_fine_search(&c->plan_fine, f, st);
    } else {
        rc = acq_fine_passes(a, det, fg, mean, d_win, nblk);
    }
    if (rc != SGX_OK) return rc;
    const double* h_pv = hsm->fine_pv;
    const long long* h_pi = hsm->fine_pi;
    SGX_HIP(hipMemcpyAsync(hsm->fine_pv, dsm->fine_pv, sizeof(double) * (size_t)n_det * nblk, hipMemcpyDeviceToHost, st));
    SGX_HIP(hipMemcpyAsync(hsm->fine_pi, dsm->fine_pi, sizeof(long long) * (size_t)n_det * nblk, hipMemcpyDeviceToHost, st));
    hipEventRecord(c->ev[2], st);
    SGX_HIP(hipStreamSynchronize(st));
    for (int d = 0; d < n_det; ++d) {
        // (from the first partial, as the device-led fold of fine_rows_kernel: where every magnitude is NaN - a sample that
        // is not finite behind the coarse blocks - the partials are (-1, first index searched), numpy's argmax of NaN)
        double bv = h_pv[d * nblk];
        long long bi = h_pi[d * nblk];
        for (int b = 1; b < nblk; ++b) {
            const double v = h_pv[d * nblk + b];
            const long long i = h_pi[d * nblk + b];
            if (v > bv || (v == bv && i < bi)) {
                bv = v;
                bi = i;
            }
        }
        acq_fine_result(a.out, det.slot[d], bi, det.phase[d], c->s.samplingFreq, fg.npts);
    }
    return SGX_OK;
}

// The tail of a host-led call: the detections' fine search (for a coherent grid with T > 1: inside one bin step of each
// detection's coarse bin) and the device times
static int acq_fine_and_times(const AcqCall& a, const AcqDets& det, long long* d_sum, const CohGrid* g) {
    std::vector<long long> win;
    if (g && g->T > 1) {
        std::vector<int> det_bin;
        for (int o : det.slot) det_bin.push_back(a.out.freqBin[o]);
        win = coh_fine_windows(*g, a.c->s, a.c->n_code, det_bin);
    }
    const int rc = acquire_fine(a, det, d_sum, win.empty() ? nullptr : &win);
    if (rc != SGX_OK) return rc;
    acq_event_times(a.c, true);
    return SGX_OK;
}
// ... behind the host's look at the page the publish kernel wrote with `seq`, decoded into the detections
static int acq_host_tail(const AcqCall& a, unsigned long long seq, long long* d_sum, const CohGrid* g) {
    const CoarseLook* look = &a.c->h_look->coarse;
    int rc = acq_look_wait(a.c, &look->seq, seq, a.env.spin);
    if (rc != SGX_OK) return rc;
    AcqDets det;
    rc = acq_look_decode(a, look->po, look->second, 0, a.n_prn, &det);
    if (rc != SGX_OK) return rc;
    return acq_fine_and_times(a, det, d_sum, g);
}

// ================================ the three paths ================================
// The round-1 path: one launch per radix pass, every Doppler bin mixed separately (any samplesPerCode).
// Padded length: N with a prime factor above 31 has no transform here, and the search needs none - it needs the circular
// correlation of length N.  That one is computed inside a circular correlation of length L = sgx_fft_corr_length(N) >=
// 2 N - 1: the mixed rows hold the signal at [0, N) and count as zero from there (the first pass reads no further: nothing
// is filled), the code rows hold the code and its wrap-around copy (acq_code_pad_kernel), and outputs k < N of the length-L
// correlation are the reference's ifft(fft(x) conj(fft(c)))[k], the same N products each.  Everything below then runs on
// rows of L elements scaled by 1 / L, and only looks at k < N.  L = N: the path as it always was.
// Its geometry, and where the fused last pass leaves its per-workgroup maxima:
struct AcqPasses {
    long long L;   // rows and transforms have this length
    bool padded;
    int n_bins, n_blocks, noncoh;
    int rows_per_prn, out_per_prn, prn_chunk, nblk_last;
    double inv_n;
    double* d_pmax;
    int* d_parg;
};
// ... with the plan and the scratch.  g (coherent search, direct path; else null): its grid's bins, n_blocks its windows
static int acq_passes_setup(const AcqCall& a, int n_blocks, int noncoh, const CohGrid* g, AcqPasses* k) {
    sgx_ctx* c = a.c;
    const long long N = a.N;
    // A4 frequency grid (acquisition.py:68,99-101)
    k->n_bins = g ? g->n_bins : acq_ref_bins(c->s);
    SGX_CHECK_ARG(k->n_bins >= 1 && k->n_bins <= (g ? ACQ_COH_MAX_BINS : ACQ_MAX_BINS));
    k->n_blocks = n_blocks;
    k->noncoh = noncoh;
    k->L = sgx_fft_corr_length(N);
    if (k->L == 0) {
        sgx_set_error("bad argument: %lld samples per code (2 .. 2^29)", N);
        return SGX_E_ARG;
    }
    k->padded = k->L != N;
    k->inv_n = 1.0 / (double)k->L;
    int rc = sgx_fft_plan_create(&c->plan_code, k->L);
    if (rc != SGX_OK) return rc;
    const int rows_fwd = n_blocks * k->n_bins;
    k->rows_per_prn = rows_fwd;
    k->out_per_prn = noncoh ? k->n_bins : k->rows_per_prn;
    SGX_CHECK_ARG(k->rows_per_prn <= ACQ_MAX_ROWS);
    k->prn_chunk = acq_passes_chunk(N, k->L, k->rows_per_prn, a.n_prn);
    const size_t row_bytes = sizeof(cplx) * (size_t)k->L;
    size_t work_rows = (size_t)k->prn_chunk * k->rows_per_prn;
    if (work_rows < (size_t)rows_fwd) work_rows = rows_fwd;
    if (work_rows < (size_t)a.n_prn) work_rows = a.n_prn;
    if ((rc = c->d_work[0].ensure(work_rows * row_bytes)) != SGX_OK) return rc;
    if ((rc = c->d_work[1].ensure(work_rows * row_bytes)) != SGX_OK) return rc;
    if ((rc = c->d_fwd.ensure((size_t)rows_fwd * row_bytes)) != SGX_OK) return rc;
    if ((rc = c->d_codefd.ensure((size_t)a.n_prn * row_bytes)) != SGX_OK) return rc;
    // per-workgroup maxima of the fused last pass live in the (otherwise unused) power buffer: what the plan's last pass
    // writes for the rows of one batch, whatever the length (acq_rowmax_finish_kernel strides over any number of them)
    k->nblk_last = sgx_fft_last_pass_blocks(&c->plan_code);
    const size_t part_slots = work_rows * (size_t)k->nblk_last;
    const size_t pow_need = noncoh ? work_rows * sizeof(double) * (size_t)N : part_slots * 12 + 4096;
    if ((rc = c->d_pow.ensure(pow_need)) != SGX_OK) return rc;
    k->d_pmax = c->d_pow;
    k->d_parg = (int*)(c->d_pow + part_slots);
    return SGX_OK;
}

// Its front: record sum, PRN list, then the PRN-independent part - every (block, bin) mixed, or every (window, bin) folded
// from g->T blocks (acq_fold_direct_kernel), and the forward spectra to d_fwd - and the code spectra to d_codefd
static int acq_passes_front(const AcqCall& a, const AcqPasses& k, const CohGrid* g) {
    sgx_ctx* c = a.c;
    hipStream_t st = c->stream;
    SgxSmall* dsm = c->d_small;
    SgxSmall* hsm = c->h_small;
    const long long N = a.N, L = k.L;
    const int rows_fwd = k.rows_per_prn;
    const size_t row_bytes = sizeof(cplx) * (size_t)L;
    hipEventRecord(c->ev[0], st);
    SGX_HIP(hipMemsetAsync(&dsm->sum, 0, 8, st));
    SGX_HIP(hipMemcpyAsync(dsm->prn, a.prn0, sizeof(int) * (size_t)a.n_prn, hipMemcpyHostToDevice, st));
    if (a.x.f64) acq_sum_f64_kernel<<<1, 1024, 0, st>>>(a.x.f64, (long long)a.n_samples, &dsm->sum);
    else acq_sum_kernel<<<256, 256, 0, st>>>(a.x.i8, (long long)a.n_samples, &dsm->sum);
    cplx* res = nullptr;
    dim3 grid((unsigned)((N + 255) / 256), (unsigned)rows_fwd);
    if (g) {
        for (int b = 0; b < k.n_bins; ++b) hsm->frq[b] = g->f0 + g->step * b;
        SGX_HIP(hipMemcpyAsync(dsm->frq, hsm->frq, sizeof(double) * (size_t)k.n_bins, hipMemcpyHostToDevice, st));
        acq_fold_direct_kernel<<<grid, 256, 0, st>>>(a.x, c->d_work[0], N, L, a.ts, dsm->frq, k.n_bins, g->T);
    } else {
        MixArgs ma;
        ma.n_bins = k.n_bins;
        ma.n_blocks = k.n_blocks;
        for (int b = 0; b < k.n_bins; ++b) ma.frq[b] = acq_ref_f0(c->s) + 500.0 * b;
        acq_mix_kernel<<<grid, 256, 0, st>>>(a.x, c->d_work[0], N, L, a.ts, ma);
    }
    int rc = sgx_fft_forward(&c->plan_code, c->d_work[0], c->d_work[1], rows_fwd, st, &res, N);
    if (rc != SGX_OK) return rc;
    SGX_HIP(hipMemcpyAsync(c->d_fwd, res, (size_t)rows_fwd * row_bytes, hipMemcpyDeviceToDevice, st));
    dim3 grid2((unsigned)((L + 255) / 256), (unsigned)a.n_prn);
    if (k.padded) acq_code_pad_kernel<<<grid2, 256, 0, st>>>(c->d_codes, dsm->prn, c->d_work[0], N, L, a.ts, a.tc);
    else acq_code_kernel<<<grid2, 256, 0, st>>>(c->d_codes, dsm->prn, c->d_work[0], N, a.ts, a.tc);
    rc = sgx_fft_forward(&c->plan_code, c->d_work[0], c->d_work[1], a.n_prn, st, &res, L);
    if (rc != SGX_OK) return rc;
    SGX_HIP(hipMemcpyAsync(c->d_codefd, res, (size_t)a.n_prn * row_bytes, hipMemcpyDeviceToDevice, st));
    return SGX_OK;
}

// The product a fused transform forms in its first pass: conj(forward spectrum) x code spectrum
static FftFuse acq_passes_fuse(sgx_ctx* c) {
    FftFuse fu;
    fu.mul_x = c->d_fwd;
    fu.mul_f = c->d_codefd;
    return fu;
}

// A chunk's peaks on the host, from its row maxima: block choice (A7), global peak (A8), exclusion list (A8b) - the
// device's peak logic, bin by bin.  sa->row: the chunk's row the second-peak search reads, per PRN.
static void acq_passes_peaks(const AcqCall& a, const AcqPasses& k, int np, PeakOut* po, SecondArgs* sa) {
    const SgxSmall* hsm = a.c->h_small;
    for (int pi = 0; pi < 32; ++pi) sa->row[pi] = -1, sa->lo0[pi] = sa->hi0[pi] = sa->lo1[pi] = sa->hi1[pi] = 0;
    memset(po, 0, sizeof(*po));
    for (int pi = 0; pi < np; ++pi) {
        AcqCand cand = {-1.0, -1, 0, 0};
        for (int b = 0; b < k.n_bins; ++b)
            cand = acq_peak_join(cand, acq_peak_bin(hsm->rowmax + pi * k.out_per_prn, hsm->rowarg + pi * k.out_per_prn, k.n_bins,
                                                    k.n_blocks, k.noncoh != 0, b, a.bad_rows));
        po->peak[pi] = cand.v;
        po->cph[pi] = cand.a;
        po->fbi[pi] = cand.k;
        po->index_error[pi] = acq_peak_ranges(cand.a, a.N, a.spc, &sa->lo0[pi], &sa->hi0[pi], &sa->lo1[pi], &sa->hi1[pi]);
        if (po->index_error[pi]) break;
        sa->row[pi] = pi * k.out_per_prn + (k.noncoh ? cand.k : cand.b * k.n_bins + cand.k);
    }
}

// The second peaks of PRNs [p0, p0 + np) to d_small->second: over the chunk's power rows (non-coherent sums), or over the
// np rows the search reads (one per PRN), transformed again
static int acq_passes_second(const AcqCall& a, const AcqPasses& k, int p0, int np, SecondArgs sa) {
    sgx_ctx* c = a.c;
    hipStream_t st = c->stream;
    SgxSmall* dsm = c->d_small;
    SgxSmall* hsm = c->h_small;
    cplx* r2 = nullptr;
    if (!k.noncoh) {
        for (int pi = 0; pi < np; ++pi) {
            hsm->row_map[pi] = make_int2(sa.row[pi] % k.rows_per_prn, p0 + pi);   // row = (pi*blocks + b)*bins + k
            sa.row[pi] = pi;
        }
        SGX_HIP(hipMemcpyAsync(dsm->row_map, hsm->row_map, sizeof(int2) * (size_t)np, hipMemcpyHostToDevice, st));
        FftFuse fu = acq_passes_fuse(c);
        fu.row_map = dsm->row_map;
        const int rc = sgx_fft_forward_fused(&c->plan_code, c->d_work[0], c->d_work[1], np, st, &r2, k.L, &fu);
        if (rc != SGX_OK) return rc;
    }
    SGX_HIP(hipMemcpyAsync(&dsm->second_args, &sa, sizeof(sa), hipMemcpyHostToDevice, st));
    SGX_HIP(hipMemsetAsync(dsm->second, 0, sizeof(double) * 32, st));
    const dim3 grid((unsigned)np, SEC_SPLIT);
    if (k.noncoh) acq_second_kernel<<<grid, 256, 0, st>>>(c->d_pow, dsm->second, a.N, &dsm->second_args);
    else acq_second_cplx_kernel<<<grid, 256, 0, st>>>(r2, dsm->second, k.L, k.inv_n, &dsm->second_args);
    return SGX_OK;
}

// g (coherent search, direct path; else null): n_blocks = the windows, each folded from g->T blocks per Doppler bin of g's
// grid in place of the 1-ms mix
static int acquire_passes(const AcqCall& a, int n_blocks, int noncoh, const CohGrid* g = nullptr) {
    sgx_ctx* c = a.c;
    hipStream_t st = c->stream;
    SgxSmall* dsm = c->d_small;
    SgxSmall* hsm = c->h_small;
    AcqPasses k;
    int rc = acq_passes_setup(a, n_blocks, noncoh, g, &k);
    if (rc != SGX_OK) return rc;
    if ((rc = acq_passes_front(a, k, g)) != SGX_OK) return rc;

    // ---- correlation + peak search, PRN chunk by chunk ---------------------------------------------
    AcqDets det;
    int status = SGX_OK;
    acq_reset_outputs(a.out, a.n_prn);
    for (int p0 = 0; p0 < a.n_prn && status == SGX_OK; p0 += k.prn_chunk) {
        const int np = (p0 + k.prn_chunk <= a.n_prn) ? k.prn_chunk : (a.n_prn - p0);
        const int rows = np * k.rows_per_prn;
        const int rows_out = np * k.out_per_prn;
        cplx* res = nullptr;
        if (noncoh) {
            // extension path: the blocks' powers are summed per sample, so rows are materialised
            dim3 grid((unsigned)((k.L + 255) / 256), (unsigned)rows);
            acq_mul_kernel<<<grid, 256, 0, st>>>(c->d_fwd, c->d_codefd, c->d_work[0], k.L, k.rows_per_prn, p0);
            rc = sgx_fft_forward(&c->plan_code, c->d_work[0], c->d_work[1], rows, st, &res, k.L);
            if (rc != SGX_OK) return rc;
            acq_power_kernel<<<rows_out, 256, 0, st>>>(res, c->d_pow, dsm->rowmax, dsm->rowarg, a.N, k.L, k.inv_n, k.n_bins,
                                                       n_blocks, 1);
        } else {
            // reference path, fused: conj(X)*F formed in the first radix pass, |.|^2 and the per-workgroup
            // maxima taken in the last one; no product rows, no power rows
            FftFuse fu = acq_passes_fuse(c);
            fu.rows_per_prn = k.rows_per_prn;
            fu.prn_base = p0;
            fu.pmax = k.d_pmax;
            fu.parg = k.d_parg;
            fu.inv_n = k.inv_n;
            fu.n_valid = k.padded ? a.N : 0;
            rc = sgx_fft_forward_fused(&c->plan_code, c->d_work[0], c->d_work[1], rows, st, &res, k.L, &fu);
            if (rc != SGX_OK) return rc;
            acq_rowmax_finish_kernel<<<rows, 64, 0, st>>>(k.d_pmax, k.d_parg, k.nblk_last, dsm->rowmax, dsm->rowarg);
        }
        SGX_HIP(hipMemcpyAsync(hsm->rowmax, dsm->rowmax, sizeof(double) * (size_t)rows_out, hipMemcpyDeviceToHost, st));
        SGX_HIP(hipMemcpyAsync(hsm->rowarg, dsm->rowarg, sizeof(int) * (size_t)rows_out, hipMemcpyDeviceToHost, st));
        SGX_HIP(hipStreamSynchronize(st));
        SecondArgs sa;
        PeakOut po;
        acq_passes_peaks(a, k, np, &po, &sa);
        status = acq_look_index_error(a, po, p0, np);
        if (status != SGX_OK) break;
        if ((rc = acq_passes_second(a, k, p0, np, sa)) != SGX_OK) return rc;
        SGX_HIP(hipMemcpyAsync(hsm->second, dsm->second, sizeof(double) * (size_t)np, hipMemcpyDeviceToHost, st));
        SGX_HIP(hipStreamSynchronize(st));
        status = acq_look_decode(a, po, hsm->second, p0, np, &det);
    }
    hipEventRecord(c->ev[1], st);
    if (status != SGX_OK) {
        hipStreamSynchronize(st);
        return status;
    }
    return acq_fine_and_times(a, det, &dsm->sum, g);
}

// The acquisition on the four-step transform (sgx_fft.hip): every 38192-point transform is two kernels with register-resident
// sub-transforms, the mixed-signal spectra are computed once per (block, phi) and read with a circular shift, results
// land where they are needed (no device-to-device copies) and the host looks at the device ONCE, at the very end of the
// call (round 4: peaks, second peaks, the detections and their fine-search results arrive in one pinned page), whatever the
// number of PRN chunks.
static int acquire_four_step(const AcqCall& a, int n_blocks, int noncoh, bool* handled, bool defer = false) {
    *handled = false;
    sgx_ctx* c = a.c;
    const sgx_settings& S = c->s;
    if (a.env.v1 || !sgx_fft4_supported(a.N)) return SGX_OK;
    const int n_bins = acq_ref_bins(S);
    if (n_bins < 1 || n_bins > ACQ_MAX_BINS) return SGX_OK;
    // f N / fs = shift + phi for every bin of the A4 grid (acquisition.py:68,99-101); the path needs few distinct phi
    // (more than PhiArgs holds: the direct path mixes every bin)
    std::vector<double> phi;
    std::vector<int2> bin_map;
    const int n_phi = acq_phi_split(acq_ref_f0(S), 500.0, n_bins, a.N, S.samplingFreq, &phi, &bin_map);
    if (n_phi > 4 || (n_phi >= n_bins && n_bins > 1)) return SGX_OK;
    *handled = true;
    int rc = sgx_fft_plan_create(&c->plan_code, a.N);
    if (rc != SGX_OK) return rc;
    const int rows_per_prn = n_blocks * n_bins;
    SGX_CHECK_ARG(rows_per_prn <= ACQ_MAX_ROWS);
    // PRN chunks of ~350 rows: a chunk's intermediate (213 MB) then stays in the 256 MiB Infinity Cache between the
    // columns kernel that writes it and the rows kernel that reads it, and the next chunk overwrites it there.  With the
    // round-3 kernels - bound by their stores and by the dirty lines on their way out, not by instruction issue or LDS
    // any more - that is 0.94 -> 0.80 ms for config 2 and 3.43 -> 3.24 ms for config 4 (tools/acq_chunk_probe.py; the
    // round-2 kernels measured no difference).
    const AcqCut cut = acq_plan(a.n_prn, n_bins, n_blocks, noncoh != 0, a.env.chunk_rows, a.env.one_queue ? 1 : 2);
    size_t work_rows = (size_t)cut.prn_chunk * rows_per_prn;
    if (work_rows < (size_t)a.n_prn * (noncoh ? n_blocks : 1)) work_rows = (size_t)a.n_prn * (noncoh ? n_blocks : 1);
    // Round 5: peak and second peak from ONE pass (acq_rowtop2_peak_kernel) when the exclusion list leaves out fewer than
    // `nres` consecutive indices (2 spc of them at most: any sampling rate below 111 MHz); SGX_ACQ_TOP2=0: the round-4
    // sequence, which transforms each PRN's winning row a second time
    const bool top2 = 2 * a.spc + 1 <= sgx_fft4_residues() && !a.env.top2_off;
    AcqCorr k;
    if ((rc = acq_corr_setup(c, &k, a.n_prn, n_bins, n_phi, n_blocks, noncoh, top2, work_rows, true)) != SGX_OK) return rc;
    long long* d_sum = nullptr;
    if ((rc = acq_front(a, k, bin_map, phi, nullptr, &d_sum)) != SGX_OK) return rc;
    acq_reset_outputs(a.out, a.n_prn);
    // all batches queued back to back; row maxima of every PRN collected on the device
    if ((rc = acq_corr_queue(a, k, cut)) != SGX_OK) return rc;
    const unsigned long long seq = ++c->look_seq;
    const FineGeom fg = acq_fine_geom(a.N);
    const bool device_led = sgx_fft_fine_supported(fg.npts) && !a.env.fine_v1 && !a.env.device_led_off && a.n_prn <= 32;
    // (two real signals per complex row; only the detections' rows are touched)
    if (device_led && (rc = acq_fine_reserve(c, fg, (a.n_prn + 1) / 2, false)) != SGX_OK) return rc;
    if ((rc = acq_peaks_publish(a, k, seq, device_led)) != SGX_OK) return rc;
    if (device_led) return acq_fine_device_led(a, d_sum, seq, defer);
    return acq_host_tail(a, seq, d_sum, nullptr);
}

// The host's ONE look at a device-led acquisition (queued by acquire_four_step; c->acq_pending says what was asked): waits
// for the result page's second word, then decodes peaks, detections and fine frequencies exactly as the eager call did.
int sgx_acquire_finish(sgx_ctx* c, const AcqOut& out) {
    AcqPending& P = c->acq_pending;
    if (P.mode == 2) {   // (the search could not be deferred and ran eagerly: its outputs were kept)
        P.mode = 0;
        acq_copy_results(out, P.res.out(), P.n_prn);
        return P.rc;
    }
    if (P.mode != 1) {
        sgx_set_error("sgx_acquire_end: no acquisition is pending on this context");
        return SGX_E_ARG;
    }
    P.mode = 0;
    AcqEnv env{};   // (only what the queued call left for its look: the environment is not read again)
    env.split_event = P.split_event;
    env.spin = P.spin;
    const AcqCall a = acq_call(c, SgxSig{nullptr, nullptr}, P.n_samples, P.prn0, P.n_prn, out, env);
    acq_reset_outputs(a.out, a.n_prn);
    const CoarseLook* look = &c->h_look->coarse;
    int rc = acq_look_wait(c, &look->seq2, P.seq, P.spin);
    if (rc != SGX_OK) return rc;
    AcqDets det;
    rc = acq_look_decode(a, look->po, look->second, 0, a.n_prn, &det);
    if (rc != SGX_OK) return rc;
    if (look->range_error) return acq_fine_range_error((long long)look->po.cph[look->range_error - 1] + P.fine_len, P.n_samples);
    if (look->n_det != (int)det.slot.size()) {   // (the same comparison on the same doubles: cannot differ)
        sgx_set_error("acquisition: device found %d detections, host %d", look->n_det, (int)det.slot.size());
        return SGX_E_HIP;
    }
    for (int d = 0; d < look->n_det; ++d)
        acq_fine_result(out, look->det_slot[d], look->fine_bi[d], look->det_phase[d], c->s.samplingFreq, P.npts);
    // (the result word is stored a moment before the last kernel retires: the device times below need its event)
    SGX_HIP(hipEventSynchronize(c->ev[2]));
    acq_event_times(c, P.split_event);
    return SGX_OK;
}

// The shift path of the coherent search: folded rows per (window, phi), their forward spectra once, the correlation
// batches of acquire_four_step (Fft4Fuse reads each bin's row with its circular shift), the same peak kernels, then one
// host look and the fine search.  All on one queue.
static int acquire_coherent_shift(const AcqCall& a, const CohGrid& g) {
    sgx_ctx* c = a.c;
    int rc = sgx_fft_plan_create(&c->plan_code, a.N);
    if (rc != SGX_OK) return rc;
    const int rows_per_prn = g.M * g.n_bins;
    const int run_rows = g.cut.runs == 1 ? g.cut.prn_chunk * rows_per_prn : g.cut.per_run * (g.noncoh ? g.M : g.n_bins);
    // peak and second peak from one pass (acq_rowtop2_peak_kernel): the four-step length has 217 residues, so any exclusion
    // list (2 spc + 1 = 75 indices at that length's rate) fits
    if (2 * a.spc + 1 > sgx_fft4_residues()) {
        sgx_set_error("coherent acquisition: %d samples per chip exceed the one-pass second-peak search", a.spc);
        return SGX_E_ARG;
    }
    AcqCorr k;
    if ((rc = acq_corr_setup(c, &k, a.n_prn, g.n_bins, g.n_phi, g.M, g.noncoh, true, (size_t)run_rows, false)) != SGX_OK) return rc;
    long long* d_sum = nullptr;
    if ((rc = acq_front(a, k, g.bin_map, g.phi, &g, &d_sum)) != SGX_OK) return rc;
    acq_reset_outputs(a.out, a.n_prn);
    if ((rc = acq_corr_queue(a, k, g.cut)) != SGX_OK) return rc;
    const unsigned long long seq = ++c->look_seq;
    if ((rc = acq_peaks_publish(a, k, seq, false)) != SGX_OK) return rc;
    return acq_host_tail(a, seq, d_sum, &g);
}


// ================================ entry points ================================
static int acquire_any(const AcqCall& a, int n_blocks, int noncoh) {
    // the four-step path (sub-transforms in registers and LDS, shifted forward spectra) where it applies
    bool handled = false;
    const int rc4 = acquire_four_step(a, n_blocks, noncoh, &handled);
    if (handled) return rc4;
    return acquire_passes(a, n_blocks, noncoh);
}

// ONE search may be pending per context, and c->acq_pending belongs to the search that ran last: every search's kernels
// write the result page and d_small->stage, so every entry point drops what an earlier sgx_acquire_begin left before it
// touches the device.  sgx_track_chained then answers SGX_E_DEFER and sgx_acquire_end SGX_E_ARG, as for "nothing pending".
static void acq_drop_pending(sgx_ctx* c) { c->acq_pending.mode = 0; }

static int acquire_source(sgx_ctx* c, const AcqSource& src, const int32_t* prn0, int32_t n_prn, int32_t n_blocks, int32_t noncoh,
                          const AcqOut& out, const AcqEnv& env) {
    SGX_CHECK_ARG(c);
    acq_drop_pending(c);
    SGX_CHECK_ARG(acq_out_non_null(out));
    SgxSig x;
    const int rc = acq_open_source(c, src, prn0, n_prn, n_blocks, &x);
    if (rc != SGX_OK) return rc;
    AcqCall a = acq_call(c, x, src.n_samples, prn0, n_prn, out, env);
    a.bad_rows = acq_bad_rows(src, a.N, 1, n_blocks);
    return acquire_any(a, n_blocks, noncoh);
}
extern "C" int sgx_acquire(sgx_ctx* c, const sgx_if* r, size_t offset, size_t n_samples, const int32_t* prn0,
                           int32_t n_prn, int32_t n_blocks, int32_t noncoh, double* carrFreq, double* codePhase,
                           double* peakMetric, int32_t* freqBin, int32_t* fineIdx) {
    const AcqOut out{carrFreq, codePhase, peakMetric, freqBin, fineIdx};
    return acquire_source(c, AcqSource{r, offset, nullptr, n_samples}, prn0, n_prn, n_blocks, noncoh, out, acq_env());
}
extern "C" int sgx_acquire_f64(sgx_ctx* c, const double* signal, size_t n_samples, const int32_t* prn0, int32_t n_prn,
                               int32_t n_blocks, int32_t noncoh, double* carrFreq, double* codePhase, double* peakMetric,
                               int32_t* freqBin, int32_t* fineIdx) {
    const AcqOut out{carrFreq, codePhase, peakMetric, freqBin, fineIdx};
    return acquire_source(c, AcqSource{nullptr, 0, signal, n_samples}, prn0, n_prn, n_blocks, noncoh, out, acq_env());
}

int sgx_prerun_enqueue(sgx_ctx* c, TrkChan* d_ch, int n_ch, long long skip_bytes, long long rec_file_offset, int sample_bytes) {
    const AcqPending& P = c->acq_pending;
    if (P.mode != 1 || n_ch < 1 || n_ch > 32) return SGX_E_DEFER;
    acq_prerun_kernel<<<1, 64, 0, c->stream>>>(&c->d_small->stage, c->d_look->coarse.fine_bi, c->d_small->prn, P.n_prn,
                                               c->s.samplingFreq, (double)P.npts, d_ch, n_ch, skip_bytes, rec_file_offset,
                                               sample_bytes, &c->d_look->step);
    SGX_HIP(hipGetLastError());
    return SGX_OK;
}

// ---- deferred acquisition (round 6) ----
// The reference's caller (initialize.py:484-506) runs acquire -> preRun -> track and looks at each result in between.  A
// caller that only wants the tracking results can queue all three: sgx_acquire_begin queues the search and returns,
// sgx_track_chained (sgx_trk.hip) queues preRun - acq_prerun_kernel - and the tracking kernel behind it and waits ONCE;
// sgx_acquire_end then decodes the search's page (no waiting left).  Outputs are those of the eager calls, bit for bit:
// the same kernels in the same order, and acq_prerun_kernel repeats the host's arithmetic.
static int acquire_begin(sgx_ctx* c, const sgx_if* r, size_t offset, size_t n_samples, const int32_t* prn0, int32_t n_prn,
                         int32_t n_blocks, int32_t noncoh, const AcqEnv& env) {
    SGX_CHECK_ARG(c);
    acq_drop_pending(c);
    SgxSig x;
    int rc = acq_open_source(c, AcqSource{r, offset, nullptr, n_samples}, prn0, n_prn, n_blocks, &x);
    if (rc != SGX_OK) return rc;
    AcqPending& P = c->acq_pending;
    const AcqCall a = acq_call(c, x, n_samples, prn0, n_prn, P.res.out(), env);
    bool handled = false;
    rc = acquire_four_step(a, n_blocks, noncoh, &handled, true);
    if (handled && P.mode == 1) return rc;          // queued; nothing has been looked at
    if (!handled) rc = acquire_passes(a, n_blocks, noncoh);
    // (a path without the device-led sequence: it ran eagerly; sgx_acquire_end hands its outputs over)
    P.mode = 2;
    P.n_prn = n_prn;
    P.rc = rc;
    return SGX_OK;
}
extern "C" int sgx_acquire_begin(sgx_ctx* c, const sgx_if* r, size_t offset, size_t n_samples, const int32_t* prn0,
                                 int32_t n_prn, int32_t n_blocks, int32_t noncoh) {
    return acquire_begin(c, r, offset, n_samples, prn0, n_prn, n_blocks, noncoh, acq_env());
}

extern "C" int sgx_acquire_end(sgx_ctx* c, double* carrFreq, double* codePhase, double* peakMetric, int32_t* freqBin,
                               int32_t* fineIdx) {
    const AcqOut out{carrFreq, codePhase, peakMetric, freqBin, fineIdx};
    SGX_CHECK_ARG(c && acq_out_non_null(out));
    SGX_HIP(hipSetDevice(c->device));
    return sgx_acquire_finish(c, out);
}

// ================================ round 6: the sharded search as ONE call ================================
// BASELINE configs[3]: the PRN loop (acquisition.py:92) shards over the ranks, the peaks are gathered.  Rounds 1-5 did the
// pack, the gather and the merge in Python around sgx_acquire (softgnss-python_amd/shard.py): 0.17-0.28 ms of host time per
// call next to a 0.45 ms shard.  Here the rank's search is queued, its peaks are packed into 40-byte records ON THE DEVICE
// behind it, one ncclAllGather follows on the same stream, a small kernel copies the gathered records to the result page and
// the host looks ONCE; the merge into the 32-entry arrays is a loop over at most 32 records.
extern "C" int sgx_acquire_sharded(sgx_ctx* c, sgx_comm* comm, int32_t rank, int32_t world, const sgx_if* r, size_t offset,
                                   size_t n_samples, int32_t n_prn_total, int32_t n_blocks, int32_t noncoh, double* carrFreq,
                                   double* codePhase, double* peakMetric, int32_t* freqBin, int32_t* fineIdx) {
    const AcqOut out{carrFreq, codePhase, peakMetric, freqBin, fineIdx};
    SGX_CHECK_ARG(c);
    // (the rank's search is queued by acquire_begin and looked at in here: nothing is pending after ANY return)
    struct DropPending {
        sgx_ctx* c;
        ~DropPending() { acq_drop_pending(c); }
    } drop{c};
    SGX_CHECK_ARG(r && acq_out_non_null(out));
    SGX_CHECK_ARG(world >= 1 && rank >= 0 && rank < world && n_prn_total >= 1 && n_prn_total <= 32);
    SGX_CHECK_ARG(!comm || (comm->n_ranks == world && comm->rank == rank && comm->ctx == c));
    const AcqEnv env = acq_env();
    acq_reset_outputs(out, 32);
    // contiguous balanced partition (shard.plan_shards)
    const int base = n_prn_total / world, extra = n_prn_total % world;
    const int first = rank * base + (rank < extra ? rank : extra);
    const int n_mine = base + (rank < extra ? 1 : 0);
    const int slots = (n_prn_total + world - 1) / world;
    int32_t prn0[32];
    for (int i = 0; i < n_mine; ++i) prn0[i] = first + i;
    SGX_HIP(hipSetDevice(c->device));
    const size_t rec_bytes = sizeof(PeakRec) * (size_t)slots;
    // where the packed records go: the communicator's send buffer, or (no communicator: one rank, or a shard run alone)
    // the context's small device area
    SgxSmall* dsm = c->d_small;
    PeakRec* d_send = comm ? (PeakRec*)comm->d_send.get() : dsm->shard;
    const PeakRec* d_all = comm ? (const PeakRec*)comm->d_recv.get() : d_send;
    const int n_ranks_seen = comm ? world : 1;
    std::vector<PeakRec> host_pack;      // a search that could not be queued: packed on the host
    bool queued = false;
    if (n_mine > 0) {
        const int rb = acquire_begin(c, r, offset, n_samples, prn0, n_mine, n_blocks, noncoh, env);
        if (rb != SGX_OK) return rb;
        queued = c->acq_pending.mode == 1;
        if (!queued) {
            AcqResults mine;
            const int re = sgx_acquire_finish(c, mine.out());
            if (re != SGX_OK && re != SGX_E_INDEX && re != SGX_E_RANGE) return re;
            host_pack.resize((size_t)slots);
            memset(host_pack.data(), 0, rec_bytes);
            for (int i = 0; i < n_mine; ++i) host_pack[(size_t)i] = peak_rec_pack(prn0[i], mine.out(), i);
            if (re != SGX_OK) host_pack[0].valid = re == SGX_E_INDEX ? -1 : -2;   // (every rank learns of it)
        }
    }
    hipStream_t st = c->stream;
    if (queued) {
        const AcqPending& P = c->acq_pending;
        acq_pack_kernel<<<1, 64, 0, st>>>(&dsm->stage, c->d_look->coarse.fine_bi, dsm->prn, P.n_prn, c->s.samplingFreq, (double)P.npts, d_send, slots);
    } else {
        if (host_pack.empty()) {
            host_pack.resize((size_t)slots);
            memset(host_pack.data(), 0, rec_bytes);
        }
        SGX_HIP(hipMemcpyAsync(d_send, host_pack.data(), rec_bytes, hipMemcpyHostToDevice, st));
    }
    if (comm) {
        const int rg = sgx_comm_allgather_device(comm, rec_bytes);
        if (rg != SGX_OK) return rg;
    }
    const int n_rec = slots * n_ranks_seen;
    if ((size_t)n_rec > sizeof(GatherLook::rec) / sizeof(PeakRec)) {
        sgx_set_error("sgx_acquire_sharded: %d ranks x %d slots do not fit the result page", world, slots);
        return SGX_E_ARG;
    }
    const unsigned long long seq = ++c->look_seq;
    GatherLook* const d_gather = &c->d_look->gather;
    const GatherLook* gather = &c->h_look->gather;
    acq_gather_publish_kernel<<<1, 256, 0, st>>>((const int*)d_all, (int)(sizeof(PeakRec) * (size_t)n_rec / 4), (int*)d_gather->rec,
                                                 &d_gather->seq, seq);
    SGX_HIP(hipGetLastError());
    const int rl = acq_look_wait(c, &gather->seq, seq, env.spin);   // the one look
    if (rl != SGX_OK) return rl;
    if (queued) {   // (device time of this rank's search; the search's own page is complete: the gather came behind it)
        SGX_HIP(hipEventSynchronize(c->ev[2]));
        acq_event_times(c, false);
    }
    for (int i = 0; i < n_rec; ++i) {
        const PeakRec& q = gather->rec[i];
        if (q.valid == 0) continue;
        if (q.valid == -1) return acq_index_error(c->n_code, q.prn0, (int)q.codePhase);
        if (q.valid == -2) return acq_fine_range_error((long long)q.codePhase + acq_fine_geom(c->n_code).len, n_samples);
        if (q.prn0 < 0 || q.prn0 >= 32) continue;
        peak_rec_merge(q, out);
    }
    return SGX_OK;
}

// ---- coherent multi-millisecond acquisition ----
// (include/sgx.h, sgx_acquire_coherent; tests/coherent_acq_spec.py is the contract in numpy.)  The search of the reference
// (acquisition.py:62-166) with T-ms windows in place of its 1-ms blocks, on a finer Doppler grid.
static int acquire_coherent_any(const AcqCall& a, const CohGrid& g) {
    if (g.path == 1) return acquire_coherent_shift(a, g);
    return acquire_passes(a, g.M, g.noncoh, &g);
}

// Everything an entry point checks before it touches the device: arguments, grid, record length.
static int coherent_checks(sgx_ctx* c, size_t n_samples, const int32_t* prn0, int32_t n_prn, const sgx_acq_params* p,
                           CohGrid* g, bool* legacy) {
    int rc = acq_check_prns(prn0, n_prn);
    if (rc != SGX_OK) return rc;
    rc = coh_grid(c->s, c->n_code, p, n_prn, g);
    if (rc != SGX_OK) return rc;
    const long long need = (long long)g->T * g->M * c->n_code;
    if ((long long)n_samples < need) {
        sgx_set_error("record window too short: %zu samples, coherent_ms %d x n_windows %d need %lld (%lld short)",
                      n_samples, g->T, g->M, need, need - (long long)n_samples);
        return SGX_E_RANGE;
    }
    *legacy = g->T == 1 && g->step == 500.0;   // the reference's grid: sgx_acquire itself
    return SGX_OK;
}

static int acquire_coherent_source(sgx_ctx* c, const AcqSource& src, const int32_t* prn0, int32_t n_prn, const sgx_acq_params* p,
                                   const AcqOut& out) {
    SGX_CHECK_ARG(c);
    acq_drop_pending(c);
    SGX_CHECK_ARG((src.r || src.signal) && prn0 && p && acq_out_non_null(out));
    if (src.r) SGX_CHECK_ARG(src.offset <= src.r->n && src.n_samples <= src.r->n - src.offset);
    const AcqEnv env = acq_env();
    CohGrid g;
    bool legacy = false;
    int rc = coherent_checks(c, src.n_samples, prn0, n_prn, p, &g, &legacy);
    if (rc != SGX_OK) return rc;
    if (legacy) return acquire_source(c, src, prn0, n_prn, g.M, g.noncoh, out, env);
    SgxSig x;
    if ((rc = acq_source_sig(c, src, &x)) != SGX_OK) return rc;
    AcqCall a = acq_call(c, x, src.n_samples, prn0, n_prn, out, env);
    a.bad_rows = acq_bad_rows(src, a.N, g.T, g.M);
    return acquire_coherent_any(a, g);
}
extern "C" int sgx_acquire_coherent(sgx_ctx* c, const sgx_if* r, size_t offset, size_t n_samples, const int32_t* prn0,
                                    int32_t n_prn, const sgx_acq_params* p, double* carrFreq, double* codePhase,
                                    double* peakMetric, int32_t* freqBin, int32_t* fineIdx) {
    const AcqOut out{carrFreq, codePhase, peakMetric, freqBin, fineIdx};
    return acquire_coherent_source(c, AcqSource{r, offset, nullptr, n_samples}, prn0, n_prn, p, out);
}
extern "C" int sgx_acquire_coherent_f64(sgx_ctx* c, const double* signal, size_t n_samples, const int32_t* prn0,
                                        int32_t n_prn, const sgx_acq_params* p, double* carrFreq, double* codePhase,
                                        double* peakMetric, int32_t* freqBin, int32_t* fineIdx) {
    const AcqOut out{carrFreq, codePhase, peakMetric, freqBin, fineIdx};
    return acquire_coherent_source(c, AcqSource{nullptr, 0, signal, n_samples}, prn0, n_prn, p, out);
}

extern "C" int sgx_acquire_coherent_plan(const sgx_settings* s, const sgx_acq_params* p, int32_t* n_bins, int32_t* n_phi,
                                         int32_t* path, int32_t* prn_chunk, int32_t* bin_runs) {
    SGX_CHECK_ARG(s && p && n_bins && n_phi && path && prn_chunk && bin_runs);
    SGX_CHECK_ARG(s->codeLength > 0 && s->codeFreqBasis > 0 && s->samplingFreq > 0);
    CohGrid g;
    const int rc = coh_grid(*s, sgx_host_samples_per_code(s), p, 32, &g);
    if (rc != SGX_OK) return rc;
    *n_bins = g.n_bins;
    *n_phi = g.n_phi;
    *path = g.path;
    *prn_chunk = g.cut.prn_chunk;
    *bin_runs = g.cut.runs;
    return SGX_OK;
}
