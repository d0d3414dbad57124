// Swept-interference excision (no reference counterpart): a real int8 record through a short-time Fourier transform -
// segments of N samples at hop N / 2 under the root-Hann window - in which every segment loses the bins that stand above
// threshold x the mean of its other bins, and back by windowed overlap-add.  tests/excise_spec.py is the contract,
// sgx_excise_core.h the arithmetic around the transform of sgx_seg_fft.h, DESIGN.md section 4.22 the account.
//
//   excise_kernel  one workgroup per tile of S = 8192 / N consecutive segments, all of them in LDS (64 KB) from the staged
//                  bytes to the output: every step of the transforms is one barrier for the whole tile.  The tile writes the
//                  (S - 1) N / 2 samples between its segments; its last segment is the next tile's first and is computed
//                  twice (1 / S more work), so no sum crosses a workgroup: no floating-point atomics, every output byte
//                  written once by one lane, the means added in a fixed order - two calls give the same bytes.
//   sgx_excise_host  the same items tile by tile in a host loop: what the kernel is held to, byte for byte.
#include <math.h>

#include "sgx_excise_core.h"
#include "sgx_stage.h"

#define EX_THREADS 256
#define EX_MAX_TILE_SEGMENTS (EX_TILE_POINTS / (EX_MIN_SEGMENT / 2))   // 128
// behind the 64 KB of the segments: the staged bytes of the tile, (S + 1) N / 2 of them and up to two granules of slack,
// later the partial sums of the means (EX_PARTS doubles fit: (S + 1) N / 2 >= 4128)
#define EX_RAW_BYTES(S, M) ((size_t)((S) + 1) * (size_t)(M) + 32)
#define EX_LDS_BYTES(S, M) (sizeof(cplx) * EX_TILE_POINTS + EX_RAW_BYTES(S, M))

// The tables of segment length n_seg on the host: tw[n_seg / 2], win[n_seg]
void ex_tables(int n_seg, cplx* tw, double* win) {
    seg_twiddles(n_seg, tw);
    for (int i = 0; i < n_seg; ++i) win[i] = sin(M_PI * (double)i / (double)n_seg);
}

// The excision's plan of segment length n_seg: tw[n_seg / 2] | win[n_seg] on the device
static int ex_prepare(SegPlan* plan, int n_seg) {
    if (plan->holds(n_seg)) return SGX_OK;
    std::vector<double> h((size_t)2 * n_seg);
    ex_tables(n_seg, reinterpret_cast<cplx*>(h.data()), h.data() + n_seg);
    return plan->upload(n_seg, h.data(), h.size());
}

// The forward steps on every segment of the tile (EX_BARRIER: the caller's)
#define EX_FORWARD(FOR_ITEMS) SEG_FORWARD(FOR_ITEMS, EX_BARRIER, buf, tw, M, g.log2m, EX_TILE_POINTS)

// counts: the stage counters (sgx_count.h), zeroed: counters 0, 1, 2 take the bins cut, the segments cut and the clipped
// outputs; cut_seg: per segment, or null
__global__ __launch_bounds__(EX_THREADS) void excise_kernel(const int8_t* __restrict__ x, int8_t* __restrict__ y,
                                                            const cplx* __restrict__ tw, const double* __restrict__ win,
                                                            ExGeom g, unsigned long long* __restrict__ counts,
                                                            uint16_t* __restrict__ cut_seg) {
    extern __shared__ __attribute__((aligned(16))) char ex_smem[];
    cplx* __restrict__ buf = reinterpret_cast<cplx*>(ex_smem);                 // [S][M]
    char* raw = ex_smem + sizeof(cplx) * EX_TILE_POINTS;
    double* __restrict__ psum = reinterpret_cast<double*>(raw);                // [S][M / EX_CHUNK], once the bytes are packed
    __shared__ int s_pcnt[EX_PARTS];
    __shared__ double s_tm[EX_MAX_TILE_SEGMENTS];
    __shared__ int s_cut[EX_MAX_TILE_SEGMENTS];
    const int tid = threadIdx.x, M = g.M, S = g.S;
    const long long t = blockIdx.x, j0 = t * (S - 1);
#define EX_BARRIER __syncthreads()
#define EX_LANES(q, count) for (int q = tid; q < (count); q += EX_THREADS)

    // the bytes of the tile, samples [p0, p0 + (S + 1) M), zero outside the record
    const int a = seg_stage(reinterpret_cast<uint4*>(raw), x, g.n, (j0 - 1) * M, (S + 1) * M, tid, EX_THREADS,
                            [](int, uint4) {});
    EX_BARRIER;
    const int8_t* __restrict__ bytes = reinterpret_cast<const int8_t*>(raw) + a;
    EX_LANES(q, EX_TILE_POINTS) {
        const int s = q >> g.log2m;
        ex_pack_item(buf + (s << g.log2m), bytes + (size_t)s * M, win, g.log2m, q & (M - 1));
    }
    EX_BARRIER;
    EX_FORWARD(EX_LANES)
    const int pairs = M / 2 + 1, parts = M / EX_CHUNK;
    EX_LANES(q, S * pairs) {
        const int s = q / pairs;
        ex_split_item(buf + (s << g.log2m), tw, M, q - s * pairs);
    }
    EX_BARRIER;
    for (int p = 0; p < g.passes; ++p) {
        EX_LANES(q, EX_PARTS) {
            const int s = q / parts;
            ex_sum_item(buf + (s << g.log2m), q - s * parts, p == 0, p == 0 ? 0.0 : s_tm[s], &psum[q], &s_pcnt[q]);
        }
        EX_BARRIER;
        EX_LANES(s, S) {
            s_tm[s] = ex_fold_item(psum + s * parts, s_pcnt + s * parts, parts, g.threshold);
            s_cut[s] = 0;
        }
        EX_BARRIER;
    }
    EX_LANES(q, S * pairs) {
        const int s = q / pairs;
        const int cut = ex_unsplit_item(buf + (s << g.log2m), tw, M, s_tm[s], q - s * pairs);
        if (cut) atomicAdd(&s_cut[s], cut);                    // integers: any order gives the same sum
    }
    EX_BARRIER;
    EX_LANES(q, EX_TILE_POINTS) ex_swap_item(buf + ((q >> g.log2m) << g.log2m), g.log2m, q & (M - 1));
    // the counters of the segments this tile owns: lanes by shuffles, one integer atomic per wave and counter on a line of
    // the slot's own (S <= 128: the first two waves)
    unsigned long long* __restrict__ slot = sgx_count_slot(counts);
    if (tid < EX_MAX_TILE_SEGMENTS) {
        unsigned bins = 0, segs = 0;
        if (tid < S && ex_owns(g, t, tid)) {
            bins = (unsigned)s_cut[tid];
            segs = bins ? 1u : 0u;
            if (cut_seg) cut_seg[j0 + tid] = (uint16_t)bins;
        }
        bins = sgx_wave_sum(bins);
        segs = sgx_wave_sum(segs);
        if ((tid & 63) == 0 && bins) {
            atomicAdd(slot, (unsigned long long)bins);
            atomicAdd(slot + 1, (unsigned long long)segs);
        }
    }
    EX_BARRIER;
    EX_FORWARD(EX_LANES)
    // the hops the tile owns, 16 samples per item: hop s lies between the segments s and s + 1 and holds the samples from
    // (j0 + s) M on
    const double inv_m = 1.0 / (double)M;
    unsigned clipped = 0;
    EX_LANES(q, (S - 1) * (M / 16)) {
        const int s = q / (M / 16), i0 = 16 * (q - s * (M / 16));
        const long long pos = (j0 + s) * M + i0;
        if (pos >= g.n) continue;
        const cplx* __restrict__ seg = buf + (s << g.log2m);
        unsigned o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            bool clip;
            const int v = ex_round_item(ex_ola_item(seg, seg + M, win, M, inv_m, i0 + e), &clip);
            clipped += (clip && pos + e < g.n) ? 1u : 0u;
            o[e >> 2] |= (unsigned)(v & 0xFF) << (8 * (e & 3));
        }
        if (pos + 16 <= g.n) {
            *reinterpret_cast<uint4*>(y + pos) = make_uint4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (pos + e < g.n) y[pos + e] = (int8_t)((o[e >> 2] >> (8 * (e & 3))) & 0xFFu);
        }
    }
    clipped = sgx_wave_sum(clipped);
    if ((tid & 63) == 0 && clipped) atomicAdd(slot + 2, (unsigned long long)clipped);
#undef EX_BARRIER
#undef EX_LANES
}

// ---- host ------------------------------------------------------------------------------------------------------------------
// The geometry of a record, or the refusal (SGX_E_ARG)
static int ex_geometry(size_t n, int32_t N, double threshold, int32_t passes, ExGeom* g) {
    if (N < EX_MIN_SEGMENT || N > EX_MAX_SEGMENT || (N & (N - 1)) != 0) {
        sgx_set_error("bad argument: the excision's segment length is a power of two in %d .. %d, not %d", EX_MIN_SEGMENT,
                      EX_MAX_SEGMENT, (int)N);
        return SGX_E_ARG;
    }
    if (!(threshold >= 1.0) || !isfinite(threshold)) {
        sgx_set_error("bad argument: the excision's threshold is finite and at least 1, not %g", threshold);
        return SGX_E_ARG;
    }
    if (passes < 1 || passes > EX_MAX_PASSES) {
        sgx_set_error("bad argument: the excision takes 1 .. %d passes, not %d", EX_MAX_PASSES, (int)passes);
        return SGX_E_ARG;
    }
    if (n == 0) {
        sgx_set_error("bad argument: the excision needs a record of at least one sample");
        return SGX_E_ARG;
    }
    g->n = (long long)n;
    g->N = N;
    g->M = N / 2;
    g->log2m = 0;
    while ((2 << g->log2m) < N) ++g->log2m;
    g->S = EX_TILE_POINTS / g->M;
    g->J = (g->n + g->M - 1) / g->M + 1;
    g->tiles = (g->J - 1 + g->S - 2) / (g->S - 1);
    g->passes = passes;
    g->threshold = threshold;
    return SGX_OK;
}

extern "C" int sgx_excise_plan(size_t n, int32_t N, int64_t* n_segments, int32_t* tile_segments) {
    SGX_CHECK_ARG(n_segments && tile_segments);
    ExGeom g;
    const int rc = ex_geometry(n, N, 1.0, 1, &g);
    if (rc != SGX_OK) return rc;
    *n_segments = (int64_t)g.J;
    *tile_segments = g.S;
    return SGX_OK;
}

extern "C" int sgx_excise_timing(sgx_ctx* c, float* kernel_ms) {
    SGX_CHECK_ARG(c && kernel_ms);
    *kernel_ms = c->stage_ms[SGX_STAGE_EXCISE];
    return SGX_OK;
}

// One tile on the host: the kernel's steps in its order, every item of a step in a loop.  spectra: where the split bins of
// the segments this tile owns go ([J][M + 1] complex), or null
static void ex_tile_host(const int8_t* x, int8_t* y, const cplx* tw, const double* win, const ExGeom& g, long long t,
                         cplx* buf, int8_t* bytes, double* psum, int* pcnt, int64_t* counts, uint16_t* cut_seg,
                         cplx* spectra) {
    const int M = g.M, S = g.S;
    const long long j0 = t * (S - 1), p0 = (j0 - 1) * M;
#define EX_BARRIER (void)0
#define EX_ALL(q, count) for (int q = 0; q < (count); ++q)
    for (long long r = 0; r < (long long)(S + 1) * M; ++r) bytes[r] = (p0 + r >= 0 && p0 + r < g.n) ? x[p0 + r] : (int8_t)0;
    EX_ALL(q, EX_TILE_POINTS) {
        const int s = q >> g.log2m;
        ex_pack_item(buf + (s << g.log2m), bytes + (size_t)s * M, win, g.log2m, q & (M - 1));
    }
    EX_FORWARD(EX_ALL)
    const int pairs = M / 2 + 1, parts = M / EX_CHUNK;
    EX_ALL(q, S * pairs) {
        const int s = q / pairs;
        ex_split_item(buf + (s << g.log2m), tw, M, q - s * pairs);
    }
    if (spectra)
        for (int s = 0; s < S; ++s) {
            if (!ex_owns(g, t, s)) continue;
            const cplx* seg = buf + (s << g.log2m);
            cplx* row = spectra + (size_t)(j0 + s) * (size_t)(M + 1);
            row[0] = make_double2(seg[0].x, 0.0);
            for (int k = 1; k < M; ++k) row[k] = seg[k];
            row[M] = make_double2(seg[0].y, 0.0);
        }
    double tm[EX_MAX_TILE_SEGMENTS];
    int cut[EX_MAX_TILE_SEGMENTS];
    for (int p = 0; p < g.passes; ++p) {
        EX_ALL(q, EX_PARTS) {
            const int s = q / parts;
            ex_sum_item(buf + (s << g.log2m), q - s * parts, p == 0, p == 0 ? 0.0 : tm[s], &psum[q], &pcnt[q]);
        }
        EX_ALL(s, S) {
            tm[s] = ex_fold_item(psum + s * parts, pcnt + s * parts, parts, g.threshold);
            cut[s] = 0;
        }
    }
    EX_ALL(q, S * pairs) {
        const int s = q / pairs;
        cut[s] += ex_unsplit_item(buf + (s << g.log2m), tw, M, tm[s], q - s * pairs);
    }
    EX_ALL(q, EX_TILE_POINTS) ex_swap_item(buf + ((q >> g.log2m) << g.log2m), g.log2m, q & (M - 1));
    EX_ALL(s, S) {
        if (!ex_owns(g, t, s)) continue;
        counts[0] += cut[s];
        counts[1] += cut[s] ? 1 : 0;
        if (cut_seg) cut_seg[j0 + s] = (uint16_t)cut[s];
    }
    EX_FORWARD(EX_ALL)
    const double inv_m = 1.0 / (double)M;
    for (int s = 0; s < S - 1; ++s) {
        const cplx* seg = buf + (s << g.log2m);
        for (int i = 0; i < M; ++i) {
            const long long pos = (j0 + s) * M + i;
            if (pos >= g.n) break;
            bool clip;
            y[pos] = (int8_t)ex_round_item(ex_ola_item(seg, seg + M, win, M, inv_m, i), &clip);
            counts[2] += clip ? 1 : 0;
        }
    }
#undef EX_BARRIER
#undef EX_ALL
}

static int ex_run_host(const int8_t* x, size_t n, int32_t N, double threshold, int32_t passes, int8_t* y,
                       sgx_excise_info* info, uint16_t* cut_per_segment, double* spectra) {
    ExGeom g;
    const int rc = ex_geometry(n, N, threshold, passes, &g);
    if (rc != SGX_OK) return rc;
    std::vector<cplx> tw((size_t)g.M), buf((size_t)EX_TILE_POINTS);
    std::vector<double> win((size_t)N), psum((size_t)EX_PARTS);
    std::vector<int> pcnt((size_t)EX_PARTS);
    std::vector<int8_t> bytes((size_t)(g.S + 1) * g.M), sink;
    if (!y) {
        sink.resize(n);
        y = sink.data();
    }
    ex_tables(N, tw.data(), win.data());
    int64_t counts[3] = {0, 0, 0};
    for (long long t = 0; t < g.tiles; ++t)
        ex_tile_host(x, y, tw.data(), win.data(), g, t, buf.data(), bytes.data(), psum.data(), pcnt.data(), counts,
                     cut_per_segment, reinterpret_cast<cplx*>(spectra));
    if (info) *info = sgx_excise_info{(int64_t)g.J, counts[0], counts[1], counts[2]};
    return SGX_OK;
}

extern "C" int sgx_excise_host(const int8_t* x, size_t n, int32_t N, double threshold, int32_t passes, int8_t* y,
                               sgx_excise_info* info, uint16_t* cut_per_segment) {
    SGX_CHECK_ARG(x && y && info);
    return ex_run_host(x, n, N, threshold, passes, y, info, cut_per_segment, nullptr);
}

extern "C" int sgx_excise_host_spectra(const int8_t* x, size_t n, int32_t N, double* spectra) {
    SGX_CHECK_ARG(x && spectra);
    return ex_run_host(x, n, N, 1.0, 1, nullptr, nullptr, nullptr, spectra);
}

extern "C" int sgx_if_excise(sgx_ctx* c, const sgx_if* rec, int32_t N, double threshold, int32_t passes, sgx_if** out,
                             sgx_excise_info* info, uint16_t* cut_per_segment) {
    SGX_CHECK_ARG(c && rec && out && info);
    SGX_CHECK_ARG(rec->device == c->device);
    ExGeom g;
    int rc = ex_geometry(rec->n, N, threshold, passes, &g);
    if (rc != SGX_OK) return rc;
    rc = sgx_stage_one_launch((unsigned long long)g.tiles,
                              "bad argument: a record of %zu samples is beyond one launch of the excision kernel", rec->n);
    if (rc == SGX_OK) rc = sgx_stage_open(c, rec, rec->n);
    if (rc == SGX_OK) rc = ex_prepare(&c->plan_excise, N);
    if (rc == SGX_OK && cut_per_segment) rc = c->d_excise_cut.ensure(sizeof(uint16_t) * (size_t)g.J);
    if (rc != SGX_OK) return rc;
    SGX_CHECK_ARG(((size_t)rec->d & 15) == 0);               // (every record starts on a granule: hipMalloc's alignment)
    const size_t lds = EX_LDS_BYTES(g.S, g.M);
    SGX_HIP(hipFuncSetAttribute((const void*)excise_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)EX_LDS_BYTES(EX_TILE_POINTS / (EX_MAX_SEGMENT / 2), EX_MAX_SEGMENT / 2)));
    const cplx* d_tw = c->plan_excise.tw();
    const double* d_win = c->plan_excise.extra();
    uint16_t* d_cut = cut_per_segment ? c->d_excise_cut.get() : nullptr;
    SgxStage st(SGX_STAGE_EXCISE, (unsigned)g.tiles, "excision kernel failed: %s", out, rec->n);
    unsigned long long* d_cnt = st.count(c);
    rc = sgx_stage_run(c, st, [&](sgx_if* r) {
        excise_kernel<<<st.grid, EX_THREADS, lds, c->stream>>>(rec->d, r->d, d_tw, d_win, g, d_cnt, d_cut);
    });
    if (rc != SGX_OK) return rc;
    if (cut_per_segment) {     // (the stage has waited: the counts of the segments are complete)
        const hipError_t e = hipMemcpy(cut_per_segment, d_cut, sizeof(uint16_t) * (size_t)g.J, hipMemcpyDeviceToHost);
        if (e != hipSuccess) {
            sgx_if_free(c, *out);
            *out = nullptr;
            sgx_set_error("excision kernel failed: %s", hipGetErrorString(e));
            return SGX_E_HIP;
        }
    }
    *info = sgx_excise_info{(int64_t)g.J, sgx_stage_count(c, 0), sgx_stage_count(c, 1), sgx_stage_count(c, 2)};
    return SGX_OK;
}
