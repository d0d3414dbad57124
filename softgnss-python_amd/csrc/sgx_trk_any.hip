// The cooperative tracking kernel for records of ANY sample type numpy reads (Settings.dataType; the reference's
// np.fromfile(fid, dataType, blksize), tracking.py:154): float32 / float64 records of arbitrary values, uint16 / int32 /
// ... records, and int16 / uint8 records at sampling rates the typed kernels exclude.  The per-sample body of
// sgx_trk_persample.h with every sample fetched where it lies, at any byte address (the reference seeks BYTES,
// tracking.py:107, so a channel may start inside a sample of the file - it does there, too), converted the way numpy's
// float64 arithmetic promotes it.  Compatibility before speed: ~5 us per code period for 8 channels (tools/any_type_probe.py).
#include "sgx_trk_persample.h"

__global__ __launch_bounds__(TRK_THREADS, 1) void trk_kernel_any(const int8_t* __restrict__ rec, const int8_t* __restrict__ codes,
    const TrkChan* __restrict__ chans, double* __restrict__ out, int* __restrict__ ms_done, TrkConst K,
    long long* __restrict__ prof, unsigned long long* __restrict__ xch, int* __restrict__ err) {
    trk_persample_body<true>(rec, codes, chans, out, ms_done, K, prof, xch, err);
}

void sgx_trk_any_launch(int n_blocks, hipStream_t st, const int8_t* rec, const int8_t* codes, const TrkChan* chans, double* out,
                        int* ms_done, const TrkConst& K, long long* prof, unsigned long long* xch, int* err) {
    trk_kernel_any<<<n_blocks, TRK_THREADS, 0, st>>>(rec, codes, chans, out, ms_done, K, prof, xch, err);
}
