// The cooperative tracking kernel for low sampling rates (fewer than ~15 samples per chip, e.g. 5.456 or 4.092
// Msps): a 16-sample group can then hold several chip switches of a code ramp, which the maps of sgx_trk2.hip
// exclude by construction, so this kernel indexes the replicas sample by sample like the reference
// (tracking.py:166-188).  int8 records; members own units c, c + split, ... (split <= 10).
#include "sgx_trk_persample.h"

__global__ __launch_bounds__(TRK_THREADS, 1) void trk_kernel_multi(const int8_t* __restrict__ rec, const int8_t* __restrict__ codes,
    const TrkChan* __restrict__ chans, double* __restrict__ out, int* __restrict__ ms_done, TrkConst K,
    long long* __restrict__ prof, unsigned long long* __restrict__ xch, int* __restrict__ err) {
    trk_persample_body<false>(rec, codes, chans, out, ms_done, K, prof, xch, err);
}

void sgx_trk_multi_launch(int n_blocks, hipStream_t st, const int8_t* rec, const int8_t* codes, const TrkChan* chans, double* out,
                          int* ms_done, const TrkConst& K, long long* prof, unsigned long long* xch, int* err) {
    trk_kernel_multi<<<n_blocks, TRK_THREADS, 0, st>>>(rec, codes, chans, out, ms_done, K, prof, xch, err);
}
