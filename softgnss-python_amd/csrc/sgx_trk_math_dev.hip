// Device evaluator of the tracking chain's arithmetic (include/sgx.h: sgx_trk_math_eval_device).  Test support only: no
// tracking kernel changes, none is launched.  tests/test_trk_math_gpu.py compares what this kernel returns - the code of
// csrc/sgx_trk_math.h and csrc/sgx_trk_common.h as the DEVICE compiles it (v_rcp_f64 / v_rsq_f64 seeds, ocml's atan, the
// device's rint, ceil and float -> int conversions, the build's -ffp-contract=off) - with numpy's IEEE arithmetic and with
// 50-digit arithmetic.
//
//   trk_math_eval_kernel   one element per thread, 256 threads per workgroup, grid-stride loop.  fn < SGX_MATH_FN_HD_END:
//                          sgx_trk_math_call (csrc/sgx_trk_math_eval.h), the function the host evaluator calls too; the
//                          others are the __device__ functions of csrc/sgx_trk_common.h:
//                            16  div_rn(a, b, c)                     c = RN(1 / b)
//                            17  sincos_turns(a)                  -> sin, cos
//                            18  ramp_setup(start a, step b, inv_step, ilo (int)d) -> k1, isw; inv_step formed from the
//                                code step c exactly as prep_code forms it
//                            20 .. 24  prep_code(K, codeFreq a, rem b) under the TrkConst the host filled for the fs and the
//                                spacing of the call -> 20: blk, remCode  21: stepE, startE  22: stepP, startP
//                                23: stepL, startL  24: inv_step, stop
#include <math.h>

#include "sgx_trk_common.h"
#include "sgx_trk_math_eval.h"

#define TM_THREADS 256
#define TM_MAX_N (1 << 20)
#define TM_MAX_BLOCKS 1024

__global__ __launch_bounds__(TM_THREADS) void trk_math_eval_kernel(int fn, long long n, const double* __restrict__ a,
                                                                   const double* __restrict__ b, const double* __restrict__ c,
                                                                   const double* __restrict__ d, double* __restrict__ out0,
                                                                   double* __restrict__ out1, TrkConst K) {
    const long long stride = (long long)gridDim.x * TM_THREADS;
    for (long long i = (long long)blockIdx.x * TM_THREADS + threadIdx.x; i < n; i += stride) {
        const double va = a[i], vb = b[i], vc = c[i], vd = d[i];
        double o0 = 0.0, o1 = 0.0;
        if (fn < SGX_MATH_FN_HD_END) {
            sgx_trk_math_call(fn, va, vb, vc, vd, o0, o1);
        } else if (fn == 16) {
            o0 = div_rn(va, vb, vc);
        } else if (fn == 17) {
            sincos_turns(va, o0, o1);
        } else if (fn == 18) {
            const double r0 = __builtin_amdgcn_rcp(vc);                       // (prep_code's b.inv_step)
            const double inv_step = __builtin_fma(r0, __builtin_fma(-vc, r0, 1.0), r0);
            int k1, isw;
            ramp_setup(va, vb, inv_step, (int)vd, k1, isw);
            o0 = (double)k1;
            o1 = (double)isw;
        } else {
            TrkState s;
            TrkBlock blk;
            prep_code(K, va, vb, 0, s, blk, true);
            switch (fn) {
                case 20: o0 = (double)blk.blk; o1 = s.remCode; break;
                case 21: o0 = blk.stepE; o1 = blk.startE; break;
                case 22: o0 = blk.stepP; o1 = blk.startP; break;
                case 23: o0 = blk.stepL; o1 = blk.startL; break;
                default: o0 = blk.inv_step; o1 = (double)blk.stop; break;
            }
        }
        out0[i] = o0;
        out1[i] = o1;
    }
}

static bool tm_known(int32_t fn) { return (fn >= 0 && fn < SGX_MATH_FN_HD_END) || (fn >= 16 && fn <= 18) || (fn >= 20 && fn <= 24); }

extern "C" int sgx_trk_math_eval_device(sgx_ctx* ctx, int32_t fn, int64_t n, const double* a, const double* b,
                                        const double* c, const double* d, double* out0, double* out1) {
    SGX_CHECK_ARG(ctx && tm_known(fn));
    SGX_CHECK_ARG(n >= 1 && n <= TM_MAX_N);
    SGX_CHECK_ARG(a && out0 && out1);
    TrkConst K;
    memset(&K, 0, sizeof(K));
    if (fn >= 20) {
        // prep_code: fs = c[0], spacing = d[0] for the whole call; the constants as csrc/sgx_trk.hip: trk_const fills them
        SGX_CHECK_ARG(c && d);
        for (int64_t i = 1; i < n; ++i) SGX_CHECK_ARG(c[i] == c[0] && d[i] == d[0]);
        sgx_settings S = ctx->s;
        S.samplingFreq = c[0];
        S.dllCorrelatorSpacing = d[0];
        SGX_CHECK_ARG(S.samplingFreq > 0 && S.codeFreqBasis > 0);
        const int64_t n_code = sgx_host_samples_per_code(&S);
        SGX_CHECK_ARG(n_code >= 4 && n_code < (1 << 30));
        K.fs = S.samplingFreq;
        K.code_basis = S.codeFreqBasis;
        K.code_len = (double)S.codeLength;
        K.spacing = S.dllCorrelatorSpacing;
        K.rec_len = 1ll << 62;
        K.nb_base = (int)n_code - 3;
        for (int k = 0; k < 8; ++k) K.inv_nb[k] = 1.0 / (double)(K.nb_base + k);
        K.inv_fs = 1.0 / S.samplingFreq;
        K.inv_pi = 1.0 / M_PI;
    }
    SGX_HIP(hipSetDevice(ctx->device));
    // one allocation: the four operands (an absent one reads as zeros), then the two results
    const size_t row = (size_t)n * sizeof(double);
    DevBuf<double> buf;
    {
        const int rc = buf.ensure(6 * row);
        if (rc != SGX_OK) return rc;
    }
    const double* src[4] = {a, b, c, d};
    for (int k = 0; k < 4; ++k) {
        double* dst = buf.get() + (size_t)k * (size_t)n;
        if (src[k]) SGX_HIP(hipMemcpyAsync(dst, src[k], row, hipMemcpyHostToDevice, ctx->stream));
        else SGX_HIP(hipMemsetAsync(dst, 0, row, ctx->stream));
    }
    double* p = buf.get();
    const size_t N = (size_t)n;
    const long long want = ((long long)n + TM_THREADS - 1) / TM_THREADS;
    const unsigned blocks = (unsigned)(want < TM_MAX_BLOCKS ? want : TM_MAX_BLOCKS);
    trk_math_eval_kernel<<<blocks, TM_THREADS, 0, ctx->stream>>>((int)fn, (long long)n, p, p + N, p + 2 * N, p + 3 * N,
                                                                 p + 4 * N, p + 5 * N, K);
    hipError_t err = hipGetLastError();
    if (err == hipSuccess) err = hipMemcpyAsync(out0, p + 4 * N, row, hipMemcpyDeviceToHost, ctx->stream);
    if (err == hipSuccess) err = hipMemcpyAsync(out1, p + 5 * N, row, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t err2 = hipStreamSynchronize(ctx->stream);
    if (err == hipSuccess) err = err2;
    if (err != hipSuccess) {
        sgx_set_error("the tracking arithmetic evaluator failed: %s", hipGetErrorString(err));
        return SGX_E_HIP;
    }
    return SGX_OK;
}
