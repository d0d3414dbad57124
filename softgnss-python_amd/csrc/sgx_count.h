// The counters of the record front-end stages ("The stage tail"): what a stage's kernel counts over
// the whole record - outputs on the rails, blanked frames, codes, cut bins - is folded per workgroup and added with integer
// atomics into ONE area of the context, SgxSmall::stage_count, which the host sums (sgx_stage.h: SgxStage::count,
// sgx_stage_count).  Every stage waits before it returns, so one call owns the area at a time.  Who counts what:
//   sgx_count_publish   requantiser (1 counter), conditioning (2), unpacker (2^bits), decimator, resampler, combiners, cancellation (1)
//   sgx_count_slot      excision (3 counters; it publishes per wave, between its own barriers)
//   sgx_wave_sum / max  those, and every other integer fold over a wave in the stage files
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

// The layout.  A workgroup adds into slot blockIdx.x % SGX_COUNT_SLOTS, and a slot is one 128-byte line of its own, room
// for 16 counters: atomics on adjacent words - one per wave, when the requantiser was first written - serialised on their
// lines and bound the kernel, so the workgroups are spread over lines and each issues one atomic per counter.
#define SGX_COUNT_SLOTS 256
#define SGX_COUNT_STRIDE 16   // 64-bit words between two slots
static_assert(SGX_COUNT_STRIDE * sizeof(unsigned long long) == 128 && SGX_COUNT_STRIDE >= 16,
              "a slot is one line and holds the unpacker's 16 code counters");

// The total of an integer over the 64 lanes of a wave, in lane 0 (the other lanes hold partial sums), and the maximum
template <typename T> __device__ __forceinline__ T sgx_wave_sum(T v) {
    static_assert(std::is_integral<T>::value, "integers: any order gives the same sum");
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    return v;
}
template <typename T> __device__ __forceinline__ T sgx_wave_max(T v) {
    static_assert(std::is_integral<T>::value, "integers");
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const T o = __shfl_down(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

// The workgroup's slot of the area `counts` (zeroed in front of the kernel); counter k is word k of it
__device__ __forceinline__ unsigned long long* sgx_count_slot(unsigned long long* counts) {
    return counts + (size_t)(blockIdx.x % SGX_COUNT_SLOTS) * SGX_COUNT_STRIDE;
}

// The lanes' NC counts v[] of a workgroup of WAVES waves into its slot: lanes by shuffles, waves through LDS in wave order
// behind one barrier, then lane k < NC adds counter k, one atomic, where it is not zero.  Every lane of the workgroup calls
// it, once.
template <int NC, int WAVES>
__device__ __forceinline__ void sgx_count_publish(const unsigned (&v)[NC], unsigned long long* __restrict__ counts) {
    static_assert(NC >= 1 && NC <= SGX_COUNT_STRIDE, "the counters of a slot");
    __shared__ unsigned s_cnt[WAVES][NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        const unsigned t = sgx_wave_sum(v[k]);
        if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6][k] = t;
    }
    __syncthreads();
    if (threadIdx.x < NC) {
        unsigned t = 0;
        for (int w = 0; w < WAVES; ++w) t += s_cnt[w][threadIdx.x];
        if (t) atomicAdd(sgx_count_slot(counts) + threadIdx.x, (unsigned long long)t);
    }
}
