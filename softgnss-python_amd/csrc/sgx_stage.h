// The host side that the record front-end stages share: the notch (sgx_filter.hip), the I/Q converter (sgx_iq.hip), the
// requantiser (sgx_requant.hip), the conditioning stage (sgx_cond.hip), the unpacker (sgx_unpack.hip), the decimator
// (sgx_decim.hip), the resampler (sgx_resamp.hip), the multi-antenna combiner (sgx_array.hip), the swept-interference
// excision (sgx_excise.hip; what its kernel shares with the record monitor's is in sgx_seg_fft.h, not here) and the
// strong-signal cancellation (sgx_cancel.hip).  Each of their fifteen entry points keeps its own argument checks, in its
// own order and with its own messages, and its launch; what comes around the launch is here once, and so is the host side
// of the one counter area that the nine counting entry points share (SgxStage::count, sgx_stage_count; the device side is
// sgx_count.h) ("The stage tail").
#pragma once
#include "sgx_count.h"
#include "sgx_internal.h"

// Opening the input, once the stage's own checks of its shape have passed: wait until the first `bytes` of a record that
// is still streaming in are resident, then select the context's device.
static inline int sgx_stage_open(sgx_ctx* c, const sgx_if* rec, size_t bytes) {
    const int rq = sgx_if_require(rec, bytes);
    if (rq != SGX_OK) return rq;
    SGX_HIP(hipSetDevice(c->device));
    return SGX_OK;
}

// The refusal of a record beyond one launch, before anything is allocated for it.  too_long: the stage's message, a format
// with one %zu for n.
static inline int sgx_stage_one_launch(unsigned long long tiles, const char* too_long, size_t n) {
    if (tiles <= 0x7FFFFFFFull) return SGX_OK;
    sgx_set_error(too_long, n);
    return SGX_E_ARG;
}

// A few bytes that cross between the host and the device around a launch; bytes 0: none
struct SgxStageCopy {
    void* dst = nullptr;
    const void* src = nullptr;
    size_t bytes = 0;
};

struct SgxStage {
    SgxStageSlot slot;     // where the kernel's time goes
    unsigned grid;         // workgroups; 0: no work
    const char* failed;    // the message of a HIP failure, a format with one %s for HIP's text
    sgx_if** out;          // a stage that makes a record: where the new record of out_n bytes goes; else null
    size_t out_n;
    SgxStageCopy up;       // host -> device in front of the kernel: the tap image, the plan
    SgxStageCopy down;     // device -> host behind it: partials, block statistics, counters
    void* counters;        // down.src where the kernel adds into it: the device side and the mirror start from zero
    SgxStage(SgxStageSlot slot_, unsigned grid_, const char* failed_, sgx_if** out_ = nullptr, size_t out_n_ = 0)
        : slot(slot_), grid(grid_), failed(failed_), out(out_), out_n(out_n_), counters(nullptr) {}
    void count_into(void* mirror, void* device, size_t bytes) {
        down = {mirror, device, bytes};
        counters = device;
    }
    // The stage's kernel counts (sgx_count.h): the context's one counter area is the stage's counters.  A stage waits
    // before it returns, so one call owns the area at a time.  Returns the device side, for the kernel.
    unsigned long long* count(sgx_ctx* c) {
        count_into(c->h_small->stage_count, c->d_small->stage_count, sizeof(SgxSmall::stage_count));
        return c->d_small->stage_count;
    }
};

// The tail of an entry point, on the context's stream: the output record is allocated, the stage's timing slot and the
// counters' pinned mirror are cleared, `up` is copied and the device counters are cleared, launch(output record) runs
// between the two events, `down` is copied, and the host waits.  The slot then holds the time of the kernel alone.  With no
// work nothing is launched, no event is recorded, the counters are not touched on the device (their mirror is zero) and
// the slot stays 0.  On a HIP failure the output record is freed and SGX_E_HIP returned with the stage's message.
template <typename Launch>
static int sgx_stage_run(sgx_ctx* c, const SgxStage& s, Launch launch) {
    sgx_if* r = nullptr;
    if (s.out) {
        const int rc = sgx_if_alloc_internal(c, s.out_n, &r);
        if (rc != SGX_OK) return rc;
    }
    float* ms = &c->stage_ms[s.slot];
    *ms = 0.0f;
    if (s.counters) memset(s.down.dst, 0, s.down.bytes);
    hipError_t err = hipSuccess;
    if (s.up.bytes) err = hipMemcpyAsync(s.up.dst, s.up.src, s.up.bytes, hipMemcpyHostToDevice, c->stream);
    if (s.grid) {
        if (err == hipSuccess && s.counters) err = hipMemsetAsync(s.counters, 0, s.down.bytes, c->stream);
        if (err == hipSuccess) {
            hipEventRecord(c->ev[0], c->stream);
            launch(r);
            hipEventRecord(c->ev[1], c->stream);
            if (s.down.bytes) err = hipMemcpyAsync(s.down.dst, s.down.src, s.down.bytes, hipMemcpyDeviceToHost, c->stream);
        }
    }
    if (err == hipSuccess) err = hipStreamSynchronize(c->stream);   // (the pinned staging areas are free again on return)
    if (err == hipSuccess) err = hipGetLastError();
    if (err != hipSuccess) {
        if (r) sgx_if_free(c, r);
        sgx_set_error(s.failed, hipGetErrorString(err));
        return SGX_E_HIP;
    }
    if (s.grid) hipEventElapsedTime(ms, c->ev[0], c->ev[1]);
    if (s.out) *s.out = r;
    return SGX_OK;
}

// Counter k of the stage that has just run (SgxStage::count): the total over the slots of the mirror
static inline int64_t sgx_stage_count(const sgx_ctx* c, int k) {
    int64_t total = 0;
    for (int i = 0; i < SGX_COUNT_SLOTS; ++i) total += (int64_t)c->h_small->stage_count[(size_t)i * SGX_COUNT_STRIDE + k];
    return total;
}
