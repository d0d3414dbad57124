// The device context of libsgx.so: creation and the one teardown, the host's wait for a word of the result page, pinned
// result buffers, timings and the compute-unit budget of cooperative launches.
#include <chrono>

#include "sgx_internal.h"

// ---- device context --------------------------------------------------------------------------

extern "C" int sgx_device_count(int* n) {
    SGX_CHECK_ARG(n);
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) {
        *n = 0;
        sgx_set_error("hipGetDeviceCount: %s", hipGetErrorString(e));
        return SGX_E_HIP;
    }
    *n = c;
    return SGX_OK;
}

extern "C" int sgx_ctx_create(const sgx_settings* s, int device, sgx_ctx** out) {
    return sgx_ctx_create_prio(s, device, 0, out);
}

static int ctx_build(sgx_ctx* c, int priority) {
    if (priority == 0) {
        SGX_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    } else {
        int least = 0, greatest = 0;   // numerically: greatest priority <= least priority
        SGX_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
        SGX_HIP(hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, priority < 0 ? greatest : least));
    }
    for (int i = 0; i < 6; ++i) SGX_HIP(hipEventCreate(&c->ev[i]));
    std::vector<int8_t> codes(32 * 1023);
    for (int p = 0; p < 32; ++p) sgx_host_ca_code(p, codes.data() + p * 1023);
    SGX_HIP(hipMalloc((void**)&c->d_codes, codes.size()));
    SGX_HIP(hipMemcpy(c->d_codes, codes.data(), codes.size(), hipMemcpyHostToDevice));
    SGX_HIP(hipMalloc((void**)&c->d_small, SGX_SMALL_BYTES));
    SGX_HIP(hipHostMalloc((void**)&c->h_small, SGX_SMALL_BYTES, hipHostMallocDefault));
    SGX_HIP(hipHostMalloc((void**)&c->h_look, sizeof(LookPage), hipHostMallocCoherent | hipHostMallocMapped));
    memset(c->h_look, 0, sizeof(LookPage));
    SGX_HIP(hipHostGetDevicePointer((void**)&c->d_look, c->h_look, 0));
    return SGX_OK;
}

extern "C" int sgx_ctx_create_prio(const sgx_settings* s, int device, int priority, sgx_ctx** out) {
    SGX_CHECK_ARG(s && out && priority >= -1 && priority <= 1);
    SGX_CHECK_ARG(s->codeLength == 1023 && s->samplingFreq > 0 && s->codeFreqBasis > 0);
    SGX_HIP(hipSetDevice(device));
    sgx_ctx* c = new sgx_ctx();
    c->s = *s;
    c->device = device;
    c->n_code = sgx_host_samples_per_code(s);
    memset(&c->timing, 0, sizeof(c->timing));
    c->priority = priority;
    const int rc = ctx_build(c, priority);
    if (rc != SGX_OK) {
        delete c;   // (a partially built context; the message of the failing call is kept)
        return rc;
    }
    *out = c;
    return SGX_OK;
}

// Device and pinned memory first, events and streams last
sgx_ctx::~sgx_ctx() {
    sgx_fft_plan_destroy(&plan_code);
    sgx_fft_plan_destroy(&plan_fine);
    for (int i = 0; i < 2; ++i)
        if (stage[i]) hipHostFree(stage[i]);
    if (d_codes) hipFree(d_codes);
    d_sig64.release();
    d_fwd.release();
    d_codefd.release();
    d_work[0].release();
    d_work[1].release();
    d_pow.release();
    d_fine[0].release();
    d_fine[1].release();
    if (d_small) hipFree(d_small);
    d_trk_out.release();
    d_trk_aux.release();
    spare.release();
    if (acq_stream2) hipStreamDestroy(acq_stream2);
    for (int i = 0; i < 2; ++i)
        if (acq_ev2[i]) hipEventDestroy(acq_ev2[i]);
    if (h_small) hipHostFree(h_small);
    if (h_look) hipHostFree(h_look);
    for (int i = 0; i < 6; ++i)
        if (ev[i]) hipEventDestroy(ev[i]);
    if (stream) hipStreamDestroy(stream);
}

extern "C" int sgx_ctx_destroy(sgx_ctx* c) {
    if (!c) return SGX_OK;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    delete c;
    return SGX_OK;
}

int sgx_look_wait(hipStream_t st, const unsigned long long* word, unsigned long long seq, bool spin, double budget_s,
                  unsigned stride, const char* unwritten, hipError_t* sync_err) {
    if (spin) {
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned it = 0;; ++it) {
            if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == seq) return SGX_OK;
            if ((it & (stride - 1)) == stride - 1 &&
                std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > budget_s)
                break;
        }
    }
    if (sync_err) {
        *sync_err = hipStreamSynchronize(st);
        if (*sync_err != hipSuccess) return SGX_OK;
    } else {
        SGX_HIP(hipStreamSynchronize(st));
    }
    if (__atomic_load_n(word, __ATOMIC_ACQUIRE) != seq) {
        sgx_set_error("%s", unwritten);
        return SGX_E_HIP;
    }
    return SGX_OK;
}

extern "C" int sgx_ctx_sync(sgx_ctx* c) {
    SGX_CHECK_ARG(c);
    SGX_HIP(hipSetDevice(c->device));
    SGX_HIP(hipStreamSynchronize(c->stream));
    return SGX_OK;
}

extern "C" int sgx_get_timing(sgx_ctx* c, sgx_timing* out) {
    SGX_CHECK_ARG(c && out);
    *out = c->timing;
    return SGX_OK;
}

// pinned host memory for result buffers (D2H at full PCIe rate); plain C pointers, caller frees
extern "C" int sgx_host_alloc(size_t bytes, void** out) {
    SGX_CHECK_ARG(out && bytes > 0);
    void* p = nullptr;
    hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
    if (e != hipSuccess) {
        sgx_set_error("hipHostMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        return SGX_E_NOMEM;
    }
    *out = p;
    return SGX_OK;
}

extern "C" int sgx_host_free(void* p) {
    if (p) hipHostFree(p);
    return SGX_OK;
}

extern "C" int sgx_replay_timing(sgx_ctx* c, float* kernel_ms, float* device_ms) {
    SGX_CHECK_ARG(c && kernel_ms && device_ms);
    *kernel_ms = c->replay_kernel_ms;
    *device_ms = c->replay_device_ms;
    return SGX_OK;
}

// ---- co-residency budget of cooperative tracking launches ---------------------------------------
static std::atomic<int> g_cu_used[64];

int sgx_cu_reserve(int device, int cus_total, int want) {
    if (device < 0 || device >= 64 || want <= 0) return 0;
    int cur = g_cu_used[device].load();
    for (;;) {
        if (cur + want > cus_total) return 0;
        if (g_cu_used[device].compare_exchange_weak(cur, cur + want)) return want;
    }
}

void sgx_cu_release(int device, int n) {
    if (device >= 0 && device < 64 && n > 0) g_cu_used[device].fetch_sub(n);
}
