// The RCCL communicator of a context: the peak gather of the sharded acquisition.
#include <dlfcn.h>

#include "sgx_internal.h"

// ---- RCCL peak gather -------------------------------------------------------------------------
// librccl is opened lazily so that the library loads (and the host helpers work) on machines
// without a GPU.

struct RcclUid {
    char internal[128];
};
typedef int (*fn_get_uid)(RcclUid*);
typedef int (*fn_init_rank)(void**, int, RcclUid, int);
typedef int (*fn_allgather)(const void*, void*, size_t, int, void*, hipStream_t);
typedef int (*fn_destroy)(void*);
typedef const char* (*fn_errstr)(int);

static struct {
    void* h;
    fn_get_uid get_uid;
    fn_init_rank init_rank;
    fn_allgather allgather;
    fn_destroy destroy;
    fn_errstr errstr;
} g_rccl = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};

static int rccl_load() {
    if (g_rccl.h) return SGX_OK;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void* h = nullptr;
    for (const char* nm : names) {
        h = dlopen(nm, RTLD_NOW | RTLD_GLOBAL);
        if (h) break;
    }
    if (!h) {
        sgx_set_error("cannot dlopen librccl: %s", dlerror());
        return SGX_E_RCCL;
    }
    g_rccl.get_uid = (fn_get_uid)dlsym(h, "ncclGetUniqueId");
    g_rccl.init_rank = (fn_init_rank)dlsym(h, "ncclCommInitRank");
    g_rccl.allgather = (fn_allgather)dlsym(h, "ncclAllGather");
    g_rccl.destroy = (fn_destroy)dlsym(h, "ncclCommDestroy");
    g_rccl.errstr = (fn_errstr)dlsym(h, "ncclGetErrorString");
    if (!g_rccl.get_uid || !g_rccl.init_rank || !g_rccl.allgather || !g_rccl.destroy) {
        sgx_set_error("librccl lacks an expected symbol");
        dlclose(h);
        return SGX_E_RCCL;
    }
    g_rccl.h = h;
    return SGX_OK;
}

// (struct sgx_comm: sgx_internal.h)

static int rccl_fail(const char* what, int code) {
    sgx_set_error("%s failed: %s", what, g_rccl.errstr ? g_rccl.errstr(code) : "rccl error");
    return SGX_E_RCCL;
}

extern "C" int sgx_comm_unique_id(uint8_t id[128]) {
    SGX_CHECK_ARG(id);
    int rc = rccl_load();
    if (rc != SGX_OK) return rc;
    RcclUid u;
    int e = g_rccl.get_uid(&u);
    if (e != 0) return rccl_fail("ncclGetUniqueId", e);
    memcpy(id, u.internal, 128);
    return SGX_OK;
}

extern "C" int sgx_comm_create(sgx_ctx* c, int32_t n_ranks, int32_t rank, const uint8_t id[128],
                               sgx_comm** out) {
    SGX_CHECK_ARG(c && id && out && n_ranks >= 1 && rank >= 0 && rank < n_ranks);
    int rc = rccl_load();
    if (rc != SGX_OK) return rc;
    SGX_HIP(hipSetDevice(c->device));
    RcclUid u;
    memcpy(u.internal, id, 128);
    void* comm = nullptr;
    int e = g_rccl.init_rank(&comm, n_ranks, u, rank);
    if (e != 0) return rccl_fail("ncclCommInitRank", e);
    sgx_comm* m = new sgx_comm();
    m->ctx = c;
    m->comm = comm;
    m->n_ranks = n_ranks;
    m->rank = rank;
    m->cap = 1 << 16;
    rc = m->d_send.ensure(m->cap);
    if (rc == SGX_OK) rc = m->d_recv.ensure(m->cap * (size_t)n_ranks);
    if (rc != SGX_OK) {
        sgx_comm_destroy(m);
        return rc;
    }
    *out = m;
    return SGX_OK;
}

extern "C" int sgx_comm_allgather(sgx_comm* m, const void* send, void* recv, size_t bytes) {
    SGX_CHECK_ARG(m && send && recv && bytes > 0 && bytes <= m->cap);
    sgx_ctx* c = m->ctx;
    SGX_HIP(hipSetDevice(c->device));
    SGX_HIP(hipMemcpyAsync(m->d_send, send, bytes, hipMemcpyHostToDevice, c->stream));
    int e = g_rccl.allgather(m->d_send, m->d_recv, bytes, /*ncclInt8*/ 0, m->comm, c->stream);
    if (e != 0) return rccl_fail("ncclAllGather", e);
    SGX_HIP(hipMemcpyAsync(recv, m->d_recv, bytes * (size_t)m->n_ranks, hipMemcpyDeviceToHost, c->stream));
    SGX_HIP(hipStreamSynchronize(c->stream));
    return SGX_OK;
}

// ncclAllGather of `bytes` per rank from m->d_send into m->d_recv on the context's stream; nothing is copied or waited for
// (sgx_acquire_sharded packs and unpacks on the device)
int sgx_comm_allgather_device(sgx_comm* m, size_t bytes) {
    if (!m || bytes == 0 || bytes > m->cap) {
        sgx_set_error("sgx_comm_allgather_device: %zu bytes per rank, room for %zu", bytes, m ? m->cap : (size_t)0);
        return SGX_E_ARG;
    }
    int e = g_rccl.allgather(m->d_send, m->d_recv, bytes, /*ncclInt8*/ 0, m->comm, m->ctx->stream);
    if (e != 0) return rccl_fail("ncclAllGather", e);
    return SGX_OK;
}

extern "C" int sgx_comm_destroy(sgx_comm* m) {
    if (!m) return SGX_OK;
    hipSetDevice(m->ctx->device);
    hipStreamSynchronize(m->ctx->stream);
    if (m->comm && g_rccl.destroy) g_rccl.destroy(m->comm);
    delete m;
    return SGX_OK;
}
