// IF records of libsgx.so: their life cycle (one way in, sgx_if_alloc_internal; one way out, sgx_if_free) and the
// file -> HBM pipeline that fills a record from a file.
#include <errno.h>
#include <fcntl.h>
#include <stdlib.h>
#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <string>

#include "sgx_internal.h"

// ---- IF records ------------------------------------------------------------------------------

// The one way out of a record, whatever state it is in: a half-made one of a failed call as well as a streaming one.
extern "C" int sgx_if_free(sgx_ctx* c, sgx_if* r) {
    if (!r) return SGX_OK;
    if (r->loader) {
        r->loader->join();
        delete r->loader;
        r->loader = nullptr;
    }
    if (c) {
        hipSetDevice(c->device);
        hipStreamSynchronize(c->stream);
    }
    if (r->copy_stream) hipStreamSynchronize(r->copy_stream);
    if (c) c->spare.park(r);   // keep ONE allocation (the larger), watermark and copy stream for the next record of this context
    if (r->copy_stream) hipStreamDestroy(r->copy_stream);
    if (r->d_mark) hipFree(r->d_mark);
    if (r->d) hipFree(r->d);
    delete r;
    return SGX_OK;
}

int sgx_if_alloc_internal(sgx_ctx* c, size_t n, sgx_if** out) {
    sgx_if* r = new sgx_if();
    r->n = n;
    r->device = c->device;
    hipError_t e = hipSuccess;
    // the allocation the last freed record left behind, when it is large enough (and not absurdly larger)
    r->d = c->spare.take(n, &r->cap);
    if (!r->d) {
        e = hipMalloc((void**)&r->d, n + SGX_IF_PAD);
        if (e != hipSuccess) {
            // the parked allocation of an earlier record may be what is in the way: give it back and try once more
            (void)hipGetLastError();
            if (c->spare.drop()) e = hipMalloc((void**)&r->d, n + SGX_IF_PAD);
        }
        r->cap = n + SGX_IF_PAD;
    }
    if (e != hipSuccess) {
        r->d = nullptr;
        sgx_if_free(c, r);
        sgx_set_error("hipMalloc(%zu) for an IF record failed: %s", n + SGX_IF_PAD, hipGetErrorString(e));
        return SGX_E_NOMEM;
    }
    e = hipMemsetAsync(r->d + n, 0, SGX_IF_PAD, c->stream);
    if (e != hipSuccess) {
        sgx_if_free(c, r);
        sgx_set_error("hipMemsetAsync failed: %s", hipGetErrorString(e));
        return SGX_E_HIP;
    }
    *out = r;
    return SGX_OK;
}

extern "C" int sgx_if_upload(sgx_ctx* c, const int8_t* host, size_t n, sgx_if** out) {
    SGX_CHECK_ARG(c && out && (host || n == 0));
    SGX_HIP(hipSetDevice(c->device));
    sgx_if* r = nullptr;
    int rc = sgx_if_alloc_internal(c, n, &r);
    if (rc != SGX_OK) return rc;
    if (n) {
        hipError_t e = hipMemcpyAsync(r->d, host, n, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // caller may free `host` on return
        if (e != hipSuccess) {
            sgx_if_free(c, r);
            sgx_set_error("H2D copy of the IF record failed: %s", hipGetErrorString(e));
            return SGX_E_HIP;
        }
    }
    *out = r;
    return SGX_OK;
}

extern "C" int sgx_if_length(const sgx_if* r, size_t* n) {
    SGX_CHECK_ARG(r && n);
    *n = r->n;
    return SGX_OK;
}

int sgx_if_require(const sgx_if* r, size_t end) {
    if (!r->loader) return SGX_OK;
    if (end > r->n) end = r->n;
    while (!r->load_done.load() && r->host_mark.load() < end) std::this_thread::sleep_for(std::chrono::microseconds(50));
    const int rc = r->load_rc.load();
    if (rc != SGX_OK) sgx_set_error("%s", r->load_err);
    return rc;
}

extern "C" int sgx_if_wait(sgx_ctx* c, sgx_if* r, size_t n) {
    SGX_CHECK_ARG(c && r);
    return sgx_if_require(r, n == 0 ? r->n : n);
}

extern "C" int sgx_if_download(sgx_ctx* c, const sgx_if* r, size_t offset, size_t n, int8_t* host) {
    SGX_CHECK_ARG(c && r && host);
    SGX_CHECK_ARG(offset <= r->n && n <= r->n - offset);
    {
        const int rq = sgx_if_require(r, offset + n);
        if (rq != SGX_OK) return rq;
    }
    SGX_HIP(hipSetDevice(c->device));
    SGX_HIP(hipMemcpyAsync(host, r->d + offset, n, hipMemcpyDeviceToHost, c->stream));
    SGX_HIP(hipStreamSynchronize(c->stream));
    return SGX_OK;
}

// ---- file -> HBM pipeline ------------------------------------------------------
// np.fromfile copies the file through the page cache into a pageable array and hipMemcpy then stages that array once
// more.  Here READERS threads pread() alternate 16 MiB chunks straight into a ring of four pinned slots while the
// issuing thread queues the slots' H2D copies in file order on one stream; a slot is read into again once the copy that
// last used it has completed.  One pread() stream moves ~21 GB/s out of the page cache (it is a CPU memcpy), three keep
// ahead of the PCIe link.
__global__ void if_mark_kernel(unsigned long long* mark, unsigned long long value) {
    __hip_atomic_store(mark, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

#define SGX_STAGE_BYTES (32u << 20)   // a pinned staging buffer: two slots
#define SGX_SLOT_BYTES (16u << 20)    // a multiple of every cache-line size: a line is never fetched half written
#define SGX_PIPE_SLOTS 4
#define SGX_PIPE_READERS 3

struct FilePipe {
    int fd = -1;
    uint64_t file_offset = 0;
    size_t n = 0;                         // bytes to move
    int8_t* dst = nullptr;                // device
    int device = 0;
    hipStream_t stream = nullptr;
    char* slot[SGX_PIPE_SLOTS] = {};
    hipEvent_t ev[SGX_PIPE_SLOTS] = {};
    unsigned long long* d_mark = nullptr; // device watermark advanced in stream order after every chunk, or null
    std::atomic<size_t>* host_mark = nullptr;   // bytes whose copy is known to have completed, or null
    std::vector<std::atomic<int>> read_ok;      // per chunk: 1 read, -1 read error
    std::atomic<long> issued{0};          // chunks whose copy and event have been queued
    std::atomic<bool> stop{false};
    std::atomic<int> err_no{0};
    std::atomic<size_t> err_off{0};
    explicit FilePipe(size_t chunks) : read_ok(chunks) {
        for (auto& f : read_ok) f.store(0);
    }
};

static const char* pipe_io_text(int err_no) {
    return err_no ? strerror(err_no) : "the file ends there (truncated while it was read?)";
}

static void pipe_reader(FilePipe* P, int t) {
    (void)hipSetDevice(P->device);
    const long chunks = (long)P->read_ok.size();
    for (long i = t; i < chunks && !P->stop.load(); i += SGX_PIPE_READERS) {
        const int sl = (int)(i % SGX_PIPE_SLOTS);
        if (i >= SGX_PIPE_SLOTS) {
            // the slot's previous chunk: its copy must have been queued, then completed
            while (P->issued.load() <= i - SGX_PIPE_SLOTS && !P->stop.load()) std::this_thread::sleep_for(std::chrono::microseconds(20));
            if (P->stop.load()) break;
            if (hipEventSynchronize(P->ev[sl]) != hipSuccess) {
                P->read_ok[(size_t)i].store(-1);
                break;
            }
            if (P->host_mark) {
                const size_t end = (size_t)(i - SGX_PIPE_SLOTS + 1) * SGX_SLOT_BYTES;
                size_t cur = P->host_mark->load();
                while (end > cur && !P->host_mark->compare_exchange_weak(cur, end)) {
                }
            }
        }
        const size_t off = (size_t)i * SGX_SLOT_BYTES;
        const size_t len = (P->n - off < SGX_SLOT_BYTES) ? (P->n - off) : SGX_SLOT_BYTES;
        size_t got = 0;
        bool bad = false;
        while (got < len) {
            const ssize_t m = pread(P->fd, P->slot[sl] + got, len - got, (off_t)(P->file_offset + off + got));
            if (m <= 0) {
                bad = true;
                P->err_no.store(m == 0 ? 0 : errno);   // 0: the file ended here (it was truncated while streaming)
                P->err_off.store(off + got);
                break;
            }
            got += (size_t)m;
        }
        P->read_ok[(size_t)i].store(bad ? -1 : 1);
        if (bad) break;
    }
}

// Runs the pipeline to completion on the calling thread (which issues the copies).  Returns hipSuccess and *io_fail.
static hipError_t pipe_run(FilePipe* P, bool* io_fail) {
    *io_fail = false;
    hipError_t e = hipSuccess;
    for (int i = 0; i < SGX_PIPE_SLOTS && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&P->ev[i], hipEventDisableTiming);
    std::vector<std::thread> readers;
    const long chunks = (long)P->read_ok.size();
    if (e == hipSuccess)
        for (int t = 0; t < SGX_PIPE_READERS && t < chunks; ++t) readers.emplace_back(pipe_reader, P, t);
    // host_mark follows the copies chunk by chunk (not only when a slot is reused, 4 chunks later): the prefix an
    // acquisition waits for is released as soon as its copy has completed.  Chunks up to issued - SLOTS are complete
    // (their slot has been refilled, which waits for their event); the events of the later ones are still their own.
    long completed = 0;
    auto advance = [&](long issued) {
        if (!P->host_mark) return;
        if (completed < issued - SGX_PIPE_SLOTS) completed = issued - SGX_PIPE_SLOTS;
        while (completed < issued && hipEventQuery(P->ev[completed % SGX_PIPE_SLOTS]) == hipSuccess) ++completed;
        size_t end = (size_t)completed * SGX_SLOT_BYTES;
        if (end > P->n) end = P->n;
        size_t cur = P->host_mark->load();
        while (end > cur && !P->host_mark->compare_exchange_weak(cur, end)) {
        }
    };
    for (long i = 0; i < chunks && e == hipSuccess; ++i) {
        int st;
        while ((st = P->read_ok[(size_t)i].load()) == 0) {
            advance(i);
            std::this_thread::sleep_for(std::chrono::microseconds(10));
        }
        if (st < 0) {
            *io_fail = true;
            break;
        }
        const int sl = (int)(i % SGX_PIPE_SLOTS);
        const size_t off = (size_t)i * SGX_SLOT_BYTES;
        const size_t len = (P->n - off < SGX_SLOT_BYTES) ? (P->n - off) : SGX_SLOT_BYTES;
        e = hipMemcpyAsync(P->dst + off, P->slot[sl], len, hipMemcpyHostToDevice, P->stream);
        if (e == hipSuccess && P->d_mark) if_mark_kernel<<<1, 1, 0, P->stream>>>(P->d_mark, (unsigned long long)(off + len));
        if (e == hipSuccess) e = hipEventRecord(P->ev[sl], P->stream);
        if (e != hipSuccess) P->err_off.store(off);   // (the chunk whose copy could not be queued)
        P->issued.store(i + 1);
    }
    if (e != hipSuccess || *io_fail) P->stop.store(true);
    for (auto& t : readers) t.join();
    // the tail: chunk by chunk as well (a record of a few chunks is all tail)
    while (P->host_mark && e == hipSuccess && !*io_fail && completed < chunks) {
        const long before = completed;
        advance(chunks);
        if (completed == before && hipEventSynchronize(P->ev[completed % SGX_PIPE_SLOTS]) != hipSuccess) break;
    }
    if (e == hipSuccess) e = hipStreamSynchronize(P->stream);
    for (int i = 0; i < SGX_PIPE_SLOTS; ++i)
        if (P->ev[i]) hipEventDestroy(P->ev[i]);
    return e;
}

// the context's two pinned staging buffers (kept between calls: pinning 64 MiB costs ~15 ms), reserved for one user
static bool stage_acquire(sgx_ctx* c) {
    bool expected = false;
    if (!c->stage_busy.compare_exchange_strong(expected, true)) return false;
    for (int i = 0; i < 2; ++i)
        if (!c->stage[i] && hipHostMalloc(&c->stage[i], SGX_STAGE_BYTES, hipHostMallocDefault) != hipSuccess) c->stage[i] = nullptr;
    if (c->stage[0] && c->stage[1]) return true;
    c->stage_busy.store(false);
    return false;
}

static bool pipe_slots(FilePipe* P, sgx_ctx* owner, void* own[2]) {
    own[0] = own[1] = nullptr;
    for (int i = 0; i < 2; ++i) {
        void* buf = owner ? owner->stage[i] : nullptr;
        if (!buf) {
            if (hipHostMalloc(&own[i], SGX_STAGE_BYTES, hipHostMallocDefault) != hipSuccess) return false;
            buf = own[i];
        }
        P->slot[2 * i] = (char*)buf;
        P->slot[2 * i + 1] = (char*)buf + SGX_SLOT_BYTES;
    }
    return true;
}

// A record for the bytes of `path` behind file_offset, n of them or as many as the file holds, and the open descriptor
// they will be read through.  On failure nothing is left open.
static int record_open(sgx_ctx* c, const char* path, uint64_t file_offset, size_t n, int* fd_out, sgx_if** out) {
    const int fd = open(path, O_RDONLY);
    if (fd < 0) {
        sgx_set_error("cannot open %s: %s", path, strerror(errno));
        return SGX_E_ARG;
    }
    struct stat sb;
    if (fstat(fd, &sb) != 0) {
        close(fd);
        sgx_set_error("fstat(%s) failed: %s", path, strerror(errno));
        return SGX_E_ARG;
    }
    size_t avail = ((uint64_t)sb.st_size > file_offset) ? (size_t)((uint64_t)sb.st_size - file_offset) : 0;
    if (avail > n) avail = n;
    const int rc = sgx_if_alloc_internal(c, avail, out);
    if (rc != SGX_OK) {
        close(fd);
        return rc;
    }
    *fd_out = fd;
    return SGX_OK;
}

// How a record's pipeline ended: rc is SGX_OK, SGX_E_ARG with the text of a failed read, or SGX_E_HIP with HIP's verdict;
// err_off is the offset in the record of the chunk that failed
struct PipeEnd {
    int rc = SGX_OK;
    hipError_t e = hipSuccess;
    size_t err_off = 0;
    char io_text[512] = "";
};

// Fills record r from fd (which it closes) on `stream`, on the calling thread: through the context's staging buffers where
// nobody else is streaming, else through two of its own.  marks: the record's device and host watermarks follow the copies.
static PipeEnd record_fill(sgx_ctx* c, sgx_if* r, int fd, uint64_t file_offset, const char* path, hipStream_t stream, bool marks) {
    PipeEnd end;
    bool io_fail = false;
    FilePipe P((r->n + SGX_SLOT_BYTES - 1) / SGX_SLOT_BYTES);
    P.fd = fd;
    P.file_offset = file_offset;
    P.n = r->n;
    P.dst = r->d;
    P.device = r->device;
    P.stream = stream;
    P.d_mark = marks ? r->d_mark : nullptr;
    P.host_mark = marks ? &r->host_mark : nullptr;
    end.e = hipSetDevice(r->device);
    if (end.e == hipSuccess) {
        sgx_ctx* owner = stage_acquire(c) ? c : nullptr;
        void* own[2];
        end.e = pipe_slots(&P, owner, own) ? pipe_run(&P, &io_fail) : hipErrorOutOfMemory;
        for (int i = 0; i < 2; ++i)
            if (own[i]) hipHostFree(own[i]);
        if (owner) owner->stage_busy.store(false);
    }
    close(fd);
    end.err_off = P.err_off.load();
    if (io_fail)
        snprintf(end.io_text, sizeof(end.io_text), "read error on %s at byte %llu: %s", path,
                 (unsigned long long)(file_offset + end.err_off), pipe_io_text(P.err_no.load()));
    end.rc = io_fail ? SGX_E_ARG : end.e != hipSuccess ? SGX_E_HIP : SGX_OK;
    return end;
}

extern "C" int sgx_if_upload_file(sgx_ctx* c, const char* path, uint64_t file_offset, size_t n, sgx_if** out) {
    SGX_CHECK_ARG(c && path && out);
    SGX_HIP(hipSetDevice(c->device));
    int fd = -1;
    sgx_if* r = nullptr;
    const int rc = record_open(c, path, file_offset, n, &fd, &r);
    if (rc != SGX_OK) return rc;
    const PipeEnd end = record_fill(c, r, fd, file_offset, path, c->stream, false);
    if (end.rc != SGX_OK) {
        sgx_if_free(c, r);
        if (end.rc == SGX_E_ARG)
            sgx_set_error("%s", end.io_text);
        else
            sgx_set_error("streaming upload of %s failed: %s", path, hipGetErrorString(end.e));
        return end.rc;
    }
    *out = r;
    return SGX_OK;
}

// ---- background streaming: the record fills in file order while acquisition and tracking already run ----------
static void if_loader_main(sgx_ctx* c, sgx_if* r, int fd, uint64_t file_offset, std::string path) {
    const PipeEnd end = record_fill(c, r, fd, file_offset, path.c_str(), r->copy_stream, true);
    if (end.rc != SGX_OK) {
        if (end.rc == SGX_E_ARG)
            snprintf(r->load_err, sizeof(r->load_err), "%s", end.io_text);
        else
            snprintf(r->load_err, sizeof(r->load_err), "streaming %s failed at byte %llu: %s", path.c_str(),
                     (unsigned long long)(file_offset + end.err_off), hipGetErrorString(end.e));
        r->load_rc.store(end.rc);
    } else {
        r->host_mark.store(r->n);
    }
    // whatever happened, nobody may wait for the watermark any longer
    if_mark_kernel<<<1, 1, 0, r->copy_stream>>>(r->d_mark, 0x7FFFFFFFFFFFFFFFull);
    hipStreamSynchronize(r->copy_stream);
    r->load_done.store(true);
}

extern "C" int sgx_if_open_file(sgx_ctx* c, const char* path, uint64_t file_offset, size_t n, sgx_if** out) {
    SGX_CHECK_ARG(c && path && out);
    SGX_HIP(hipSetDevice(c->device));
    int fd = -1;
    sgx_if* r = nullptr;
    const int rc = record_open(c, path, file_offset, n, &fd, &r);
    if (rc != SGX_OK) return rc;
    hipError_t e = hipStreamSynchronize(c->stream);   // the zero pad is in place
    if (e == hipSuccess) {
        // A stream of the highest priority: HIP keeps separate hardware queues per priority, so the copies and the
        // watermark updates never queue up behind the (normal-priority) stream that runs the tracking kernel.
        int lo = 0, hi = 0;
        e = hipDeviceGetStreamPriorityRange(&lo, &hi);
        const char* pe = getenv("SGX_STREAM_PRIO");   // test hook: "0" = a normal-priority copy stream
        if (pe && pe[0] == '0') hi = 0;
        if (c->priority < 0) hi = 0;   // the context itself runs at the highest priority: copies go one level below
        if (!(pe && pe[0] == '0')) r->copy_stream = c->spare.take_stream();
        r->d_mark = c->spare.take_mark();
        if (e == hipSuccess && !r->copy_stream) e = hipStreamCreateWithPriority(&r->copy_stream, hipStreamNonBlocking, hi);
        if (e != hipSuccess) {   // no stream priorities here: an ordinary stream (the kernel's bounded wait covers it)
            (void)hipGetLastError();
            e = hipStreamCreateWithFlags(&r->copy_stream, hipStreamNonBlocking);
        }
    }
    if (e == hipSuccess && !r->d_mark) e = hipMalloc((void**)&r->d_mark, 256);
    if (e == hipSuccess) e = hipMemsetAsync(r->d_mark, 0, 256, r->copy_stream);
    if (e == hipSuccess) e = hipStreamSynchronize(r->copy_stream);
    if (e != hipSuccess) {
        close(fd);
        sgx_if_free(c, r);
        sgx_set_error("cannot set up the streaming record: %s", hipGetErrorString(e));
        return SGX_E_HIP;
    }
    r->loader = new std::thread(if_loader_main, c, r, fd, file_offset, std::string(path));
    *out = r;
    return SGX_OK;
}
