// Ownership of device resources: the error macros, the one owning device buffer, and the one owning handle behind the events, streams and
// page-locked buffers of libpoccala_hip.so.
// Needs only the declarations below (the pool, the error sink, the context's device ordinal), so that tests/test_devbuf_host.py can compile
// the types against a malloc-backed stub pool.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdio.h>

#include <utility>

#include "../../include/poccala_hip.h"

struct pcl_ctx;
void pcl_set_error(pcl_ctx *ctx, const char *msg);
int pcl_ctx_device(const pcl_ctx *ctx);

#define PCL_FAIL(ctx, code, ...)                         \
    do {                                                 \
        char _b[512];                                    \
        snprintf(_b, sizeof(_b), __VA_ARGS__);           \
        pcl_set_error((ctx), _b);                        \
        return (code);                                   \
    } while (0)
#define HIPCHK(ctx, call)                                                                         \
    do {                                                                                          \
        hipError_t _e = (call);                                                                   \
        if (_e != hipSuccess) PCL_FAIL(ctx, PCL_ERR_HIP, "%s: %s", #call, hipGetErrorString(_e)); \
    } while (0)
// ... with the entry point's name in front, where several entry points share the code
#define HIPWHO(ctx, who, call)                                                                                   \
    do {                                                                                                         \
        hipError_t _e = (call);                                                                                  \
        if (_e != hipSuccess) PCL_FAIL(ctx, PCL_ERR_HIP, "%s: %s: %s", who, #call, hipGetErrorString(_e));       \
    } while (0)
#define TRY(x)                    \
    do {                          \
        int _r = (x);             \
        if (_r != PCL_OK) return _r; \
    } while (0)

// Device memory comes from a process-wide caching pool (pcl_pool.hip): hipMalloc / hipFree cost 0.1-1 ms each and hipFree
// waits for the whole device, which a library that creates and drops a batch per utterance (the drop-in classes) or per
// chunk (streaming) cannot afford.  A freed block goes back to the pool; dev_free first waits for the device, as hipFree
// did, unless the caller has already made sure the GPU is done with the block (pcl_free_synced_scope).
void *pcl_pool_alloc(int device, size_t bytes);           // nullptr: out of memory even after the cache was released
void pcl_pool_free(void *p);
extern thread_local int pcl_tls_free_synced;              // > 0: dev_free skips its device-wide wait
struct pcl_free_synced_scope {
    pcl_free_synced_scope() { ++pcl_tls_free_synced; }
    ~pcl_free_synced_scope() { --pcl_tls_free_synced; }
    pcl_free_synced_scope(const pcl_free_synced_scope &) = delete;
    pcl_free_synced_scope &operator=(const pcl_free_synced_scope &) = delete;
};
template <typename T>
static inline int dev_alloc(pcl_ctx *ctx, T **p, size_t n) {
    if (n == 0) n = 1;
    *p = static_cast<T *>(pcl_pool_alloc(pcl_ctx_device(ctx), n * sizeof(T)));
    if (!*p) PCL_FAIL(ctx, PCL_ERR_NOMEM, "device memory: %zu bytes", n * sizeof(T));
    return PCL_OK;
}
template <typename T>
static inline void dev_free(T *&p) {
    if (p) pcl_pool_free((void *)p);
    p = nullptr;
}

// THE owner of a device array: a pointer and a capacity in elements.  The block goes back to the pool when the buffer is released,
// re-allocated, assigned over or destroyed -- through dev_free, so with its device-wide wait unless a pcl_free_synced_scope is open
// (locals are destroyed in reverse order of declaration: a scope that is to cover a buffer's release is declared BEFORE the buffer).
// Reads as a plain T* wherever one is expected (kernel arguments, copies, `if (!buf)`).
template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
            cap = std::exchange(o.cap, 0);
        }
        return *this;
    }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    operator T *() const { return p; }
    void release() { dev_free(p); cap = 0; }
    int alloc(pcl_ctx *ctx, size_t n) {                     // exactly n elements (a block even for n = 0); what was held goes first
        release();
        TRY(dev_alloc(ctx, &p, n));
        cap = n;
        return PCL_OK;
    }
    int reserve(pcl_ctx *ctx, size_t n) {                   // room for n elements, grows only; nothing is copied: the contents are undefined after a growth
        return n <= cap ? PCL_OK : alloc(ctx, n);
    }
};

// THE owner of anything else the runtime hands out: a handle and the function that gives it back.  Ops has `static hipError_t create(H *)` (for
// make(), where a handle is made without arguments) and `static void destroy(H)`.  Move-only, reads as the plain handle, null (H{}) until made
// and after a move or a destroy().  tests/devbuf_host_check.cpp instantiates it with counting stubs.
template <typename H, typename Ops>
struct Owned {
    H h{};
    Owned() = default;
    Owned(Owned &&o) noexcept : h(std::exchange(o.h, H{})) {}
    Owned &operator=(Owned &&o) noexcept {
        if (this != &o) {
            destroy();
            h = std::exchange(o.h, H{});
        }
        return *this;
    }
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    ~Owned() { destroy(); }
    operator H() const { return h; }
    hipError_t make() { return h ? hipSuccess : Ops::create(&h); }   // on first use: a second make() keeps what is there
    void destroy() {
        if (h) Ops::destroy(h);
        h = H{};
    }
};
// Two of them made as a pair or not at all.
template <typename H, typename Ops>
struct OwnedPair {
    Owned<H, Ops> first, second;
    hipError_t make() {
        hipError_t e = first.make();
        if (e == hipSuccess && (e = second.make()) != hipSuccess) first.destroy();
        return e;
    }
};

template <unsigned Flags>
struct EventOps {
    static hipError_t create(hipEvent_t *e) { return hipEventCreateWithFlags(e, Flags); }
    static void destroy(hipEvent_t e) { (void)hipEventDestroy(e); }
};
// An event without timing, created on first use (most batches never fetch, most contexts never stage): make() before the first record.
using LazyEvent = Owned<hipEvent_t, EventOps<hipEventDisableTiming>>;
// The two timing events around one launch of a KernelTimer group.
using TimedEventPair = OwnedPair<hipEvent_t, EventOps<hipEventDefault>>;

// A stream in one of the three flavours the runtime uses, chosen where it is made.
enum class StreamKind { Plain, HighPriority, NonBlocking };
struct StreamOps {
    static void destroy(hipStream_t s) { (void)hipStreamDestroy(s); }
};
struct Stream : Owned<hipStream_t, StreamOps> {
    hipError_t make(StreamKind k) {
        if (h) return hipSuccess;
        if (k == StreamKind::HighPriority) return hipStreamCreateWithPriority(&h, hipStreamDefault, -1);
        return k == StreamKind::NonBlocking ? hipStreamCreateWithFlags(&h, hipStreamNonBlocking) : hipStreamCreate(&h);
    }
};

// Page-locked host memory: a pointer and a capacity in elements, as DevBuf.  reserve grows only and copies nothing; a failed allocation
// leaves the buffer empty.  (Memory the CALLER owns -- pcl_host_alloc / pcl_host_free -- does not come through here.)
struct PinBlock {
    void *p = nullptr;
    size_t cap = 0;
    explicit operator bool() const { return p != nullptr; }
};
struct PinOps {
    static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void destroy(PinBlock b) { (void)hipHostFree(b.p); }
};
template <typename T, typename Ops = PinOps>
struct PinBuf : Owned<PinBlock, Ops> {
    operator T *() const { return static_cast<T *>(this->h.p); }
    size_t cap() const { return this->h.cap; }
    hipError_t reserve(size_t n) {
        if (n <= this->h.cap) return hipSuccess;
        this->destroy();
        void *p = nullptr;
        const hipError_t e = Ops::alloc(&p, n * sizeof(T));
        if (e == hipSuccess) this->h = PinBlock{p, n};
        return e;
    }
};
