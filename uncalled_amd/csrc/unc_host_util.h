// Host-side helpers shared by the translation units behind the C ABI (unc_host.cpp, unc_dtw.cpp, unc_align.cpp with unc_refseq.cpp, unc_mask.cpp):
// the error message of the calling thread, the one owner of device memory, the owners of timing events and of a stream, and the hand-over of a
// per-query output to the host.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/uncalled_hip.h"

namespace unc {
// stores the message unc_last_error() returns to the calling thread and returns `code` (defined in unc_host.cpp)
int fail(int code, const char *fmt, ...);
// the HIP device an index was loaded to (defined in unc_host.cpp, which owns the struct)
int index_device(const unc_index_t *ix);
// what the kernels take of an index: pointers into its device memory, valid while the index lives (unc_dev_types.h)
struct DevIndex;
const DevIndex &index_dev(const unc_index_t *ix);
}  // namespace unc

#define HIPCHK(expr)                                                                                         \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess) return unc::fail(UNC_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                               __FILE__, __LINE__);                                          \
    } while (0)

// The one owner of device memory in the host library (PlacementSpacer apart, which holds untyped memory for a moment).  Pointer and capacity
// travel together: p == nullptr exactly when cap == 0; the destructor frees; a move leaves the source empty.  `cap` counts the elements
// the holder may use; `slack` more elements may lie behind them that belong to the allocation and not to the capacity (the raw signal's
// 64 samples past the end).
template <class T> struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    // a fresh allocation of (n + slack) * sizeof(T) bytes (n == 0: one element); whatever was held is freed first
    hipError_t alloc(size_t n, size_t slack = 0) {
        release();
        if (!n) n = 1;
        const hipError_t e = hipMalloc((void **)&p, (n + slack) * sizeof(T));
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = n;
        return hipSuccess;
    }
    // grows only.  A growth that fails leaves the buffer EMPTY (cap 0), never a capacity without memory behind it: the next call
    // allocates again
    hipError_t reserve(size_t n, size_t slack = 0) { return n <= cap ? hipSuccess : alloc(n, slack); }
};

// The one owner of timing events (the process-wide reference event of unc_host.cpp apart).  create(n) makes events until there are n: a fixed set is made once, a growing
// one as it grows.  The hipError_t of every member goes through HIPCHK at the call, as DevBuf's do.
struct DevEvents {
    std::vector<hipEvent_t> e;
    DevEvents() = default;
    DevEvents(const DevEvents &) = delete;
    DevEvents &operator=(const DevEvents &) = delete;
    ~DevEvents() { for (hipEvent_t x : e) (void)hipEventDestroy(x); }
    hipError_t create(size_t n) {
        for (hipEvent_t x = nullptr; e.size() < n; e.push_back(x))
            if (hipError_t rc = hipEventCreate(&x)) return rc;
        return hipSuccess;
    }
    hipError_t record(size_t i, hipStream_t st) { return hipEventRecord(e[i], st); }
    // milliseconds from event i to event j, once the stream has been waited for
    hipError_t elapsed(size_t i, size_t j, float *ms) { return hipEventElapsedTime(ms, e[i], e[j]); }
};

// The one owner of a stream, in the same style: made once, destroyed with its holder.
struct DevStream {
    hipStream_t s = nullptr;
    DevStream() = default;
    DevStream(const DevStream &) = delete;
    DevStream &operator=(const DevStream &) = delete;
    ~DevStream() { if (s) (void)hipStreamDestroy(s); }
    hipError_t create() { return hipStreamCreate(&s); }
};

// n elements of a device array into h, queued on the stream and not waited for
template <class T> hipError_t download(std::vector<T> &h, const T *d, size_t n, hipStream_t st) {
    h.resize(n);
    return n ? hipMemcpyAsync(h.data(), d, n * sizeof(T), hipMemcpyDeviceToHost, st) : hipSuccess;
}

// The hand-over of a per-query output: one copy of the whole device array, waited for, then count(q) elements from element src(q)
// of it to dst(q) for every query.  Nothing outside a query's count is written
template <class T, class Count, class Src, class Dst>
hipError_t deal_out(const T *d, size_t n, hipStream_t st, uint32_t n_queries, Count count, Src src, Dst dst) {
    std::vector<T> h;
    if (hipError_t rc = download(h, d, n, st)) return rc;
    if (hipError_t rc = hipStreamSynchronize(st)) return rc;
    for (uint32_t q = 0; q < n_queries; ++q) memcpy(dst(q), h.data() + src(q), (size_t)count(q) * sizeof(T));
    return hipSuccess;
}
