// Host-side helpers shared by the translation units behind the C ABI (unc_host.cpp, unc_dtw.cpp): the error message of the calling
// thread and the one owner of device memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/uncalled_hip.h"

namespace unc {
// stores the message unc_last_error() returns to the calling thread and returns `code` (defined in unc_host.cpp)
int fail(int code, const char *fmt, ...);
// the HIP device an index was loaded to (defined in unc_host.cpp, which owns the struct)
int index_device(const unc_index_t *ix);
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
