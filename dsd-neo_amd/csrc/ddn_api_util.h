// ddn_api_util.h - what every C-ABI translation unit of libdsdneo_hip.so repeats: the error macros and the owner of a chain object's
// device buffers.  Host code only (not installed).
#ifndef DDN_API_UTIL_H
#define DDN_API_UTIL_H

#include <hip/hip_runtime.h>
#include <stdlib.h>

#include "ddn_internal.h"

// leave the calling function with the library's code for a failed HIP call (the message names the call and where it stands)
#define HIP_TRY(expr)                                                                                                  \
    do {                                                                                                               \
        hipError_t e_ = (expr);                                                                                        \
        if (e_ != hipSuccess) {                                                                                        \
            ddn_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);                  \
            return (e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice || e_ == hipErrorNoBinaryForGpu)             \
                       ? DDN_ENODEV                                                                                    \
                       : (e_ == hipErrorOutOfMemory ? DDN_ENOMEM : DDN_EHIP);                                          \
        }                                                                                                              \
    } while (0)
// ... and with the code of a failed library call (its message stands)
#define DDN_TRY(expr)                                                                                                  \
    do {                                                                                                               \
        const int rc_ = (expr);                                                                                        \
        if (rc_ != DDN_OK) {                                                                                           \
            return rc_;                                                                                                \
        }                                                                                                              \
    } while (0)
// HIP_TRY as the dPMR / D-STAR / EDACS batch calls report a failed launch: no place in the message, and a missing device or code
// object is DDN_EHIP like every other failure but out-of-memory
#define DDN_LAUNCH_TRY(expr)                                                                                           \
    do {                                                                                                               \
        const hipError_t e_ = (expr);                                                                                  \
        if (e_ != hipSuccess) {                                                                                        \
            ddn_set_error("%s failed: %s", #expr, hipGetErrorString(e_));                                              \
            return e_ == hipErrorOutOfMemory ? DDN_ENOMEM : DDN_EHIP;                                                  \
        }                                                                                                              \
    } while (0)

// The device buffers of one object: every buffer its own hipMalloc with 16 bytes of slack behind it (kernels may read past an
// array's end into the slack), zero-filled, all freed together.  All-zero is the empty pool; release() leaves it empty, so it may
// run twice, after a create that failed half way, and before the pool is filled again.
struct __attribute__((visibility("hidden"))) DdnPool {
    void** bufs;
    size_t n, cap;

    // exactly `bytes`, not cleared: the buffers made on first use
    template <typename T>
    hipError_t
    alloc_bytes(T** p, size_t bytes) {
        if (n == cap) {
            void** grown = (void**)realloc(bufs, (cap ? 2 * cap : 64) * sizeof(void*));
            if (!grown) {
                return hipErrorOutOfMemory;
            }
            bufs = grown;
            cap = cap ? 2 * cap : 64;
        }
        void* q = nullptr;
        const hipError_t e = hipMalloc(&q, bytes);
        if (e == hipSuccess) {
            bufs[n++] = q;
            *p = (T*)q;
        }
        return e;
    }

    template <typename T>
    bool
    alloc(T** p, size_t count) {
        return alloc_bytes(p, count * sizeof(T) + 16) == hipSuccess && hipMemset(*p, 0, count * sizeof(T)) == hipSuccess;
    }

    void
    release() {
        while (n) {
            (void)hipFree(bufs[--n]);
        }
        free(bufs);
        bufs = nullptr;
        cap = 0;
    }
};

#endif
