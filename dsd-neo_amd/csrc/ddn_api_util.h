// ddn_api_util.h - what every C-ABI translation unit of libdsdneo_hip.so repeats: the error macros, the device check, the owner of
// an object's device buffers (DdnPool), the staging of a host-buffer variant's arguments (DdnStaged) and the stream-ordered scratch
// of a batched call (DdnScratch).  Host code only (not installed).
#ifndef DDN_API_UTIL_H
#define DDN_API_UTIL_H

#include <hip/hip_runtime.h>
#include <stdlib.h>

#include "ddn_internal.h"

// the library's code for a failed HIP call (include/ddn_hip.h): no device or no code object, out of memory, anything else
static inline int
ddn_hip_code(hipError_t e) {
    return (e == hipErrorNoDevice || e == hipErrorInvalidDevice || e == hipErrorNoBinaryForGpu) ? DDN_ENODEV
                                                                                                : (e == hipErrorOutOfMemory ? DDN_ENOMEM : DDN_EHIP);
}

// leave the calling function with the library's code for a failed HIP call (the message names the call and where it stands)
#define HIP_TRY(expr)                                                                                                  \
    do {                                                                                                               \
        hipError_t e_ = (expr);                                                                                        \
        if (e_ != hipSuccess) {                                                                                        \
            ddn_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);                  \
            return ddn_hip_code(e_);                                                                                   \
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

// DDN_OK where a HIP device is there; the answer of every create() and of the calls that say so before they launch
static inline int
ddn_have_device() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        ddn_set_error("no HIP device available");
        return DDN_ENODEV;
    }
    return DDN_OK;
}

// the answer to a bad argument, for the check a batched call shares with its host-buffer variant: `who` names the pair
static inline int
ddn_bad_argument(const char* who) {
    ddn_set_error("%s: bad argument", who);
    return DDN_EINVAL;
}

// 1 where a tap set holds a zero (the FIR kernels then take the path that keeps the reference's skipped products)
static inline int
taps_have_zero(const float* taps, int n) {
    for (int i = 0; i < n; i++) {
        if (taps[i] == 0.0f) {
            return 1;
        }
    }
    return 0;
}

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

    // a buffer that is replaced during the object's life (a longer call, a re-armed list): frees the entry that holds *p and
    // allocates anew in its place (a new entry where *p is null); *p is null after a failure
    template <typename T>
    hipError_t
    realloc_bytes(T** p, size_t bytes) {
        size_t k = 0;
        while (k < n && bufs[k] != (void*)*p) {
            k++;
        }
        if (!*p || k == n) {
            return alloc_bytes(p, bytes);
        }
        (void)hipFree(bufs[k]);
        bufs[k] = bufs[--n]; // (the list keeps no order: the last entry takes the freed one's place)
        *p = nullptr;
        return alloc_bytes(p, bytes);
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

// The arguments of a host-buffer variant (`_host`), staged through the device: every buffer comes from a pool of the call's own
// (zero-filled, 16 bytes of slack, so a request of zero bytes is a valid pointer too) and leaves with the call, on every path.
// Sizes are in bytes.  The first HIP error is kept and every later request answers null: a variant stages, asks staged(), runs
// its batched twin on the null stream and returns finish().
struct __attribute__((visibility("hidden"))) DdnStaged {
    DdnPool pool = {};
    struct {
        void* host;
        const void* dev;
        size_t bytes;
    } back[16];
    int n_back = 0;
    hipError_t err = hipSuccess;

    DdnStaged() = default;
    DdnStaged(const DdnStaged&) = delete;
    DdnStaged& operator=(const DdnStaged&) = delete;
    ~DdnStaged() { pool.release(); }

    // an input: allocated and uploaded
    template <typename T>
    T*
    in(const T* h, size_t bytes) {
        return (T*)stage(h, nullptr, bytes);
    }

    // an optional input: no host pointer, no buffer
    template <typename T>
    T*
    in_opt(const T* h, size_t bytes) {
        return h ? in(h, bytes) : nullptr;
    }

    // an output: zero-filled, downloaded by finish() where the caller gave a host pointer (the device pointer is valid without)
    template <typename T>
    T*
    out(T* h, size_t bytes) {
        return (T*)stage(nullptr, h, bytes);
    }

    // uploaded, then downloaded by finish(); without a host pointer it is the zero-filled buffer of out()
    template <typename T>
    T*
    inout(T* h, size_t bytes) {
        return (T*)stage(h, h, bytes);
    }

    int
    staged() {
        if (err != hipSuccess) {
            ddn_set_error("staging host buffers through the device failed: %s", hipGetErrorString(err));
            return ddn_hip_code(err);
        }
        return DDN_OK;
    }

    // the downloads (behind the null stream's work); the library's code for the first error of the call's staging
    int
    finish() {
        for (int k = 0; k < n_back && err == hipSuccess; k++) {
            err = hipMemcpy(back[k].host, back[k].dev, back[k].bytes, hipMemcpyDeviceToHost);
        }
        return staged();
    }

  private:
    void*
    stage(const void* up, void* down, size_t bytes) {
        uint8_t* d = nullptr;
        if (err != hipSuccess) {
            return nullptr;
        }
        if (down && bytes && n_back == (int)(sizeof(back) / sizeof(back[0]))) {
            err = hipErrorOutOfMemory;
            return nullptr;
        }
        err = pool.alloc_bytes(&d, bytes + 16);
        if (err == hipSuccess) {
            err = hipMemset(d, 0, bytes + 16);
        }
        if (err == hipSuccess && up && bytes) {
            err = hipMemcpy(d, up, bytes, hipMemcpyHostToDevice);
        }
        if (err != hipSuccess) {
            return nullptr;
        }
        if (down && bytes) {
            back[n_back].host = down;
            back[n_back].dev = d;
            back[n_back].bytes = bytes;
            n_back++;
        }
        return d;
    }
};

// The scratch of one batched call, stream-ordered so that concurrent calls on different streams never share it: arenas (one
// hipMallocAsync each, carved by get() in steps of 256 bytes), released in stream order when the call leaves, also on its error paths
struct __attribute__((visibility("hidden"))) DdnScratch {
    hipStream_t st;
    void* p[4];
    int n = 0;
    uint8_t* cur = nullptr;
    size_t left = 0;
    explicit DdnScratch(hipStream_t s) : st(s) {}
    DdnScratch(const DdnScratch&) = delete;
    DdnScratch& operator=(const DdnScratch&) = delete;
    ~DdnScratch() {
        for (int i = 0; i < n; i++) {
            (void)hipFreeAsync(p[i], st);
        }
    }
    hipError_t arena(size_t bytes) {
        void* q = nullptr;
        const hipError_t e = n < 4 ? hipMallocAsync(&q, bytes + 256, st) : hipErrorOutOfMemory;
        if (e == hipSuccess) {
            p[n++] = q;
            cur = (uint8_t*)q;
            left = bytes + 256;
        }
        return e;
    }
    static size_t pad(size_t b) { return (b + 255) & ~(size_t)255; }
    template <class T>
    hipError_t get(T** out, size_t count) {
        const size_t b = pad((count ? count : 1) * sizeof(T));
        if (b > left) {
            *out = nullptr;
            return hipErrorOutOfMemory;
        }
        *out = (T*)cur;
        cur += b;
        left -= b;
        return hipSuccess;
    }
};

#endif
