// ddn_gf64_dev.h - GF(2^6) over x^6 + x + 1, the field of every P25 block code here: BCH(63,16,11) of the NID (ddn_nid_dev.h),
// the Phase 1 Reed-Solomon codes and the Phase 2 RS(63,35) sections (ddn_rs.hip).  exp / log tables in LDS (per-lane random
// access), and the 6-bit "hex" symbols of the reference's one-bit-per-byte arrays.
#ifndef DDN_GF64_DEV_H
#define DDN_GF64_DEV_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ddn_gf64 {

struct Gf {
    const uint8_t* ex; // [128]: alpha^i, i = 0 .. 127 (two periods, so a sum of two logarithms indexes it directly)
    const uint8_t* lg; // [64]
    __device__ __forceinline__ int mul(int a, int b) const { return (a && b) ? ex[lg[a] + lg[b]] : 0; }
    __device__ __forceinline__ int div(int a, int b) const { return a ? ex[lg[a] + 63 - lg[b]] : 0; }
    __device__ __forceinline__ int mul_exp(int a, int e) const { return a ? ex[(lg[a] + e) % 63] : 0; } // a * alpha^e, e >= 0
};

__device__ inline void
gf_fill(uint8_t* ex, uint8_t* lg) { // one thread
    int x = 1;
    for (int i = 0; i < 63; i++) {
        ex[i] = (uint8_t)x;
        ex[i + 63] = (uint8_t)x;
        lg[x] = (uint8_t)i;
        x <<= 1;
        if (x & 64) {
            x ^= 0x43; // x^6 = x + 1
        }
    }
    ex[126] = ex[0];
    ex[127] = ex[1];
    lg[0] = 0;
}

// the workgroup's table: thread 0 fills it, everyone waits (every thread of the workgroup calls this)
__device__ __forceinline__ void
gf_fill_wg(uint8_t* ex, uint8_t* lg) {
    if (threadIdx.x == 0) {
        gf_fill(ex, lg);
    }
    __syncthreads();
}

// six bytes, MSB first, any non-zero byte a one -> symbol
__device__ __forceinline__ int
hex_pack(const uint8_t* q) {
    int v = 0;
#pragma unroll
    for (int b = 0; b < 6; b++) {
        v = (v << 1) | (q[b] != 0);
    }
    return v;
}

// symbol -> six 0/1 bytes, MSB first
__device__ __forceinline__ void
hex_unpack(int v, uint8_t* q) {
#pragma unroll
    for (int b = 0; b < 6; b++) {
        q[b] = (uint8_t)((v >> (5 - b)) & 1);
    }
}

} // namespace ddn_gf64
#endif
