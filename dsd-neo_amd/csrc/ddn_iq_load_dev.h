/* ddn_iq_load_dev.h — input widening on the device: one raw complex sample of any input format -> (I, Q) as binary32.
 * The one place the kernels that take raw I/Q (ddn_front_end.hip, ddn_halfband.hip, ddn_cqpsk.hip) get it from.
 *
 *   DDN_IN_CU8   two bytes, I then Q:              (float(u) - 127.5f) * (1.0f / 127.5f)
 *                                                  widen_u8_to_f32_bias127, src/dsp/simd_widen.cpp:139-149
 *   DDN_IN_CS16  two little-endian int16, I then Q: float(s) * (1.0f / 32768.0f)
 *                                                  soapy_copy_cs16_samples, src/io/radio/rtl_device.cpp:1247-1264, scale :1316
 *   DDN_IN_CF32  two floats, I then Q:              as they are
 *
 * Every int16 is exact in binary32 and the scale is a power of two, so the cs16 result is exact: the same bits as the cf32 path
 * fed float(s) * 2^-15, however it is computed.
 *
 * A kernel that fetches ahead of use keeps the RAW sample in a register (ddn_iq_fetch) and widens it where it is consumed
 * (ddn_iq_unpack): cu8 and cs16 both ride one 32-bit register per sample (cu8 in its low half), cf32 rides the float pair.
 * cs16 is ONE aligned dword load per complex sample; the sample array must therefore be 4-byte aligned (the API checks). */
#ifndef DDN_IQ_LOAD_DEV_H
#define DDN_IQ_LOAD_DEV_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddn_internal.h"

typedef float ddn_iq_f2 __attribute__((ext_vector_type(2)));

/* the raw sample `idx` of a cu8 / cs16 array in one register */
template <int FMT>
__device__ __forceinline__ uint32_t
ddn_iq_fetch(const void* base, size_t idx) {
    static_assert(FMT == DDN_IN_CU8 || FMT == DDN_IN_CS16, "cf32 samples are fetched as float pairs");
    if constexpr (FMT == DDN_IN_CU8) {
        return ((const uint16_t*)base)[idx];
    } else {
        return ((const uint32_t*)base)[idx];
    }
}

template <int FMT>
__device__ __forceinline__ ddn_iq_f2
ddn_iq_unpack(uint32_t r) {
    static_assert(FMT == DDN_IN_CU8 || FMT == DDN_IN_CS16, "cf32 samples need no unpacking");
    ddn_iq_f2 v;
    if constexpr (FMT == DDN_IN_CU8) {
        const float inv = 1.0f / 127.5f;
        v.x = ((float)(r & 0xFF) - 127.5f) * inv;
        v.y = ((float)(r >> 8) - 127.5f) * inv; /* (ddn_iq_fetch zero-extends the 16 bits: nothing above the Q byte) */
    } else {
        /* low half I, high half Q, both SIGNED: a sign-extending extract of the low half, an arithmetic shift of the high one */
        const int32_t s = (int32_t)r;
        const float scale = 1.0f / 32768.0f;
        v.x = (float)(int32_t)(int16_t)s * scale;
        v.y = (float)(s >> 16) * scale;
    }
    return v;
}

template <int FMT>
__device__ __forceinline__ ddn_iq_f2
ddn_iq_load(const void* base, size_t idx) {
    if constexpr (FMT == DDN_IN_CF32) {
        return ((const ddn_iq_f2*)base)[idx];
    } else {
        return ddn_iq_unpack<FMT>(ddn_iq_fetch<FMT>(base, idx));
    }
}

/* format known at run time only (the carry kernel); the caller has refused unknown formats */
__device__ __forceinline__ ddn_iq_f2
ddn_iq_load_rt(const void* base, int fmt, size_t idx) {
    if (fmt == DDN_IN_CU8) {
        return ddn_iq_load<DDN_IN_CU8>(base, idx);
    }
    if (fmt == DDN_IN_CS16) {
        return ddn_iq_load<DDN_IN_CS16>(base, idx);
    }
    return ddn_iq_load<DDN_IN_CF32>(base, idx);
}

#endif
