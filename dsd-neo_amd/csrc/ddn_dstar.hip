// ddn_dstar.hip - D-STAR frames behind the fsk4 loop's syncs (DDN_FSK4_DSTAR, the reference's -fd): the radio header and the voice
// superframe (21 AMBE frames and the slow data).
//
// reference: src/protocol/dstar/dstar.c - processDSTAR() :21-66 (21 x 72 voice dibits, each frame followed - but the last - by 24
// slow-data dibits), processDSTAR_HD() :68-80 (660 soft symbols first); dstar_header.c / dstar_header_utils.c:11-184 (soft cost,
// PN x^7 + x^4 + 1 seeded 0x07, the 24-stride de-interleave, the 4-state soft Viterbi, 41 octets LSB first, dstar_crc16);
// dstar_slow_data.c:56-441 (processDSTAR_SD() without APRS); the two-level slice digitize() src/core/frames/dsd_dibit.c:892-948,1019-1029
// and gmsk_soft_symbol_to_viterbi_cost() :1150-1167,1245-1281.  One wavefront per sync slot in both kernels.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddn_api_util.h"
#include "ddn_crc_dev.h"
#include "ddn_expf.h"
#include "ddn_fsk4.h"
#include "ddn_internal.h"
#include "ddn_tables_dstar.h"

namespace {

constexpr int kCoded = DDN_DSTAR_HEADER_CODED, kInfo = kCoded / 2, kVoice = DDN_DSTAR_VOICE_SYMBOLS;
constexpr int kFrames = 21, kFrameCells = 4 * 24;
__constant__ uint8_t c_dstar_map[72][2] = DDN_DSTAR_AMBE_MAP_INIT;

__device__ __forceinline__ float
rec_symbol(const uint8_t* r) { // bytes 6..9 of a 10-byte record (2-byte aligned)
    const uint32_t xb = (uint32_t)((const uint16_t*)r)[3] | ((uint32_t)((const uint16_t*)r)[4] << 16);
    return __uint_as_float(xb);
}

// gmsk_soft_symbol_to_viterbi_cost(): thr = {center, umid, lmid, max, min}; 0 = a strong 0, 65535 = a strong 1 (a high symbol)
__device__ __forceinline__ uint32_t
gmsk_cost(float symbol, const float* thr) {
    const float center = thr[0];
    float max_val = thr[3], min_val = thr[4];
    if (!(min_val < center && center < max_val)) {
        float span = max_val - min_val;
        if (span < 1e-3f) {
            span = 2.0f;
        }
        const float half = span * 0.5f;
        min_val = center - half;
        max_val = center + half;
    }
    const float mu0 = 0.5f * (min_val + center), mu1 = 0.5f * (center + max_val);
    float sigma = (max_val - min_val) / 4.0f;
    if (sigma < 1e-3f) {
        sigma = 1e-3f;
    }
    const float inv_2sigma2 = 0.5f / (sigma * sigma);
    const float d0 = symbol - mu0, d1 = symbol - mu1;
    const float llr = ((d1 * d1) - (d0 * d0)) * inv_2sigma2;
    if (llr >= 16.0f) {
        return 0u;
    }
    if (llr <= -16.0f) {
        return 65535u;
    }
    const float pr1 = 1.0f / (1.0f + ddn_expf(llr));
    long long q = __float2ll_rn(pr1 * 65535.0f); // lrintf
    q = q < 0 ? 0 : (q > 65535 ? 65535 : q);
    return (uint32_t)q;
}

__device__ __forceinline__ bool
header_crc_ok(const uint8_t* h41) { // dstar_crc16() over 39 octets; the frame carries the low byte first
    return ddn_crc::of_bytes(ddn_crc::DSTAR_X25, h41, 39) == (((uint32_t)h41[40] << 8) | h41[39]);
}

// slot (ch, k) of the loop's outputs: its pattern row and first symbol, or false when the slot holds no sync / its part is not inside
// this call's records
__device__ __forceinline__ bool
slot_unit(const int32_t* counts, size_t stride, const int32_t* sync_pos, const uint8_t* sync_pat, const int32_t* n_sync, int max_syncs,
          int ch, int k, int pre, int len, bool header_only, int* pos, int* pat) {
    if (k >= n_sync[ch] || k >= max_syncs) {
        return false;
    }
    const size_t slot = (size_t)ch * max_syncs + k;
    *pos = sync_pos[slot];
    *pat = sync_pat[slot];
    if (*pat > 3 || (header_only && *pat < 2) || *pos < 0) {
        return false;
    }
    const long have = counts[ch] < (long)stride ? (long)counts[ch] : (long)stride;
    const int off = *pat >= 2 ? pre : 0;
    return (long)*pos + 1 + off + len <= have;
}

__global__ __launch_bounds__(64) void
k_dstar_header(const uint8_t* __restrict__ rec, size_t stride, const int32_t* __restrict__ counts, const int32_t* __restrict__ sync_pos,
               const uint8_t* __restrict__ sync_pat, const int32_t* __restrict__ n_sync, const float* __restrict__ sync_thr, int max_syncs,
               uint8_t* __restrict__ hdr41, uint8_t* __restrict__ crc_ok, uint8_t* __restrict__ valid) {
    __shared__ uint16_t cost[kCoded]; // descrambled, de-interleaved
    __shared__ uint8_t dec[kInfo][4];
    __shared__ uint8_t bits[kInfo];
    __shared__ uint8_t h[41];
    const int ch = blockIdx.y, k = blockIdx.x, lane = threadIdx.x;
    const size_t slot = (size_t)ch * max_syncs + k;
    int pos = 0, pat = 0;
    if (!slot_unit(counts, stride, sync_pos, sync_pat, n_sync, max_syncs, ch, k, 0, kCoded, true, &pos, &pat)) {
        if (lane < 41) {
            hdr41[slot * 41 + lane] = 0;
        }
        if (lane == 0) {
            crc_ok[slot] = 0;
            valid[slot] = 0;
        }
        return;
    }
    // the two generators.  PN x^7 + x^4 + 1 seeded 0x07, MSb out: the 127-bit period as a mask in registers (the same on every lane).
    // The 24-stride de-interleave (out[k_i] = in[i], k += 24, -671 past 671, -647 past 659) in closed form: the coded bits lie in 24
    // columns, columns 0..11 28 deep and 12..23 27 deep, and air bit i walks them column by column.
    uint64_t pn_lo = 0, pn_hi = 0;
    {
        unsigned reg = 0x07u;
        for (int i = 0; i < 127; i++) {
            const uint64_t b = (reg >> 6) & 1u;
            if (i < 64) {
                pn_lo |= b << i;
            } else {
                pn_hi |= b << (i - 64);
            }
            const unsigned fb = ((reg >> 6) ^ (reg >> 3)) & 1u;
            reg = ((reg << 1) & 0x7Eu) | fb;
        }
    }
    const float* thr = sync_thr + slot * 5;
    const uint8_t* r0 = rec + ((size_t)ch * stride + (size_t)pos + 1) * 10;
    for (int i = lane; i < kCoded; i += 64) {
        const uint32_t c = gmsk_cost(rec_symbol(r0 + (size_t)i * 10), thr);
        const int m = i % 127;
        const bool flip = ((m < 64 ? pn_lo >> m : pn_hi >> (m - 64)) & 1u) != 0;
        const int perm = i < 12 * 28 ? (i / 28) + 24 * (i % 28) : 12 + (i - 12 * 28) / 27 + 24 * ((i - 12 * 28) % 27);
        cost[perm] = (uint16_t)(flip ? (0xFFFFu - c) : c);
    }
    __syncthreads();
    // add-compare-select: lane st < 4 holds state st's path metric; predecessors {0, 2} for states 0 / 1, {1, 3} for 2 / 3; the first
    // candidate's references {0,0} {1,1} {1,0} {0,1}, the second's their complements; ties keep the first
    const int st = lane & 3;
    const uint32_t r1 = (st == 1 || st == 2) ? 1u : 0u, r0b = (st == 1 || st == 3) ? 1u : 0u;
    uint32_t pm = 0;
    for (int n = 0; n < kInfo; n++) {
        const uint32_t s1 = cost[2 * n], s0 = cost[2 * n + 1];
        const uint32_t pa = (uint32_t)__shfl((int)pm, st < 2 ? 0 : 1, 64), pb = (uint32_t)__shfl((int)pm, st < 2 ? 2 : 3, 64);
        const uint32_t ba = (r1 ? 0xFFFFu - s1 : s1) + (r0b ? 0xFFFFu - s0 : s0);
        const uint32_t bb = (r1 ? s1 : 0xFFFFu - s1) + (r0b ? s0 : 0xFFFFu - s0);
        const uint32_t ma = ba + pa, mb = bb + pb;
        const int d = ma <= mb ? 0 : 1;
        pm = d ? mb : ma;
        if (lane < 4) {
            dec[n][st] = (uint8_t)d;
        }
    }
    const uint32_t m0 = (uint32_t)__shfl((int)pm, 0, 64), m1 = (uint32_t)__shfl((int)pm, 1, 64);
    const uint32_t m2 = (uint32_t)__shfl((int)pm, 2, 64), m3 = (uint32_t)__shfl((int)pm, 3, 64);
    __syncthreads();
    if (lane == 0) {
        int s = 0;
        uint32_t best = m0;
        if (m1 < best) {
            best = m1;
            s = 1;
        }
        if (m2 < best) {
            best = m2;
            s = 2;
        }
        if (m3 < best) {
            s = 3;
        }
        for (int i = kInfo - 1; i >= 0; i--) {
            bits[i] = (uint8_t)(s & 1);
            s = (s >> 1) + 2 * dec[i][s];
        }
    }
    __syncthreads();
    if (lane < 41) {
        uint8_t o = 0;
        for (int b = 0; b < 8; b++) {
            o |= (uint8_t)(bits[8 * lane + b] << b);
        }
        h[lane] = o;
        hdr41[slot * 41 + lane] = o;
    }
    __syncthreads();
    if (lane == 0) {
        crc_ok[slot] = (uint8_t)(header_crc_ok(h) ? 1 : 0);
        valid[slot] = 1;
    }
}

__device__ __forceinline__ uint8_t
sanitized(const uint8_t* b, int i) { // dstar_sd_sanitize_bytes() for byte i >= 1, reading the unsanitised neighbour
    uint8_t v = b[i];
    if (v < 0x20 || v > 0x7E) {
        v = 0x20;
    }
    if (v == 0x66 && (i == 59 || b[i + 1] == 0x66)) {
        v = 0; // (a 0x66 neighbour is never rewritten before it is read: the pass runs upwards and 0x66 survives the range rule)
    }
    return v;
}

__global__ __launch_bounds__(64) void
k_dstar_voice(const uint8_t* __restrict__ rec, size_t stride, const int32_t* __restrict__ counts, const int32_t* __restrict__ sync_pos,
              const uint8_t* __restrict__ sync_pat, const int32_t* __restrict__ n_sync, const float* __restrict__ sync_thr, int max_syncs,
              uint8_t* __restrict__ ambe, uint8_t* __restrict__ sd_bytes, uint8_t* __restrict__ sd_kind, uint8_t* __restrict__ sd_hdr41,
              uint8_t* __restrict__ sd_crc_ok, uint8_t* __restrict__ sd_text, uint8_t* __restrict__ valid) {
    __shared__ uint8_t fr[kFrames * kFrameCells];
    __shared__ uint8_t sd[480];
    __shared__ uint8_t by[60], hd[60], sb[60];
    const int ch = blockIdx.y, k = blockIdx.x, lane = threadIdx.x;
    const size_t slot = (size_t)ch * max_syncs + k;
    int pos = 0, pat = 0;
    uint8_t* a_out = ambe + slot * (kFrames * kFrameCells);
    if (!slot_unit(counts, stride, sync_pos, sync_pat, n_sync, max_syncs, ch, k, kCoded, kVoice, false, &pos, &pat)) {
        for (int i = lane; i < kFrames * kFrameCells; i += 64) {
            a_out[i] = 0;
        }
        if (lane < 60) {
            sd_bytes[slot * 60 + lane] = 0;
            sd_text[slot * 60 + lane] = 0;
        }
        if (lane < 41) {
            sd_hdr41[slot * 41 + lane] = 0;
        }
        if (lane == 0) {
            sd_kind[slot] = 0;
            sd_crc_ok[slot] = 0;
            valid[slot] = 0;
        }
        return;
    }
    for (int i = lane; i < kFrames * kFrameCells; i += 64) {
        fr[i] = 0;
    }
    __syncthreads();
    // the two-level slice: positive word -> (symbol > center ? 0 : 1), negative word -> the complement
    const float center = sync_thr[slot * 5];
    const uint8_t flip = (uint8_t)(pat & 1);
    const uint8_t* r0 = rec + ((size_t)ch * stride + (size_t)pos + 1 + (pat >= 2 ? kCoded : 0)) * 10;
    for (int t = lane; t < kVoice; t += 64) {
        const uint8_t b = (uint8_t)((rec_symbol(r0 + (size_t)t * 10) > center ? 0 : 1) ^ flip);
        const int j = t / 96, r = t - 96 * j;
        if (r < 72) {
            fr[j * kFrameCells + c_dstar_map[r][0] * 24 + c_dstar_map[r][1]] = b;
        } else {
            sd[j * 24 + r - 72] = b;
        }
    }
    __syncthreads();
    for (int i = lane; i < kFrames * kFrameCells; i += 64) {
        a_out[i] = fr[i];
    }
    if (lane < 60) { // descramble, reverse, pack MSB first: byte 59 - i from reversed bits 8 i .. 8 i + 7
        uint8_t o = 0;
        for (int b = 0; b < 8; b++) {
            const int src = 479 - (8 * lane + b);
            const uint8_t pbit = (uint8_t)((DDN_DSTAR_SD_PATTERN >> (23 - src % 24)) & 1u);
            o = (uint8_t)((o << 1) | (sd[src] ^ pbit));
        }
        by[59 - lane] = o;
        sd_bytes[slot * 60 + 59 - lane] = o;
    }
    __syncthreads();
    if (lane == 0) { // the truncated-payload reload (bytes that sit at multiples of the payload length are skipped)
        const int len = (by[0] & 0xF) + 1;
        for (int i = 0, j = 0; i < 60; i++) {
            if (i < 50) {
                j++;
                hd[i] = by[j];
                for (int m = 1; m <= 9; m++) {
                    if (j == len * m - 1) {
                        j++;
                    }
                }
            } else {
                hd[i] = 0;
            }
        }
        sd_crc_ok[slot] = (uint8_t)(header_crc_ok(hd) ? 1 : 0);
        sb[0] = by[0];
    }
    __syncthreads();
    if (lane < 41) {
        sd_hdr41[slot * 41 + lane] = hd[lane];
    }
    if (lane >= 1 && lane < 60) {
        sb[lane] = sanitized(by, lane);
    }
    __syncthreads();
    // kind: 0x55 header format, 0x40 text, 0x35 fixed form (its "$$CRC" type is APRS: not decoded here, no text); dstar_txt's 60 bytes
    const uint8_t m0 = sb[0];
    const bool aprs = m0 == 0x35 && sb[1] == '$' && sb[2] == '$' && sb[3] == 'C' && sb[4] == 'R' && sb[5] == 'C';
    const int kind = m0 == 0x55 ? 1 : (m0 == 0x40 ? 2 : (m0 == 0x35 ? 3 : 0));
    const bool has_text = (kind == 2 || kind == 3) && !aprs;
    if (lane < 60) {
        uint8_t t = 0;
        if (has_text) {
            t = 0x20;
            if (lane == 59) {
                t = 0;
            } else if (lane >= 1 && lane % 6 != 0 && sb[lane] > 0x19 && sb[lane] < 0x7F) {
                t = sb[lane];
            }
        }
        sd_text[slot * 60 + lane] = t;
    }
    if (lane == 0) {
        sd_kind[slot] = (uint8_t)kind;
        valid[slot] = 1;
    }
}

} // namespace

extern "C" int
ddn_dstar_header_decode_batch(const uint8_t* d_records10, size_t stride_symbols, const int32_t* d_counts, const int32_t* d_sync_pos,
                              const uint8_t* d_sync_pat, const int32_t* d_n_sync, const float* d_sync_thr5, int n_channels, size_t max_syncs,
                              uint8_t* d_hdr41, uint8_t* d_hdr_crc_ok, uint8_t* d_valid, void* hip_stream) {
    if (n_channels < 0 || n_channels > 65535 || max_syncs > 65535) { // (grid x = sync slot, y = channel)
        ddn_set_error("ddn_dstar_header_decode_batch: bad arguments (n_channels and max_syncs at most 65535)");
        return DDN_EINVAL;
    }
    if (n_channels == 0 || max_syncs == 0) {
        return DDN_OK;
    }
    if (!d_records10 || !d_counts || !d_sync_pos || !d_sync_pat || !d_n_sync || !d_sync_thr5 || !d_hdr41 || !d_hdr_crc_ok || !d_valid) {
        ddn_set_error("ddn_dstar_header_decode_batch: null pointer");
        return DDN_EINVAL;
    }
    hipLaunchKernelGGL(k_dstar_header, dim3((unsigned)max_syncs, (unsigned)n_channels), dim3(64), 0, (hipStream_t)hip_stream, d_records10,
                       stride_symbols, d_counts, d_sync_pos, d_sync_pat, d_n_sync, d_sync_thr5, (int)max_syncs, d_hdr41, d_hdr_crc_ok, d_valid);
    DDN_LAUNCH_TRY(hipGetLastError());
    return DDN_OK;
}

extern "C" int
ddn_dstar_voice_decode_batch(const uint8_t* d_records10, size_t stride_symbols, const int32_t* d_counts, const int32_t* d_sync_pos,
                             const uint8_t* d_sync_pat, const int32_t* d_n_sync, const float* d_sync_thr5, int n_channels, size_t max_syncs,
                             uint8_t* d_ambe_fr, uint8_t* d_sd_bytes, uint8_t* d_sd_kind, uint8_t* d_sd_hdr41, uint8_t* d_sd_crc_ok,
                             uint8_t* d_sd_text, uint8_t* d_valid, void* hip_stream) {
    if (n_channels < 0 || n_channels > 65535 || max_syncs > 65535) { // (grid x = sync slot, y = channel)
        ddn_set_error("ddn_dstar_voice_decode_batch: bad arguments (n_channels and max_syncs at most 65535)");
        return DDN_EINVAL;
    }
    if (n_channels == 0 || max_syncs == 0) {
        return DDN_OK;
    }
    if (!d_records10 || !d_counts || !d_sync_pos || !d_sync_pat || !d_n_sync || !d_sync_thr5 || !d_ambe_fr || !d_sd_bytes || !d_sd_kind
        || !d_sd_hdr41 || !d_sd_crc_ok || !d_sd_text || !d_valid) {
        ddn_set_error("ddn_dstar_voice_decode_batch: null pointer");
        return DDN_EINVAL;
    }
    hipLaunchKernelGGL(k_dstar_voice, dim3((unsigned)max_syncs, (unsigned)n_channels), dim3(64), 0, (hipStream_t)hip_stream, d_records10,
                       stride_symbols, d_counts, d_sync_pos, d_sync_pat, d_n_sync, d_sync_thr5, (int)max_syncs, d_ambe_fr, d_sd_bytes,
                       d_sd_kind, d_sd_hdr41, d_sd_crc_ok, d_sd_text, d_valid);
    DDN_LAUNCH_TRY(hipGetLastError());
    return DDN_OK;
}
