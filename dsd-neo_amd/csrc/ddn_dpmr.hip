// ddn_dpmr.hip - the dPMR voice superframe behind the fsk4 loop's FS2 syncs (DDN_FSK4_DPMR, the reference's -fm): the two control
// channels (CCH), the colour code, the identity rules and the eight AMBE 3600x2450 voice frames.
//
// reference: src/protocol/dpmr/dpmr_voice.c - processdPMRvoice() :397-425 (layout: CCH 36 dibits, 4 x 36 TCH, colour code 12, CCH 36,
// 4 x 36 TCH behind the 12-symbol sync), the CCH decode :139-178 (descramble x^9 + x^5 + 1 seeded 0x1FF per CCH, dpmr_data.c:80-117;
// 6 x 12 de-interleave :431-452; six Hamming(12,8) words; CRC7 over 41 bits :455-474), dpmr_extract_superframe_part() /
// dpmr_update_superframe_part() :180-274, dpmr_play_voice_frames() :354-395; dpmr_read_dibit() :67-73 (dibit ^ 2 under -xd).
// Hamming(12,8) is ddn_bcode_dev.h's, the code of the generic entry (ddn_fec3.hip), so the decode stays pinned with it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddn_api_util.h"
#include "ddn_bcode_dev.h"
#include "ddn_crc_dev.h"
#include "ddn_device.h"
#include "ddn_fec3.h"
#include "ddn_fsk4.h"
#include "ddn_internal.h"
#include "ddn_tables_ambe.h"
#include "ddn_tables_dpmr.h"

namespace {

constexpr int kFrame = 372;                                                  // dibits behind FS2
constexpr int kCch[2] = {0, 192}, kCc = 180;                                 // dibit offsets behind the sync
__constant__ uint16_t c_voice_at[8] = {36, 72, 108, 144, 228, 264, 300, 336}; // TCH frames
__constant__ uint8_t c_dpmr_ambe_map[36][4] = DDN_AMBE2450_MAP_INIT;
static_assert(DDN_DPMR_COLOR_CODES == 64, "colour-code table");

// the scrambler's output for an all-zero input from seed 0x1FF (the seed is fixed per CCH: a constant 72-bit mask)
__device__ __forceinline__ void
scramble_mask(uint8_t* m72) {
    unsigned sh = 0x1FFu; // bit i = register stage i
    for (int i = 0; i < 72; i++) {
        m72[i] = (uint8_t)(sh & 1u);
        const unsigned fb = ((sh >> 4) ^ sh) & 1u;
        sh = (sh >> 1) | (fb << 8);
    }
}

__device__ __forceinline__ unsigned
value_of(const uint8_t* b, int n) { // MSB first
    unsigned v = 0;
    for (int i = 0; i < n; i++) {
        v = (v << 1) | b[i];
    }
    return v;
}

// one CCH: 36 dibits -> 48 decoded bits, per-word Hamming status, CRC7 status
__device__ void
decode_cch(const uint8_t* dib36, uint8_t* b48, uint8_t* ham6, uint8_t* crc_ok) {
    uint8_t m[72], s[72];
    scramble_mask(m);
    for (int i = 0; i < 36; i++) {
        s[2 * i] = (uint8_t)(((dib36[i] >> 1) & 1) ^ m[2 * i]);
        s[2 * i + 1] = (uint8_t)((dib36[i] & 1) ^ m[2 * i + 1]);
    }
    for (int w = 0; w < 6; w++) {
        uint32_t word = 0; // bit j = de-interleaved bit w * 12 + j = scrambled-out bit j * 6 + w
        for (int j = 0; j < 12; j++) {
            word |= (uint32_t)s[j * 6 + w] << j;
        }
        ham6[w] = ddn_bcode::decode(ddn_bcode::HAMMING_12_8, word) ? 1 : 0;
        for (int j = 0; j < 8; j++) {
            b48[w * 8 + j] = (uint8_t)((word >> j) & 1u);
        }
    }
    *crc_ok = ddn_crc::of_bits_u8(ddn_crc::DPMR_CRC7, 41, b48) == value_of(b48 + 41, 7) ? 1 : 0;
}

// One workgroup per sync slot: the 372 dibits into LDS, lanes 0 / 1 decode a CCH each, lane 2 the colour code, then every lane
// writes.  A slot without a whole superframe in the call's records (or past the sync list) is written as zeros, colour -1.
__global__ __launch_bounds__(64) void
k_dpmr_superframe(const uint8_t* __restrict__ rec, size_t stride, const int32_t* __restrict__ counts, const int32_t* __restrict__ sync_pos,
                  const int32_t* __restrict__ n_sync, int max_syncs, int inverted,
                  uint8_t* __restrict__ bits96, uint8_t* __restrict__ ham12, uint8_t* __restrict__ crc2, int32_t* __restrict__ fields16,
                  int32_t* __restrict__ id, int32_t* __restrict__ color, uint8_t* __restrict__ valid) {
    __shared__ uint8_t d[kFrame], b[2][48], hm[2][6], cr[2];
    __shared__ int32_t col;
    const int k = blockIdx.x, c = blockIdx.y, t = threadIdx.x;
    const size_t so = (size_t)c * max_syncs + k;
    const int ns = n_sync[c] < max_syncs ? n_sync[c] : max_syncs;
    const long pos = k < ns ? (long)sync_pos[so] : -1;
    const bool ok = pos >= 0 && pos + kFrame < (long)counts[c] && (size_t)(pos + 1 + kFrame) <= stride;
    if (ok) {
        const uint8_t* r = rec + ((size_t)c * stride + (size_t)pos + 1) * 10;
        for (int i = t; i < kFrame; i += 64) {
            d[i] = (uint8_t)((r[(size_t)i * 10] & 3) ^ (inverted ? 2 : 0));
        }
    }
    __syncthreads();
    if (ok && t < 2) {
        decode_cch(d + kCch[t], b[t], hm[t], &cr[t]);
    } else if (ok && t == 2) {
        uint8_t cc[24];
        for (int i = 0; i < 12; i++) {
            cc[2 * i] = (d[kCc + i] >> 1) & 1;
            cc[2 * i + 1] = d[kCc + i] & 1;
        }
        const uint32_t code = value_of(cc, 24) | 0x555555u;
        int v = -1;
        for (int i = 0; i < DDN_DPMR_COLOR_CODES && v < 0; i++) {
            v = ddn_dpmr_color_codes[i][0] == code ? (int)ddn_dpmr_color_codes[i][1] : -1;
        }
        col = v;
    }
    __syncthreads();
    for (int i = t; i < 96; i += 64) {
        bits96[so * 96 + i] = ok ? b[i / 48][i % 48] : 0;
    }
    if (t < 12) {
        ham12[so * 12 + t] = ok ? hm[t / 6][t % 6] : 0;
    }
    if (t < 2) {
        crc2[so * 2 + t] = ok ? cr[t] : 0;
    }
    if (t < 16) {
        // {frame number, ID half, communication mode, version, format, emergency, reserved, slow data} per CCH (dpmr_voice.c:139-178)
        const uint8_t* q = b[t / 8];
        const int f = t % 8;
        const int at[8] = {0, 2, 14, 17, 19, 21, 22, 23}, len[8] = {2, 12, 3, 2, 2, 1, 1, 18};
        fields16[so * 16 + t] = ok ? (int32_t)value_of(q + at[f], len[f]) : 0;
    }
    if (t == 0) {
        id[so] = ok ? (int32_t)(((value_of(b[0] + 2, 12) << 12) & 0xFFF000u) | (value_of(b[1] + 2, 12) & 0xFFFu)) : 0;
        color[so] = ok ? col : -1;
        valid[so] = ok ? 1 : 0;
    }
}

// The identity state of dpmr_update_superframe_part() (dpmr_voice.c:197-274), one lane per channel walking its superframes in sync
// order: state {tg, src, next} (raw 24-bit IDs, -1 = none) carried from call to call.  A slot without a whole superframe does not touch it.
__global__ void
k_dpmr_identity(const int32_t* __restrict__ n_sync, int n_channels, int max_syncs, const uint8_t* __restrict__ valid,
                const int32_t* __restrict__ fields16, const uint8_t* __restrict__ ham12, const uint8_t* __restrict__ crc2,
                const int32_t* __restrict__ id, int32_t* __restrict__ state3, uint8_t* __restrict__ kind, uint8_t* __restrict__ strong,
                int32_t* __restrict__ tg, int32_t* __restrict__ src) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_channels) {
        return;
    }
    int32_t* st = state3 + (size_t)c * 3;
    int s_tg = st[0], s_src = st[1], s_next = st[2];
    const int ns = n_sync[c] < max_syncs ? n_sync[c] : max_syncs;
    for (int k = 0; k < max_syncs; k++) {
        const size_t so = (size_t)c * max_syncs + k;
        int kd = 0, sg = 0;
        if (k < ns && valid[so]) {
            const uint8_t* h = ham12 + so * 12;
            const uint8_t* cr = crc2 + so * 2;
            const int fn0 = fields16[so * 16], fn1 = fields16[so * 16 + 8];
            sg = (cr[0] || (h[0] && h[1])) && (cr[1] || (h[6] && h[7]));
            if (((cr[0] || h[0]) && fn0 == 0) || ((cr[1] || h[6]) && fn1 == 1)) {
                kd = 1, s_next = 2; // called
            } else if (((cr[0] || h[0]) && fn0 == 2) || ((cr[1] || h[6]) && fn1 == 3)) {
                kd = 2, s_next = 1; // calling
            } else {
                s_next = s_next == 1 ? 2 : (s_next == 2 ? 1 : 0);
            }
            if (kd && sg) {
                if (kd == 1) {
                    s_tg = id[so];
                } else {
                    s_src = id[so];
                }
            }
        }
        kind[so] = (uint8_t)kd;
        strong[so] = (uint8_t)sg;
        tg[so] = s_tg;
        src[so] = s_src;
    }
    st[0] = s_tg, st[1] = s_src, st[2] = s_next;
}

// The eight TCH frames of every slot through the AMBE 3600x2450 schedule (hard bits), and which halves dpmr_play_voice_frames()
// synthesises: communication mode 0, 1 or 5; version 3 (scrambled) is muted without a key.  One workgroup per slot.
__global__ __launch_bounds__(64) void
k_dpmr_voice_gather(const uint8_t* __restrict__ rec, size_t stride, const int32_t* __restrict__ sync_pos, const int32_t* __restrict__ n_sync,
                    int max_syncs, int inverted, const int32_t* __restrict__ fields16, const uint8_t* __restrict__ valid,
                    uint8_t* __restrict__ fr, uint8_t* __restrict__ voiced2, uint8_t* __restrict__ muted2) {
    const int k = blockIdx.x, c = blockIdx.y, t = threadIdx.x;
    const size_t so = (size_t)c * max_syncs + k;
    const int ns = n_sync[c] < max_syncs ? n_sync[c] : max_syncs;
    const bool ok = k < ns && valid[so];
    uint8_t* o = fr + so * 8 * 96;
    for (int i = t; i < 8 * 96; i += 64) {
        o[i] = 0;
    }
    if (t < 2) {
        const int mode = ok ? fields16[so * 16 + t * 8 + 2] : -1, version = ok ? fields16[so * 16 + t * 8 + 3] : 0;
        voiced2[so * 2 + t] = (mode == 0 || mode == 1 || mode == 5) ? 1 : 0;
        muted2[so * 2 + t] = (ok && version == 3) ? 1 : 0;
    }
    __syncthreads();
    if (!ok) {
        return;
    }
    const uint8_t* r = rec + ((size_t)c * stride + (size_t)sync_pos[so] + 1) * 10;
    for (int i = t; i < 8 * 36; i += 64) {
        const int f = i / 36, j = i % 36;
        const int dib = (r[(size_t)(c_voice_at[f] + j) * 10] & 3) ^ (inverted ? 2 : 0);
        uint8_t* q = o + f * 96;
        q[c_dpmr_ambe_map[j][0] * 24 + c_dpmr_ambe_map[j][1]] = (uint8_t)((dib >> 1) & 1);
        q[c_dpmr_ambe_map[j][2] * 24 + c_dpmr_ambe_map[j][3]] = (uint8_t)(dib & 1);
    }
}

// (chain object) the voiced halves of every channel in air order -> talk path = channel, four frames per half, vf frames per channel;
// the rest of the row is skipped (silence, history untouched)
__global__ __launch_bounds__(64) void
k_dpmr_voice_file(const int32_t* __restrict__ n_sync, int max_syncs, const uint8_t* __restrict__ fr_slot, const uint8_t* __restrict__ voiced2,
                  const uint8_t* __restrict__ muted2, int vf, uint8_t* __restrict__ fr, int32_t* __restrict__ v_n, int32_t* __restrict__ v_slot,
                  uint8_t* __restrict__ v_half, uint8_t* __restrict__ v_muted, uint8_t* __restrict__ v_skip) {
    const int c = blockIdx.x, t = threadIdx.x;
    const int ns = n_sync[c] < max_syncs ? n_sync[c] : max_syncs;
    int j = 0; // frames filed
    for (int k = 0; k < ns; k++) {
        const size_t so = (size_t)c * max_syncs + k;
        for (int h = 0; h < 2; h++) {
            if (!voiced2[so * 2 + h] || j + 4 > vf) {
                continue;
            }
            const uint8_t* src = fr_slot + (so * 8 + 4 * h) * 96;
            uint8_t* dst = fr + ((size_t)c * vf + j) * 96;
            for (int i = t; i < 4 * 96; i += 64) {
                dst[i] = src[i];
            }
            if (t < 4) {
                const size_t q = (size_t)c * vf + j + t;
                v_slot[q] = k, v_half[q] = (uint8_t)h, v_muted[q] = muted2[so * 2 + h], v_skip[q] = 0;
            }
            j += 4;
        }
    }
    for (int i = j * 96 + t; i < vf * 96; i += 64) {
        fr[(size_t)c * vf * 96 + i] = 0;
    }
    for (int i = j + t; i < vf; i += 64) {
        const size_t q = (size_t)c * vf + i;
        v_slot[q] = -1, v_half[q] = 0, v_muted[q] = 0, v_skip[q] = 1;
    }
    if (t == 0) {
        v_n[c] = j;
    }
}

} // namespace

extern "C" hipError_t
ddn_dev_dpmr_voice_file(const int32_t* n_sync, int n_channels, int max_syncs, const uint8_t* fr_slot, const uint8_t* voiced2,
                        const uint8_t* muted2, int vf, uint8_t* fr, int32_t* v_n, int32_t* v_slot, uint8_t* v_half, uint8_t* v_muted,
                        uint8_t* v_skip, hipStream_t st) {
    if (n_channels <= 0 || vf <= 0) {
        return hipSuccess;
    }
    hipLaunchKernelGGL(k_dpmr_voice_file, dim3((unsigned)n_channels), dim3(64), 0, st, n_sync, max_syncs, fr_slot, voiced2, muted2, vf, fr,
                       v_n, v_slot, v_half, v_muted, v_skip);
    return hipGetLastError();
}

extern "C" int
ddn_dpmr_superframe_decode_batch(const uint8_t* d_records10, size_t stride_symbols, const int32_t* d_counts, const int32_t* d_sync_pos,
                                 const int32_t* d_n_sync, int n_channels, size_t max_syncs, int inverted, uint8_t* d_cch_bits2x48,
                                 uint8_t* d_ham_ok2x6, uint8_t* d_crc_ok2, int32_t* d_fields2x8, int32_t* d_id, int32_t* d_color,
                                 uint8_t* d_valid, void* hip_stream) {
    if (n_channels < 0 || (inverted != 0 && inverted != 1) || max_syncs > 65535) {
        ddn_set_error("ddn_dpmr_superframe_decode_batch: bad arguments");
        return DDN_EINVAL;
    }
    if (n_channels == 0 || max_syncs == 0) {
        return DDN_OK;
    }
    if (!d_records10 || !d_counts || !d_sync_pos || !d_n_sync || !d_cch_bits2x48 || !d_ham_ok2x6 || !d_crc_ok2 || !d_fields2x8 || !d_id
        || !d_color || !d_valid) {
        ddn_set_error("ddn_dpmr_superframe_decode_batch: null pointer");
        return DDN_EINVAL;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(k_dpmr_superframe, dim3((unsigned)max_syncs, (unsigned)n_channels), dim3(64), 0, st, d_records10, stride_symbols,
                       d_counts, d_sync_pos, d_n_sync, (int)max_syncs, inverted, d_cch_bits2x48, d_ham_ok2x6, d_crc_ok2, d_fields2x8, d_id,
                       d_color, d_valid);
    DDN_LAUNCH_TRY(hipGetLastError());
    return DDN_OK;
}

extern "C" int
ddn_dpmr_identity_batch(const int32_t* d_n_sync, int n_channels, size_t max_syncs, const uint8_t* d_valid, const int32_t* d_fields2x8,
                        const uint8_t* d_ham_ok2x6, const uint8_t* d_crc_ok2, const int32_t* d_id, int32_t* d_state3, uint8_t* d_kind,
                        uint8_t* d_strong, int32_t* d_tg, int32_t* d_src, void* hip_stream) {
    if (n_channels < 0) {
        ddn_set_error("ddn_dpmr_identity_batch: bad arguments");
        return DDN_EINVAL;
    }
    if (n_channels == 0 || max_syncs == 0) {
        return DDN_OK;
    }
    if (!d_n_sync || !d_valid || !d_fields2x8 || !d_ham_ok2x6 || !d_crc_ok2 || !d_id || !d_state3 || !d_kind || !d_strong || !d_tg || !d_src) {
        ddn_set_error("ddn_dpmr_identity_batch: null pointer");
        return DDN_EINVAL;
    }
    hipLaunchKernelGGL(k_dpmr_identity, dim3((unsigned)((n_channels + 63) / 64)), dim3(64), 0, (hipStream_t)hip_stream, d_n_sync, n_channels,
                       (int)max_syncs, d_valid, d_fields2x8, d_ham_ok2x6, d_crc_ok2, d_id, d_state3, d_kind, d_strong, d_tg, d_src);
    DDN_LAUNCH_TRY(hipGetLastError());
    return DDN_OK;
}

extern "C" int
ddn_dpmr_voice_gather(const uint8_t* d_records10, size_t stride_symbols, const int32_t* d_sync_pos, const int32_t* d_n_sync, int n_channels,
                      size_t max_syncs, int inverted, const int32_t* d_fields2x8, const uint8_t* d_valid, uint8_t* d_ambe_fr,
                      uint8_t* d_voiced2, uint8_t* d_muted2, void* hip_stream) {
    if (n_channels < 0 || (inverted != 0 && inverted != 1) || max_syncs > 65535) {
        ddn_set_error("ddn_dpmr_voice_gather: bad arguments");
        return DDN_EINVAL;
    }
    if (n_channels == 0 || max_syncs == 0) {
        return DDN_OK;
    }
    if (!d_records10 || !d_sync_pos || !d_n_sync || !d_fields2x8 || !d_valid || !d_ambe_fr || !d_voiced2 || !d_muted2) {
        ddn_set_error("ddn_dpmr_voice_gather: null pointer");
        return DDN_EINVAL;
    }
    hipLaunchKernelGGL(k_dpmr_voice_gather, dim3((unsigned)max_syncs, (unsigned)n_channels), dim3(64), 0, (hipStream_t)hip_stream, d_records10,
                       stride_symbols, d_sync_pos, d_n_sync, (int)max_syncs, inverted, d_fields2x8, d_valid, d_ambe_fr, d_voiced2, d_muted2);
    DDN_LAUNCH_TRY(hipGetLastError());
    return DDN_OK;
}

// dpmr_convert_air_interface_id() (dpmr_voice.c:477-546): seven digits of the AI ID in base 11 with '*' for ten.  The first digit is
// not bounded: at and above 11 x 1464100 the reference writes '0' + 11 there, and so does this.
extern "C" void
ddn_dpmr_air_interface_id(uint32_t ai_id, char out[8]) {
    static const uint32_t div[7] = {1464100u, 146410u, 14641u, 1331u, 121u, 11u, 1u};
    uint32_t v = ai_id;
    for (int i = 0; i < 7; i++) {
        const uint32_t d = v / div[i];
        v %= div[i];
        out[i] = d == 10 ? '*' : (char)('0' + d);
    }
    out[7] = '\0';
}
