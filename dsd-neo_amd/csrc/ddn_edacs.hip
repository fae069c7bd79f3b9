// ddn_edacs.hip - EDACS control-channel frames behind the fsk4 loop's syncs (DDN_FSK4_EDACS, the reference's -fh / -fH / -fe / -fE).
//
// reference: src/protocol/edacs/edacs-fme.c - edacs() :2012-2066 (240 bits behind the sync, six 40-bit words, vote, BCH re-encode),
// edacs_build_raw_frames() :1973-1990, edacs_vote_frames() :157-175 (the middle copy is sent inverted), edacs_process_valid_frame()
// :1993-2010 (esk_mask << 20), the standard message types :1915-1940 and site ID :1748-1781, the EA message types :1265-1284 and site
// ID :944-955; edacs_bch() src/protocol/edacs/edacs-bch3.c (BCH(40,28): the 28-bit message above 12 parity bits, g(x) = 0x1539); the
// two-level slice store_two_level_dibit() src/core/frames/dsd_dibit.c:938-948,1024-1029.  One wavefront per sync slot: the 40 symbols
// of a word are read by 40 lanes and gathered with a ballot, one lane votes, re-encodes and classifies.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddn_api_util.h"
#include "ddn_fsk4.h"
#include "ddn_internal.h"

namespace {

constexpr int kWords = 6, kWordBits = 40, kFrame = DDN_EDACS_FRAME_SYMBOLS;
constexpr unsigned long long kMask40 = 0xFFFFFFFFFFull;
constexpr uint32_t kGen = 0x1539u; // x^12 + x^10 + x^8 + x^5 + x^4 + x^3 + 1

__device__ __forceinline__ float
rec_symbol(const uint8_t* r) { // bytes 6..9 of a 10-byte record (2-byte aligned)
    const uint32_t xb = (uint32_t)((const uint16_t*)r)[3] | ((uint32_t)((const uint16_t*)r)[4] << 16);
    return __uint_as_float(xb);
}

// the systematic BCH(40,28) codeword of a 28-bit message: message in bits 39..12, the remainder of x^12 m(x) mod g(x) below
__device__ __forceinline__ unsigned long long
bch_encode(uint32_t msg) {
    msg &= 0x0FFFFFFFu;
    unsigned long long r = (unsigned long long)msg << 12;
    for (int b = 39; b >= 12; b--) {
        if ((r >> b) & 1ull) {
            r ^= (unsigned long long)kGen << (b - 12);
        }
    }
    return ((unsigned long long)msg << 12) | (r & 0xFFFull);
}

__global__ __launch_bounds__(64) void
k_edacs_frame(const uint8_t* __restrict__ rec, size_t stride, const int32_t* __restrict__ counts, const int32_t* __restrict__ sync_pos,
              const uint8_t* __restrict__ sync_pat, const int32_t* __restrict__ n_sync, const float* __restrict__ sync_thr, int max_syncs,
              int ea_mode, int esk_mask, unsigned long long* __restrict__ raw40, unsigned long long* __restrict__ vote40,
              uint8_t* __restrict__ bch_ok, uint8_t* __restrict__ frame_ok, uint32_t* __restrict__ msg28, uint8_t* __restrict__ kind,
              uint8_t* __restrict__ types, int32_t* __restrict__ site6, uint8_t* __restrict__ valid) {
    const int k = blockIdx.x, ch = blockIdx.y, lane = threadIdx.x;
    const size_t slot = (size_t)ch * max_syncs + k;
    bool ok = k < n_sync[ch];
    int pos = 0, pat = 0;
    if (ok) {
        pos = sync_pos[slot];
        pat = sync_pat[slot];
        const long have = counts[ch] < (long)stride ? (long)counts[ch] : (long)stride;
        ok = pat <= 1 && pos >= 0 && (long)pos + 1 + kFrame <= have;
    }
    if (!ok) {
        if (lane < kWords) {
            raw40[slot * kWords + lane] = 0;
        }
        if (lane < 2) {
            vote40[slot * 2 + lane] = 0;
            bch_ok[slot * 2 + lane] = 0;
            msg28[slot * 2 + lane] = 0;
        }
        if (lane < 3) {
            types[slot * 3 + lane] = 0;
        }
        if (lane < 6) {
            site6[slot * 6 + lane] = 0;
        }
        if (lane == 0) {
            frame_ok[slot] = 0;
            kind[slot] = 0;
            valid[slot] = 0;
        }
        return;
    }
    // pattern 1 = INV_EDACS_SYNC = DSD_SYNC_EDACS_POS: a high symbol is a 0; pattern 0 (NEG): a high symbol is a 1
    const float center = sync_thr[slot * 5];
    const bool high_one = pat == 0;
    const uint8_t* r0 = rec + ((size_t)ch * stride + (size_t)pos + 1) * 10;
    unsigned long long w[kWords];
#pragma unroll
    for (int j = 0; j < kWords; j++) {
        bool bit = false;
        if (lane < kWordBits) {
            const bool high = rec_symbol(r0 + (size_t)(j * kWordBits + lane) * 10) > center;
            bit = high == high_one;
        }
        // lane i = bit i of the word, the first one received the most significant (edacs_build_raw_frames())
        w[j] = __brevll(__ballot(bit)) >> (64 - kWordBits);
    }
    if (lane != 0) {
        return;
    }
    unsigned long long v[2];
    uint32_t m[2];
    uint8_t good[2];
    for (int h = 0; h < 2; h++) {
        const unsigned long long a = w[3 * h], b = ~w[3 * h + 1] & kMask40, c = w[3 * h + 2];
        v[h] = ((a & b) | (a & c) | (b & c)) & kMask40;
        const uint32_t msg = (uint32_t)(v[h] >> 12);
        good[h] = bch_encode(msg) == v[h] ? 1 : 0;
        m[h] = msg ^ ((uint32_t)esk_mask << 20);
    }
    const bool fok = good[0] && good[1];
    const uint32_t m1 = m[0];
    uint8_t t0, t1, t2;
    int32_t f[6] = {0, 0, 0, 0, 0, 0};
    bool site;
    if (ea_mode) {
        t0 = (uint8_t)((m1 >> 23) & 0x1F);
        t1 = (uint8_t)((m1 >> 19) & 0xF);
        t2 = 0;
        site = t0 == 0x1F && t1 == 0xA;
        if (site) {
            f[0] = (int32_t)(((m1 & 0x7000u) >> 7) | (m1 & 0x1Fu));
            f[1] = (int32_t)((m1 & 0xFE0u) >> 5);
        }
    } else {
        t0 = (uint8_t)((m1 >> 25) & 7);
        t1 = (uint8_t)((m1 >> 22) & 7);
        t2 = (uint8_t)((m1 >> 17) & 0x1F);
        site = t0 == 7 && t1 == 7 && t2 >= 0x08 && t2 <= 0x0B;
        if (site) {
            f[0] = (int32_t)(m1 & 0x1F);
            f[1] = (int32_t)((m1 >> 9) & 7);
            f[2] = (int32_t)((m1 >> 12) & 0x1F);
            f[3] = (int32_t)((m1 >> 7) & 1);
            f[4] = (int32_t)((m1 >> 6) & 1);
            f[5] = (int32_t)((m1 >> 5) & 1);
        }
    }
    site = site && fok;
    for (int j = 0; j < kWords; j++) {
        raw40[slot * kWords + j] = w[j];
    }
    for (int h = 0; h < 2; h++) {
        vote40[slot * 2 + h] = v[h];
        bch_ok[slot * 2 + h] = good[h];
        msg28[slot * 2 + h] = m[h];
    }
    types[slot * 3] = t0;
    types[slot * 3 + 1] = t1;
    types[slot * 3 + 2] = t2;
    for (int j = 0; j < 6; j++) {
        site6[slot * 6 + j] = site ? f[j] : 0;
    }
    frame_ok[slot] = fok ? 1 : 0;
    kind[slot] = (uint8_t)(fok ? (ea_mode ? 2 : 1) + (site ? 2 : 0) : 0);
    valid[slot] = 1;
}

} // namespace

extern "C" int
ddn_edacs_frame_decode_batch(const uint8_t* d_records10, size_t stride_symbols, const int32_t* d_counts, const int32_t* d_sync_pos,
                             const uint8_t* d_sync_pat, const int32_t* d_n_sync, const float* d_sync_thr5, int n_channels, size_t max_syncs,
                             int ea_mode, int esk_mask, uint64_t* d_raw40, uint64_t* d_vote40, uint8_t* d_bch_ok, uint8_t* d_frame_ok,
                             uint32_t* d_msg28, uint8_t* d_kind, uint8_t* d_types, int32_t* d_site6, uint8_t* d_valid, void* hip_stream) {
    if (n_channels < 0 || n_channels > 65535 || max_syncs > 65535 || (ea_mode != 0 && ea_mode != 1) || (esk_mask != 0 && esk_mask != 0xA0)) {
        ddn_set_error("ddn_edacs_frame_decode_batch: bad arguments (n_channels and max_syncs at most 65535, ea_mode 0 / 1, esk_mask 0 / 0xA0)");
        return DDN_EINVAL;
    }
    if (n_channels == 0 || max_syncs == 0) {
        return DDN_OK;
    }
    if (!d_records10 || !d_counts || !d_sync_pos || !d_sync_pat || !d_n_sync || !d_sync_thr5 || !d_raw40 || !d_vote40 || !d_bch_ok
        || !d_frame_ok || !d_msg28 || !d_kind || !d_types || !d_site6 || !d_valid) {
        ddn_set_error("ddn_edacs_frame_decode_batch: null pointer");
        return DDN_EINVAL;
    }
    hipLaunchKernelGGL(k_edacs_frame, dim3((unsigned)max_syncs, (unsigned)n_channels), dim3(64), 0, (hipStream_t)hip_stream, d_records10,
                       stride_symbols, d_counts, d_sync_pos, d_sync_pat, d_n_sync, d_sync_thr5, (int)max_syncs, ea_mode, esk_mask,
                       (unsigned long long*)d_raw40, (unsigned long long*)d_vote40, d_bch_ok, d_frame_ok, d_msg28, d_kind, d_types, d_site6,
                       d_valid);
    DDN_LAUNCH_TRY(hipGetLastError());
    return DDN_OK;
}
