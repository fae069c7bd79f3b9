// ddn_m17_data.hip - M17 packet and BERT frames behind the receive loop's syncs, and the per-channel state that carries a packet of up
// to 33 frames and the BERT receiver across calls.
//
// processM17PKT() (src/protocol/m17/m17.c:3076-3155): the 184 payload symbols as soft symbols -> soft_symbol_to_viterbi_cost() per bit
// against the thresholds the sync left -> de-randomised (the cost complemented where the randomiser bit is 1) -> de-interleaved ->
// de-punctured with pattern P3, 0x7FFF where a bit was cut (m17_soft_depuncture_p3 :2991-3001) -> viterbi_decode(420 costs) (k_k5_m17,
// ddn_trellis.hip) -> bytes 1..26 = 25 chunk bytes + the metadata byte.
//   k_m17_pkt_cost    one wavefront per (channel, j): the channel's j-th packet sync (pattern 10 / 11) whose frame lies inside the
//                     records -> its 420 de-punctured costs
//   k_m17_pkt_finish  one lane per (channel, j): the 26 bytes scattered to the sync's slot
//
// processM17BRT() (:1325-1340): the 184 payload dibits as hard bits -> de-randomised -> de-interleaved -> de-punctured with P2 to 402
// symbol values bit << 1, the cut bit reads 0 (m17_depuncture_p2_hard :1232-1245, m17_decode_bert_payload_bits :1247-1276) ->
// CNXDNConvolution over 201 steps, 197 bits chained back (k_k5_nxdn).
//   k_m17_brt_bits    one wavefront per (channel, j): the channel's j-th BERT sync (pattern 6 / 7) with a complete frame -> 402 symbols
//   k_m17_brt_finish  one lane per (channel, j): 25 packed bytes (most significant bit first, the last three bits zero) to the slot
//
//   k_m17_data_walk   one lane per channel: the channel's syncs of the call in order.  Packet frames go through processM17PKT()'s
//                     checks in its own order (:3100-3150, m17_pkt_finalize_eot :3052-3074), BERT frames through the PRBS9 receiver
//                     (m17_process_bert_payload :1302-1323 over m17_prbs9_rx_push_bit, m17_algorithms.c:125-167), EOT markers apply
//                     dispatch_m17.c:39-50, and a sync that follows 1800 hunted symbols applies the carrier-loss reset
//                     (no_carrier_reset_m17_and_sample_buffers, src/engine/engine.c:2169-2184)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddn_crc_dev.h"
#include "ddn_expf.h"

// What a channel carries from call to call (all zeros = a stream's start; its size is ddn_m17_data_state_bytes()).
struct DdnM17DataState {
    int32_t hunt_base; // record index of the first symbol hunted after the last lock, in the row indexing of the call to come (saturates)
    int32_t pbc;       // state->m17_pbc_ct
    int32_t fill;      // no byte of pkt[] at or behind this index is non-zero (what a clear has to touch)
    // {locked, lfsr, lock_count, window_bits, window_errors, total_bits, total_errors, resyncs}: state->m17_bert_*; an lfsr of 0 reads
    // 1, as m17_prbs9_rx_init() has it
    int32_t brt[8];
    uint8_t pkt[852]; // state->m17_pkt[850]
};

namespace {

#include "ddn_m17_dev.h" // k_m17_rand, m17_soft_cost, m17_find_sync

__global__ __launch_bounds__(64) void
k_m17_pkt_cost(const uint8_t* __restrict__ rec, size_t stride, const int32_t* __restrict__ counts, const int32_t* __restrict__ sync_pos,
               const uint8_t* __restrict__ sync_pat, const int32_t* __restrict__ n_sync, const float* __restrict__ sync_thr, int max_syncs,
               int lmax, uint16_t* __restrict__ cost420, int32_t* __restrict__ slot_sync, uint8_t* __restrict__ slot_want) {
    __shared__ uint16_t il[368]; // de-randomised costs in received order
    const int ch = blockIdx.x, j = blockIdx.y, lane = threadIdx.x;
    const size_t slot = (size_t)ch * lmax + j;
    int ns = n_sync[ch];
    ns = ns < max_syncs ? ns : max_syncs;
    const int found = m17_find_sync(sync_pos + (size_t)ch * max_syncs, sync_pat + (size_t)ch * max_syncs, ns, counts[ch], j, 10, 11, lane);
    if (lane == 0) {
        slot_sync[slot] = found;
        slot_want[slot] = found >= 0 ? 1 : 0;
    }
    if (found < 0) {
        return; // (the decoder leaves an unwanted slot alone)
    }
    const size_t so = (size_t)ch * max_syncs + found;
    const int pos = sync_pos[so];
    const float* thr = sync_thr + so * 5;
    const uint8_t* r0 = rec + ((size_t)ch * stride + (size_t)pos + 1) * 10;
    for (int i = lane; i < 368; i += 64) {
        const uint8_t* r = r0 + (size_t)(i >> 1) * 10;
        const uint32_t xb = (uint32_t)((const uint16_t*)r)[3] | ((uint32_t)((const uint16_t*)r)[4] << 16);
        const uint32_t c = m17_soft_cost(__uint_as_float(xb), thr, i & 1);
        const int rb = (k_m17_rand[i >> 3] >> (7 - (i & 7))) & 1;
        il[i] = (uint16_t)(rb ? (0xFFFFu - c) : c);
    }
    __syncthreads();
    // P3 = {1, 1, 1, 1, 1, 1, 1, 0}: seven of eight kept; 420 = 52 groups + 4, 368 kept.  Kept bit number k reads the de-interleaved
    // stream: bits[k] = il[(45 k + 92 k^2) mod 368]
    uint16_t* out = cost420 + slot * 420;
    for (int i = lane; i < 420; i += 64) {
        const int g = i >> 3, q = i & 7;
        uint16_t v = 0x7FFFu;
        if (q != 7) {
            const int k = g * 7 + q;
            v = il[(45 * k + 92 * k * k) % 368];
        }
        out[i] = v;
    }
}

__global__ void
k_m17_pkt_finish(const uint8_t* __restrict__ dec, int dec_stride, const uint32_t* __restrict__ cost, const int32_t* __restrict__ slot_sync,
                 int n_channels, int lmax, int max_syncs, uint8_t* __restrict__ pkt26, uint8_t* __restrict__ status,
                 uint32_t* __restrict__ path_cost) {
    const int slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= n_channels * lmax) {
        return;
    }
    const int k = slot_sync[slot];
    if (k < 0) {
        return;
    }
    const size_t so = (size_t)(slot / lmax) * max_syncs + k;
    const uint8_t* by = dec + (size_t)slot * dec_stride + 1; // viterbi_decode()'s bytes 1 .. 26
    for (int i = 0; i < 26; i++) {
        pkt26[so * 26 + i] = by[i];
    }
    status[so] = 1;
    if (path_cost) {
        path_cost[so] = cost[slot];
    }
}

__global__ __launch_bounds__(64) void
k_m17_brt_bits(const uint8_t* __restrict__ rec, size_t stride, const int32_t* __restrict__ counts, const int32_t* __restrict__ sync_pos,
               const uint8_t* __restrict__ sync_pat, const int32_t* __restrict__ n_sync, int max_syncs, int lmax,
               uint8_t* __restrict__ sym402, int32_t* __restrict__ slot_sync, uint8_t* __restrict__ slot_want) {
    __shared__ uint8_t bits[368]; // de-randomised, de-interleaved
    const int ch = blockIdx.x, j = blockIdx.y, lane = threadIdx.x;
    const size_t slot = (size_t)ch * lmax + j;
    int ns = n_sync[ch];
    ns = ns < max_syncs ? ns : max_syncs;
    const int found = m17_find_sync(sync_pos + (size_t)ch * max_syncs, sync_pat + (size_t)ch * max_syncs, ns, counts[ch], j, 6, 7, lane);
    if (lane == 0) {
        slot_sync[slot] = found;
        slot_want[slot] = found >= 0 ? 1 : 0;
    }
    if (found < 0) {
        return;
    }
    const int pos = sync_pos[(size_t)ch * max_syncs + found];
    const uint8_t* r0 = rec + ((size_t)ch * stride + (size_t)pos + 1) * 10;
    for (int i = lane; i < 368; i += 64) {
        const int x = (45 * i + 92 * i * i) % 368; // bits[i] = rnd[x] ^ rand(x)
        const int d = r0[(size_t)(x >> 1) * 10] & 3;
        const int b = (x & 1) ? (d & 1) : (d >> 1);
        bits[i] = (uint8_t)((b ^ ((k_m17_rand[x >> 3] >> (7 - (x & 7))) & 1)) & 1);
    }
    __syncthreads();
    // P2 = eleven kept + one cut: 402 = 33 groups + 6 would keep 369 bits; the 368 there are fill it and the last entry reads 0
    uint8_t* out = sym402 + slot * 402;
    for (int i = lane; i < 402; i += 64) {
        const int g = i / 12, q = i - g * 12;
        const int x = g * 11 + q;
        const int b = (q < 11 && x < 368) ? bits[x] : 0;
        out[i] = (uint8_t)(b << 1);
    }
}

__global__ void
k_m17_brt_finish(const uint8_t* __restrict__ dec, int dec_stride, const int32_t* __restrict__ slot_sync, int n_channels, int lmax,
                 int max_syncs, uint8_t* __restrict__ bits25, uint8_t* __restrict__ status) {
    const int slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= n_channels * lmax) {
        return;
    }
    const int k = slot_sync[slot];
    if (k < 0) {
        return;
    }
    const size_t so = (size_t)(slot / lmax) * max_syncs + k;
    for (int i = 0; i < 25; i++) {
        bits25[so * 25 + i] = dec[(size_t)slot * dec_stride + i];
    }
    status[so] = 1;
}

__device__ __forceinline__ void
m17_pkt_clear(DdnM17DataState* s, int& pbc) { // DSD_MEMSET(state->m17_pkt, 0, ..); state->m17_pbc_ct = 0
    const int fill = s->fill;
    if (fill > 0) {
        for (int i = 0; i < fill; i++) {
            s->pkt[i] = 0;
        }
        s->fill = 0;
    }
    pbc = 0;
}

__device__ __forceinline__ void
m17_brt_init(int32_t* b) { // m17_prbs9_rx_init(rx, 1)
    b[0] = 0, b[1] = 1, b[2] = 0, b[3] = 0, b[4] = 0, b[5] = 0, b[6] = 0, b[7] = 0;
}

// One lane per channel.  k_m17_lich's buffer (state->m17_lsf) is not touched here although processM17PKT() and the carrier-loss reset
// zero it too: a stream sync is only accepted after an LSF or a stream sync (dsd_frame_sync.c:972-992), and a complete LSF overwrites
// all thirty bytes, so no LICH chunk ever lands in a buffer that either clear would have changed - neither is observable there.
__global__ void
k_m17_data_walk(const uint8_t* __restrict__ sync_pat, const int32_t* __restrict__ sync_pos, const int32_t* __restrict__ n_sync,
                const int32_t* __restrict__ advance, int n_channels, int max_syncs, const uint8_t* __restrict__ pkt26,
                const uint8_t* __restrict__ pkt_frame_status, const uint8_t* __restrict__ bits25,
                const uint8_t* __restrict__ brt_frame_status, DdnM17DataState* __restrict__ state, uint8_t* __restrict__ pkt_status,
                uint8_t* __restrict__ pkt_count, int32_t* __restrict__ brt_state, uint8_t* __restrict__ packet,
                int32_t* __restrict__ packet_app_len, uint8_t* __restrict__ packet_crc_ok, int32_t* __restrict__ packet_slot,
                int32_t* __restrict__ n_packets, int max_packets) {
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= n_channels) {
        return;
    }
    DdnM17DataState* s = state + ch;
    int32_t brt[8];
    for (int i = 0; i < 8; i++) {
        brt[i] = s->brt[i];
    }
    brt[1] = (brt[1] & 0x1FF) ? (brt[1] & 0x1FF) : 1; // m17_load_bert_rx_state -> m17_prbs9_rx_init: masked, 0 reads 1
    int hunt_base = s->hunt_base, np = 0, pbc = s->pbc;
    int ns = n_sync[ch];
    ns = ns < max_syncs ? ns : max_syncs;
    for (int k = 0; k < ns; k++) {
        const size_t so = (size_t)ch * max_syncs + k;
        const int pat = sync_pat[so], pos = sync_pos[so];
        // The loop counts the symbols it hunts since the last lock ended and declares carrier loss at the 1800th without a sync
        // (a sync is looked for before the count moves, so the 1800th symbol itself may still carry one); only a preamble is
        // accepted after that, and it finds everything below reset.
        if (pos - hunt_base >= 1800) {
            m17_pkt_clear(s, pbc);
            m17_brt_init(brt);
        }
        // (a call of noise holds hundreds of preamble syncs: they cost two loads each and write nothing - the status arrays were cleared)
        if (pat == 2 || pat == 3) { // EOT (dispatch_m17.c:39-50): the count, not the buffer; the BERT receiver starts over
            pbc = 0;
            m17_brt_init(brt);
        } else if ((pat == 10 || pat == 11) && pkt_frame_status[so] != 0) {
            const uint8_t* p = pkt26 + so * 26;
            const int meta = p[25], eof = meta >> 7, val = (meta >> 2) & 0x1F, cnt = pbc;
            uint8_t* buf = s->pkt;
            int st;
            if ((meta & 3) != 0 || (eof && (val == 0 || val > 25))) { // m17_packet_parse_metadata_byte
                st = 1;
                m17_pkt_clear(s, pbc);
            } else if (!eof && val != cnt) {
                st = 2;
                m17_pkt_clear(s, pbc);
            } else if (eof && (cnt >= 33 || cnt * 25 + val < 2)) { // m17_packet_app_bytes_from_eof (val is 1 .. 25 here)
                st = 3;
                m17_pkt_clear(s, pbc);
            } else {
                int ptr = cnt * 25; // m17_pkt_ptr_clamped
                ptr = ptr > 825 ? 825 : ptr;
                for (int i = 0; i < 25; i++) {
                    buf[ptr + i] = p[i];
                }
                s->fill = s->fill > ptr + 25 ? s->fill : ptr + 25;
                if (eof) { // m17_pkt_finalize_eot: reported whatever the CRC says, then cleared
                    int app = cnt * 25 + val - 2;
                    app = app > 823 ? 823 : app;
                    const int end = ptr + val;
                    const bool ok = ddn_crc::of_bytes(ddn_crc::M17, buf, app) == (((uint32_t)buf[app] << 8) | buf[app + 1]);
                    if (np < max_packets) {
                        const size_t po = (size_t)ch * max_packets + np;
                        uint8_t* o = packet + po * 832;
                        for (int i = 0; i < 832; i++) {
                            o[i] = i < end ? buf[i] : 0;
                        }
                        packet_app_len[po] = app;
                        packet_crc_ok[po] = ok ? 1 : 0;
                        packet_slot[po] = k;
                    }
                    np++;
                    st = ok ? 7 : 6;
                    m17_pkt_clear(s, pbc);
                } else if (cnt >= 32) { // (a 5-bit counter that equals the count never gets here; kept as the reference has it)
                    st = 5;
                    m17_pkt_clear(s, pbc);
                } else {
                    st = 4;
                    pbc = cnt + 1;
                }
            }
            pkt_status[so] = (uint8_t)st;
            pkt_count[so] = (uint8_t)cnt;
        } else if ((pat == 6 || pat == 7) && brt_frame_status[so] != 0) {
            const uint8_t* p = bits25 + so * 25;
            uint32_t locked = (uint32_t)brt[0], lfsr = (uint32_t)brt[1] & 0x1FFu, lock_count = (uint32_t)brt[2], wbits = (uint32_t)brt[3];
            uint32_t werr = (uint32_t)brt[4], tbits = (uint32_t)brt[5], terr = (uint32_t)brt[6], resync = (uint32_t)brt[7];
            lfsr = lfsr == 0 ? 1u : lfsr;
            // the 25 bytes into registers first: in noise a channel is in (false) BERT frames most of the time, and 197 dependent byte
            // loads per frame on one lane per channel were the stage's longest kernel
            uint32_t w[7] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int q = 0; q < 25; q++) {
                w[q >> 2] |= (uint32_t)p[q] << (24 - 8 * (q & 3));
            }
#pragma unroll
            for (int wi = 0; wi < 7; wi++) {
                uint32_t word = w[wi];
                const int nb = wi < 6 ? 32 : 5;
                for (int b = 0; b < nb; b++) { // m17_prbs9_rx_push_bit
                    const uint32_t bit = word >> 31;
                    word <<= 1;
                    lfsr = lfsr == 0 ? 1u : lfsr;
                    const uint32_t expected = ((lfsr >> 8) ^ (lfsr >> 4)) & 1u;
                    if (locked) {
                        lfsr = ((lfsr << 1) | expected) & 0x1FFu;
                        tbits++;
                        wbits++;
                        if (expected != bit) {
                            terr++;
                            werr++;
                        }
                        if (wbits >= 128) {
                            if (werr > 18) {
                                locked = 0;
                                lock_count = 0;
                                resync++;
                            }
                            wbits = 0;
                            werr = 0;
                        }
                    } else {
                        lock_count = expected == bit ? lock_count + 1 : 0;
                        lfsr = ((lfsr << 1) | bit) & 0x1FFu;
                        if (lock_count >= 18) {
                            locked = 1;
                            wbits = 0;
                            werr = 0;
                        }
                    }
                }
            }
            brt[0] = (int32_t)locked, brt[1] = (int32_t)lfsr, brt[2] = (int32_t)lock_count, brt[3] = (int32_t)wbits;
            brt[4] = (int32_t)werr, brt[5] = (int32_t)tbits, brt[6] = (int32_t)terr, brt[7] = (int32_t)resync;
            for (int i = 0; i < 8; i++) {
                brt_state[so * 8 + i] = brt[i];
            }
        }
        hunt_base = pos + (pat < 2 ? 8 : 184) + 1; // the lock: eight symbols behind a preamble word, 184 behind every other
    }
    // into the next call's row indexing
    const int adv = advance ? advance[ch] : 0;
    long long hb = (long long)hunt_base - adv;
    hb = hb < -(1ll << 30) ? -(1ll << 30) : hb;
    s->hunt_base = (int32_t)hb;
    s->pbc = pbc;
    for (int i = 0; i < 8; i++) {
        s->brt[i] = brt[i];
    }
    n_packets[ch] = np;
}
} // namespace

extern "C" size_t
ddn_dev_m17_data_state_bytes(void) {
    return sizeof(DdnM17DataState);
}

extern "C" hipError_t
ddn_dev_m17_pkt_cost(const uint8_t* rec, size_t stride, const int32_t* counts, const int32_t* sync_pos, const uint8_t* sync_pat,
                     const int32_t* n_sync, const float* sync_thr, int n_channels, int max_syncs, int lmax, uint16_t* cost420,
                     int32_t* slot_sync, uint8_t* slot_want, hipStream_t st) {
    hipLaunchKernelGGL(k_m17_pkt_cost, dim3((unsigned)n_channels, (unsigned)lmax), dim3(64), 0, st, rec, stride, counts, sync_pos, sync_pat,
                       n_sync, sync_thr, max_syncs, lmax, cost420, slot_sync, slot_want);
    return hipGetLastError();
}

extern "C" hipError_t
ddn_dev_m17_pkt_finish(const uint8_t* dec, int dec_stride, const uint32_t* cost, const int32_t* slot_sync, int n_channels, int lmax,
                       int max_syncs, uint8_t* pkt26, uint8_t* status, uint32_t* path_cost, hipStream_t st) {
    const int n = n_channels * lmax;
    hipLaunchKernelGGL(k_m17_pkt_finish, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, st, dec, dec_stride, cost, slot_sync, n_channels,
                       lmax, max_syncs, pkt26, status, path_cost);
    return hipGetLastError();
}

extern "C" hipError_t
ddn_dev_m17_brt_bits(const uint8_t* rec, size_t stride, const int32_t* counts, const int32_t* sync_pos, const uint8_t* sync_pat,
                     const int32_t* n_sync, int n_channels, int max_syncs, int lmax, uint8_t* sym402, int32_t* slot_sync,
                     uint8_t* slot_want, hipStream_t st) {
    hipLaunchKernelGGL(k_m17_brt_bits, dim3((unsigned)n_channels, (unsigned)lmax), dim3(64), 0, st, rec, stride, counts, sync_pos, sync_pat,
                       n_sync, max_syncs, lmax, sym402, slot_sync, slot_want);
    return hipGetLastError();
}

extern "C" hipError_t
ddn_dev_m17_brt_finish(const uint8_t* dec, int dec_stride, const int32_t* slot_sync, int n_channels, int lmax, int max_syncs,
                       uint8_t* bits25, uint8_t* status, hipStream_t st) {
    const int n = n_channels * lmax;
    hipLaunchKernelGGL(k_m17_brt_finish, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, st, dec, dec_stride, slot_sync, n_channels, lmax,
                       max_syncs, bits25, status);
    return hipGetLastError();
}

extern "C" hipError_t
ddn_dev_m17_data_walk(const uint8_t* sync_pat, const int32_t* sync_pos, const int32_t* n_sync, const int32_t* advance, int n_channels,
                      int max_syncs, const uint8_t* pkt26, const uint8_t* pkt_frame_status, const uint8_t* bits25,
                      const uint8_t* brt_frame_status, void* state, uint8_t* pkt_status, uint8_t* pkt_count, int32_t* brt_state,
                      uint8_t* packet, int32_t* packet_app_len, uint8_t* packet_crc_ok, int32_t* packet_slot, int32_t* n_packets,
                      int max_packets, hipStream_t st) {
    hipLaunchKernelGGL(k_m17_data_walk, dim3((unsigned)((n_channels + 63) / 64)), dim3(64), 0, st, sync_pat, sync_pos, n_sync, advance,
                       n_channels, max_syncs, pkt26, pkt_frame_status, bits25, brt_frame_status, (DdnM17DataState*)state, pkt_status,
                       pkt_count, brt_state, packet, packet_app_len, packet_crc_ok, packet_slot, n_packets, max_packets);
    return hipGetLastError();
}
