// ddn_dmr_ms.hip - DMR MS and direct-mode bursts behind the fsk4 receive loop (include/ddn_fsk4.h, "DMR MS / direct mode").
//
// The loop holds fixed counts behind the MS / direct-mode words (sync patterns 2..7): 264 symbols behind a data word, 1704 behind a
// voice word - what dmrMSData() and dmrMSBootstrap() + dmrMS() read (src/protocol/dmr/dmr_ms.c:420-497, 384-417, 323-381), neither
// with an early exit.  Where the bursts lie is therefore known from the sync alone; p = row index of the sync's last symbol:
//   data word    one burst: dibits 0..89 = the hand-over made at the sync, 90..143 = records p + 1 .. p + 54
//   voice word   the bootstrap burst ("VC*", VC 1) laid out the same way, then bursts k = 0..4 (VC k + 2) of 144 records from
//                p + 199 + 288 k (54 live + skipDibit(144) + 1, then 144 read / 144 skipped)
//   k_dmr_ms_walk          one lane per channel: this call's decode list and the open voice unit carried in the state -> the bursts
//                          that end in this call, in air order; TACT / slot type / EMB through ddn_bcode_dev.h; the sync fields filed
//                          under VC 2..6 (dmr_ms_collect_sync_bits(), :125-137) and the 8 x 16 matrix of dmr_dburst_handle_emb()
//                          (dmr_dburst.c:363-394) at VC 6; the colour code the reference would print
//   k_dmr_ms_data_gather   one workgroup per data burst: slot type, the 196 info bits, the 98 info dibits + reliabilities; zeros for
//                          a burst whose TACT or slot type failed (dmr_data_sync() stops there)
//   k_dmr_ms_voice_gather  one workgroup per voice burst: its three AMBE frames as 36 dibits each (hard: processMbeFrame gets no soft
//                          frame, :198-199)
// Everything behind the gathers is the BS path's: Golay(20,8), BPTC(196,96), RS(12,9), k_dmr_data_prep / _finish, the rate 3/4
// decoders and k_dmr_r34_pick, BPTC(128,77), k_dmr_emb_finish, the AMBE schedule, frame FEC and synthesis (ddn_api_dmr_ms.cpp).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddn_bcode_dev.h"
#include "ddn_device.h"

namespace {

constexpr int32_t UNUSED = INT32_MIN; // a start can lie up to 89 records before the row (those dibits come from the hand-over)

struct MsState {
    int32_t unit_pos; // the open voice unit's sync position in the row of the next call
    int32_t next;     // its next burst k, 5 = no unit open
    int32_t cc;       // state->dmr_color_code, 16 until one is learnt
    int32_t dropped;  // bursts that found no slot, since the start
    uint8_t frag[5][48]; // dmr_embedded_signalling[0][VC - 1], VC 2..6
};

__global__ void
k_dmr_ms_state_init(MsState* __restrict__ st, int n_channels) {
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= n_channels) {
        return;
    }
    MsState* s = st + ch;
    s->unit_pos = 0;
    s->next = 5;
    s->cc = 16;
    s->dropped = 0;
    for (int i = 0; i < 5 * 48; i++) {
        (&s->frag[0][0])[i] = 0;
    }
}

struct WalkArgs {
    const uint8_t* rec;
    const int32_t *counts, *n_new, *sync_pos, *n_sync;
    const uint8_t *sync_pat, *pre90;
    size_t max_sym;
    int n_channels, max_syncs, max_data, max_voice, max_lc;
    MsState* state;
    int32_t *n_data, *data_start, *data_pre, *data_gate;
    uint8_t *data_pat, *data_slot, *data_status, *data_cc;
    int32_t *n_voice, *voice_start, *voice_pre;
    uint8_t *voice_vc, *voice_tact, *voice_emb_ok, *voice_emb_cc, *voice_power, *voice_sync48;
    int32_t *n_lc, *lc_pos;
    uint8_t* lc_in128;
    int32_t *cc, *dropped, *phase;
};

// dibit d of a burst that starts at row index `start`; ps >= 0: its first 90 dibits are hand-over ps
__device__ __forceinline__ int
burst_dibit(const WalkArgs& a, int ch, int start, long ps, int d) {
    if (ps >= 0 && d < 90) {
        return a.pre90[(size_t)ps * 90 + d] & 3;
    }
    return a.rec[((size_t)ch * a.max_sym + (size_t)(start + d)) * 10] & 3;
}

// One lane per channel.  Cycle bursts are emitted in the call whose row holds their last symbol (their first is at most 143 records
// back, inside the carry), data and bootstrap bursts in the call that decodes their sync (the carry exceeds 54).
__global__ __launch_bounds__(64) void
k_dmr_ms_walk(const WalkArgs a) {
    const int ch = blockIdx.x * 64 + threadIdx.x;
    if (ch >= a.n_channels) {
        return;
    }
    MsState* s = a.state + ch;
    int unit = s->unit_pos, next = s->next, cc = s->cc, lost = 0;
    int nd = 0, nv = 0, nl = 0;
    const int cnt = a.counts[ch] < (long)a.max_sym ? a.counts[ch] : (int)a.max_sym;
    const int ns = a.n_sync[ch] < a.max_syncs ? a.n_sync[ch] : a.max_syncs;

    // a voice burst: EMB QR(16,7,6) (dmr_ms_decode_embedded_color_code(), :139-152), the sync field's 48 bits
    auto voice = [&](int start, long ps, int vc) {
        uint32_t emb = 0, tact = 0;
        uint8_t* frag = vc >= 2 ? s->frag[vc - 2] : nullptr;
        const bool have = nv < a.max_voice;
        const size_t so = (size_t)ch * a.max_voice + nv;
        for (int i = 0; i < 24; i++) {
            const int d = burst_dibit(a, ch, start, ps, 66 + i);
            const uint8_t hi = (uint8_t)(d >> 1), lo = (uint8_t)(d & 1);
            if (frag) {
                frag[2 * i] = hi;
                frag[2 * i + 1] = lo;
            }
            if (have) {
                a.voice_sync48[so * 48 + 2 * i] = hi;
                a.voice_sync48[so * 48 + 2 * i + 1] = lo;
            }
            if (i < 4) {
                emb |= (uint32_t)hi << (2 * i) | (uint32_t)lo << (2 * i + 1);
            } else if (i >= 20) {
                emb |= (uint32_t)hi << (8 + 2 * (i - 20)) | (uint32_t)lo << (9 + 2 * (i - 20));
            }
        }
        int emb_ok = 0xFF, emb_cc = 0xFF, power = 9, tact_ok = 0xFF;
        if (vc >= 2) {
            // dmr_ms_decode_tact() (:95-101) hands the first seven CACH dibits over as if they were bits: their low bits decide the
            // syndrome.  The reference ignores the answer; it is reported as computed
            for (int i = 0; i < 7; i++) {
                tact |= (uint32_t)(burst_dibit(a, ch, start, ps, i) & 1) << i;
            }
            tact_ok = ddn_bcode::decode(ddn_bcode::HAMMING_7_4, tact) ? 1 : 0;
            emb_ok = ddn_bcode::decode(ddn_bcode::QR_16_7_6, emb) ? 1 : 0;
            if (emb_ok) {
                emb_cc = (int)(((emb & 1) << 3) | (((emb >> 1) & 1) << 2) | (((emb >> 2) & 1) << 1) | ((emb >> 3) & 1));
                power = (int)((emb >> 4) & 1);
                cc = emb_cc;
            }
        }
        if (have) {
            a.voice_start[so] = start;
            a.voice_pre[so] = (int32_t)ps;
            a.voice_vc[so] = (uint8_t)vc;
            a.voice_tact[so] = (uint8_t)tact_ok;
            a.voice_emb_ok[so] = (uint8_t)emb_ok;
            a.voice_emb_cc[so] = (uint8_t)emb_cc;
            a.voice_power[so] = (uint8_t)power;
            nv++;
        } else {
            lost++;
        }
        if (vc == 6) { // dmr_ms_handle_vc6_ops(): dmr_data_burst_handler(.., 0xEB, ..) over the fragments of VC 2..5
            if (nl < a.max_lc) {
                const size_t lo = (size_t)ch * a.max_lc + nl;
                uint8_t* m = a.lc_in128 + lo * 128;
                int q = 0, burst = 0;
                for (int col = 0; col < 16; col++) {
                    for (int row = 0; row < 8; row++) {
                        m[row * 16 + col] = s->frag[burst][q + 8];
                        if (++q >= 32) {
                            q = 0;
                            burst++;
                        }
                    }
                }
                a.lc_pos[lo] = start + 143;
                nl++;
            } else {
                lost++;
            }
        }
    };
    // the open unit's bursts whose last symbol this row holds and that begin before row index `before`
    auto cycle = [&](int before) {
        while (next < 5) {
            const int start = unit + 199 + 288 * next;
            if (start + 143 >= cnt || start >= before || start < 0) {
                break;
            }
            voice(start, -1, next + 2);
            next++;
        }
    };

    for (int j = 0; j < ns; j++) {
        const size_t sj = (size_t)ch * a.max_syncs + j;
        const int p = a.sync_pos[sj], pat = a.sync_pat[sj];
        if (pat < 2 || pat > 7 || p < 0 || p + 54 >= cnt) { // BS / RC words; a stream that ends inside the burst (the flush)
            continue;
        }
        cycle(p);
        if (pat == 3 || pat >= 6) { // dmrMSBootstrap()
            voice(p - 89, (long)sj, 1);
            unit = p;
            next = 0;
            continue;
        }
        // dmrMSData() -> dmr_data_sync() with dmr_stereo = 1, dmr_ms_mode = 1: TACT over the de-interleaved CACH (the seven TACT bits
        // are the high bits of CACH dibits 0, 2, 4, 6, 7, 9, 11: dmr_cach_interleave[], dmr_cach.h), slot type, no confidence gate
        int status = 0, bcc = 0xFF;
        uint32_t tact = 0, st = 0;
        for (int i = 0; i < 7; i++) {
            const int d = a.pre90[sj * 90 + ((0xB976420u >> (4 * i)) & 0xF)];
            tact |= (uint32_t)((d >> 1) & 1) << i;
        }
        if (!ddn_bcode::decode(ddn_bcode::HAMMING_7_4, tact)) {
            status = 1;
        } else {
            for (int i = 0; i < 5; i++) {
                const int x = a.pre90[sj * 90 + 61 + i] & 3, y = burst_dibit(a, ch, p - 89, -1, 90 + i);
                st |= (uint32_t)((x >> 1) & 1) << (2 * i) | (uint32_t)(x & 1) << (2 * i + 1);
                st |= (uint32_t)((y >> 1) & 1) << (10 + 2 * i) | (uint32_t)(y & 1) << (11 + 2 * i);
            }
            if (!ddn_bcode::decode(ddn_bcode::GOLAY_20_8, st)) {
                status = 2;
            } else {
                bcc = (int)(((st & 1) << 3) | (((st >> 1) & 1) << 2) | (((st >> 2) & 1) << 1) | ((st >> 3) & 1));
                cc = bcc; // state->dmr_color_code = state->color_code (dmr_data.c:246-248)
            }
        }
        if (nd < a.max_data) {
            const size_t so = (size_t)ch * a.max_data + nd;
            a.data_start[so] = p - 89;
            a.data_pre[so] = (int32_t)sj;
            a.data_gate[so] = status == 0 ? 0 : -1;
            a.data_pat[so] = (uint8_t)pat;
            a.data_slot[so] = pat == 5 ? 1 : 0; // dmr_data_collect_sync(): the direct-mode TS2 data word names slot 2
            a.data_status[so] = (uint8_t)status;
            a.data_cc[so] = (uint8_t)bcc;
            nd++;
        } else {
            lost++;
        }
    }
    cycle(0x7FFFFFFF);

    for (int k = nd; k < a.max_data; k++) {
        const size_t so = (size_t)ch * a.max_data + k;
        a.data_start[so] = UNUSED;
        a.data_pre[so] = -1;
        a.data_gate[so] = -1;
        a.data_pat[so] = a.data_slot[so] = a.data_status[so] = a.data_cc[so] = 0xFF;
    }
    for (int k = nv; k < a.max_voice; k++) {
        const size_t so = (size_t)ch * a.max_voice + k;
        a.voice_start[so] = UNUSED;
        a.voice_pre[so] = -1;
        a.voice_vc[so] = 0;
        a.voice_tact[so] = a.voice_emb_ok[so] = a.voice_emb_cc[so] = a.voice_power[so] = 0xFF;
        for (int i = 0; i < 48; i++) {
            a.voice_sync48[so * 48 + i] = 0;
        }
    }
    for (int k = nl; k < a.max_lc; k++) {
        const size_t lo = (size_t)ch * a.max_lc + k;
        a.lc_pos[lo] = -1;
        for (int i = 0; i < 128; i++) {
            a.lc_in128[lo * 128 + i] = 0;
        }
    }
    a.n_data[ch] = nd;
    a.n_voice[ch] = nv;
    a.n_lc[ch] = nl;
    s->unit_pos = unit - a.n_new[ch];
    s->next = next;
    s->cc = cc;
    s->dropped += lost;
    a.cc[ch] = cc;
    a.dropped[ch] = s->dropped;
    a.phase[ch] = next;
}

__global__ __launch_bounds__(64) void
k_dmr_ms_data_gather(const uint8_t* __restrict__ rec, size_t max_sym, const int32_t* __restrict__ dstart, const int32_t* __restrict__ dpre,
                     const int32_t* __restrict__ gate, const uint8_t* __restrict__ pre90, const uint8_t* __restrict__ prel90, int max_data,
                     uint8_t* __restrict__ slot_type, uint8_t* __restrict__ info, uint8_t* __restrict__ td98, uint8_t* __restrict__ rel98) {
    const int k = blockIdx.x, ch = blockIdx.y, t = threadIdx.x;
    const size_t so = (size_t)ch * max_data + k;
    const bool live = gate[so] >= 0;
    const long start = live ? (long)dstart[so] : 0, ps = live ? (long)dpre[so] : 0;
    for (int d = 12 + t; d < 144; d += 64) {
        int dibit = 0, rel = 0;
        if (live && d < 90) {
            dibit = pre90[(size_t)ps * 90 + d] & 3;
            rel = prel90[(size_t)ps * 90 + d];
        } else if (live) {
            const uint8_t* rr = rec + ((size_t)ch * max_sym + (size_t)(start + d)) * 10;
            dibit = rr[0] & 3;
            rel = rr[1];
        }
        const uint8_t hi = (uint8_t)((dibit >> 1) & 1), lo = (uint8_t)(dibit & 1);
        if (d < 61) {
            info[so * 196 + 2 * (d - 12)] = hi;
            info[so * 196 + 2 * (d - 12) + 1] = lo;
            td98[so * 98 + (d - 12)] = (uint8_t)dibit;
            rel98[so * 98 + (d - 12)] = (uint8_t)rel;
        } else if (d < 66) {
            slot_type[so * 20 + 2 * (d - 61)] = hi;
            slot_type[so * 20 + 2 * (d - 61) + 1] = lo;
        } else if (d < 90) {
            // the sync word
        } else if (d < 95) {
            slot_type[so * 20 + 10 + 2 * (d - 90)] = hi;
            slot_type[so * 20 + 10 + 2 * (d - 90) + 1] = lo;
        } else {
            info[so * 196 + 98 + 2 * (d - 95)] = hi;
            info[so * 196 + 98 + 2 * (d - 95) + 1] = lo;
            td98[so * 98 + 49 + (d - 95)] = (uint8_t)dibit;
            rel98[so * 98 + 49 + (d - 95)] = (uint8_t)rel;
        }
    }
}

// frame 1 = dibits 12..47, frame 2 = 48..65 + 90..107, frame 3 = 108..143 (dmr_ms_decode_bootstrap_voice(), :285-291; dmrMS(), :352-357)
__global__ __launch_bounds__(128) void
k_dmr_ms_voice_gather(const uint8_t* __restrict__ rec, size_t max_sym, const int32_t* __restrict__ vstart, const int32_t* __restrict__ vpre,
                      const uint8_t* __restrict__ vc, const uint8_t* __restrict__ pre90, int max_voice, uint8_t* __restrict__ dib108,
                      uint8_t* __restrict__ skip3) {
    const int k = blockIdx.x, ch = blockIdx.y, t = threadIdx.x;
    const size_t so = (size_t)ch * max_voice + k;
    const bool live = vc[so] != 0;
    if (t < 3) {
        skip3[so * 3 + t] = live ? 0 : 0xFF;
    }
    if (t >= 108) {
        return;
    }
    const int d = t < 54 ? 12 + t : 90 + (t - 54);
    int dibit = 0;
    if (live) {
        const long ps = vpre[so];
        dibit = (ps >= 0 && d < 90) ? pre90[(size_t)ps * 90 + d] & 3 : rec[((size_t)ch * max_sym + (size_t)((long)vstart[so] + d)) * 10] & 3;
    }
    dib108[so * 108 + t] = (uint8_t)dibit;
}

} // namespace

extern "C" size_t
ddn_dev_dmr_ms_state_bytes(void) {
    return sizeof(MsState);
}

extern "C" hipError_t
ddn_dev_dmr_ms_state_init(void* state, int n_channels, hipStream_t st) {
    hipLaunchKernelGGL(k_dmr_ms_state_init, dim3((unsigned)((n_channels + 63) / 64)), dim3(64), 0, st, (MsState*)state, n_channels);
    return hipGetLastError();
}

extern "C" hipError_t
ddn_dev_dmr_ms_walk(const DdnDmrMsWalk* w, hipStream_t st) {
    WalkArgs a;
    a.rec = w->rec, a.counts = w->counts, a.n_new = w->n_new, a.sync_pos = w->sync_pos, a.n_sync = w->n_sync, a.sync_pat = w->sync_pat;
    a.pre90 = w->pre90, a.max_sym = w->max_sym, a.n_channels = w->n_channels, a.max_syncs = w->max_syncs, a.max_data = w->max_data;
    a.max_voice = w->max_voice, a.max_lc = w->max_lc, a.state = (MsState*)w->state, a.n_data = w->n_data, a.data_start = w->data_start;
    a.data_pre = w->data_pre, a.data_gate = w->data_gate, a.data_pat = w->data_pat, a.data_slot = w->data_slot;
    a.data_status = w->data_status, a.data_cc = w->data_cc, a.n_voice = w->n_voice, a.voice_start = w->voice_start;
    a.voice_pre = w->voice_pre, a.voice_vc = w->voice_vc, a.voice_tact = w->voice_tact, a.voice_emb_ok = w->voice_emb_ok;
    a.voice_emb_cc = w->voice_emb_cc, a.voice_power = w->voice_power, a.voice_sync48 = w->voice_sync48, a.n_lc = w->n_lc;
    a.lc_pos = w->lc_pos, a.lc_in128 = w->lc_in128, a.cc = w->cc, a.dropped = w->dropped, a.phase = w->phase;
    hipLaunchKernelGGL(k_dmr_ms_walk, dim3((unsigned)((w->n_channels + 63) / 64)), dim3(64), 0, st, a);
    return hipGetLastError();
}

extern "C" hipError_t
ddn_dev_dmr_ms_data_gather(const uint8_t* rec, size_t max_sym, const int32_t* dstart, const int32_t* dpre, const int32_t* gate,
                           const uint8_t* pre90, const uint8_t* prel90, int max_data, int n_channels, uint8_t* slot_type, uint8_t* info,
                           uint8_t* td98, uint8_t* rel98, hipStream_t st) {
    hipLaunchKernelGGL(k_dmr_ms_data_gather, dim3((unsigned)max_data, (unsigned)n_channels), dim3(64), 0, st, rec, max_sym, dstart, dpre, gate,
                       pre90, prel90, max_data, slot_type, info, td98, rel98);
    return hipGetLastError();
}

extern "C" hipError_t
ddn_dev_dmr_ms_voice_gather(const uint8_t* rec, size_t max_sym, const int32_t* vstart, const int32_t* vpre, const uint8_t* vc,
                            const uint8_t* pre90, int max_voice, int n_channels, uint8_t* dib108, uint8_t* skip3, hipStream_t st) {
    hipLaunchKernelGGL(k_dmr_ms_voice_gather, dim3((unsigned)max_voice, (unsigned)n_channels), dim3(128), 0, st, rec, max_sym, vstart, vpre, vc,
                       pre90, max_voice, dib108, skip3);
    return hipGetLastError();
}
