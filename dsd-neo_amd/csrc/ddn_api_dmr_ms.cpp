// ddn_api_dmr_ms.cpp - C-ABI of the DMR MS / direct-mode stage (include/ddn_fsk4.h, "DMR MS / direct mode"; kernels in ddn_dmr_ms.hip,
// everything behind the gathers is the BS data-burst / embedded-signalling / voice path's).  Device pointers, asynchronous on the stream.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ddn_api_util.h"
#include "ddn_device.h"
#include "ddn_fsk4.h"
#include "ddn_hip.h"
#include "ddn_mbe.h"

extern "C" size_t
ddn_dmr_ms_state_bytes(void) {
    return ddn_dev_dmr_ms_state_bytes();
}

extern "C" int
ddn_dmr_ms_state_init(void* d_state, size_t n_channels, void* hip_stream) {
    if (!d_state || n_channels == 0 || n_channels > (1u << 24)) {
        ddn_set_error("ddn_dmr_ms_state_init: bad argument");
        return DDN_EINVAL;
    }
    HIP_TRY(ddn_dev_dmr_ms_state_init(d_state, (int)n_channels, (hipStream_t)hip_stream));
    return DDN_OK;
}

// what all three calls ask of the rows and of the list sizes
static bool
shape_ok(const ddn_dmr_ms_input* in, const ddn_dmr_ms_bursts* b) {
    const int cap = 1 << 20;
    return in && b && in->n_channels > 0 && in->n_channels <= (1 << 24) && in->max_symbols > 0 && in->max_symbols <= ((size_t)1 << 30)
           && in->max_syncs > 0 && in->max_syncs <= (1u << 24) && (size_t)in->n_channels * in->max_syncs <= ((size_t)1 << 30) && in->d_records10
           && b->max_data > 0 && b->max_data <= cap && b->max_voice > 0 && b->max_voice <= cap && b->max_lc > 0 && b->max_lc <= cap;
}

extern "C" int
ddn_dmr_ms_walk_batch(const ddn_dmr_ms_input* in, void* d_state, const ddn_dmr_ms_bursts* o, void* hip_stream) {
    if (!shape_ok(in, o) || !d_state || !in->d_counts || !in->d_new || !in->d_sync_pos || !in->d_sync_pat || !in->d_n_sync || !in->d_pre
        || !o->d_n_data || !o->d_data_start || !o->d_data_sync || !o->d_data_gate || !o->d_data_pat || !o->d_data_slot || !o->d_data_status
        || !o->d_data_cc || !o->d_n_voice || !o->d_voice_start || !o->d_voice_pre || !o->d_voice_vc || !o->d_voice_tact_ok || !o->d_voice_emb_ok
        || !o->d_voice_emb_cc || !o->d_voice_power || !o->d_voice_sync48 || !o->d_n_lc || !o->d_lc_pos || !o->d_lc_in128 || !o->d_cc
        || !o->d_dropped || !o->d_phase) {
        ddn_set_error("ddn_dmr_ms_walk_batch: bad argument (records, counts, d_new, the sync list with its hand-overs, the state and every "
                      "list of ddn_dmr_ms_bursts given; 1 .. 2^20 entries per list)");
        return DDN_EINVAL;
    }
    const DdnDmrMsWalk w{in->d_records10, in->d_counts,   in->d_new,         in->d_sync_pos,    in->d_n_sync,      in->d_sync_pat,   in->d_pre,
                         in->max_symbols, in->n_channels, (int)in->max_syncs, o->max_data,      o->max_voice,      o->max_lc,        d_state,
                         o->d_n_data,     o->d_data_start, o->d_data_sync,   o->d_data_gate,    o->d_data_pat,     o->d_data_slot,   o->d_data_status,
                         o->d_data_cc,    o->d_n_voice,   o->d_voice_start,  o->d_voice_pre,    o->d_voice_vc,     o->d_voice_tact_ok, o->d_voice_emb_ok,
                         o->d_voice_emb_cc, o->d_voice_power, o->d_voice_sync48, o->d_n_lc,     o->d_lc_pos,       o->d_lc_in128,    o->d_cc,
                         o->d_dropped,    o->d_phase};
    HIP_TRY(ddn_dev_dmr_ms_walk(&w, (hipStream_t)hip_stream));
    return DDN_OK;
}

extern "C" int
ddn_dmr_ms_data_batch(const ddn_dmr_ms_input* in, const ddn_dmr_ms_bursts* b, const ddn_dmr_ms_data* o, void* hip_stream) {
    if (!shape_ok(in, b) || !o || !in->d_pre || !in->d_pre_rel || !b->d_data_start || !b->d_data_sync || !b->d_data_gate || !o->d_type
        || !o->d_info196 || !o->d_bits96 || !o->d_bytes12 || !o->d_errs || !o->d_crc || !o->d_r34_unconfirmed || !o->d_r34_confirmed
        || !o->d_r34_confirmed_crc || !o->d_r34_pool || !o->d_r34_pool_n) {
        ddn_set_error("ddn_dmr_ms_data_batch: bad argument (records, both hand-over arrays, the walk's d_data_start / _sync / _gate and every "
                      "array of ddn_dmr_ms_data given)");
        return DDN_EINVAL;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    const size_t D = (size_t)in->n_channels * (size_t)b->max_data;
    DdnScratch s(st);
    uint8_t *sty, *st_ok, *td, *rel, *r3, *cw, *rsres, *rsfound, *want, *hard, *soft, *list, *backs;
    int32_t* listn;
    HIP_TRY(s.arena(D * (20 + 1 + 98 + 98 + 3 + 12 + 1 + 1 + 1 + 18 + 18 + 32 * 24 + 49 * 8 * 32 + 4) + 15 * 256));
    HIP_TRY(s.get(&sty, D * 20));
    HIP_TRY(s.get(&st_ok, D));
    HIP_TRY(s.get(&td, D * 98));
    HIP_TRY(s.get(&rel, D * 98));
    HIP_TRY(s.get(&r3, D * 3));
    HIP_TRY(s.get(&cw, D * 12));
    HIP_TRY(s.get(&rsres, D));
    HIP_TRY(s.get(&rsfound, D));
    HIP_TRY(s.get(&want, D));
    HIP_TRY(s.get(&hard, D * 18));
    HIP_TRY(s.get(&soft, D * 18));
    HIP_TRY(s.get(&list, D * 32 * 24));
    HIP_TRY(s.get(&backs, D * 49 * 8 * 32));
    HIP_TRY(s.get(&listn, D));
    HIP_TRY(ddn_dev_dmr_ms_data_gather(in->d_records10, in->max_symbols, b->d_data_start, b->d_data_sync, b->d_data_gate, in->d_pre, in->d_pre_rel,
                                       b->max_data, in->n_channels, sty, o->d_info196, td, rel, st));
    // from here on: dmr_decode()'s data-burst stage (ddn_api_chain_fsk4.cpp) on this list; d_data_gate stands in for its start array
    DDN_TRY(ddn_fec_block_code_batch(5 /* DDN_CODE_GOLAY_20_8 */, sty, D, 1, nullptr, st_ok, st));
    DDN_TRY(ddn_fec_bptc_196x96_batch(o->d_info196, 1, D, o->d_bits96, r3, o->d_errs, st));
    HIP_TRY(ddn_dev_dmr_data_prep(b->d_data_gate, sty, st_ok, o->d_bits96, (int)D, o->d_type, o->d_bytes12, cw, st));
    DDN_TRY(ddn_fec_rs_12_9_batch(cw, D, rsres, rsfound, nullptr, st));
    HIP_TRY(ddn_dev_dmr_data_finish(o->d_type, o->d_bits96, o->d_info196, cw, rsres, (int)D, o->d_bytes12, o->d_crc, want, st));
    DDN_TRY(ddn_fec_r34_batch(td, nullptr, D, hard, st));
    DDN_TRY(ddn_fec_r34_batch(td, rel, D, soft, st));
    HIP_TRY(ddn_dev_r34_list_wanted(td, rel, (int)D, 32, want, backs, (uint32_t*)list, listn, st));
    HIP_TRY(ddn_dev_dmr_r34_pick(td, rel, want, hard, soft, list, listn, (int)D, (uint8_t*)o->d_r34_pool, o->d_r34_pool_n, o->d_r34_unconfirmed,
                                 o->d_r34_confirmed, o->d_r34_confirmed_crc, st));
    return DDN_OK;
}

extern "C" int
ddn_dmr_ms_voice_batch(const ddn_dmr_ms_input* in, const ddn_dmr_ms_bursts* b, const ddn_dmr_ms_voice* o, void* mbe_batch, void* hip_stream) {
    if (!shape_ok(in, b) || !o || !in->d_pre || !b->d_voice_start || !b->d_voice_pre || !b->d_voice_vc || !b->d_lc_pos || !b->d_lc_in128
        || !o->d_ambe_frames || !o->d_skip || !o->d_lc77 || !o->d_lc_errs || !o->d_lc_ok
        || (mbe_batch && (!o->d_ambe_bits || !o->d_ambe_result || !o->d_pcm))) {
        ddn_set_error("ddn_dmr_ms_voice_batch: bad argument (records, the hand-overs, the walk's d_voice_start / _pre / _vc and d_lc_pos / "
                      "_in128, the frame, skip and link-control arrays given; with a vocoder batch d_ambe_bits, d_ambe_result and d_pcm too)");
        return DDN_EINVAL;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    const size_t V = (size_t)in->n_channels * (size_t)b->max_voice, L = (size_t)in->n_channels * (size_t)b->max_lc;
    DdnScratch s(st);
    uint8_t* dib;
    int32_t* res;
    HIP_TRY(s.arena(V * 108 + V * 3 * 5 * sizeof(int32_t) + 2 * 256));
    HIP_TRY(s.get(&dib, V * 108));
    HIP_TRY(s.get(&res, V * 3 * 5));
    HIP_TRY(ddn_dev_dmr_ms_voice_gather(in->d_records10, in->max_symbols, b->d_voice_start, b->d_voice_pre, b->d_voice_vc, in->d_pre, b->max_voice,
                                        in->n_channels, dib, o->d_skip, st));
    HIP_TRY(ddn_dev_ambe2450_deinterleave(dib, nullptr, (int)(V * 3), o->d_ambe_frames, nullptr, st));
    DDN_TRY(ddn_fec_bptc_128x77_batch(b->d_lc_in128, L, o->d_lc77, o->d_lc_errs, st));
    HIP_TRY(ddn_dev_dmr_emb_finish(o->d_lc77, b->d_lc_pos, (int)L, o->d_lc_ok, st));
    if (mbe_batch) { // hard bits: processMbeFrame(opts, state, NULL, ambe_fr, NULL), dmr_ms.c:198-199
        DDN_TRY(ddn_mbe_frame_decode_batch(DDN_MBE_AMBE_3600X2450, o->d_ambe_frames, nullptr, V * 3, o->d_ambe_bits, res, st));
        DDN_TRY(ddn_mbe_result_skip_batch(o->d_skip, V * 3, res, st));
        DDN_TRY(ddn_mbe_synth_batch((ddn_mbe_batch*)mbe_batch, o->d_ambe_bits, res, (size_t)b->max_voice * 3, o->d_pcm, o->d_ambe_result, st));
    }
    return DDN_OK;
}
