// ddn_api_nxdn_ctrl.cpp - C-ABI of the NXDN control and data channels (include/ddn_fsk4.h, "NXDN control and data channels"; kernels
// in ddn_nxdn_ctrl.hip, the two decoders in ddn_trellis.hip and ddn_fec3.hip).  Device pointers, asynchronous on the stream.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ddn_api_util.h"
#include "ddn_device.h"
#include "ddn_fsk4.h"

extern "C" size_t
ddn_nxdn_ctrl_state_bytes(void) {
    return ddn_dev_nxdn_ctrl_state_bytes();
}

extern "C" int
ddn_nxdn_ctrl_state_init(void* d_state, size_t n_channels, void* hip_stream) {
    if (!d_state || n_channels == 0 || n_channels > (1u << 24)) {
        ddn_set_error("ddn_nxdn_ctrl_state_init: bad argument");
        return DDN_EINVAL;
    }
    HIP_TRY(ddn_dev_nxdn_ctrl_state_init(d_state, (int)n_channels, (hipStream_t)hip_stream));
    return DDN_OK;
}

// what both calls ask of the slot layout
static bool
slots_ok(const ddn_nxdn_ctrl_input* in) {
    return in && in->n_channels > 0 && in->max_syncs > 0 && in->max_syncs <= (1u << 24) && in->d_n_sync
           && (size_t)in->n_channels * in->max_syncs <= ((size_t)1 << 30);
}

extern "C" int
ddn_nxdn_ctrl_decode_batch(const ddn_nxdn_ctrl_input* in, const ddn_nxdn_ctrl_frames* out, void* hip_stream) {
    if (!slots_ok(in) || !out || !in->d_records10 || !in->d_counts || !in->d_sync_pos || in->max_symbols == 0 || !out->d_kind) {
        ddn_set_error("ddn_nxdn_ctrl_decode_batch: bad argument (records, counts, sync positions and counts, d_kind given)");
        return DDN_EINVAL;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    const size_t S = (size_t)in->n_channels * in->max_syncs;
    // the decoders' rows: 175 steps (CAC) and 203 (FACCH2 / UDCH) - symbols, reliabilities, hard bits; their results; the wanted flags
    DdnScratch s(st);
    uint8_t *sym_c, *rel_c, *hard_c, *sym_f, *rel_f, *hard_f, *soft_c, *soft_f, *dec_c, *dec_f, *want_c, *want_f;
    HIP_TRY(s.arena(S * (3 * 350 + 3 * 406 + 2 * 26 + 2 * 208 + 2) + 12 * 256));
    HIP_TRY(s.get(&sym_c, S * 350));
    HIP_TRY(s.get(&rel_c, S * 350));
    HIP_TRY(s.get(&hard_c, S * 350));
    HIP_TRY(s.get(&sym_f, S * 406));
    HIP_TRY(s.get(&rel_f, S * 406));
    HIP_TRY(s.get(&hard_f, S * 406));
    HIP_TRY(s.get(&soft_c, S * 26));
    HIP_TRY(s.get(&soft_f, S * 26));
    HIP_TRY(s.get(&dec_c, S * 208));
    HIP_TRY(s.get(&dec_f, S * 208));
    HIP_TRY(s.get(&want_c, S));
    HIP_TRY(s.get(&want_f, S));
    HIP_TRY(ddn_dev_nxdn_ctrl_gather(in->d_records10, in->d_counts, in->max_symbols, in->d_sync_pos, in->d_n_sync, in->n_channels,
                                     (int)in->max_syncs, out->d_kind, sym_c, rel_c, hard_c, sym_f, rel_f, hard_f, want_c, want_f, st));
    // (blocks of 16 slots none of which is wanted are left alone by the soft decoder, single slots by the greedy one)
    HIP_TRY(ddn_dev_k5_nxdn_wanted(sym_c, rel_c, (int)S, 175, 171, nullptr, soft_c, 26, want_c, 1, st));
    HIP_TRY(ddn_dev_trellis_greedy_wanted(hard_c, 350, S, 171, dec_c, 208, want_c, st));
    HIP_TRY(ddn_dev_k5_nxdn_wanted(sym_f, rel_f, (int)S, 203, 199, nullptr, soft_f, 26, want_f, 1, st));
    HIP_TRY(ddn_dev_trellis_greedy_wanted(hard_f, 406, S, 199, dec_f, 208, want_f, st));
    HIP_TRY(ddn_dev_nxdn_ctrl_finish(out->d_kind, soft_c, soft_f, dec_c, dec_f, S, out->d_bits208, out->d_bytes26, out->d_crc_ok,
                                     out->d_fallback, out->d_ran, out->d_sf, st));
    return DDN_OK;
}

extern "C" int
ddn_nxdn_ctrl_walk_batch(const ddn_nxdn_ctrl_input* in, const ddn_nxdn_ctrl_frames* fr, void* d_state, const ddn_nxdn_ctrl_messages* out,
                         void* hip_stream) {
    if (!slots_ok(in) || !fr || !d_state || !out || !in->d_lich || !in->d_valid || !in->d_sacch || !in->d_sacch_ok || !in->d_sacch_hard
        || !in->d_sacch_hard_ok || !fr->d_kind || !fr->d_crc_ok || !fr->d_ran || !fr->d_sf) {
        ddn_set_error("ddn_nxdn_ctrl_walk_batch: bad argument (LICH, valid and the four SACCH arrays, d_kind, d_crc_ok, d_ran, d_sf and the "
                      "state given)");
        return DDN_EINVAL;
    }
    HIP_TRY(ddn_dev_nxdn_ctrl_walk(in->d_n_sync, in->n_channels, (int)in->max_syncs, in->d_lich, in->d_valid, in->d_sacch, in->d_sacch_ok,
                                   in->d_sacch_hard, in->d_sacch_hard_ok, fr->d_kind, fr->d_crc_ok, fr->d_ran, fr->d_sf, d_state,
                                   out->d_sacch_status, out->d_pf, out->d_seq_ok, out->d_msg72, out->d_msg_status, out->d_last_ran,
                                   out->d_cac_fail, (hipStream_t)hip_stream));
    return DDN_OK;
}
