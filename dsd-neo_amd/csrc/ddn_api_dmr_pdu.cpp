// ddn_api_dmr_pdu.cpp - C-ABI of the DMR protocol layer behind the data bursts (include/ddn_fsk4.h, "DMR data PDUs"; kernels in
// ddn_dmr_pdu.hip).  Device pointers, asynchronous on the stream.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ddn_api_util.h"
#include "ddn_device.h"
#include "ddn_fsk4.h"

extern "C" size_t
ddn_dmr_pdu_state_bytes(void) {
    return ddn_dev_dmr_pdu_state_bytes();
}

extern "C" int
ddn_dmr_pdu_walk_batch(const ddn_dmr_pdu_input* in, void* d_state, const ddn_dmr_pdu_output* o, void* hip_stream) {
    if (!in || !o || !d_state || in->n_channels <= 0 || in->max_bursts <= 0 || in->max_bursts > (1 << 20) || in->max_marks <= 0
        || in->max_marks > (1 << 20) || !in->d_n_bursts || !in->d_slot || !in->d_type || !in->d_bytes12 || !in->d_info196 || !in->d_errs
        || !in->d_crc || !in->d_unconfirmed18 || !in->d_pool || !in->d_pool_n || !in->d_n_resets || !in->d_reset_before || !in->d_n_losses
        || !in->d_loss_before || o->max_pdus < 1 || o->max_pdus > 8 || !o->d_burst_conf || !o->d_burst_counter || !o->d_burst_crc
        || !o->d_burst_dbsn || !o->d_burst_pick || !o->d_burst_status || !o->d_n_pdus || !o->d_pdu_kind || !o->d_pdu_slot || !o->d_pdu_burst
        || !o->d_pdu_len || !o->d_pdu_bytes || !o->d_pdu_crc4 || !o->d_pdu_block_crc || !o->d_pdu_header9) {
        ddn_set_error("ddn_dmr_pdu_walk_batch: bad argument (1 .. 8 PDU slots, every array given)");
        return DDN_EINVAL;
    }
    HIP_TRY(ddn_dev_dmr_pdu_walk(in->d_n_bursts, in->n_channels, in->max_bursts, in->d_slot, in->d_type, in->d_bytes12, in->d_info196, in->d_errs,
                                 in->d_crc, in->d_unconfirmed18, in->d_pool, in->d_pool_n, in->d_n_resets, in->d_reset_before, in->d_n_losses,
                                 in->d_loss_before, in->max_marks, d_state, o->d_burst_conf, o->d_burst_counter, o->d_burst_crc, o->d_burst_dbsn,
                                 o->d_burst_pick, o->d_burst_status, o->d_pdu_kind, o->d_pdu_slot, o->d_pdu_burst, o->d_pdu_len, o->d_pdu_bytes,
                                 o->d_pdu_crc4, o->d_pdu_block_crc, o->d_pdu_header9, o->max_pdus, o->d_n_pdus, (hipStream_t)hip_stream));
    return DDN_OK;
}

extern "C" int
ddn_dmr_pdu_marks_batch(const int32_t* d_events, const int32_t* d_n_events, size_t max_events, const uint8_t* d_flags, size_t stride_symbols,
                        int carry_symbols, const int32_t* d_new, const int32_t* d_burst_start, const int32_t* d_n_bursts, int n_channels,
                        int max_bursts, void* d_state, int32_t* d_reset_before, int32_t* d_n_resets, int32_t* d_loss_before, int32_t* d_n_losses,
                        int max_marks, void* hip_stream) {
    if (!d_events || !d_n_events || max_events == 0 || max_events > (1u << 24) || !d_flags || stride_symbols == 0 || carry_symbols < 0 || !d_new
        || !d_burst_start || !d_n_bursts || n_channels <= 0 || max_bursts <= 0 || !d_state || !d_reset_before || !d_n_resets || !d_loss_before
        || !d_n_losses || max_marks <= 0) {
        ddn_set_error("ddn_dmr_pdu_marks_batch: bad argument");
        return DDN_EINVAL;
    }
    HIP_TRY(ddn_dev_dmr_pdu_marks(d_events, d_n_events, (int)max_events, d_flags, stride_symbols, carry_symbols, d_new, d_burst_start, d_n_bursts,
                                  n_channels, max_bursts, d_state, d_reset_before, d_n_resets, d_loss_before, d_n_losses, max_marks,
                                  (hipStream_t)hip_stream));
    return DDN_OK;
}
