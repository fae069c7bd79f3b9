// ddn_api_m17.cpp - C-ABI of the M17 frame decoders behind the receive loop (include/ddn_fsk4.h, "M17"): link setup frames through
// the K = 5 decoder of SURVEY row a17 (ddn_fec_viterbi_k5_batch).  Device pointers, asynchronous on the stream; the scratch is
// stream-ordered (DdnScratch), so concurrent calls on different streams never share it.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "ddn_api_util.h"
#include "ddn_device.h"
#include "ddn_fsk4.h"

extern "C" int
ddn_m17_lsf_decode_batch(const uint8_t* d_records10, size_t stride_symbols, const int32_t* d_counts, const int32_t* d_sync_pos,
                         const uint8_t* d_sync_pat, const int32_t* d_n_sync, const float* d_sync_thr5, int n_channels, size_t max_syncs,
                         uint8_t* d_lsf30, uint8_t* d_status, uint32_t* d_path_cost, void* hip_stream) {
    if (!d_records10 || !d_counts || !d_sync_pos || !d_sync_pat || !d_n_sync || !d_sync_thr5 || !d_lsf30 || !d_status || n_channels <= 0
        || max_syncs == 0 || max_syncs > (1u << 24) || stride_symbols == 0) {
        ddn_set_error("ddn_m17_lsf_decode_batch: bad argument");
        return DDN_EINVAL;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    // an LSF frame follows a preamble and takes 192 symbols: at most stride / 192 + 1 of them per channel and call
    const int lmax = (int)(stride_symbols / 192 + 1);
    const size_t S = (size_t)n_channels * (size_t)lmax;
    DdnScratch s(st);
    uint16_t* cost;
    uint8_t* dec;
    uint32_t* pc;
    int32_t* slot;
    HIP_TRY(s.arena(S * (488 * sizeof(uint16_t) + 32 + sizeof(uint32_t) + sizeof(int32_t)) + 4 * 256));
    HIP_TRY(s.get(&cost, S * 488));
    HIP_TRY(s.get(&dec, S * 32));
    HIP_TRY(s.get(&pc, S));
    HIP_TRY(s.get(&slot, S));
    HIP_TRY(hipMemsetAsync(d_status, 0, (size_t)n_channels * max_syncs, st));
    HIP_TRY(ddn_dev_m17_lsf_cost(d_records10, stride_symbols, d_counts, d_sync_pos, d_sync_pat, d_n_sync, d_sync_thr5, n_channels, (int)max_syncs,
                                 lmax, cost, slot, st));
    DDN_TRY(ddn_fec_viterbi_k5_batch(cost, S, 488, nullptr, 0, dec, 32, pc, st));
    HIP_TRY(ddn_dev_m17_lsf_finish(dec, 32, pc, slot, n_channels, lmax, (int)max_syncs, d_lsf30, d_status, d_path_cost, st));
    return DDN_OK;
}

extern "C" int
ddn_m17_str_decode_batch(const uint8_t* d_records10, size_t stride_symbols, const int32_t* d_counts, const int32_t* d_sync_pos,
                         const uint8_t* d_sync_pat, const int32_t* d_n_sync, int n_channels, size_t max_syncs, uint8_t* d_lich6,
                         uint8_t* d_lich_cnt, uint8_t* d_fn_payload18, uint8_t* d_status, void* hip_stream) {
    if (!d_records10 || !d_counts || !d_sync_pos || !d_sync_pat || !d_n_sync || !d_lich6 || !d_lich_cnt || !d_fn_payload18 || !d_status
        || n_channels <= 0 || max_syncs == 0 || max_syncs > (1u << 24) || stride_symbols == 0) {
        ddn_set_error("ddn_m17_str_decode_batch: bad argument");
        return DDN_EINVAL;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    const int lmax = (int)(stride_symbols / 192 + 1); // a stream frame takes 192 symbols
    const size_t S = (size_t)n_channels * (size_t)lmax;
    DdnScratch s(st);
    uint8_t *sym, *dec, *l6, *cnt, *ok;
    int32_t* slot;
    HIP_TRY(s.arena(S * (296 + 18 + sizeof(int32_t) + 6 + 1 + 1) + 6 * 256));
    HIP_TRY(s.get(&sym, S * 296));
    HIP_TRY(s.get(&dec, S * 18));
    HIP_TRY(s.get(&slot, S));
    HIP_TRY(s.get(&l6, S * 6));
    HIP_TRY(s.get(&cnt, S));
    HIP_TRY(s.get(&ok, S));
    HIP_TRY(hipMemsetAsync(d_status, 0, (size_t)n_channels * max_syncs, st));
    HIP_TRY(ddn_dev_m17_str_bits(d_records10, stride_symbols, d_counts, d_sync_pos, d_sync_pat, d_n_sync, n_channels, (int)max_syncs, lmax, sym, slot,
                                 l6, cnt, ok, st));
    // (blocks of 16 frames none of which has a LICH that decoded write zeros and leave)
    HIP_TRY(ddn_dev_k5_nxdn_wanted(sym, nullptr, (int)S, 148, 144, nullptr, dec, 18, ok, 1, st));
    HIP_TRY(ddn_dev_m17_str_finish(dec, 18, slot, l6, cnt, ok, n_channels, lmax, (int)max_syncs, d_lich6, d_lich_cnt, d_fn_payload18, d_status, st));
    return DDN_OK;
}

extern "C" int
ddn_m17_lich_assemble_batch(const uint8_t* d_sync_pat, const int32_t* d_n_sync, int n_channels, size_t max_syncs, const uint8_t* d_lsf30,
                            const uint8_t* d_lsf_status, const uint8_t* d_lich6, const uint8_t* d_lich_cnt, const uint8_t* d_str_status,
                            uint8_t* d_assembly32, uint8_t* d_lich_lsf30, uint8_t* d_lich_status, void* hip_stream) {
    if (!d_sync_pat || !d_n_sync || !d_lich6 || !d_lich_cnt || !d_str_status || !d_assembly32 || !d_lich_lsf30 || !d_lich_status
        || n_channels <= 0 || max_syncs == 0 || max_syncs > (1u << 24) || ((d_lsf30 == nullptr) != (d_lsf_status == nullptr))) {
        ddn_set_error("ddn_m17_lich_assemble_batch: bad argument");
        return DDN_EINVAL;
    }
    HIP_TRY(ddn_dev_m17_lich(d_sync_pat, d_n_sync, n_channels, (int)max_syncs, d_lsf30, d_lsf_status, d_lich6, d_lich_cnt, d_str_status,
                             d_assembly32, d_lich_lsf30, d_lich_status, (hipStream_t)hip_stream));
    return DDN_OK;
}

extern "C" int
ddn_ysf_fich_decode_batch(const uint8_t* d_records10, size_t stride_symbols, const int32_t* d_counts, const int32_t* d_sync_pos,
                          const int32_t* d_n_sync, int n_channels, size_t max_syncs, uint8_t* d_fich4, uint8_t* d_status, uint32_t* d_v_error,
                          void* hip_stream) {
    if (!d_records10 || !d_counts || !d_sync_pos || !d_n_sync || !d_fich4 || !d_status || n_channels <= 0 || max_syncs == 0
        || max_syncs > (1u << 24) || stride_symbols == 0) {
        ddn_set_error("ddn_ysf_fich_decode_batch: bad argument");
        return DDN_EINVAL;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    // syncs are at least a window (20 symbols) + the FICH apart
    const int lmax = (int)(stride_symbols / 120 + 1);
    const size_t S = (size_t)n_channels * (size_t)lmax;
    DdnScratch s(st);
    uint16_t* cost;
    uint8_t* dec;
    uint32_t* pc;
    int32_t* slot;
    HIP_TRY(s.arena(S * (200 * sizeof(uint16_t) + 16 + sizeof(uint32_t) + sizeof(int32_t)) + 4 * 256));
    HIP_TRY(s.get(&cost, S * 200));
    HIP_TRY(s.get(&dec, S * 16));
    HIP_TRY(s.get(&pc, S));
    HIP_TRY(s.get(&slot, S));
    HIP_TRY(hipMemsetAsync(d_status, 0, (size_t)n_channels * max_syncs, st));
    HIP_TRY(ddn_dev_ysf_fich_cost(d_records10, stride_symbols, d_counts, d_sync_pos, d_n_sync, n_channels, (int)max_syncs, lmax, cost, slot, st));
    static const uint8_t none[4] = {1, 1, 1, 1}; // DSD_YSF_PUNCTURE_NONE
    DDN_TRY(ddn_fec_viterbi_k5_batch(cost, S, 200, none, 4, dec, 16, pc, st));
    HIP_TRY(ddn_dev_ysf_fich_finish(dec, 16, pc, slot, n_channels, lmax, (int)max_syncs, d_fich4, d_status, d_v_error, st));
    return DDN_OK;
}

// include/ddn_fsk4.h
extern "C" int
ddn_ysf_payload_decode_batch(const uint8_t* d_records10, size_t stride_symbols, const int32_t* d_counts, const int32_t* d_sync_pos,
                             const int32_t* d_n_sync, int n_channels, size_t max_syncs, const uint8_t* d_fich4, const uint8_t* d_fich_status,
                             uint8_t* d_last_dt_fi, uint8_t* d_info2, uint8_t* d_dch40, uint8_t* d_dch_status2, uint32_t* d_dch_cost2,
                             uint8_t* d_ambe49x5, uint8_t* d_errs2x5, uint8_t* d_frames184x5, uint8_t* d_n_frames, void* hip_stream) {
    if (!d_records10 || !d_counts || !d_sync_pos || !d_n_sync || !d_fich4 || !d_fich_status || !d_last_dt_fi || !d_info2 || !d_dch40
        || !d_dch_status2 || !d_dch_cost2 || !d_ambe49x5 || !d_errs2x5 || !d_frames184x5 || !d_n_frames || n_channels <= 0 || max_syncs == 0 || max_syncs > (1u << 24)
        || stride_symbols == 0) {
        ddn_set_error("ddn_ysf_payload_decode_batch: bad argument");
        return DDN_EINVAL;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    // frames are a sync window + the lock (20 + 460 symbols) apart
    const int lmax = (int)(stride_symbols / 480 + 2);
    const size_t S = (size_t)n_channels * (size_t)lmax, SO = (size_t)n_channels * max_syncs;
    DdnScratch s(st);
    uint16_t* cA;
    uint8_t *cBw, *dA, *dB;
    uint32_t *pA, *pB;
    int32_t* slot;
    HIP_TRY(s.arena(S * ((200 + 2 * 360) * sizeof(uint16_t) + 3 + 16 + 2 * 32 + 3 * sizeof(uint32_t) + sizeof(int32_t)) + 7 * 256));
    HIP_TRY(s.get(&cA, S * 200));
    HIP_TRY(s.get(&cBw, S * (2 * 360 * sizeof(uint16_t) + 3)));
    HIP_TRY(s.get(&dA, S * 16));
    HIP_TRY(s.get(&dB, S * 2 * 32));
    HIP_TRY(s.get(&pA, S));
    HIP_TRY(s.get(&pB, S * 2));
    HIP_TRY(s.get(&slot, S));
    uint16_t* cB = (uint16_t*)cBw;
    uint8_t* wA = cBw + S * 2 * 360 * sizeof(uint16_t); // which code words of the two lists hold a block (cleared with the costs)
    uint8_t* wB = wA + S;
    HIP_TRY(hipMemsetAsync(cA, 0, (size_t)(dA - (uint8_t*)cA), st));
    HIP_TRY(hipMemsetAsync(slot, 0xFF, DdnScratch::pad(S * sizeof(int32_t)), st));
    HIP_TRY(hipMemsetAsync(d_dch_status2, 0, SO * 2, st));
    HIP_TRY(hipMemsetAsync(d_dch_cost2, 0, SO * 2 * sizeof(uint32_t), st));
    HIP_TRY(hipMemsetAsync(d_dch40, 0, SO * 40, st));
    HIP_TRY(hipMemsetAsync(d_frames184x5, 0, SO * 5 * 184, st));
    HIP_TRY(hipMemsetAsync(d_n_frames, 0, SO, st));
    HIP_TRY(ddn_dev_ysf_plan(d_sync_pos, d_n_sync, d_counts, n_channels, (int)max_syncs, lmax, d_fich4, d_fich_status, d_last_dt_fi, d_info2, slot, st));
    HIP_TRY(ddn_dev_ysf_payload_costs(d_records10, stride_symbols, d_sync_pos, n_channels, (int)max_syncs, lmax, d_info2, slot, cA, cB, d_ambe49x5,
                                      d_errs2x5, wA, wB, d_frames184x5, d_n_frames, st));
    static const uint8_t none[4] = {1, 1, 1, 1}; // DSD_YSF_PUNCTURE_NONE
    DDN_TRY(ddn_fec_viterbi_k5_batch_wanted(cA, S, 200, none, 4, dA, 16, pA, wA, st));
    DDN_TRY(ddn_fec_viterbi_k5_batch_wanted(cB, S * 2, 360, none, 4, dB, 32, pB, wB, st));
    HIP_TRY(ddn_dev_ysf_dch_finish(dA, pA, dB, pB, slot, d_info2, n_channels, lmax, (int)max_syncs, d_dch40, d_dch_status2, d_dch_cost2, st));
    return DDN_OK;
}

// ---- M17 packet and BERT frames (include/ddn_fsk4.h) --------------------------------------------------------------------------------------
extern "C" int
ddn_m17_pkt_decode_batch(const uint8_t* d_records10, size_t stride_symbols, const int32_t* d_counts, const int32_t* d_sync_pos,
                         const uint8_t* d_sync_pat, const int32_t* d_n_sync, const float* d_sync_thr5, int n_channels, size_t max_syncs,
                         uint8_t* d_pkt26, uint8_t* d_status, uint32_t* d_path_cost, void* hip_stream) {
    if (!d_records10 || !d_counts || !d_sync_pos || !d_sync_pat || !d_n_sync || !d_sync_thr5 || !d_pkt26 || !d_status || n_channels <= 0
        || max_syncs == 0 || max_syncs > (1u << 24) || stride_symbols == 0) {
        ddn_set_error("ddn_m17_pkt_decode_batch: bad argument");
        return DDN_EINVAL;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    const int lmax = (int)(stride_symbols / 192 + 1); // a packet frame takes 192 symbols
    const size_t S = (size_t)n_channels * (size_t)lmax;
    DdnScratch s(st);
    uint16_t* cost;
    uint8_t *dec, *want;
    uint32_t* pc;
    int32_t* slot;
    HIP_TRY(s.arena(S * (420 * sizeof(uint16_t) + 32 + sizeof(uint32_t) + sizeof(int32_t) + 1) + 5 * 256));
    HIP_TRY(s.get(&cost, S * 420));
    HIP_TRY(s.get(&dec, S * 32));
    HIP_TRY(s.get(&pc, S));
    HIP_TRY(s.get(&slot, S));
    HIP_TRY(s.get(&want, S));
    HIP_TRY(hipMemsetAsync(d_status, 0, (size_t)n_channels * max_syncs, st));
    HIP_TRY(ddn_dev_m17_pkt_cost(d_records10, stride_symbols, d_counts, d_sync_pos, d_sync_pat, d_n_sync, d_sync_thr5, n_channels, (int)max_syncs,
                                 lmax, cost, slot, want, st));
    // (blocks of 16 slots none of which holds a packet frame are left alone)
    DDN_TRY(ddn_fec_viterbi_k5_batch_wanted(cost, S, 420, nullptr, 0, dec, 32, pc, want, st));
    HIP_TRY(ddn_dev_m17_pkt_finish(dec, 32, pc, slot, n_channels, lmax, (int)max_syncs, d_pkt26, d_status, d_path_cost, st));
    return DDN_OK;
}

extern "C" int
ddn_m17_brt_decode_batch(const uint8_t* d_records10, size_t stride_symbols, const int32_t* d_counts, const int32_t* d_sync_pos,
                         const uint8_t* d_sync_pat, const int32_t* d_n_sync, int n_channels, size_t max_syncs, uint8_t* d_bits25,
                         uint8_t* d_status, void* hip_stream) {
    if (!d_records10 || !d_counts || !d_sync_pos || !d_sync_pat || !d_n_sync || !d_bits25 || !d_status || n_channels <= 0 || max_syncs == 0
        || max_syncs > (1u << 24) || stride_symbols == 0) {
        ddn_set_error("ddn_m17_brt_decode_batch: bad argument");
        return DDN_EINVAL;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    const int lmax = (int)(stride_symbols / 192 + 1); // a BERT frame takes 192 symbols
    const size_t S = (size_t)n_channels * (size_t)lmax;
    DdnScratch s(st);
    uint8_t *sym, *dec, *want;
    int32_t* slot;
    HIP_TRY(s.arena(S * (402 + 25 + sizeof(int32_t) + 1) + 4 * 256));
    HIP_TRY(s.get(&sym, S * 402));
    HIP_TRY(s.get(&dec, S * 25));
    HIP_TRY(s.get(&slot, S));
    HIP_TRY(s.get(&want, S));
    HIP_TRY(hipMemsetAsync(d_status, 0, (size_t)n_channels * max_syncs, st));
    HIP_TRY(ddn_dev_m17_brt_bits(d_records10, stride_symbols, d_counts, d_sync_pos, d_sync_pat, d_n_sync, n_channels, (int)max_syncs, lmax, sym, slot,
                                 want, st));
    // 201 steps (197 bits + 4 flush), 197 bits chained back
    HIP_TRY(ddn_dev_k5_nxdn_wanted(sym, nullptr, (int)S, 201, 197, nullptr, dec, 25, want, 1, st));
    HIP_TRY(ddn_dev_m17_brt_finish(dec, 25, slot, n_channels, lmax, (int)max_syncs, d_bits25, d_status, st));
    return DDN_OK;
}

extern "C" size_t
ddn_m17_data_state_bytes(void) {
    return ddn_dev_m17_data_state_bytes();
}

extern "C" int
ddn_m17_data_assemble_batch(const uint8_t* d_sync_pat, const int32_t* d_sync_pos, const int32_t* d_n_sync, const int32_t* d_advance,
                            int n_channels, size_t max_syncs, const uint8_t* d_pkt26, const uint8_t* d_pkt_frame_status,
                            const uint8_t* d_bits25, const uint8_t* d_brt_frame_status, void* d_state, uint8_t* d_pkt_status,
                            uint8_t* d_pkt_count, int32_t* d_brt_state, uint8_t* d_packet, int32_t* d_packet_app_len,
                            uint8_t* d_packet_crc_ok, int32_t* d_packet_slot, int32_t* d_n_packets, int max_packets, void* hip_stream) {
    if (!d_sync_pat || !d_sync_pos || !d_n_sync || !d_pkt26 || !d_pkt_frame_status || !d_bits25 || !d_brt_frame_status || !d_state
        || !d_pkt_status || !d_pkt_count || !d_brt_state || !d_packet || !d_packet_app_len || !d_packet_crc_ok || !d_packet_slot
        || !d_n_packets || n_channels <= 0 || max_syncs == 0 || max_syncs > (1u << 24) || max_packets < 1 || max_packets > 33) {
        ddn_set_error("ddn_m17_data_assemble_batch: bad argument");
        return DDN_EINVAL;
    }
    // (the walk writes the slots of packet and BERT frames only)
    HIP_TRY(hipMemsetAsync(d_pkt_status, 0, (size_t)n_channels * max_syncs, (hipStream_t)hip_stream));
    HIP_TRY(hipMemsetAsync(d_pkt_count, 0, (size_t)n_channels * max_syncs, (hipStream_t)hip_stream));
    HIP_TRY(ddn_dev_m17_data_walk(d_sync_pat, d_sync_pos, d_n_sync, d_advance, n_channels, (int)max_syncs, d_pkt26, d_pkt_frame_status,
                                  d_bits25, d_brt_frame_status, d_state, d_pkt_status, d_pkt_count, d_brt_state, d_packet, d_packet_app_len,
                                  d_packet_crc_ok, d_packet_slot, d_n_packets, max_packets, (hipStream_t)hip_stream));
    return DDN_OK;
}
