// ddn_api_m17.cpp - C-ABI of the M17 frame decoders behind the receive loop (include/ddn_fsk4.h, "M17"): link setup frames through
// the K = 5 decoder of SURVEY row a17 (ddn_fec_viterbi_k5_batch).  Device pointers, asynchronous on the stream; the scratch is
// stream-ordered (hipMallocAsync), so concurrent calls on different streams never share it.
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
    const size_t b_cost = ((S * 488 * sizeof(uint16_t)) + 255) & ~(size_t)255, b_dec = ((S * 32) + 255) & ~(size_t)255;
    const size_t b_pc = ((S * sizeof(uint32_t)) + 255) & ~(size_t)255, b_slot = ((S * sizeof(int32_t)) + 255) & ~(size_t)255;
    uint8_t* scratch = nullptr;
    HIP_TRY(hipMallocAsync((void**)&scratch, b_cost + b_dec + b_pc + b_slot, st));
    uint16_t* cost = (uint16_t*)scratch;
    uint8_t* dec = scratch + b_cost;
    uint32_t* pc = (uint32_t*)(dec + b_dec);
    int32_t* slot = (int32_t*)((uint8_t*)pc + b_pc);
    int rc = DDN_OK;
    hipError_t e = hipMemsetAsync(d_status, 0, (size_t)n_channels * max_syncs, st);
    if (e == hipSuccess) {
        e = ddn_dev_m17_lsf_cost(d_records10, stride_symbols, d_counts, d_sync_pos, d_sync_pat, d_n_sync, d_sync_thr5, n_channels, (int)max_syncs,
                                 lmax, cost, slot, st);
    }
    if (e == hipSuccess) {
        rc = ddn_fec_viterbi_k5_batch(cost, S, 488, nullptr, 0, dec, 32, pc, st);
    }
    if (e == hipSuccess && rc == DDN_OK) {
        e = ddn_dev_m17_lsf_finish(dec, 32, pc, slot, n_channels, lmax, (int)max_syncs, d_lsf30, d_status, d_path_cost, st);
    }
    const hipError_t ef = hipFreeAsync(scratch, st);
    if (rc != DDN_OK) {
        return rc;
    }
    HIP_TRY(e);
    HIP_TRY(ef);
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
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_sym = up(S * 296), b_dec = up(S * 18), b_slot = up(S * sizeof(int32_t)), b_l6 = up(S * 6), b_1 = up(S);
    uint8_t* scratch = nullptr;
    HIP_TRY(hipMallocAsync((void**)&scratch, b_sym + b_dec + b_slot + b_l6 + 2 * b_1, st));
    uint8_t* sym = scratch;
    uint8_t* dec = sym + b_sym;
    int32_t* slot = (int32_t*)(dec + b_dec);
    uint8_t* l6 = (uint8_t*)slot + b_slot;
    uint8_t* cnt = l6 + b_l6;
    uint8_t* ok = cnt + b_1;
    hipError_t e = hipMemsetAsync(d_status, 0, (size_t)n_channels * max_syncs, st);
    if (e == hipSuccess) {
        e = ddn_dev_m17_str_bits(d_records10, stride_symbols, d_counts, d_sync_pos, d_sync_pat, d_n_sync, n_channels, (int)max_syncs, lmax, sym,
                                 slot, l6, cnt, ok, st);
    }
    if (e == hipSuccess) { // (blocks of 16 frames none of which has a LICH that decoded write zeros and leave)
        e = ddn_dev_k5_nxdn_wanted(sym, nullptr, (int)S, 148, 144, nullptr, dec, 18, ok, 1, st);
    }
    if (e == hipSuccess) {
        e = ddn_dev_m17_str_finish(dec, 18, slot, l6, cnt, ok, n_channels, lmax, (int)max_syncs, d_lich6, d_lich_cnt, d_fn_payload18, d_status, st);
    }
    const hipError_t ef = hipFreeAsync(scratch, st);
    HIP_TRY(e);
    HIP_TRY(ef);
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
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_cost = up(S * 200 * sizeof(uint16_t)), b_dec = up(S * 16), b_pc = up(S * sizeof(uint32_t)), b_slot = up(S * sizeof(int32_t));
    uint8_t* scratch = nullptr;
    HIP_TRY(hipMallocAsync((void**)&scratch, b_cost + b_dec + b_pc + b_slot, st));
    uint16_t* cost = (uint16_t*)scratch;
    uint8_t* dec = scratch + b_cost;
    uint32_t* pc = (uint32_t*)(dec + b_dec);
    int32_t* slot = (int32_t*)((uint8_t*)pc + b_pc);
    int rc = DDN_OK;
    hipError_t e = hipMemsetAsync(d_status, 0, (size_t)n_channels * max_syncs, st);
    if (e == hipSuccess) {
        e = ddn_dev_ysf_fich_cost(d_records10, stride_symbols, d_counts, d_sync_pos, d_n_sync, n_channels, (int)max_syncs, lmax, cost, slot, st);
    }
    if (e == hipSuccess) {
        static const uint8_t none[4] = {1, 1, 1, 1}; // DSD_YSF_PUNCTURE_NONE
        rc = ddn_fec_viterbi_k5_batch(cost, S, 200, none, 4, dec, 16, pc, st);
    }
    if (e == hipSuccess && rc == DDN_OK) {
        e = ddn_dev_ysf_fich_finish(dec, 16, pc, slot, n_channels, lmax, (int)max_syncs, d_fich4, d_status, d_v_error, st);
    }
    const hipError_t ef = hipFreeAsync(scratch, st);
    if (rc != DDN_OK) {
        return rc;
    }
    HIP_TRY(e);
    HIP_TRY(ef);
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
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_cA = up(S * 200 * sizeof(uint16_t)), b_cB = up(S * 2 * 360 * sizeof(uint16_t) + S * 3), b_dA = up(S * 16), b_dB = up(S * 2 * 32),
                 b_pA = up(S * sizeof(uint32_t)), b_pB = up(S * 2 * sizeof(uint32_t)), b_slot = up(S * sizeof(int32_t));
    uint8_t* scratch = nullptr;
    HIP_TRY(hipMallocAsync((void**)&scratch, b_cA + b_cB + b_dA + b_dB + b_pA + b_pB + b_slot, st));
    uint16_t* cA = (uint16_t*)scratch;
    uint16_t* cB = (uint16_t*)(scratch + b_cA);
    uint8_t* wA = scratch + b_cA + S * 2 * 360 * sizeof(uint16_t); // which code words of the two lists hold a block (cleared with the costs)
    uint8_t* wB = wA + S;
    uint8_t* dA = scratch + b_cA + b_cB;
    uint8_t* dB = dA + b_dA;
    uint32_t* pA = (uint32_t*)(dB + b_dB);
    uint32_t* pB = (uint32_t*)((uint8_t*)pA + b_pA);
    int32_t* slot = (int32_t*)((uint8_t*)pB + b_pB);
    int rc = DDN_OK;
    hipError_t e = hipMemsetAsync(cA, 0, b_cA + b_cB, st);
    if (e == hipSuccess) {
        e = hipMemsetAsync(slot, 0xFF, b_slot, st);
    }
    if (e == hipSuccess) {
        e = hipMemsetAsync(d_dch_status2, 0, SO * 2, st);
    }
    if (e == hipSuccess) {
        e = hipMemsetAsync(d_dch_cost2, 0, SO * 2 * sizeof(uint32_t), st);
    }
    if (e == hipSuccess) {
        e = hipMemsetAsync(d_dch40, 0, SO * 40, st);
    }
    if (e == hipSuccess) {
        e = hipMemsetAsync(d_frames184x5, 0, SO * 5 * 184, st);
    }
    if (e == hipSuccess) {
        e = hipMemsetAsync(d_n_frames, 0, SO, st);
    }
    if (e == hipSuccess) {
        e = ddn_dev_ysf_plan(d_sync_pos, d_n_sync, d_counts, n_channels, (int)max_syncs, lmax, d_fich4, d_fich_status, d_last_dt_fi, d_info2,
                             slot, st);
    }
    if (e == hipSuccess) {
        e = ddn_dev_ysf_payload_costs(d_records10, stride_symbols, d_sync_pos, n_channels, (int)max_syncs, lmax, d_info2, slot, cA, cB,
                                      d_ambe49x5, d_errs2x5, wA, wB, d_frames184x5, d_n_frames, st);
    }
    static const uint8_t none[4] = {1, 1, 1, 1}; // DSD_YSF_PUNCTURE_NONE
    if (e == hipSuccess) {
        rc = ddn_fec_viterbi_k5_batch_wanted(cA, S, 200, none, 4, dA, 16, pA, wA, st);
    }
    if (e == hipSuccess && rc == DDN_OK) {
        rc = ddn_fec_viterbi_k5_batch_wanted(cB, S * 2, 360, none, 4, dB, 32, pB, wB, st);
    }
    if (e == hipSuccess && rc == DDN_OK) {
        e = ddn_dev_ysf_dch_finish(dA, pA, dB, pB, slot, d_info2, n_channels, lmax, (int)max_syncs, d_dch40, d_dch_status2, d_dch_cost2, st);
    }
    const hipError_t ef = hipFreeAsync(scratch, st);
    if (rc != DDN_OK) {
        return rc;
    }
    HIP_TRY(e);
    HIP_TRY(ef);
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
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_cost = up(S * 420 * sizeof(uint16_t)), b_dec = up(S * 32), b_pc = up(S * sizeof(uint32_t)), b_slot = up(S * sizeof(int32_t)),
                 b_want = up(S);
    uint8_t* scratch = nullptr;
    HIP_TRY(hipMallocAsync((void**)&scratch, b_cost + b_dec + b_pc + b_slot + b_want, st));
    uint16_t* cost = (uint16_t*)scratch;
    uint8_t* dec = scratch + b_cost;
    uint32_t* pc = (uint32_t*)(dec + b_dec);
    int32_t* slot = (int32_t*)((uint8_t*)pc + b_pc);
    uint8_t* want = (uint8_t*)slot + b_slot;
    int rc = DDN_OK;
    hipError_t e = hipMemsetAsync(d_status, 0, (size_t)n_channels * max_syncs, st);
    if (e == hipSuccess) {
        e = ddn_dev_m17_pkt_cost(d_records10, stride_symbols, d_counts, d_sync_pos, d_sync_pat, d_n_sync, d_sync_thr5, n_channels, (int)max_syncs,
                                 lmax, cost, slot, want, st);
    }
    if (e == hipSuccess) { // (blocks of 16 slots none of which holds a packet frame are left alone)
        rc = ddn_fec_viterbi_k5_batch_wanted(cost, S, 420, nullptr, 0, dec, 32, pc, want, st);
    }
    if (e == hipSuccess && rc == DDN_OK) {
        e = ddn_dev_m17_pkt_finish(dec, 32, pc, slot, n_channels, lmax, (int)max_syncs, d_pkt26, d_status, d_path_cost, st);
    }
    const hipError_t ef = hipFreeAsync(scratch, st);
    if (rc != DDN_OK) {
        return rc;
    }
    HIP_TRY(e);
    HIP_TRY(ef);
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
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_sym = up(S * 402), b_dec = up(S * 25), b_slot = up(S * sizeof(int32_t)), b_want = up(S);
    uint8_t* scratch = nullptr;
    HIP_TRY(hipMallocAsync((void**)&scratch, b_sym + b_dec + b_slot + b_want, st));
    uint8_t* sym = scratch;
    uint8_t* dec = sym + b_sym;
    int32_t* slot = (int32_t*)(dec + b_dec);
    uint8_t* want = (uint8_t*)slot + b_slot;
    hipError_t e = hipMemsetAsync(d_status, 0, (size_t)n_channels * max_syncs, st);
    if (e == hipSuccess) {
        e = ddn_dev_m17_brt_bits(d_records10, stride_symbols, d_counts, d_sync_pos, d_sync_pat, d_n_sync, n_channels, (int)max_syncs, lmax, sym,
                                 slot, want, st);
    }
    if (e == hipSuccess) { // 201 steps (197 bits + 4 flush), 197 bits chained back
        e = ddn_dev_k5_nxdn_wanted(sym, nullptr, (int)S, 201, 197, nullptr, dec, 25, want, 1, st);
    }
    if (e == hipSuccess) {
        e = ddn_dev_m17_brt_finish(dec, 25, slot, n_channels, lmax, (int)max_syncs, d_bits25, d_status, st);
    }
    const hipError_t ef = hipFreeAsync(scratch, st);
    HIP_TRY(e);
    HIP_TRY(ef);
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
