/* ddn_internal.h — shared between the C-ABI translation units of libdsdneo_hip.so (not installed). */
#ifndef DDN_INTERNAL_H
#define DDN_INTERNAL_H

#include "../../include/ddn_hip.h"

#define DDN_MAX_TAPS   143 /* odd; reference kChannelLpfTaps = 144 (src/dsp/demod_pipeline.cpp:129) */
#define DDN_MAX_CENTER 71

#ifdef __cplusplus
extern "C" {
#endif
int ddn_design_channel_lpf(int rate_hz, int profile, float* taps, int max_taps);
#define DDN_FLL_MAX_TAPS 48 /* FLL_BAND_EDGE_MAX_TAPS, include/dsd-neo/dsp/costas.h:60 */
int ddn_design_fll_band_edge(int sps, float* taps4, float* alpha, float* beta);
int ddn_design_resampler(int L, int M, float* taps);
#define DDN_RESAMP_MAX_L 512
int ddn_p25p1_layout_nid(int32_t out32[32]);
int ddn_p25p1_layout_trellis_block(int block, int32_t out98[98]);
int ddn_p25p1_layout_ldu_words(int ldu, int32_t out120[120]);
int ddn_p25p1_layout_ldu_imbe(int32_t first9[9], int32_t status9[9]);
int ddn_p25p1_layout_hdu(int32_t hex3[36 * 3], int32_t par6[36 * 6]);
int ddn_p25p1_layout_tdulc(int32_t data6[72], int32_t par6[72]);
int ddn_p25p1_layout_ldu_lsd(int32_t out16[16]);
void ddn_set_error(const char* fmt, ...);
/* the next ddn_p25_rx_run() records this HIP event between its matched filter and its loop kernel (one shot) */
int ddn_p25_rx_mark_loop_start(ddn_p25_rx* b, void* hip_event);
/* the next ddn_p25_rx_run() makes its stream wait for this HIP event between its matched filter and its loop kernel (one shot) */
int ddn_p25_rx_gate_loop(ddn_p25_rx* b, void* hip_event);
/* the mixed chain's shared front end: a part's stage 0 without its own front-end launch, and where that launch has to write */
struct ddn_p25_chain;
struct ddn_fsk4_chain;
int ddn_p25_chain_stage0_prepare(struct ddn_p25_chain* c, void* hip_stream, float** disc_out);
float* ddn_fsk4_chain_disc_buffer(struct ddn_fsk4_chain* c);
void* ddn_fsk4_chain_reads_done_event(struct ddn_fsk4_chain* c);
/* the mixed chain's overlapped schedule: a second discriminator buffer for the odd steps (ddn_api_chain.cpp) */
int ddn_p25_chain_double_disc(struct ddn_p25_chain* c);
/* ddn_fec_viterbi_k5_batch over the code words d_wanted [n] marks, 0 = leave undecoded (ddn_api_fec.cpp): an unmarked code word's
 * d_out row and d_cost are left unwritten where none of the 16 code words of its group is marked, and decoded otherwise
 * (ddn_dev_k5_m17_wanted in ddn_device.h) */
int ddn_fec_viterbi_k5_batch_wanted(const uint16_t* d_soft, size_t n, int in_len, const uint8_t* punct, int p_len, uint8_t* d_out,
                                    int out_stride, uint32_t* d_cost, const uint8_t* d_wanted, void* hip_stream);
/* the two kernels of ddn_mbe_synth_batch as separate calls (ddn_api_mbe.cpp) */
struct ddn_mbe_batch;
int ddn_mbe_params_only(struct ddn_mbe_batch* b, const uint8_t* d_bits, const int32_t* d_result_in, size_t n_frames, const int32_t* d_n_ldu,
                        int32_t* d_result_out, void* hip_stream);
int ddn_mbe_synth_batch_live(struct ddn_mbe_batch* b, const uint8_t* d_bits, const int32_t* d_result_in, size_t n_frames, const int32_t* d_n_ldu,
                             const int32_t* d_live_slot, const int32_t* d_n_live, float* d_pcm, int32_t* d_result_out, void* hip_stream);
int ddn_mbe_synth_only(struct ddn_mbe_batch* b, size_t n_frames, const int32_t* d_live_slot, const int32_t* d_n_live, float* d_pcm,
                       void* hip_stream);
/* the chain object's voice stage over the live slots of a call: the voice index without the slots behind a channel's
 * LDUs + the per-channel prefix sums of the live slots and their total, and the de-interleave / frame decode + skip flag over the
 * list those make (ddn_dev_voice_live_fill, ddn_device.h) */
struct ddn_p25p1_framer;
int ddn_p25p1_framer_voice_live(struct ddn_p25p1_framer* f, const int32_t* d_nid4, const int32_t* d_counts, int max_ldu_per_channel,
                                size_t max_symbols, int64_t* d_first_record, int32_t* d_status_count, int32_t* d_n_ldu, int32_t* d_live_off,
                                int32_t* d_n_live, void* hip_stream);
int ddn_p25p1_imbe_deinterleave_live(const uint8_t* d_records10, size_t n_records, const int64_t* d_first_record, const int32_t* d_status_count,
                                     size_t n_slots, const int32_t* d_live_slot, const int32_t* d_n_live, uint8_t* d_imbe_fr,
                                     uint8_t* d_imbe_soft, uint8_t* d_flags, int32_t* d_status_count_out, void* hip_stream);
int ddn_mbe_frame_decode_live(const uint8_t* d_frames, const uint8_t* d_skip, size_t n_slots, const int32_t* d_live_slot,
                              const int32_t* d_n_live, uint8_t* d_bits, int32_t* d_result, void* hip_stream);
#ifdef __cplusplus
}
#endif
#endif
