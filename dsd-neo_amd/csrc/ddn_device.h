/* ddn_device.h — kernel argument structs shared by the .hip kernels and the C-ABI host code. */
#ifndef DDN_DEVICE_H
#define DDN_DEVICE_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ddn_internal.h"

/* Experiment knobs.  The product build reads nothing from the environment: DDN_EXP_ENV(name) is NULL there, so every "if the variable
 * is set" branch folds away and the library's schedule depends on its arguments alone.  The timing tools build a second library
 * with -DDDN_EXPERIMENTS (tools/build_variant.sh exp), in which the knobs DESIGN / profiles/README.md name are live. */
#ifdef DDN_EXPERIMENTS
#include <stdlib.h>
#define DDN_EXP_ENV(name) getenv(name)
#else
#define DDN_EXP_ENV(name) ((const char*)0)
#endif

#define DDN_TILE 256        /* time tile (samples) of the fused front-end kernel */
#define DDN_DEFAULT_GROUP 8 /* channels per workgroup */
#define DDN_CARRY_LEN 72 /* >= DDN_MAX_CENTER widened samples of FIR look-back per channel */

typedef struct DdnFskState { /* == the fields of dsd_fsk_modem_state the path carries */
    float prev_i, prev_q;
    int have_prev;
    float dc_est, peak_est;
} DdnFskState;

typedef float ddn_f2 __attribute__((ext_vector_type(2)));

typedef struct DdnIqCondConfig { /* optional IQ conditioning switches of struct demod_state (row a5) + squelch gate */
    int dc_enable, dc_shift, bal_enable, squelch_on;
    float bal_thr, bal_ema_a, squelch_level;
} DdnIqCondConfig;
typedef struct DdnIqCondState { /* iq_dc_avg_r/i, iqbal_alpha_ema_r/i */
    float dc_r, dc_i, er, ei;
} DdnIqCondState;

typedef struct DdnFmAudioState { /* the words of demod_state the audio-monitor path carries per channel (ddn_fm_audio.hip) */
    float pre_r, pre_j;                                  /* dsd_fm_demod history */
    float deemph_avg, audio_lpf_state, dc_avg, now_lpr;  /* the post filters and low_pass_real */
    float squelch_env;
    int history_valid, gate_open;                        /* fm_demod_history_valid, squelch_gate_open */
    int initialised;                                     /* 0 after a reset: squelch_env = 1, gate open on first use */
} DdnFmAudioState;
typedef struct DdnFmAudioArgs {
    const void* in;  /* [B][stride] complex channel-LPF output */
    float* out;      /* [B][out_stride] audio, compacted */
    DdnFmAudioState* state;
    float* ring;     /* [B][16] decimator inputs before this call, oldest first (read and written when M > 1) */
    size_t stride, out_stride;
    long n;          /* complex samples per channel in this call (after the half-band cascade) */
    int block_len;   /* samples per full_demod() block at that rate */
    int n_channels;
    int squelch_on;
    float squelch_level;
    int M, phase0;   /* post_downsample (1 = off) and post_polydecim_phase at the call's first sample */
    float taps[16];
    int deemph_on, lpf_on, dc_on;
    float deemph_a, lpf_alpha, dc_scale; /* already clamped to [0, 1] as the filters do */
    int lpr_on, lpr_fast, lpr_slow, lpr_index0;
    float lpr_recip;
    float env_attack, env_release;
} DdnFmAudioArgs;

typedef struct DdnFusedArgs {
    const void* in;       /* [B][ch_stride] complex samples (cu8 pairs or float pairs) */
    float* out;           /* [B][out_stride] discriminator samples */
    const ddn_f2* carry;  /* [B][DDN_CARRY_LEN] FIR look-back from the previous call */
    ddn_f2* carry_out;    /* same array when the kernel itself refreshes it at the end (n >= DDN_CARRY_LEN), else NULL */
    DdnFskState* state;   /* [B] */
    const float* taps_dev; /* [taps_len] channel LPF taps (first half + centre are read) */
    size_t ch_stride;
    size_t out_stride;
    long n;               /* complex samples per channel in this call */
    long n_tiles;         /* n_blocks * tiles_per_block */
    int n_channels;
    int in_fmt;
    int block_len;
    int tiles_per_block;
    int center;
    int squelch_on;
    float squelch_level;
    long long* dbg_out; /* optional: per-wave phase timings of workgroup 0 (DDN_DBG bit 6) */
    int dbg; /* timing experiments only (DDN_DBG env): 1 skip recurrences, 2 skip filter, 4 skip finish, 8 skip staging */
    /* (round 6) segments: the batch's channel index is cut into up to three runs [seg_first1, seg_first2) ... with an input array, an
     * output array and a tap set of their own (same tap count) - three protocol groups of a mixed batch in ONE launch, so the grid is
     * ceil(total / G) workgroups however the groups' sizes fall (a workgroup may hold channels of two groups).  n_seg <= 1: in / out /
     * taps_dev above, as before.  carry / state are the batch's arrays, indexed by the batch's channel index either way. */
    int n_seg, seg_first1, seg_first2;
    const void *seg_in0, *seg_in1, *seg_in2;
    float *seg_out0, *seg_out1, *seg_out2;
    const float *seg_taps1, *seg_taps2; /* (segment 0's are taps_dev) */
} DdnFusedArgs;

#define DDN_TED_DL 100 /* == TED_DL_SIZE (include/dsd-neo/dsp/ted.h:19) */
typedef struct DdnTedState { /* == the carried fields of ted_state_t */
    float mu, omega, omega_mid, omega_min, omega_max, omega_rel;
    float last_r, last_j, lock_accum;
    int lock_count, dl_index, twice_sps, sps;
} DdnTedState;

typedef struct DdnSlicerState { /* per-channel slicer words of dsd_state the P25p1 path carries */
    float center, umid, lmid, max, min;
    int sidx, midx, sums_valid;
    double min_sum, max_sum;
} DdnSlicerState;

typedef struct DdnRxConfig { /* fixed-protocol P25p1 receive loop (ddn_rx.hip) */
    int out_rate, sym_rate, lock_symbols, use_filter;
    int dbg; /* profiling only (env DDN_RX_DBG): 1 = skip symbol commit, 2 = skip record stores, 4 = skip sample loop body */
    int handlers;      /* 1 = the reference's per-DUID handlers decide the in-frame length (lock_symbols ignored) */
    int nid_threshold; /* p25p1_get_erasure_threshold() */
    int max_events;    /* capacity of the per-channel event list */
    int32_t* event_data; /* [B][max_events][4] what each decision decoded (NULL = not wanted): NID {status, nac, duid, errors}, TSBK /
                            PDU header block {12 bytes as three words, crc good | candidate << 8 | block << 16} */
} DdnRxConfig;

typedef struct DdnP25HState { /* per-channel words of the P25p1 handlers (ddn_p25h_dev.h) carried across calls */
    int phase, block, end, skipdibit, nac, p2_cc, r0, r1;
} DdnP25HState;

typedef struct DdnRxState { /* per-channel words of dsd_state / frame_sync_runtime_ctx the P25p1 loop carries */
    double min_sum, max_sum;
    long long filt_start, n_abs; /* absolute sample index of the filter's first sample / of the next input sample */
    float center, umid, lmid, max, min, maxref, minref;
    float fill_min, fill_max; /* value the extrema rings were last refilled with */
    float sum, lastsample, lmin, lmax;
    int sidx, midx, since_fill; /* since_fill: ring pushes since the refill, saturating at 1024 */
    int sps_accum, jitter, in_symbol, span, centre, i, count;
    int filter_on, have_sync, lock_left, lastsync; /* lastsync: 0 none, 1 +P25p1, 2 -P25p1 */
    int lidx, level_count, hist_count, shead, scount;
    uint32_t hist_bits;
    int hunt_pos;   /* rt.synctest_pos: symbols hunted since the hunt (re)started */
    int need_reset; /* noCarrier() ran: the next symbol start re-initialises timing and slicer */
    /* handler mode: hphase != 0 = a handler decision falls due when lock_left runs out (1 the NID, 2 a trellis block);
       hw = symbols written to the in-frame history ring; hn = symbols of the current phase; hnc = noCarrier() ran since the
       last NID (the handlers' NAC memory is cleared with it, engine.c:1889) */
    int hphase, hw, hn, hnc;
    int dbg_nreq;           /* timing experiments (cfg.dbg bit 65536): handler requests / cycles spent waiting for the answers */
    long long dbg_wait;
} DdnRxState;

/* ---- fsk4 receive loop (the protocols of ddn_fsk4_proto.h), ddn_rx4.hip ---- */
#define DDN_FSK4_MAX_PAT  20
#define DDN_FSK4_MAX_TAPS 135
#define DDN_FSK4_HIST     128 /* symbol / payload history kept per channel: 90 reachable + what the helper wave lags */
#define DDN_FSK4_PRE      90
#ifndef DDN_FSK4_DMR_RC_PAT
#define DDN_FSK4_DMR_RC_PAT 8 /* == include/ddn_fsk4.h: the DMR table's MS reverse-channel row */
#endif
/* What k_fsk4_rx reads at run time; a protocol's constants are compiled in (ddn_fsk4_proto.h).  The order is part of the kernel: its
 * scalar loads come out in address order, and two scalars side by side are fused into one wider load, either of which moves the
 * kernel's registers.  So the scalars keep their order and stay apart, with the byte tables and `handlers` (which the kernel does not
 * read) between them; only sync_thr and pat_hi are meant to be fetched together. */
typedef struct DdnFsk4Config {
    int out_rate;
    uint8_t pat_type[DDN_FSK4_MAX_PAT];
    int rf_mod;
    uint8_t pat_neg[DDN_FSK4_MAX_PAT];
    uint32_t pat_bits[DDN_FSK4_MAX_PAT];
    int use_filter;
    uint8_t pat_class[DDN_FSK4_MAX_PAT];
    int dbg; /* profiling only (env DDN_RX4_DBG) */
    int handlers;   /* 1 = the reference's handlers decide the in-frame length (ddn_fsk4h_dev.h) */
    int max_events; /* capacity of the per-channel event list */
    float* sync_thr; /* optional [B][max_sync][5]: {center, umid, lmid, max, min} as every accepted sync leaves them (after the warm
                        start) - what a frame decoder that works on soft symbols needs (M17 LSF: thresholds are static inside a frame) */
    uint32_t pat_hi[DDN_FSK4_MAX_PAT]; /* win_len > 24 (EDACS): sign bits 24..47 of each pattern, pat_bits holding bits 0..23 */
} DdnFsk4Config;
typedef struct DdnFsk4State {
    long long filt_start, n_abs;
    float center, umid, lmid, max, min, maxref, minref;
    float sum, lastsample, lmin, lmax;
    int sps_accum, jitter, in_symbol, span, centre, i, count;
    int filter_on, have_sync, lock_left, lastsync, cur_pat;
    int lidx, level_count, hist_count, shead, scount;
    uint32_t hist_bits;
    int hunt_pos, need_reset;
    int hmode, hidx; /* handler mode: phase (ddn_fsk4h_dev.h) and the index of the next dibit inside the burst / frame */
    union {
        int hlich;        /* NXDN: the LICH's high bits so far (M17: the polarity) */
        uint32_t hist_hi; /* win_len > 24 (EDACS, no handlers): sign history bits 24..47, hist_bits holding bits 0..23 */
    };
} DdnFsk4State;
typedef struct DdnFsk4RxArgs { /* one launch of the loop (ddn_dev_fsk4_rx); B = n_channels */
    const float* raw;       /* [B][stride] discriminator samples of this call */
    const float* filt;      /* [B][stride] the always-on matched-filter stream of the same samples (read when cfg->use_filter) */
    const float* prev_tail; /* [B][DDN_FSK4_MAX_TAPS - 1] the samples before this call, right-aligned */
    float* fstale;          /* [B][DDN_FSK4_MAX_TAPS - 1] the gated filter's stale memory */
    const float* taps;      /* [DDN_FSK4_MAX_TAPS] */
    long n;                 /* samples per channel in this call */
    size_t stride;
    int n_channels;
    const DdnFsk4Config* cfg; /* device memory */
    DdnFsk4State* state;      /* [B] */
    float *lbuf_store, *shist_store;     /* [24][B] level ring, [DDN_FSK4_HIST][B] symbol history */
    uint8_t *phist_store, *rhist_store;  /* [DDN_FSK4_HIST][B] payload dibit / reliability history */
    uint8_t *rec, *flags, *pay;          /* [B][max_sym][10], [B][max_sym], [B][max_sym][2] */
    int32_t* counts;                     /* [B] */
    size_t max_sym;
    const int32_t* lock4;                /* [B][4] symbols read behind a sync, per sync class */
    int32_t* sync_pos;                   /* [B][max_sync] */
    uint8_t *sync_pat, *pre, *pre_rel;   /* [B][max_sync], [B][max_sync][DDN_FSK4_PRE] x 2 */
    int32_t* n_sync;                     /* [B] */
    int max_sync;
    int channels_per_wave;  /* 1, 2 .. 32 */
    int samples_per_symbol; /* out_rate / symbol rate, rounded up */
    int protocol;           /* DDN_FSK4_* */
    int handlers;           /* == cfg->handlers; then hwords [B][32] and hpay [B][144] carry the handlers' words and burst dibits */
    int32_t* hwords;
    uint8_t* hpay;
    int32_t *events, *n_events; /* [B][cfg->max_events][4], [B], or both NULL */
} DdnFsk4RxArgs;

typedef struct DdnCqpskState { /* per-channel words of demod_state the CQPSK chain carries besides ted_state_t */
    float agc_avg;                          /* cqpsk_agc_avg */
    float fll_phase, fll_freq;              /* fll_band_edge_state */
    int fll_idx;
    float diff_r, diff_j;                   /* cqpsk_diff_prev_r/j */
    float cos_phase, cos_freq, cos_err, cos_es, cos_alpha, cos_beta; /* costas_state */
    int cos_init;
} DdnCqpskState;

typedef struct DdnPuncture { /* puncture pattern of the K=5 decoder, expanded on the host */
    int p_len;               /* 0 = not punctured */
    int ones_total;
    uint8_t keep[64];
    uint8_t ones_before[64]; /* kept positions before pattern index r */
} DdnPuncture;

#ifdef __cplusplus
extern "C" {
#endif
hipError_t ddn_dev_gardner(const void* in, long n, size_t in_stride, int n_channels, int sps, float ted_gain,
                           int symbol_rate_hz, long block_len, DdnTedState* state, float* dl_store, void* out,
                           size_t out_stride, int* out_count, hipStream_t st);
hipError_t ddn_dev_p25_slicer(const float* sym, long n, size_t sym_stride, int n_channels, int negative,
                              DdnSlicerState* state, float* sbuf_store, float* minring, float* maxring, uint8_t* rec,
                              size_t rec_stride, hipStream_t st);
hipError_t ddn_dev_p25_slicer_par(const float* sym, long n, size_t sym_stride, int n_channels, int negative,
                                  DdnSlicerState* state, float* sbuf_store, float* minring, float* maxring,
                                  float* scratch4, uint8_t* rec, size_t rec_stride, hipStream_t st);
hipError_t ddn_dev_p25_matched_filter(const float* in, long n, size_t stride, int n_channels, float* hist, float* out,
                                      hipStream_t st);
#define DDN_MAX_HB_PASSES 4
hipError_t ddn_dev_hb_decim2(const void* in, int in_fmt, long n_in, size_t in_stride, int block_in, int n_channels,
                             int taps_len, void* hist, void* out, size_t out_stride, hipStream_t st);
hipError_t ddn_dev_fm_audio(const DdnFmAudioArgs* args, hipStream_t st);
hipError_t ddn_dev_p25_matched_filter_only(const float* in, long n, size_t stride, int n_channels, const float* hist,
                                           float* out, hipStream_t st);
hipError_t ddn_dev_p25_filter_hist_update(const float* in, long n, size_t stride, int n_channels, float* hist,
                                          hipStream_t st);
int ddn_dev_p25_rx_fuses_filter(const DdnRxConfig* cfg, int channels_per_wave, int n_channels);
hipError_t ddn_dev_p25_rx(const float* raw, const float* filt, const float* prev_tail, float* fstale, long n, size_t stride,
                          int n_channels, const DdnRxConfig* cfg, DdnRxState* state, float* sbuf_store,
                          float* lbuf_store, float* shist_store, float* minring, float* maxring, uint8_t* rec,
                          uint8_t* flags, int32_t* counts, size_t max_sym, int channels_per_wave,
                          const int32_t* lock_cfg, DdnP25HState* hstate, float* hh_store, int32_t* events,
                          int32_t* n_events, hipStream_t st);
/* tap_set: ddn_fsk4::Taps (ddn_fsk4_proto.h), which also gives the tap count */
hipError_t ddn_dev_fsk4_matched_filter(int tap_set, const float* in, long n, size_t stride, int n_channels, const float* hist,
                                       float* out, hipStream_t st);
hipError_t ddn_dev_fsk4_filter_hist_update(int tap_set, const float* in, long n, size_t stride, int n_channels, float* hist,
                                           hipStream_t st);
hipError_t ddn_dev_fsk4_rx(const DdnFsk4RxArgs* args, hipStream_t st);
hipError_t ddn_dev_dmr_burst_gather(const uint8_t* rec, const int32_t* counts, size_t max_sym, const int32_t* sync_pos,
                                    const uint8_t* sync_pat, const uint8_t* pre, const int32_t* n_sync, int n_channels, int max_sync, int inverted,
                                    uint8_t* slot_type, uint8_t* info, uint8_t* cach, uint8_t* valid, hipStream_t st);
hipError_t ddn_dev_ambe2450_deinterleave(const uint8_t* dibits, const uint8_t* reliab, int n, uint8_t* fr, uint8_t* rl,
                                         hipStream_t st);
hipError_t ddn_dev_nxdn_voice_gather(const uint8_t* rec, const int32_t* counts, size_t max_sym, const int32_t* sync_pos,
                                     const int32_t* n_sync, int max_sync, int n_channels, uint8_t* fr, uint8_t* rl,
                                     uint8_t* valid, hipStream_t st);
hipError_t ddn_dev_dmr_voice_gather(const uint8_t* rec, const int32_t* counts, size_t max_sym, const int32_t* burst_start,
                                    int max_bursts, int n_channels, int inverted, uint8_t* fr, uint8_t* rl, uint8_t* sync48,
                                    uint8_t* cach24, uint8_t* valid, hipStream_t st);
hipError_t ddn_dev_dmr_voice_select(const int32_t* events, const int32_t* n_events, int max_events, int carry, const int32_t* sync_pos,
                                    const int32_t* n_sync, int max_syncs, int n_channels, int max_bursts, int32_t* vstart,
                                    int32_t* vpre, int32_t* vn, const int32_t* out_pos, const int32_t* out_n, int max_out,
                                    const int32_t* n_new, hipStream_t st);
hipError_t ddn_dev_dmr_voice_gather_paths(const uint8_t* rec, const int32_t* counts, size_t max_sym, const int32_t* vstart,
                                          const int32_t* vpre, const uint8_t* pre90, int max_bursts, int n_channels, int inverted,
                                          uint8_t* fr, uint8_t* skip3, const uint8_t* pre90_out, long split, hipStream_t st);
hipError_t ddn_dev_nxdn_frame_gather(const uint8_t* rec, const int32_t* counts, size_t max_sym, const int32_t* sync_pos,
                                     const int32_t* n_sync, int n_channels, int max_sync, uint8_t* lich, uint8_t* sacch_sym,
                                     uint8_t* sacch_rel, uint8_t* facch_sym, uint8_t* facch_rel, uint8_t* valid, hipStream_t st);
hipError_t ddn_dev_nxdn_crc(const uint8_t* bytes, int stride, int n, int kind, uint8_t* ok, hipStream_t st);
hipError_t ddn_dev_audio_s16(const float* pcm, int n_streams, int n_frames, float audio_gain, int use_hpf, int use_agsm, float coef,
                             int16_t* out, float* state, float* gain_a, hipStream_t st);
hipError_t ddn_dev_agf(float* pcm, int n_streams, int n_frames, float gain, float* aout_gain, hipStream_t st);
hipError_t ddn_dev_channel_lpf_c2c(const void* in, int in_fmt, long n, size_t in_stride, int block_len, int n_channels,
                                   const float* taps_dev, int taps_len, int has_zero_tap, void* hist, void* out,
                                   size_t out_stride, hipStream_t st);
hipError_t ddn_dev_cqpsk_agc_fll(const void* in, long n, size_t stride, int n_channels, int nt, float alpha, float beta,
                                 const float* d_fll_taps,
                                 DdnCqpskState* state, float* delay_store, void* out, hipStream_t st);
hipError_t ddn_dev_cqpsk_symbols(const void* sym, size_t stride, const int* counts, int n_channels, DdnCqpskState* state,
                                 float* out, size_t out_stride, hipStream_t st);
hipError_t ddn_dev_nid_decode(const uint8_t* bits63, const uint8_t* rel63, const int32_t* obs_nac, const uint8_t* parity,
                              const uint8_t* parity_rel, int threshold, int n, int32_t* out4, hipStream_t st);
hipError_t ddn_dev_golay24(uint8_t* data, const uint8_t* parity, int len, int n, uint8_t* status, int32_t* fixed,
                           hipStream_t st);
hipError_t ddn_dev_golay24_soft(uint8_t* data, const uint8_t* parity, const int32_t* reliab, int len, int n,
                                uint8_t* status, int32_t* fixed, hipStream_t st);
hipError_t ddn_dev_hamming_10_6_3_soft(const uint8_t* bits, const int32_t* reliab, int n, uint8_t* out, uint8_t* status,
                                       hipStream_t st);
hipError_t ddn_dev_isch_lookup(const uint64_t* words, const uint8_t* reliab40, int n, int32_t* out, hipStream_t st);
hipError_t ddn_dev_p25p2_mac_crc(int kind, const uint8_t* payload_bits, int n, uint8_t* crc12_ok, uint8_t* crc16_ok, hipStream_t st);
hipError_t ddn_dev_p25p2_ess(const uint8_t* payload_bits, const int16_t* payload_llr, const uint8_t* parity_bits, const int16_t* parity_llr,
                             int n, int threshold, uint8_t* work, int8_t* erasures28, uint8_t* n_total, int32_t* status,
                             uint8_t* used_dynamic, hipStream_t st);
hipError_t ddn_dev_p25p2_voice_unpack(const uint8_t* xbits360, const int16_t* xllr360, int n, int frame_count, uint8_t* fr, uint8_t* rl,
                                      hipStream_t st);
hipError_t ddn_dev_p25p2_scramble_bits(const uint64_t* seed44, int n, int bit_count, uint8_t* out, hipStream_t st);
hipError_t ddn_dev_p25p2_descramble(const uint8_t* bits, const int16_t* llr, const uint8_t* lbits4320, const int32_t* offset,
                                    const int32_t* seq_of, int n, int n_bits, int n_llr, uint8_t* xbits, int16_t* xllr, hipStream_t st);
hipError_t ddn_dev_p25p2_burst_fields(const uint8_t* bits360, const int16_t* llr360, int n, int threshold, int32_t* duid,
                                      uint64_t* isch_word, uint8_t* isch_rel, hipStream_t st);
hipError_t ddn_dev_p25p2_xcch(int kind, const uint8_t* bits360, const int16_t* llr360, int n, int threshold, uint8_t* payload_bits,
                              uint8_t* parity_bits, int8_t* erasures28, uint8_t* n_total, int32_t* status, uint8_t* used_dynamic,
                              hipStream_t st);
hipError_t ddn_dev_rs28(int kind, uint8_t* payload_bits, const uint8_t* parity_bits, const int8_t* erasures,
                        const uint8_t* n_erasures, int n, int32_t* status, hipStream_t st);
// ddn_rs.hip, for the Phase 2 stages (ddn_p25p2_burst.hip): the decode with the first n_fixed erasures of each section's list, then,
// for the sections that failed, the retries with 1 .. max_add more; ess_rule: a plain decode that located 15 symbols or more is not taken
// (between two files of the library only: not exported)
__attribute__((visibility("hidden"))) hipError_t ddn_rs28_ranked(int kind, uint8_t* payload_bits, const uint8_t* parity_bits, const int8_t* erasures28, const uint8_t* n_total,
                           int n, int32_t* status, uint8_t* used_dynamic, int n_fixed, int max_add, int ess_rule, hipStream_t st);
hipError_t ddn_dev_rs63_soft(uint8_t* data6, const uint8_t* parity6, const uint8_t* data_rel, const uint8_t* parity_rel,
                             int n_par, int n_data, int t, int threshold, int n, uint8_t* status, hipStream_t st);
hipError_t ddn_dev_rs63(uint8_t* data6, const uint8_t* parity6, int n_par, int n_data, int t, int n, uint8_t* status,
                        hipStream_t st);
hipError_t ddn_dev_hamming_10_6_3(uint8_t* bits10, int n, uint8_t* errs, hipStream_t st);
hipError_t ddn_dev_p25_crc16(const uint8_t* bytes, int item_bytes, int n, uint8_t* ok, hipStream_t st);
hipError_t ddn_dev_p25_lsd(uint8_t* bits16, const int16_t* llr16, int n, uint8_t* ok, hipStream_t st);
hipError_t ddn_dev_iq_cond_disc(const void* in, long n, size_t stride, int block_len, int n_channels,
                                const DdnIqCondConfig* cfg, DdnFskState* fsk, DdnIqCondState* cond, float* out,
                                size_t out_stride, hipStream_t st);
hipError_t ddn_dev_find_syncs(const uint8_t* flags, const int32_t* counts, int n_channels, size_t max_sym, int max_frames,
                              int32_t* sync_pos, int32_t* n_syncs, int32_t* dropped, hipStream_t st);
hipError_t ddn_dev_gather_fields(const uint8_t* rec, size_t max_sym, const int32_t* counts, const int32_t* sync_pos,
                                 const int32_t* n_syncs, int n_channels, int max_frames, const int32_t* offsets, int n_off,
                                 int max_off, uint8_t* bits, uint8_t* rel, int16_t* llr, int stride, int split_last,
                                 uint8_t* last_bit, uint8_t* last_rel, uint8_t* valid, uint8_t* dibits,
                                 uint8_t* dibit_rel, hipStream_t st);
hipError_t ddn_dev_rs_pack(const uint8_t* words, long n_slots, int n_words, int wstride, int n_data, uint8_t* data,
                           uint8_t* parity, hipStream_t st);
hipError_t ddn_dev_tdulc_rs_pack(const uint8_t* words, long n_slots, uint8_t* data, uint8_t* parity, hipStream_t st);
hipError_t ddn_dev_voice_index(const int32_t* sync_pos, const int32_t* n_syncs, const int32_t* nid4, const int32_t* counts, int n_channels,
                               int max_frames, int max_ldu, size_t max_sym, const int32_t* first9, const int32_t* status9,
                               int64_t* first, int32_t* status, int32_t* n_ldu, int fill_tail, hipStream_t st);
// live voice slots: live_off [n_channels + 1] = prefix sums of 9 * n_ldu in channel order, *n_live = the total (a device word)
hipError_t ddn_dev_voice_live_scan(const int32_t* n_ldu, int n_channels, int max_ldu, int32_t* live_off, int32_t* n_live, hipStream_t st);
hipError_t ddn_dev_imbe_index(const int32_t* sync_pos, const int32_t* n_syncs, int n_channels, int max_frames,
                              size_t max_sym, const int32_t* first9, const int32_t* status9, int64_t* first,
                              int32_t* status, hipStream_t st);
hipError_t ddn_dev_resample(const float* in, long n, size_t in_stride, int n_channels, float* hist, const float* taps,
                            int L, int M, int p0, long n_out, float* out, size_t out_stride, hipStream_t st);
hipError_t ddn_dev_imbe_deinterleave(const uint8_t* rec, long n_records, const int64_t* first, const int32_t* status_count,
                                     int n_frames, uint8_t* fr, uint8_t* soft, uint8_t* flags, int32_t* status_out,
                                     hipStream_t st);
// The chain object's voice kernels walk the call's live list (live_slot [*n_live], k_voice_live_fill) by a grid that does not depend on
// the count, which stays on the device: min(what the slots would need, a cap) single-wave workgroups, each striding through the list.
// The caps, by how evenly a kernel's frames cost:
//   de-interleave  every frame costs the same: one workgroup per wave slot of the device (256 CUs x 4 SIMDs x 8), ten frames each on
//                  the bench shape
//   frame decode   a pass of 32 frames costs the same: a workgroup per 32 slots up to the cap, so a pass each at most on the bench
//                  shape (with fewer workgroups than passes some would take two where others take one)
//   synthesis      a frame costs by its harmonics (9 .. 56) and voicing: few frames per workgroup, so that the dispatcher evens the
//                  load out as it did with a workgroup per slot; a workgroup past the list's end leaves at once
#define DDN_VOICE_LIVE_GRID        8192
#define DDN_VOICE_LIVE_GRID_DECODE 16384
#define DDN_VOICE_LIVE_GRID_SYNTH  65536
hipError_t ddn_dev_imbe_deinterleave_live(const uint8_t* rec, long n_records, const int64_t* first, const int32_t* status_count, int n_slots,
                                          const int32_t* live_slot, const int32_t* n_live, uint8_t* fr, uint8_t* soft, uint8_t* flags,
                                          int32_t* status_out, hipStream_t st);
hipError_t ddn_dev_r34_list(const uint8_t* dibits, const uint8_t* reliab, int n, int max_cand, uint8_t* backs,
                            uint32_t* cand, int32_t* count, hipStream_t st);
/* The sparse forms below take `wanted` [n] (one byte per item, 0 = nobody reads this item; NULL = every item is wanted).  A wanted
 * item reads exactly what the dense form gives for it.  What an UNWANTED item reads differs from family to family and is written at
 * each declaration, as the kernels do it and as the chains rely on it (tests/test_fec_sparse_gpu.py holds every line against
 * sentinel-filled buffers).  Nothing is written outside items [0, n) in any of them. */
/* unwanted item: count = 0, its eight candidates left unwritten.  (Wanted item: candidates [count .. 8) are left unwritten too; the
 * skip is per item - one workgroup per item, min(n, 65536) workgroups that walk the items with that stride.) */
hipError_t ddn_dev_p25_mbf34_list(const int16_t* llr, int n, int max_cand, const uint8_t* wanted, uint8_t* cand24, int32_t* count,
                                  hipStream_t st);
hipError_t ddn_dev_p25_half_rate_list(const int16_t* llr, int n, int max_cand, uint32_t* cand, int32_t* count,
                                      hipStream_t st);
hipError_t ddn_dev_p25_half_rate(const int16_t* llr, int n, uint8_t* out, int32_t* metric, hipStream_t st);
hipError_t ddn_dev_r34(const uint8_t* dibits, const uint8_t* reliab, int n, uint8_t* out, hipStream_t st);
/* with a list: groups of 4 items, at most 1024 workgroups (16384 in the _wide form) that walk the groups with that stride.  Unwanted
 * item in a group with no wanted item: count = 0, candidates left unwritten.  Unwanted item beside a wanted one (same group of 4): decoded
 * like a wanted item (count and candidates of the dense form).  So count > 0 always comes with valid candidates, which is what
 * ddn_dev_chain_pdu_take_first reads.  Candidates [count .. 8) of a decoded item are zero.  wanted = NULL: the dense form (groups of 32). */
hipError_t ddn_dev_p25_half_rate_list_wanted(const int16_t* llr, int n, int max_cand, const uint8_t* wanted, uint32_t* cand, int32_t* count,
                                             hipStream_t st);
hipError_t ddn_dev_p25_half_rate_list_wanted_wide(const int16_t* llr, int n, int max_cand, const uint8_t* wanted, uint32_t* cand,
                                                  int32_t* count, hipStream_t st);
/* groups of 16 rows; row i is wanted where wanted[i / wanted_div] != 0 (wanted_div = 2: the two FACCH halves of one slot).  Unwanted row
 * in a group with no wanted row: its (n_bits + 7) / 8 output bytes are zero.  Unwanted row beside a wanted one: decoded like a wanted row.
 * Either way the bytes of a row beyond (n_bits + 7) / 8 and an unwanted row's metrics_io are left as they were (the chains pass no
 * metrics and read unwanted rows nowhere).  n_steps is the caller's to check against ddn_dev_k5_nxdn_lds: a length that does not fit is
 * answered with hipErrorInvalidValue and not launched. */
hipError_t ddn_dev_k5_nxdn_lds(int n_steps, bool soft, size_t* need, size_t* limit);
hipError_t ddn_dev_k5_nxdn_wanted(const uint8_t* sym, const uint8_t* rel, int n, int n_steps, int n_bits, uint16_t* metrics_io,
                                  uint8_t* out, int out_stride, const uint8_t* wanted, int wanted_div, hipStream_t st);
/* unwanted row (per row, groups of 64 play no part): its result_len output bytes are zero */
hipError_t ddn_dev_trellis_greedy_wanted(const uint8_t* src, int src_stride, size_t n, int result_len, uint8_t* out, int out_stride,
                                         const uint8_t* wanted, hipStream_t st);
/* groups of 8 items, one workgroup each.  Unwanted item, whatever its neighbours: count = 0, its 32 candidates left unwritten (and its
 * part of `backs` untouched).  Candidates [count .. 32) of a wanted item are zero. */
hipError_t ddn_dev_r34_list_wanted(const uint8_t* dibits, const uint8_t* reliab, int n, int max_cand, const uint8_t* wanted, uint8_t* backs,
                                   uint32_t* cand, int32_t* count, hipStream_t st);
// the DMR chain's data-burst / embedded-signalling stages (ddn_dmr_data.hip, k_dmr_r34_pick in ddn_trellis.hip)
hipError_t ddn_dev_dmr_data_select(const int32_t* events, const int32_t* n_events, int max_events, int carry, int n_channels,
                                   int max_bursts, const int32_t* sync_pos, const int32_t* n_sync, int max_syncs, const int32_t* out_pos,
                                   const int32_t* out_n, int max_out, const int32_t* n_new, int32_t* dstart, uint8_t* dslot,
                                   int32_t* dpre, int32_t* dn, hipStream_t st);
hipError_t ddn_dev_dmr_data_gather(const uint8_t* rec, size_t max_sym, const int32_t* dstart, const int32_t* dpre, const uint8_t* pre90,
                                   const uint8_t* prel90, const uint8_t* pre90_out, const uint8_t* prel90_out, long split, int max_bursts,
                                   int n_channels, uint8_t* slot_type, uint8_t* info, uint8_t* td98, uint8_t* rel98, hipStream_t st);
hipError_t ddn_dev_dmr_data_prep(const int32_t* dstart, const uint8_t* slot_type, const uint8_t* st_ok, const uint8_t* pdu96, int n,
                                 uint8_t* type, uint8_t* bytes12, uint8_t* cw12, hipStream_t st);
hipError_t ddn_dev_dmr_data_finish(const uint8_t* type, const uint8_t* pdu96, const uint8_t* info, const uint8_t* cw12,
                                   const uint8_t* rs_result, int n, uint8_t* bytes12, uint8_t* crc, uint8_t* r34_wanted, hipStream_t st);
/* one thread per burst (workgroups of 64).  Unwanted burst: pool_n = 0, conf_crc = 0, unconf18 and conf18 zero, its pool24 entries left
 * unwritten (hard18 / soft18 / list24 / list_n of that burst are not read).  Pool entries [pool_n .. 34) of a wanted burst are left
 * unwritten as well. */
hipError_t ddn_dev_dmr_r34_pick(const uint8_t* td98, const uint8_t* rel98, const uint8_t* wanted, const uint8_t* hard18,
                                const uint8_t* soft18, const uint8_t* list24, const int32_t* list_n, int n, uint8_t* pool24,
                                int32_t* pool_n, uint8_t* unconf18, uint8_t* conf18, uint8_t* conf_crc, hipStream_t st);
hipError_t ddn_dev_dmr_emb_collect(const int32_t* events, const int32_t* n_events, int max_events, int carry, const uint8_t* rec,
                                   size_t max_sym, int n_channels, int max_lc, uint8_t* sig, uint8_t* in128, int32_t* lc_pos,
                                   int32_t* lc_n, hipStream_t st);
hipError_t ddn_dev_dmr_emb_finish(const uint8_t* out77, const int32_t* lc_pos, int n, uint8_t* ok, hipStream_t st);
// NXDN CAC / FACCH2 / UDCH frames and the SACCH superframe state (ddn_nxdn_ctrl.hip).  gather: kind and the two wanted flags of
// every slot, the K = 5 decoders' rows of the wanted ones ([S][350] CAC, [S][406] FACCH2 / UDCH: symbols, reliabilities, hard bits);
// finish: soft rows of stride 26, hard rows of stride 208, any output may be null
size_t ddn_dev_nxdn_ctrl_state_bytes(void);
hipError_t ddn_dev_nxdn_ctrl_state_init(void* state, int n_channels, hipStream_t st);
hipError_t ddn_dev_nxdn_ctrl_gather(const uint8_t* rec, const int32_t* counts, size_t max_sym, const int32_t* sync_pos, const int32_t* n_sync,
                                    int n_channels, int max_sync, uint8_t* kind, uint8_t* sym_c, uint8_t* rel_c, uint8_t* hard_c,
                                    uint8_t* sym_f, uint8_t* rel_f, uint8_t* hard_f, uint8_t* want_c, uint8_t* want_f, hipStream_t st);
hipError_t ddn_dev_nxdn_ctrl_finish(const uint8_t* kind, const uint8_t* soft_c, const uint8_t* soft_f, const uint8_t* hard_c,
                                    const uint8_t* hard_f, size_t n, uint8_t* bits208, uint8_t* bytes26, uint8_t* crc_ok, uint8_t* fallback,
                                    uint8_t* ran, uint8_t* sf, hipStream_t st);
hipError_t ddn_dev_nxdn_ctrl_walk(const int32_t* n_sync, int n_channels, int max_sync, const uint8_t* lich, const uint8_t* valid,
                                  const uint8_t* sacch, const uint8_t* sacch_ok, const uint8_t* sacch_hard, const uint8_t* sacch_hard_ok,
                                  const uint8_t* kind, const uint8_t* crc_ok, const uint8_t* ran, const uint8_t* sf, void* state,
                                  uint8_t* sacch_status, uint8_t* pf, uint8_t* seq_ok, uint8_t* msg72, uint8_t* msg_status, int32_t* last_ran,
                                  int32_t* cac_fail, hipStream_t st);
// DMR MS / direct-mode bursts (ddn_dmr_ms.hip).  walk: one lane per channel, every array required; gathers: one workgroup per burst
// slot, a slot the walk left unused (gate < 0 / vc = 0) writes zeros
struct DdnDmrMsWalk {
    const uint8_t* rec;
    const int32_t *counts, *n_new, *sync_pos, *n_sync;
    const uint8_t *sync_pat, *pre90;
    size_t max_sym;
    int n_channels, max_syncs, max_data, max_voice, max_lc;
    void* state;
    int32_t *n_data, *data_start, *data_pre, *data_gate;
    uint8_t *data_pat, *data_slot, *data_status, *data_cc;
    int32_t *n_voice, *voice_start, *voice_pre;
    uint8_t *voice_vc, *voice_tact, *voice_emb_ok, *voice_emb_cc, *voice_power, *voice_sync48;
    int32_t *n_lc, *lc_pos;
    uint8_t* lc_in128;
    int32_t *cc, *dropped, *phase;
};
size_t ddn_dev_dmr_ms_state_bytes(void);
hipError_t ddn_dev_dmr_ms_state_init(void* state, int n_channels, hipStream_t st);
hipError_t ddn_dev_dmr_ms_walk(const DdnDmrMsWalk* w, hipStream_t st);
hipError_t ddn_dev_dmr_ms_data_gather(const uint8_t* rec, size_t max_sym, const int32_t* dstart, const int32_t* dpre, const int32_t* gate,
                                      const uint8_t* pre90, const uint8_t* prel90, int max_data, int n_channels, uint8_t* slot_type,
                                      uint8_t* info, uint8_t* td98, uint8_t* rel98, hipStream_t st);
hipError_t ddn_dev_dmr_ms_voice_gather(const uint8_t* rec, size_t max_sym, const int32_t* vstart, const int32_t* vpre, const uint8_t* vc,
                                       const uint8_t* pre90, int max_voice, int n_channels, uint8_t* dib108, uint8_t* skip3, hipStream_t st);
// the DMR protocol layer behind the data bursts: resets / carrier loss between them, the walk to completed PDUs (ddn_dmr_pdu.hip)
size_t ddn_dev_dmr_pdu_state_bytes(void);
hipError_t ddn_dev_dmr_pdu_marks(const int32_t* events, const int32_t* n_events, int max_events, const uint8_t* flags, size_t stride,
                                 int carry, const int32_t* n_new, const int32_t* dstart, const int32_t* dn, int n_channels, int max_bursts,
                                 void* state, int32_t* reset_before, int32_t* n_resets, int32_t* loss_before, int32_t* n_losses,
                                 int max_marks, hipStream_t st);
hipError_t ddn_dev_dmr_pdu_walk(const int32_t* n_bursts, int n_channels, int max_bursts, const uint8_t* bslot, const uint8_t* btype,
                                const uint8_t* bytes12, const uint8_t* info196, const uint32_t* errs, const uint8_t* crcflags,
                                const uint8_t* unconf18, const void* pool, const int32_t* pool_n, const int32_t* n_resets,
                                const int32_t* reset_before, const int32_t* n_losses, const int32_t* loss_before, int max_marks, void* state,
                                uint8_t* o_conf, int32_t* o_counter, uint8_t* o_crc, uint8_t* o_dbsn, int32_t* o_pick, uint8_t* o_status,
                                uint8_t* pdu_kind, uint8_t* pdu_slot, int32_t* pdu_burst, int32_t* pdu_len, uint8_t* pdu_bytes,
                                uint8_t* pdu_crc4, uint8_t* pdu_block_crc, int32_t* pdu_header9, int max_pdus, int32_t* n_pdus,
                                hipStream_t st);
hipError_t ddn_dev_k5_nxdn(const uint8_t* sym, const uint8_t* rel, int n, int n_steps, int n_bits, uint16_t* metrics_io,
                           uint8_t* out, int out_stride, hipStream_t st);
hipError_t ddn_dev_k5_m17(const uint16_t* in, int n, int in_len, int u_len, const DdnPuncture* pu, uint8_t* out,
                          int out_stride, uint32_t* cost, hipStream_t st);
/* groups of 16 code words.  Unwanted code word in a group with no wanted one: out and cost LEFT UNWRITTEN (whatever the buffers held
 * stays: the callers in ddn_api_m17.cpp read a row only where the same flag is set).  Unwanted beside a wanted one: decoded like a wanted
 * code word.  A decoded row's out_stride bytes are all written (zero beyond the decoded bits). */
hipError_t ddn_dev_k5_m17_wanted(const uint16_t* in, int n, int in_len, int u_len, const DdnPuncture* pu, uint8_t* out, int out_stride,
                                 uint32_t* cost, const uint8_t* wanted, hipStream_t st);
hipError_t ddn_dev_launch_fused(const DdnFusedArgs* a, const float* taps_host, int group, hipStream_t st);
hipError_t ddn_dev_launch_fused_ex(const DdnFusedArgs* a, bool has_zero, int group, hipStream_t st);
hipError_t ddn_dev_launch_carry(const void* in, int in_fmt, size_t ch_stride, long n, void* carry, int n_channels,
                                hipStream_t st);
hipError_t ddn_dev_zero(void* p, size_t bytes, hipStream_t st);
/* Frame-slot selection for the per-slot framer / FEC launches of a chain (ddn_api_chain.cpp): a launch made while a selection is
 * set walks `*count` frame slots taken from `list` (per_slot items each) instead of every slot - the work follows the frames of
 * that type, not the slot capacity; the other slots' outputs are left as they are.  Thread-local, set around the launches it is
 * meant for; list == NULL = every item. */
/* Workgroup size of the chains' small decode kernels (gathers, packs, block codes, selections): ONE wavefront.  In the pipelined chain
 * they run beside the next call's front-end kernel, whose ten waves per CU take every register of two of a CU's four SIMDs (3 x 168):
 * a workgroup of several waves needs room on every SIMD at once and waited for a front-end workgroup to end (~2 ms, measured);
 * single-wave workgroups go to the SIMDs that have room. */
#define DDN_WG 64
typedef struct DdnSel {
    const int32_t* list;  /* frame slots of the type, any order */
    const int32_t* count; /* device word: entries in list */
    int per_slot;         /* items of this launch per frame slot */
} DdnSel;
void ddn_sel_set(const int32_t* list, const int32_t* count);
void ddn_sel_clear(void);
DdnSel ddn_sel_for(int per_slot);
/* blocks for a launch of n_blocks_full blocks when a selection is active (the list decides the work, the grid only has to fill the
 * device) */
static inline unsigned
ddn_sel_grid(const DdnSel* sel, unsigned long n_blocks_full) {
    const unsigned long cap = 4096; /* x DDN_WG (64 threads) */
    return (unsigned)((sel->list && n_blocks_full > cap) ? cap : (n_blocks_full ? n_blocks_full : 1));
}
hipError_t ddn_dev_chain_pcm_compact(const int32_t* result5, const float* pcm, int n_slots, long capacity, int32_t* block_cnt,
                                     int32_t* block_off, float* dense, int32_t* slot_of, int32_t* total, hipStream_t st);
/* what a voice slot without a frame holds in the chain object's result arrays: taken once, at create, from the kernels themselves
 * (one all-zero IMBE frame with its skip flag through the frame decode, the parameter kernel and the synthesis) */
typedef struct {
    uint8_t bits[88];   /* d_imbe_bits: the decode of the all-zero frame */
    int32_t res[5];     /* d_imbe_result: its result words, the skip flag or-ed in */
    int32_t res_out[5]; /* d_synth_result: the silent record's result words */
    int32_t pad;
    float pcm[160];     /* d_pcm: the silent frame */
} DdnVoiceDead;
/* k_voice_live_fill: the live list of a call + the dead pattern back into the slots that left it.  was_*: one "live when this array
 * was last written" byte per slot and array; an array that is not kept (null was_*) is left alone */
typedef struct {
    int n_slots, max_ldu;    /* n_slots = channels * max_ldu * 9 */
    const int32_t* n_ldu;    /* [channels] */
    const int32_t* live_off; /* [channels + 1] (k_voice_live_scan) */
    int32_t* live_slot;      /* [n_slots] out: the first live_off[channels] entries */
    const DdnVoiceDead* dead;
    uint8_t *bits, *was_bits;
    int32_t* res;
    uint8_t* was_res;
    int32_t* res_out;
    uint8_t* was_res_out;
    float* pcm;
    uint8_t* was_pcm;
} DdnVoiceLive;
hipError_t ddn_dev_voice_live_fill(const DdnVoiceLive* a, hipStream_t st);
hipError_t ddn_dev_chain_pack2(const uint8_t* rec, const uint8_t* fl, size_t n, uint8_t* out2, hipStream_t st);
hipError_t ddn_dev_chain_carry(const uint8_t* rec_prev, const uint8_t* fl_prev, const int32_t* cnt_prev, int have_prev,
                               uint8_t* rec_cur, uint8_t* fl_cur, size_t stride_sym, int T, int n_channels, hipStream_t st);
hipError_t ddn_dev_chain_counts(const int32_t* cnt_new, int T, int n_channels, int flush, int32_t* cnt_scan, int32_t* cnt_full,
                                hipStream_t st);
/* ---- ddn_cqrx.hip: the symbol-rate receive loop behind the CQPSK demodulator ---- */
typedef struct DdnCqConfig {
    int protocol;      /* 0 P25 Phase 1, 1 P25 Phase 2 */
    int sync_len;      /* 24 / 20 dibits */
    int t_max;         /* level ring: 24 / 19 */
    int lock_symbols;  /* < 0: the P25p1 handlers decide; Phase 2: 700 */
    int snr_scale;     /* the CQPSK SNR weight as the numerator over 256 (204 + (w256 >> 2)), -1 = no weight (SNR not available) */
    int nid_threshold; /* p25p1_get_erasure_threshold() */
    int max_events;
    int dbg;           /* A/B experiments (ddn_cq_rx_set_debug_flags): 1 = no hard-path short cut ahead of the half-rate decoder */
    uint64_t target[2][4]; /* [polarity][identity, X2400, N1200, P1200]: the sync word as raw dibits, oldest in the high bits */
} DdnCqConfig;
typedef struct DdnCqState { /* one channel, carried from call to call */
    float minbuf[1024], maxbuf[1024]; /* the extrema average's window (dsd_state: minbuf / maxbuf, msize 1024) */
    float sbuf[128];                  /* the slicer window (ssize 128) */
    float lbuf[24], shist[24];        /* level ring of the frame search, symbol history */
    int32_t d[100];                   /* a trellis block being read: de-interleaved LLR pairs */
    uint8_t nb[64], nr[64];           /* a NID being read: bits / reliabilities */
    double min_sum, max_sum;
    uint64_t hist;
    float max, min, lmin, lmax;
    int32_t sidx, midx, sums_valid;
    int32_t have_sync, lock_left, lastsync, map_idx, lidx, level_count, hist_count, shead, scount, hunt_pos;
    int32_t h_phase, h_idx, h_left, h_block, h_end, h_skip, h_k, h_nac, h_p2cc;
    int32_t pad_;
} DdnCqState;
hipError_t ddn_dev_cq_rx_init(DdnCqState* states, int n_channels, hipStream_t st);
hipError_t ddn_dev_cq_rx(const float* symbols, const int32_t* counts_in, size_t sym_stride, int n_fixed, int n_channels, const DdnCqConfig* cfg,
                         DdnCqState* states, uint8_t* rec, uint8_t* flags, int32_t* counts_out, size_t max_sym, int32_t* events,
                         int32_t* n_events, int32_t* event_data, hipStream_t st);
hipError_t ddn_dev_zero_words(int32_t* p, int n, hipStream_t st);
hipError_t ddn_dev_fill_words(int32_t* p, int n, int32_t value, hipStream_t st);
hipError_t ddn_dev_chain_events(const int32_t* list_prev, const int32_t* data_prev, const int32_t* n_prev, const int32_t* new_prev,
                                int have_prev, const int32_t* ev_new, const int32_t* evd_new, const int32_t* n_new, int E, int EL, int T,
                                int n_channels, int32_t* list_cur, int32_t* data_cur, int32_t* n_cur, hipStream_t st);
hipError_t ddn_dev_chain_pdu_index(const int32_t* list, const int32_t* data, const int32_t* n_list, int EL, const int32_t* sync_pos,
                                   const int32_t* n_syncs, const int32_t* nid4, int n_channels, int F, int off0, int PF,
                                   int32_t* pdu_slot, uint8_t* pdu_hdr, int32_t* pdu_info, int32_t* n_pdu, hipStream_t st);
hipError_t ddn_dev_chain_pdu_gather(const uint8_t* rec, const int32_t* counts, size_t max_sym, const int32_t* sync_pos,
                                    const int32_t* pdu_slot, const int32_t* pdu_info, int n_channels, int F, int PF, int PB,
                                    int16_t* llr, uint8_t* valid, hipStream_t st);
hipError_t ddn_dev_chain_pdu_finish(const int32_t* pdu_slot, const uint8_t* blocks12, const uint8_t* valid, const uint8_t* blocks18,
                                    const uint8_t* hcand16, const int32_t* hcount, const uint8_t* hwanted, int n_entries, int PB,
                                    uint8_t* pdu_hdr, int32_t* pdu_info, hipStream_t st);
hipError_t ddn_dev_chain_pdu_combine(const uint8_t* rec, const int32_t* counts, size_t max_sym, const int32_t* sync_pos,
                                     const int32_t* pdu_slot, const int32_t* pdu_info, const int16_t* llr, const uint8_t* valid,
                                     const uint8_t* blocks12, int n_entries, int PF, int PB, int16_t* hllr, uint8_t* wanted, hipStream_t st);
hipError_t ddn_dev_chain_pdu_take_first(const uint8_t* cand16, const int32_t* counts, int n_blocks, uint8_t* blocks12, int32_t* metric,
                                        hipStream_t st);
hipError_t ddn_dev_chain_pdu_r34_wanted(const int32_t* pdu_slot, const uint8_t* pdu_hdr, const int32_t* pdu_info, const uint8_t* valid,
                                        int n_blocks, int PB, uint8_t* wanted, hipStream_t st);
hipError_t ddn_dev_chain_pdu_r34_select(const uint8_t* cand24, const int32_t* counts, const uint8_t* wanted, int n_blocks,
                                        uint8_t* blocks18, uint8_t* crc9_ok, hipStream_t st);
/* long data units (ddn_p25_chain_set_long_data_units): the per-channel state carried across calls, the block store, the work list
 * and the outputs.  Block store: units [2 B] (two carry buffers per channel) then [B * P] (the output entries), MB blocks each. */
typedef struct DdnLongPdu {
    int B, MB, P, W, PB;
    int32_t* open;      /* [B] 1 = a unit is open at the end of the last decode */
    int32_t* open_buf;  /* [B] carry buffer (0 / 1) of the open unit */
    int32_t* sync;      /* [B] its sync's row index in the last decode's row */
    int32_t* next;      /* [B] its next data block to decode (1 ..) */
    int32_t* end;       /* [B] blocks the reference reads, header included */
    int64_t* base;      /* [B] new records of every decode before this one (since the switch was set) */
    int64_t* open_rec;  /* [B] stream record of the open unit's sync */
    uint8_t* open_hdr;  /* [B][12] */
    uint8_t *blocks, *valid, *blocks18, *crc9; /* store: [U][MB][12], [U][MB], [U][MB][18], [U][MB] */
    int32_t* n;         /* [B] units finished in this call */
    int64_t* out_rec;   /* [B][P] */
    uint8_t* out_hdr;   /* [B][P][12] */
    int32_t* out_info;  /* [B][P][4] */
    int32_t* fin;       /* [B][P] store unit the entry's blocks are copied from at finish, -1 = decoded in place */
    int32_t* nw;        /* [B] work slots used */
    int32_t *wk_row, *wk_dst; /* [B][W] row index of the unit's frame start (sync - 23); store unit * MB + block - 1 */
    uint8_t *wk_want, *wk_want34;
    int16_t* wk_llr;    /* [B][W][196] */
    uint8_t* wk_cand;   /* [B][W][8][24] */
    int32_t *wk_cnt, *wk_metric;
    uint8_t *wk_b12, *wk_b18, *wk_c9;
} DdnLongPdu;
hipError_t ddn_dev_lpdu_index(const DdnLongPdu* lp, const int32_t* list, const int32_t* data, const int32_t* n_list, int EL,
                              const int32_t* sync_pos, const int32_t* n_syncs, const int32_t* nid4, const int32_t* cnt_full,
                              size_t max_sym, const int32_t* new_prev, int have_prev, int flush, int F, int T, int off0, hipStream_t st);
hipError_t ddn_dev_lpdu_gather(const DdnLongPdu* lp, const uint8_t* rec, const int32_t* cnt_full, size_t max_sym, hipStream_t st);
hipError_t ddn_dev_lpdu_scatter(const DdnLongPdu* lp, hipStream_t st);
hipError_t ddn_dev_lpdu_finish(const DdnLongPdu* lp, hipStream_t st);
hipError_t ddn_dev_chain_frames(const int32_t* list,const int32_t* data, const int32_t* n_list, int EL, const int32_t* sync_pos,
                                const int32_t* n_syncs, int n_channels, int F, int off0, int off1, int off2, int32_t* nid4,
                                uint8_t* tsbk, uint8_t* tsbk_crc, uint8_t* cls, int32_t* lists, int32_t* list_n, hipStream_t st);
enum { DDN_CLS_LDU1 = 1, DDN_CLS_LDU2 = 2, DDN_CLS_HDU = 4, DDN_CLS_TDULC = 8 }; /* frame-type bits of a slot's class byte */
enum { DDN_LIST_LDU1 = 0, DDN_LIST_LDU2 = 1, DDN_LIST_HDU = 2, DDN_LIST_TDULC = 3, DDN_LIST_LSD = 4, DDN_LIST_COUNT = 5 }; /* work lists [k][S] */
hipError_t ddn_dev_nxdn_voice_select(const int32_t* sync_pos, const int32_t* n_sync, const uint8_t* lich, const uint8_t* valid,
                                     int n_channels, int my, int vf, int32_t* v_pos, int32_t* v_n, uint8_t* skip4, hipStream_t st);
hipError_t ddn_dev_fsk4_chain_syncs(const int32_t* c_pos, const uint8_t* c_pat, const uint8_t* c_pre, const uint8_t* c_prel,
                                    const int32_t* c_n, int myc, const int32_t* s_pos, const uint8_t* s_pat, const uint8_t* s_pre,
                                    const uint8_t* s_prel, const int32_t* s_n, int my, const int32_t* n_new, int T, int flush,
                                    int32_t* d_pos, uint8_t* d_pat, uint8_t* d_pre, uint8_t* d_prel, int32_t* d_n, int myd,
                                    int32_t* o_pos, uint8_t* o_pat, uint8_t* o_pre, uint8_t* o_prel, int32_t* o_n, int32_t* dropped,
                                    int n_channels, hipStream_t st);
hipError_t ddn_dev_fsk4_chain_syncs_thr(const int32_t* c_pos, const uint8_t* c_pat, const uint8_t* c_pre, const uint8_t* c_prel,
                                        const int32_t* c_n, int myc, const int32_t* s_pos, const uint8_t* s_pat, const uint8_t* s_pre,
                                        const uint8_t* s_prel, const int32_t* s_n, int my, const int32_t* n_new, int T, int flush,
                                        int32_t* d_pos, uint8_t* d_pat, uint8_t* d_pre, uint8_t* d_prel, int32_t* d_n, int myd,
                                        int32_t* o_pos, uint8_t* o_pat, uint8_t* o_pre, uint8_t* o_prel, int32_t* o_n, int32_t* dropped,
                                        int n_channels, const float* c_thr, const float* s_thr, float* d_thr, float* o_thr, hipStream_t st);
/* ---- ddn_m17.hip / ddn_dpmr.hip: the launchers behind the M17, YSF and dPMR frame decoders (ddn_api_m17.cpp, the fsk4 chain) ---- */
hipError_t ddn_dev_m17_lsf_cost(const uint8_t* rec, size_t stride, const int32_t* counts, const int32_t* sync_pos,
                                const uint8_t* sync_pat, const int32_t* n_sync, const float* sync_thr, int n_channels,
                                int max_syncs, int lmax, uint16_t* cost488, int32_t* slot_sync, hipStream_t st);
hipError_t ddn_dev_m17_lsf_finish(const uint8_t* dec, int dec_stride, const uint32_t* cost, const int32_t* slot_sync,
                                  int n_channels, int lmax, int max_syncs, uint8_t* lsf30, uint8_t* status,
                                  uint32_t* path_cost, hipStream_t st);
hipError_t ddn_dev_m17_str_bits(const uint8_t* rec, size_t stride, const int32_t* counts, const int32_t* sync_pos,
                                const uint8_t* sync_pat, const int32_t* n_sync, int n_channels, int max_syncs, int lmax,
                                uint8_t* sym296, int32_t* slot_sync, uint8_t* slot_lich6, uint8_t* slot_cnt, uint8_t* slot_ok,
                                hipStream_t st);
hipError_t ddn_dev_m17_str_finish(const uint8_t* dec, int dec_stride, const int32_t* slot_sync, const uint8_t* slot_lich6,
                                  const uint8_t* slot_cnt, const uint8_t* slot_ok, int n_channels, int lmax, int max_syncs,
                                  uint8_t* lich6, uint8_t* lich_cnt, uint8_t* fn_payload18, uint8_t* status, hipStream_t st);
hipError_t ddn_dev_m17_lich(const uint8_t* sync_pat, const int32_t* n_sync, int n_channels, int max_syncs, const uint8_t* lsf30,
                            const uint8_t* lsf_status, const uint8_t* lich6, const uint8_t* lich_cnt, const uint8_t* str_status,
                            uint8_t* asm30, uint8_t* lich_lsf30, uint8_t* lich_status, hipStream_t st);
// M17 packet / BERT frames and the per-channel state behind them (ddn_m17_data.hip)
size_t ddn_dev_m17_data_state_bytes(void);
hipError_t ddn_dev_m17_pkt_cost(const uint8_t* rec, size_t stride, const int32_t* counts, const int32_t* sync_pos, const uint8_t* sync_pat,
                                const int32_t* n_sync, const float* sync_thr, int n_channels, int max_syncs, int lmax, uint16_t* cost420,
                                int32_t* slot_sync, uint8_t* slot_want, hipStream_t st);
hipError_t ddn_dev_m17_pkt_finish(const uint8_t* dec, int dec_stride, const uint32_t* cost, const int32_t* slot_sync, int n_channels,
                                  int lmax, int max_syncs, uint8_t* pkt26, uint8_t* status, uint32_t* path_cost, hipStream_t st);
hipError_t ddn_dev_m17_brt_bits(const uint8_t* rec, size_t stride, const int32_t* counts, const int32_t* sync_pos, const uint8_t* sync_pat,
                                const int32_t* n_sync, int n_channels, int max_syncs, int lmax, uint8_t* sym402, int32_t* slot_sync,
                                uint8_t* slot_want, hipStream_t st);
hipError_t ddn_dev_m17_brt_finish(const uint8_t* dec, int dec_stride, const int32_t* slot_sync, int n_channels, int lmax, int max_syncs,
                                  uint8_t* bits25, uint8_t* status, hipStream_t st);
hipError_t ddn_dev_m17_data_walk(const uint8_t* sync_pat, const int32_t* sync_pos, const int32_t* n_sync, const int32_t* advance,
                                 int n_channels, int max_syncs, const uint8_t* pkt26, const uint8_t* pkt_frame_status,
                                 const uint8_t* bits25, const uint8_t* brt_frame_status, void* state, uint8_t* pkt_status,
                                 uint8_t* pkt_count, int32_t* brt_state, uint8_t* packet, int32_t* packet_app_len, uint8_t* packet_crc_ok,
                                 int32_t* packet_slot, int32_t* n_packets, int max_packets, hipStream_t st);
hipError_t ddn_dev_ysf_fich_cost(const uint8_t* rec, size_t stride, const int32_t* counts, const int32_t* sync_pos,
                                 const int32_t* n_sync, int n_channels, int max_syncs, int lmax, uint16_t* cost200,
                                 int32_t* slot_sync, hipStream_t st);
hipError_t ddn_dev_ysf_fich_finish(const uint8_t* dec, int dec_stride, const uint32_t* cost, const int32_t* slot_sync,
                                   int n_channels, int lmax, int max_syncs, uint8_t* fich4, uint8_t* status, uint32_t* v_error,
                                   hipStream_t st);
hipError_t ddn_dev_ysf_plan(const int32_t* sync_pos, const int32_t* n_sync, const int32_t* counts, int n_channels, int max_syncs,
                            int lmax, const uint8_t* fich4, const uint8_t* fich_status, uint8_t* last2, uint8_t* info,
                            int32_t* slot_sync, hipStream_t st);
hipError_t ddn_dev_ysf_payload_costs(const uint8_t* rec, size_t stride, const int32_t* sync_pos, int n_channels, int max_syncs,
                                     int lmax, const uint8_t* info, const int32_t* slot_sync, uint16_t* cost200,
                                     uint16_t* cost360, uint8_t* ambe49, uint8_t* errs2, uint8_t* want200, uint8_t* want360,
                                     uint8_t* frames, uint8_t* n_frames, hipStream_t st);
hipError_t ddn_dev_ysf_dch_finish(const uint8_t* decA, const uint32_t* pcA, const uint8_t* decB, const uint32_t* pcB,
                                  const int32_t* slot_sync, const uint8_t* info, int n_channels, int lmax, int max_syncs,
                                  uint8_t* dch40, uint8_t* dch_status, uint32_t* dch_cost, hipStream_t st);
hipError_t ddn_dev_ysf_voice_file(const int32_t* n_sync, int n_channels, int max_syncs, const uint8_t* info, const uint8_t* ambe49,
                                  const uint8_t* errs2, const uint8_t* bits_fd, const int32_t* res_fd, const uint8_t* n_frames,
                                  int mode, int vf, uint8_t* bits, int32_t* res, uint8_t* skip, int32_t* v_n, int32_t* v_slot,
                                  hipStream_t st);
hipError_t ddn_dev_dpmr_voice_file(const int32_t* n_sync, int n_channels, int max_syncs, const uint8_t* fr_slot,
                                   const uint8_t* voiced2, const uint8_t* muted2, int vf, uint8_t* fr, int32_t* v_n, int32_t* v_slot,
                                   uint8_t* v_half, uint8_t* v_muted, uint8_t* v_skip, hipStream_t st);
hipError_t ddn_dev_ysf_pack96(const uint8_t* frames184, size_t n, uint8_t* frames96, hipStream_t st);
hipError_t ddn_dev_u8_shr1(const uint8_t* in, size_t n, uint8_t* out, hipStream_t st);
hipError_t ddn_dev_tsbk_select(const uint8_t* cand, const int32_t* counts, size_t n, uint8_t* out12, uint8_t* crc_ok, uint8_t* sel,
                               hipStream_t st);
#ifdef __cplusplus
}
#endif
#if defined(__HIPCC__)
/* f(item) for every item of the launch: all n_items, or the selected slots' items, grid-strided */
template <typename F>
__device__ __forceinline__ void
ddn_sel_for_each(const DdnSel& sel, long n_items, F&& f) {
    const long stride = (long)gridDim.x * (long)blockDim.x;
    long t = (long)blockIdx.x * (long)blockDim.x + (long)threadIdx.x;
    if (!sel.list) {
        for (; t < n_items; t += stride) {
            f(t);
        }
        return;
    }
    const long total = (long)(*sel.count) * (long)sel.per_slot;
    for (; t < total; t += stride) {
        const long e = t / sel.per_slot;
        f((long)sel.list[e] * (long)sel.per_slot + (t - e * (long)sel.per_slot));
    }
}
#endif

#endif
