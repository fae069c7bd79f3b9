/* ddn_fsk4.h - C-ABI of the batched fixed-protocol receive loop for DMR and NXDN48 (BASELINE configs[3]);
 * P25 Phase 1 has its own entry points in ddn_hip.h (ddn_p25_rx_*).  Device pointers + stream, like the rest of the library.
 *
 * Replaces, per channel and per call, the loop a dsd-neo decoder thread runs between rtl_stream_read() and the protocol
 * handler for one enabled protocol: getFrameSync() (src/dsp/dsd_frame_sync.c:3098-3148; DMR matchers :1102-1314 with
 * dmr_resample_on_sync() src/dsp/dmr_sync.c:63-131; NXDN matcher :1507-1556) around getSymbol()
 * (src/dsp/dsd_symbol.c:1854-1880) and get_dibit_and_analog_signal() (src/core/frames/dsd_dibit.c:1045-1076).
 * What is fixed per batch instead of decided at run time: one protocol, the modulation lock (-mc: rf_mod 0, -mg: rf_mod 2),
 * signal polarity (inverted = the reference's -xr for DMR), and how many symbols the handler of a sync class consumes
 * (lock_symbols[]: DMR data 120 = 54 live + 66 skipped, src/protocol/dmr/dmr_data.c:213-302; DMR voice = 54 + 288 per
 * superframe pair the host expects, src/protocol/dmr/dmr_bs.c:840-948; NXDN 182).
 */
#ifndef DDN_FSK4_H
#define DDN_FSK4_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { DDN_FSK4_DMR = 1, DDN_FSK4_NXDN48 = 2, DDN_FSK4_NXDN96 = 3, DDN_FSK4_M17 = 4, DDN_FSK4_YSF = 5, DDN_FSK4_DPMR = 6, DDN_FSK4_DSTAR = 7,
       DDN_FSK4_EDACS = 8 };
/* EDACS control channel (-fh, -fH, -fe, -fE; decode_mode_apply_edacs_pv(), src/runtime/decode_mode.c:431-456): two levels at 9600
 * symbols/s on the 9600_2 hunt profile - 5 samples per symbol at 48 ksps (out_rate_hz must be 9600 x 5..10), level ring 24 - with no
 * matched filter (use_matched_filter is ignored), rf_mod 2 (what -fh sets) or 0, inverted refused (both polarities are hunted).
 * The two 48-symbol words are compared exactly (frame_sync_try_provoice(), src/dsp/dsd_frame_sync.c:1421-1450;
 * include/dsd-neo/core/sync_patterns.h:107-108) and accepted with the basic lock and a 48-symbol outer-only warm start
 * (frame_sync_accept_edacs(), :1399-1409).  Sync pattern index: 0 = EDACS_SYNC, accepted as DSD_SYNC_EDACS_NEG (negative polarity,
 * flags bit 4), 1 = INV_EDACS_SYNC, accepted as DSD_SYNC_EDACS_POS - the reference's own mapping.  lock_symbols[0] = 240 = the bits
 * edacs() reads behind a sync (edacs_collect_bits(), src/protocol/edacs/edacs-fme.c:1966-1970); no handler family.  Thresholds stay
 * static inside the frame (use_symbol(), dsd_dibit.c:261-275): the bit of a symbol is (symbol > center ? 0 : 1) after pattern 1 (POS)
 * and (symbol > center ? 1 : 0) after pattern 0 (NEG) (store_two_level_dibit(), dsd_dibit.c:938-948,1024-1029).
 * Deviations: the ProVoice words the same hunt compares (32 symbols, and the conventional short words) are not hunted - ProVoice voice
 * is IMBE 7100x4400, which include/ddn_mbe.h refuses; a ProVoice word is a 2^-32 event per position on a control channel.  The dotting
 * sequences do nothing here (frame_sync_handle_edacs_dotting() acts only while a trunk tune is active, :1411-1419). */
#define DDN_EDACS_FRAME_SYMBOLS 240
#define DDN_EDACS_TYPE_POS 38 /* DSD_SYNC_EDACS_POS + 1 (this project's type ids) */
#define DDN_EDACS_TYPE_NEG 39
/* D-STAR (-fd): the first two-level protocol.  4800 symbols/s on the 4800_2 hunt profile (level ring 24), no matched filter
 * (use_matched_filter is ignored, as for M17), rf_mod 2 (decode_mode_apply_dstar()) or 0, inverted refused.  The four 24-symbol words
 * are compared exactly (frame_sync_try_dstar(), src/dsp/dsd_frame_sync.c:1452-1503) with a 24-symbol outer-only warm start.
 * Sync pattern index: 0 +voice (DSTAR_SYNC), 1 -voice, 2 +header (DSTAR_HD), 3 -header; odd rows are negative polarity (flags bit 4).
 * Sync class: voice = DDN_FSK4_CLASS_VOICE, lock_symbols[1] = 1992 = 21 x 72 voice + 20 x 24 slow-data symbols (processDSTAR());
 * header = DDN_FSK4_CLASS_DATA, lock_symbols[0] = 2652 = the 660 header symbols + 1992 (processDSTAR_HD()).  No handler family.
 * Thresholds stay static inside a frame under both rf_mod values (use_symbol(), dsd_dibit.c:264-275), so the records' symbols and the
 * thresholds the sync left (ddn_fsk4_rx_set_sync_thresholds) are all the frame decoders need: the two-level bit of a symbol is
 * (symbol > center ? 0 : 1) after a positive word and its complement after a negative one (dsd_dibit.c:935-946,1019-1029).  The
 * records' four-level dibits are those of the four-level slicer and are not what the reference's two-level digitize() stores. */
#define DDN_DSTAR_VOICE_SYMBOLS 1992
#define DDN_DSTAR_HEADER_SYMBOLS 2652
#define DDN_DSTAR_HEADER_CODED 660
/* dPMR (-fm): NXDN48's rate and hunt profile (2400 symbols/s, level ring 12), frame sync 2 compared exactly over 12 symbols in one
 * polarity - the plain word, or with inverted = 1 (-xd) the inverted one (frame_sync_try_dpmr(), src/dsp/dsd_frame_sync.c:832-862;
 * pattern index 0) -, 12-symbol warm start, dpmr_filter (RRC alpha 0.2, 135 taps at 20 samples per symbol, measured:
 * tools/gen_tables_dpmr.py), lock_symbols[0] = 372 = the dibits processdPMRvoice() reads (CCH, 4 x 36 AMBE, colour code, CCH,
 * 4 x 36 AMBE); no handler family.  Records hold the dibits as sliced: the -xd XOR with 2 belongs to the frame decoder. */
/* YSF (-fy): the 20-symbol FUSION_SYNC compared exactly in both polarities (frame_sync_try_ysf(), src/dsp/dsd_frame_sync.c:770-797;
 * pattern index 0 = +YSF, 1 = -YSF), 20-symbol warm start, the DMR matched filter, lock_symbols[0] = 460 = the 100 FICH + 360 payload
 * dibits processYSF() reads (every frame type but FI = 3 with DT != 1, which reads the FICH alone); no handler family. */
/* NXDN96: NXDN's rules at 4800 symbols/s (level ring 24, the DMR matched filter: src/dsp/dsd_frame_sync.c:1525-1556, dsd_symbol.c:323-335).
 * M17 (-fz): C4FM lock at 4800 symbols/s, no matched filter (use_matched_filter is ignored), frame_sync_try_m17()'s matcher
 * (src/dsp/dsd_frame_sync.c:865-1100: eight-symbol words with one error allowed, each accepted only after the sync type that may precede
 * it, polarity learnt from the preamble and cleared by EOT / carrier loss), fixed counts behind a sync (dispatch_m17.c:25-68):
 * lock_symbols[0] = 184 for every frame type and the EOT marker, lock_symbols[1] = 8 for the preamble; no handler family.
 * Sync pattern index: 0 / 1 preamble + / -, 2 / 3 EOT, 4 / 5 LSF, 6 / 7 BERT, 8 / 9 stream, 10 / 11 packet. */
enum { DDN_FSK4_CLASS_DATA = 0, DDN_FSK4_CLASS_VOICE = 1, DDN_FSK4_CLASS_RC = 2 }; /* index into lock_symbols[] */
/* sync pattern index reported in flags bits 3..6 / d_sync_pat.  DMR: 0 BS data word, 1 BS voice word, 2 MS data, 3 MS voice,
 * 4 / 5 direct-mode TS1 / TS2 data, 6 / 7 direct-mode TS1 / TS2 voice (with inverted = 1 the data words mark voice bursts and
 * vice versa, as with -xr), 8 the MS reverse-channel word (DMR_MS_RC_SYNC; with inverted = 1 its complement DMR_MS_RC_SYNC_INV,
 * which is never claimed at normal polarity - src/dsp/dsd_frame_sync.c:1318-1334): lock class 2, default 12 symbols (dmr_rc.c:39-44
 * reads 48 dibits, 36 of them already behind the sync).  The RC PDU is not decoded: the DMR burst consumers skip pattern 8.
 * NXDN48: 0..4 FSW variants positive, 5..9 inverted. */
#define DDN_FSK4_DMR_RC_PAT 8
#define DDN_FSK4_PRE 90 /* payload dibits handed over with every accepted sync */

typedef struct ddn_fsk4_rx_config {
    int n_channels;
    int out_rate_hz;        /* discriminator sample rate (48000) */
    int protocol;           /* DDN_FSK4_* */
    int rf_mod;             /* 0 = C4FM window / slip / clip rules (-mc), 2 = GFSK rules (-mg; what an unlocked dsd-neo
                               switches to on a DMR sync, dsd_frame_sync.c:595-600) */
    int inverted;           /* DMR: opts->inverted_dmr; dPMR: opts->inverted_dpmr (which FS2 word is hunted); others 0 (D-STAR
                               hunts both polarities) */
    int use_matched_filter; /* opts->use_cosine_filter (default 1 in the reference) */
    int lock_symbols[4];    /* per sync class; all zero = the defaults above (DMR voice default 54 + 6 * 288, DMR RC 12) */
} ddn_fsk4_rx_config;
typedef struct ddn_fsk4_rx ddn_fsk4_rx;

int ddn_fsk4_rx_create(const ddn_fsk4_rx_config* cfg, ddn_fsk4_rx** out);
void ddn_fsk4_rx_destroy(ddn_fsk4_rx* b);
/* a fresh stream for every channel (waits for the device first).  Configuration made through setters before the reset survives
 * it; state does not: ddn_fsk4_rx_set_lock_symbols, the handlers, channels per wave and the armed event buffers stay; timing,
 * slicer words, histories and the handlers' words (DMR colour code 16, confidence cleared) start afresh. */
int ddn_fsk4_rx_reset(ddn_fsk4_rx* b);
/* enable != 0: the reference's own handlers decide how long a frame is read in frame (plain -fs / -fi, inverted = 0), inside the
 * loop - lock_symbols[] then only serves the DMR MS / direct-mode and RC words, which need no handler: dmrMSData() and dmrMS() read
 * fixed counts (DDN_DMR_MS_LOCK_DATA / _VOICE below) and the stage behind the loop decodes them ("DMR MS / direct mode"):
 *   DMR BS data word   dmr_data_sync() (src/protocol/dmr/dmr_data.c:117-343): TACT Hamming(7,4) on the cached CACH (fails: no live
 *                      dibit), 5 live dibits, slot type Golay(20,8) (fails: stop) + colour-code gate, 49 more; then skipDibit(66)
 *   DMR BS voice word  dmrBSBootstrap() + dmrBS() (src/protocol/dmr/dmr_bs.c:697-948): 54 live dibits, then 144 per burst with the
 *                      TACT / repeated-carrier / sync-word / EMB QR(16,7,6) / colour-code-gate decisions
 *                      (src/protocol/dmr/dmr_confidence.c) - this is the path that prints the reference's "Color Code=02" on its
 *                      dmr_voice / dmr_t3_cc captures (tests/CMakeLists.txt:8925-8930)
 *   NXDN               nxdn_frame() (src/protocol/nxdn/nxdn_frame.c:181-233,592-640): 8 LICH dibits, parity + profile; rejected ->
 *                      the handler returns and lastsynctype is cleared
 * ddn_fsk4_rx_set_events: device buffers for the handlers' decisions of the next runs, d_events i32 [B][max_events][4] =
 * {output index of the deciding symbol, kind, a, b | c << 16}, d_n_events i32 [B]:
 *   kind 4 NXDN LICH        a = accepted, b = LICH (7 bits), c = parity ok
 *   kind 5 DMR data burst   a = slot type ok, b = colour code (-1 Golay failed, -2 TACT failed), c = data type | reject << 8 | pending << 9
 *   kind 6 "Color Code="    a = the value the reference prints (16 = XX), b = VC (0: data burst), c = slot
 *   kind 7 DMR voice burst  a = slot, b = EMB colour code (25: none), c = voice sync word | action << 4 (1 on, 2 end) | the VC the
 *                           burst's sync segment was read under << 8 (2..6: filed as that burst's embedded signalling)
 *   kind 8 DMR voice end    a = 1 bootstrap / 0 loop, b = TACT ok, c = EMB / sync ok */
int ddn_fsk4_rx_set_handlers(ddn_fsk4_rx* b, int enable);
int ddn_fsk4_rx_set_events(ddn_fsk4_rx* b, int32_t* d_events, int32_t* d_n_events, size_t max_events);
/* host convenience: event buffers owned by the batch object (arm once), copied to host arrays [B][max_events][4] / [B] after a run */
int ddn_fsk4_rx_events_host_arm(ddn_fsk4_rx* b, size_t max_events);
int ddn_fsk4_rx_events_host_read(ddn_fsk4_rx* b, int32_t* events, int32_t* n_events);
size_t ddn_fsk4_rx_max_symbols(const ddn_fsk4_rx* b, size_t n);
size_t ddn_fsk4_rx_max_syncs(const ddn_fsk4_rx* b, size_t n);
/* per-channel handler lengths, host array int32 [n_channels][4] */
int ddn_fsk4_rx_set_lock_symbols(ddn_fsk4_rx* b, const int32_t* lock4);
/* d_disc f32 [B][n] -> d_records10 u8 [B][max_symbols][10] (the reference's symbol-capture record), d_flags u8 [B][max_symbols]
 * (1 in frame, 2 sync accepted on this symbol, 4 negative polarity, pattern index << 3 on the accepting symbol), d_payload2
 * u8 [B][max_symbols][2] = {payload dibit, reliability} (dmr_payload_buf / dmr_soft_buf contents), d_counts i32 [B];
 * per accepted sync k < d_n_sync[c] (capacity max_syncs per channel): d_sync_pos i32 = index of the sync's last symbol,
 * d_sync_pat u8, d_pre / d_pre_rel u8 [DDN_FSK4_PRE] = the payload dibits / reliabilities ending at that symbol, after DMR's
 * re-digitisation.  State carries across calls. */
int ddn_fsk4_rx_run(ddn_fsk4_rx* b, const float* d_disc, size_t n, uint8_t* d_records10, uint8_t* d_flags,
                    uint8_t* d_payload2, int32_t* d_counts, size_t max_symbols, int32_t* d_sync_pos, uint8_t* d_sync_pat,
                    uint8_t* d_pre, uint8_t* d_pre_rel, int32_t* d_n_sync, size_t max_syncs, void* hip_stream);
int ddn_fsk4_rx_run_host(ddn_fsk4_rx* b, const float* disc, size_t n, uint8_t* records10, uint8_t* flags, uint8_t* payload2,
                         int32_t* counts, size_t max_symbols, int32_t* sync_pos, uint8_t* sync_pat, uint8_t* pre,
                         uint8_t* pre_rel, int32_t* n_sync, size_t max_syncs);
int ddn_fsk4_rx_get_thresholds(ddn_fsk4_rx* b, int channel, float out7[7]); /* center umid lmid max min maxref minref */
/* kernel shape: channels per recurrence wavefront (1, 2, 4 ... 32; results do not depend on it).  The default is the fewest that
 * keeps every workgroup resident for this batch alone; a host that runs other loops beside this one on the same GPU (the mixed
 * chain does) picks it for the whole device's channel count. */
int ddn_fsk4_rx_set_channels_per_wave(ddn_fsk4_rx* b, int channels_per_wave);
/* A/B selectors of the loop kernel's schedule (which of two equivalent code paths a launch takes; the results never depend on them):
 * 65536 = the bulk hunting passes one owner lane at a time.  For the parity tests and timing tools; 0 = the product's choice. */
int ddn_fsk4_rx_set_debug_flags(ddn_fsk4_rx* b, int flags);
/* optional output beside d_sync_pos / d_sync_pat: the slicer thresholds {center, umid, lmid, max, min} as every accepted sync leaves them
 * (after the warm start), [B][max_syncs][5] floats in device memory, NULL = off.  Thresholds are static inside a DMR / NXDN / M17 frame,
 * so these are what a soft-symbol frame decoder reads (M17 LSF: soft_symbol_to_viterbi_cost(), src/core/frames/dsd_dibit.c:1189-1242) */
int ddn_fsk4_rx_set_sync_thresholds(ddn_fsk4_rx* b, float* d_thr5);

/* ---- M17 link setup frames behind the loop (the consumer of the libM17-style K = 5 decoder, ddn_fec_viterbi_k5_*) ---------------------
 * == processM17LSF() (src/protocol/m17/m17.c:1395-1408) for every accepted LSF sync (pattern 4 / 5) of a DDN_FSK4_M17 loop call whose 184
 * payload symbols lie inside the call's records: soft symbols -> soft_symbol_to_viterbi_cost() per bit against the thresholds the sync left
 * (d_sync_thr5: ddn_fsk4_rx_set_sync_thresholds; src/core/frames/dsd_dibit.c:1189-1242 - its expf evaluated as the host's libm does) ->
 * de-randomise -> de-interleave -> de-puncture P1 -> viterbi_decode(488 costs) -> the 30 LSF bytes (DST 48, SRC 48, TYPE 16, META 112,
 * CRC 16: m17_parse_lsf(), src/protocol/m17/m17_parse.c:369-420) + CRC16 (m17_crc16, m17_algorithms.c:19-35).
 * d_records10 [B][stride_symbols][10], d_counts [B] = records of the call per channel, d_sync_pos / d_sync_pat [B][max_syncs], d_n_sync [B]:
 * the loop's outputs.  Out, per sync slot [B][max_syncs]: d_lsf30 [..][30], d_status (0 = not an LSF sync or its frame is not complete in
 * this call, 1 = decoded with a bad CRC, 2 = CRC good), d_path_cost (optional) = the decoder's path cost. */
int ddn_m17_lsf_decode_batch(const uint8_t* d_records10, size_t stride_symbols, const int32_t* d_counts, const int32_t* d_sync_pos,
                             const uint8_t* d_sync_pat, const int32_t* d_n_sync, const float* d_sync_thr5, int n_channels, size_t max_syncs,
                             uint8_t* d_lsf30, uint8_t* d_status, uint32_t* d_path_cost, void* hip_stream);
/* == processM17STR() (src/protocol/m17/m17.c:1122-1176) for every accepted stream sync (pattern 8 / 9) whose frame is complete: hard dibits ->
 * de-randomise -> de-interleave -> LICH = four Golay(24,12) words (m17_lich_decode_bits) -> 48 content bits (d_lich6, packed) with the
 * 3-bit chunk counter (d_lich_cnt); when all four decode and the counter is < 6: P2 de-puncture -> CNXDNConvolution (148 steps) ->
 * d_fn_payload18 = frame number (2 bytes, big endian) + the 16 payload bytes.  d_status: 0 = not a stream sync / frame not complete,
 * 1 = LICH failed (no payload, as the reference), 2 = decoded. */
int ddn_m17_str_decode_batch(const uint8_t* d_records10, size_t stride_symbols, const int32_t* d_counts, const int32_t* d_sync_pos,
                             const uint8_t* d_sync_pat, const int32_t* d_n_sync, int n_channels, size_t max_syncs, uint8_t* d_lich6,
                             uint8_t* d_lich_cnt, uint8_t* d_fn_payload18, uint8_t* d_status, void* hip_stream);
/* ---- YSF frame information channel behind the loop (the K = 5 decoder's second consumer) --------------------------------------------
 * == ysf_conv_fich() (src/protocol/ysf/ysf.c:357-424) for every accepted sync of a DDN_FSK4_YSF loop call whose 100 FICH dibits lie inside
 * the records: dibit de-interleave (20 x 5) -> dsd_ysf_soft_viterbi_decode (hard costs through viterbi_decode_punctured, ysf_frame.c:82-126)
 * -> four Golay(24,12) words -> CRC16.  d_fich4 [B][max_syncs][4] = the 32 information bits packed (FI 2, CS 2, CM 2, BN 2, BT 2, FN 3,
 * FT 3, reserved 2, MR 3, VoIP path 1, DT 2, SQL type 1, SQL code 7: ysf_parse_fich() :534-546); d_status 0 = no complete FICH behind this
 * sync in this call, 1 = good, 2 = a Golay word failed (err -1), 3 = CRC failed (err -2); d_v_error (optional) the decoder's path cost. */
int ddn_ysf_fich_decode_batch(const uint8_t* d_records10, size_t stride_symbols, const int32_t* d_counts, const int32_t* d_sync_pos,
                              const int32_t* d_n_sync, int n_channels, size_t max_syncs, uint8_t* d_fich4, uint8_t* d_status,
                              uint32_t* d_v_error, void* hip_stream);

/* The payload behind the FICH == ysf_dispatch_payload() (src/protocol/ysf/ysf.c:908-922) for every frame of the call (a sync of the
 * decode list with d_fich_status != 0), in stream order per channel:
 *   the type a frame is read as: FI / DT of its FICH, or - when the FICH failed - of the last good frame of the channel (ysf_parse_fich's
 *     statics, :553-555): d_last_dt_fi u8 [n_channels][2] {DT, FI}, zero before the first call, carried by the caller from call to call;
 *   d_info2 [S][2]: [0] = what was decoded, a bit mask: 1 V/D mode 1 (FI 1, DT 0), 2 V/D mode 2 (FI 1, DT 2), 4 full-rate voice
 *     (FI 1, DT 3), 8 full-rate data (DT 1 or FI 0 / 2) - 0 when the frame's 360 payload dibits are not inside the records;
 *     [1] = FI | DT << 2 | 16 (FICH failed: type taken over) | 32 (a frame) | 64 (more frames than a row holds 480 symbols apart:
 *     left undecoded) | 128 (full-rate voice in the CSD3 layout);
 *   V/D mode 2: the five voice sub-frames, ysf_read_type2_vech_bits + ysf_build_type2_ambe (:687-722): d_ambe49x5 [S][5][49] = ambe_d
 *     (what mbe_processAmbe2450Dataf takes), d_errs2x5 [S][5] = errs2; the data channel, ysf_conv_dch2 (:245-300): d_dch40 [S][2][20]
 *     block 0 bytes 0 .. 9, d_dch_status2 [S][2] (0 none, 1 CRC16 good, 3 CRC16 failed), d_dch_cost2 [S][2] = the decoder's path cost;
 *   V/D mode 1: the data channel, ysf_conv_dch (:302-355), block 0 bytes 0 .. 19; its voice blocks as ysf_ehr() (:425-476) hands them
 *     to processMbeFrame: d_frames184x5 [S][5][184], the first four frames, ambe_fr[4][24] as row * 24 + column (d_n_frames [S] = 4);
 *   full-rate voice (FI 1, DT 3): five IMBE 7200x4400 frames as dsd_ysf_unpack_full_rate_imbe (ysf_frame.c:138-163) builds them,
 *     imbe_fr[8][23] as row * 23 + column (d_n_frames = 5); with FT = 1 and FN = 0 (CSD3, d_info2[1] bit 128) two frames behind a data
 *     block that goes through ysf_conv_dch into block 0 (ysf_handle_full_rate_voice :824-842);
 *   full-rate data (a frame that is nothing else): both blocks, in turn (ysf_handle_full_rate_data :844-864).
 * S = n_channels x max_syncs, slots as d_sync_pos.  The frames of V/D mode 1 and of full-rate voice are handed back as frames here; the
 * chain object (include/ddn_chain.h, vocoder = 1) takes them through ddn_mbe_frame_decode_batch and ddn_mbe_synth_batch. */
int ddn_ysf_payload_decode_batch(const uint8_t* d_records10, size_t stride_symbols, const int32_t* d_counts, const int32_t* d_sync_pos,
                                 const int32_t* d_n_sync, int n_channels, size_t max_syncs, const uint8_t* d_fich4,
                                 const uint8_t* d_fich_status, uint8_t* d_last_dt_fi, uint8_t* d_info2, uint8_t* d_dch40,
                                 uint8_t* d_dch_status2, uint32_t* d_dch_cost2, uint8_t* d_ambe49x5, uint8_t* d_errs2x5,
                                 uint8_t* d_frames184x5, uint8_t* d_n_frames, void* hip_stream);
/* The LSF reassembled from the LICH chunks, in the order of the syncs of a call: a decoded LSF frame seeds the buffer (m17_decode_lsf_soft_
 * bits), an EOT marker clears it (dispatch_m17.c:39), chunk c fills bytes 5 c .. 5 c + 4, chunk 5 closes it: d_lich_lsf30 [B][max_syncs][30]
 * + d_lich_status (0 none here, 1 CRC bad, 2 CRC good: M17finalizeLICH), then the buffer is cleared.  d_assembly32 [B][32] is the carried
 * buffer (zero it before a stream's first call).  d_lsf30 / d_lsf_status = ddn_m17_lsf_decode_batch's outputs, or both NULL. */
int ddn_m17_lich_assemble_batch(const uint8_t* d_sync_pat, const int32_t* d_n_sync, int n_channels, size_t max_syncs, const uint8_t* d_lsf30,
                                const uint8_t* d_lsf_status, const uint8_t* d_lich6, const uint8_t* d_lich_cnt, const uint8_t* d_str_status,
                                uint8_t* d_assembly32, uint8_t* d_lich_lsf30, uint8_t* d_lich_status, void* hip_stream);
/* ---- M17 packet and BERT frames behind the loop ------------------------------------------------------------------------------------------
 * == processM17PKT() up to its checks (src/protocol/m17/m17.c:3076-3098) for every accepted packet sync (pattern 10 / 11) whose 184 payload
 * symbols lie inside the call's records: soft symbols -> soft_symbol_to_viterbi_cost() against the thresholds the sync left (d_sync_thr5,
 * as ddn_m17_lsf_decode_batch) -> de-randomise -> de-interleave -> de-puncture P3 to 420 costs, 0x7FFF where a bit was cut (:2991-3001) ->
 * viterbi_decode -> its bytes 1 .. 26: d_pkt26 [B][max_syncs][26] = the 25 chunk bytes + the metadata byte.  d_status: 0 = not a packet
 * sync, or the frame is not complete in this call; 1 = decoded.  d_path_cost (optional) = the decoder's path cost. */
int ddn_m17_pkt_decode_batch(const uint8_t* d_records10, size_t stride_symbols, const int32_t* d_counts, const int32_t* d_sync_pos,
                             const uint8_t* d_sync_pat, const int32_t* d_n_sync, const float* d_sync_thr5, int n_channels, size_t max_syncs,
                             uint8_t* d_pkt26, uint8_t* d_status, uint32_t* d_path_cost, void* hip_stream);
/* == processM17BRT() up to the receiver (:1325-1336; m17_decode_bert_payload_bits :1247-1276) for every accepted BERT sync (pattern 6 / 7)
 * with a complete frame: hard dibits -> de-randomise -> de-interleave -> de-puncture P2 to 402 symbol values bit << 1, the cut bit reads 0
 * (:1232-1245) -> CNXDNConvolution over 201 steps, 197 bits chained back: d_bits25 [B][max_syncs][25], most significant bit first, the last
 * three bits zero.  d_status as above. */
int ddn_m17_brt_decode_batch(const uint8_t* d_records10, size_t stride_symbols, const int32_t* d_counts, const int32_t* d_sync_pos,
                             const uint8_t* d_sync_pat, const int32_t* d_n_sync, int n_channels, size_t max_syncs, uint8_t* d_bits25,
                             uint8_t* d_status, void* hip_stream);
/* What the reference does with those frames, in the order of the syncs of a call, on a state carried per channel from call to call
 * (d_state: n_channels x ddn_m17_data_state_bytes() bytes of device memory, all zeros before a stream's first call):
 *   a packet frame goes through processM17PKT()'s checks in their order (:3100-3150): the metadata byte (m17_packet_parse_metadata_byte,
 *     m17_algorithms.c:367-386), the counter against the carried count, the EOF byte count (m17_packet_app_bytes_from_eof :336-353), the
 *     25-byte copy at 25 x count, on EOF m17_pkt_finalize_eot (:3052-3074: CRC16 over the application bytes against the two behind them;
 *     the packet is reported whatever the verdict, buffer and count cleared), else the overflow check and the increment; every rejection
 *     clears buffer and count;
 *   a BERT frame's 197 bits go through m17_prbs9_rx_push_bit (m17_algorithms.c:125-167; lock after 18 bits, 128-bit windows, resync above
 *     18 errors in one);
 *   an EOT marker (pattern 2 / 3) zeroes the count - not the buffer - and restarts the BERT receiver (dispatch_m17.c:39-50);
 *   carrier loss (no_carrier_reset_m17_and_sample_buffers, src/engine/engine.c:2169-2184: buffer, count and BERT receiver) is applied at
 *     the sync that follows it: the loop declares it at the 1800th hunted symbol without a sync, so at a sync whose position lies more
 *     than 1800 symbols behind the last symbol of the previous lock (8 symbols behind a preamble sync, 184 behind any other).
 * d_advance [n_channels] (NULL = zeros): by how many records the next call's rows begin behind this call's (a chain's new records of the
 * call; single calls on fresh rows pass NULL) - it carries the end of the last lock into the next call's positions.
 * d_pkt26 / d_pkt_frame_status, d_bits25 / d_brt_frame_status: the two calls above.  Out, per sync slot: d_pkt_status (0 none, 1 metadata
 * invalid, 2 counter mismatch, 3 EOF byte count invalid, 4 chunk filed, 5 filed, then frame count overflow, 6 final, CRC mismatch, 7 final,
 * CRC good), d_pkt_count = the count before a packet frame (0 elsewhere), d_brt_state [..][8] = {locked, lfsr, lock_count, window_bits,
 * window_errors, total_bits, total_errors, resyncs} after a BERT frame (the slots of other syncs are not written).  Out, per channel and call: d_n_packets [B] = packets completed (every one, also
 * those past max_packets, which are not stored - their slots still read 6 / 7), and for the first max_packets (1 .. 33) of them
 * d_packet [B][max_packets][832] = bytes [0, end) of the reference's buffer at finalisation (end = 25 x count + the EOF value), zeros
 * behind, d_packet_app_len, d_packet_crc_ok, d_packet_slot (the sync slot of the EOF frame). */
size_t ddn_m17_data_state_bytes(void);
int ddn_m17_data_assemble_batch(const uint8_t* d_sync_pat, const int32_t* d_sync_pos, const int32_t* d_n_sync, const int32_t* d_advance,
                                int n_channels, size_t max_syncs, const uint8_t* d_pkt26, const uint8_t* d_pkt_frame_status,
                                const uint8_t* d_bits25, const uint8_t* d_brt_frame_status, void* d_state, uint8_t* d_pkt_status,
                                uint8_t* d_pkt_count, int32_t* d_brt_state, uint8_t* d_packet, int32_t* d_packet_app_len,
                                uint8_t* d_packet_crc_ok, int32_t* d_packet_slot, int32_t* d_n_packets, int max_packets, void* hip_stream);
int ddn_fsk4_rx_set_timing(ddn_fsk4_rx* b, int enable);
int ddn_fsk4_rx_get_timing(ddn_fsk4_rx* b, float* ms2); /* {matched filter, receive loop} of the last run */

/* DMR burst fields from the per-sync hand-over + the live symbols after the sync (SURVEY 8f rank 3 seam: what
 * dmr_data_sync() / dmrBSBootstrap() assemble, src/protocol/dmr/dmr_data.c:117-262, dmr_bs.c:700-760).  For sync k of channel
 * c (slot c * max_syncs + k): d_slot_type u8 [20] bits (Golay(20,8) input order), d_info u8 [196] bits (BPTC input order,
 * first half from d_pre, second half live = the records' dibits, i.e. getDibitSoft()'s polarity-corrected return values),
 * d_cach u8 [24] bits de-interleaved (TACT first), d_valid = 1 when the 54 live dibits lie inside this call's records.
 * inverted != 0 applies the reference's dibit ^= 2 to the cached half (dmr_data.c:84-86). */
int ddn_dmr_burst_gather(const uint8_t* d_records10, const int32_t* d_counts, size_t max_symbols, const int32_t* d_sync_pos,
                         const uint8_t* d_pre, const int32_t* d_n_sync, int n_channels, size_t max_syncs, int inverted,
                         uint8_t* d_slot_type, uint8_t* d_info, uint8_t* d_cach, uint8_t* d_valid, void* hip_stream);

/* NXDN frame fields from the records after each accepted frame sync (what nxdn_frame() assembles before its decoders,
 * src/protocol/nxdn/nxdn_frame.c:181-199,311-331,596-621 + nxdn_descramble.c + nxdn_deperm.c:123-172): per sync slot
 * (c * max_syncs + k) d_lich u8 = the 7-bit LICH, bit 7 set when its parity checks; d_sacch_sym / _rel u8 [36][2] and
 * d_facch_sym / _rel u8 [2][96][2] = de-scrambled, de-interleaved, de-punctured symbol / reliability pairs in the layout
 * ddn_fec_nxdn_conv_batch takes (36 steps -> 32 bits, 96 steps -> 92 bits; pass d_rel = NULL there for the hard-decision
 * retry the reference falls back to when the soft decode fails its CRC, nxdn_deperm.c:1128-1135,1195-1200);
 * d_valid = 1 when the 182 dibits lie inside this call's records. */
int ddn_nxdn_frame_gather(const uint8_t* d_records10, const int32_t* d_counts, size_t max_symbols, const int32_t* d_sync_pos,
                          const int32_t* d_n_sync, int n_channels, size_t max_syncs, uint8_t* d_lich, uint8_t* d_sacch_sym,
                          uint8_t* d_sacch_rel, uint8_t* d_facch_sym, uint8_t* d_facch_rel, uint8_t* d_valid, void* hip_stream);
/* AMBE 3600x2450 voice frames ("AMBE interleave"): the 36-dibit interleave schedule the reference's DMR,
 * NXDN and YSF voice paths share (include/dsd-neo/core/ambe_interleave.h:25-38; users dmr_bs.c:137-160, dmr_ms.c:73-77,
 * nxdn_voice.c:57-74).  Outputs feed ddn_mbe_frame_decode_batch(DDN_MBE_AMBE_3600X2450, frames, reliabilities, ...):
 *   d_ambe_fr  u8 [..][4][24] one bit per byte (char ambe_fr[4][24]; the cells the schedule never writes are 0)
 *   d_ambe_rel u8 [..][4][24] per-bit reliability = its dibit's (dsd_vocoder_soft_bit.reliability), or NULL
 * ddn_ambe2450_deinterleave_batch: n frames of 36 dibits (+ optional reliabilities) that the caller has already cut out.
 * ddn_nxdn_voice_gather: for sync k of channel c (slot c * max_syncs + k, as ddn_nxdn_frame_gather) the four voice frames
 *   behind LICH + SACCH, de-scrambled (nxdn_frame.c:181-199, nxdn_voice.c:57-66): [slots][4][4][24]; d_valid (or NULL) = 1
 *   when the frame's 182 dibits lie inside this call's records.  Which of the four carry voice is the LICH's business.
 * ddn_dmr_voice_burst_gather: d_burst_start i32 [n_channels][max_bursts] = record index of a voice burst's first CACH dibit
 *   (< 0: unused slot) -> the burst's three voice frames [slots][3][4][24] (frame 2 straddles the 24 sync / EMB dibits),
 *   d_sync48 u8 [slots][48] sync / EMB bits, d_cach24 u8 [slots][24] de-interleaved CACH bits (TACT first) - either may be
 *   NULL; inverted != 0 applies the MS path's dibit ^= 2 (dmr_ms.c:55-64). */
int ddn_ambe2450_deinterleave_batch(const uint8_t* d_dibits36, const uint8_t* d_reliab36, size_t n, uint8_t* d_ambe_fr,
                                    uint8_t* d_ambe_rel, void* hip_stream);
int ddn_nxdn_voice_gather(const uint8_t* d_records10, const int32_t* d_counts, size_t max_symbols, const int32_t* d_sync_pos,
                          const int32_t* d_n_sync, int n_channels, size_t max_syncs, uint8_t* d_ambe_fr, uint8_t* d_ambe_rel,
                          uint8_t* d_valid, void* hip_stream);
int ddn_dmr_voice_burst_gather(const uint8_t* d_records10, const int32_t* d_counts, size_t max_symbols,
                               const int32_t* d_burst_start, int n_channels, size_t max_bursts, int inverted,
                               uint8_t* d_ambe_fr, uint8_t* d_ambe_rel, uint8_t* d_sync48, uint8_t* d_cach24, uint8_t* d_valid,
                               void* hip_stream);

/* ---- dPMR voice superframe behind the loop's FS2 syncs (DDN_FSK4_DPMR, -fm; ddn_dpmr.hip) -------------------------------------
 * ddn_dpmr_superframe_decode_batch == processdPMRvoice()'s control part (src/protocol/dpmr/dpmr_voice.c:397-425) for every accepted sync:
 * the 372 dibits behind it (record byte 0 & 3 from sync_pos + 1; inverted = 1 applies dpmr_read_dibit()'s ^ 2, :67-73), then per CCH
 * (dibit offsets 0 and 192; dpmr_voice.c:139-178): descramble x^9 + x^5 + 1 seeded 0x1FF (dpmr_data.c:80-117), 6 x 12 de-interleave
 * (:431-452), six Hamming(12,8) words (the generic entry's matrix and correction table), CRC7 over 41 bits against bits 41..47 (:455-474).
 * Per slot c * max_syncs + k (as d_sync_pos):
 *   d_cch_bits2x48 u8 [S][2][48]  decoded CCH bits         d_ham_ok2x6 u8 [S][2][6]  1 = Hamming word j corrected / clean
 *   d_crc_ok2      u8 [S][2]      1 = CRC7 good            d_fields2x8 i32 [S][2][8] {frame number, 12-bit ID half, communication
 *     mode, version, format, emergency, reserved, 18 bits of slow data} (dpmr_extract_superframe_part(), :180-195)
 *   d_id i32 [S]  24-bit ID (first CCH's half high)         d_color i32 [S] colour code: the 12 dibits at offset 180 | 0x555555
 *     looked up in the 64-entry table (tests/golden/dpmr_vectors.json -> ddn_tables_dpmr.h), -1 = no match
 *   d_valid u8 [S] 1 = all 372 dibits lie inside this call's records (d_counts); a slot that is not valid is written as zeros, colour -1.
 * ddn_dpmr_identity_batch == dpmr_update_superframe_part() (:197-274) over each channel's valid slots in sync order: kind (0 none,
 *   1 called: frame number 0 / 1 in CCH 0 / 1, 2 calling: 2 / 3) and strong (both CCHs pass CRC7 or their first two Hamming words); a
 *   strong called ID publishes TG, a strong calling ID Src.  d_state3 i32 [B][3] = {tg, src, next part} carried from call to call
 *   (initialise to {-1, -1, 0}); d_tg / d_src i32 [S] = raw 24-bit values as they stand after the slot's superframe, -1 = none
 *   (ddn_dpmr_air_interface_id turns them into the digits the reference prints).
 * ddn_dpmr_voice_gather == the eight TCH frames (dibit offsets 36, 72, 108, 144, 228, 264, 300, 336) through the AMBE 3600x2450
 *   schedule, hard bits as processMbeFrame(opts, state, NULL, ambe_fr[i], NULL) takes them: d_ambe_fr u8 [S][8][4][24]; per half
 *   (dpmr_play_voice_frames(), :354-395) d_voiced2 [S][2] = 1 where the half's communication mode is 0, 1 or 5 (its four frames go
 *   to the vocoder), d_muted2 [S][2] = 1 where its version is 3 (scrambled: synthesised, audio not permitted without a key).
 *   d_fields2x8 / d_valid = the superframe decode's. */
int ddn_dpmr_superframe_decode_batch(const uint8_t* d_records10, size_t stride_symbols, const int32_t* d_counts, const int32_t* d_sync_pos,
                                     const int32_t* d_n_sync, int n_channels, size_t max_syncs, int inverted, uint8_t* d_cch_bits2x48,
                                     uint8_t* d_ham_ok2x6, uint8_t* d_crc_ok2, int32_t* d_fields2x8, int32_t* d_id, int32_t* d_color,
                                     uint8_t* d_valid, void* hip_stream);
int ddn_dpmr_identity_batch(const int32_t* d_n_sync, int n_channels, size_t max_syncs, const uint8_t* d_valid, const int32_t* d_fields2x8,
                            const uint8_t* d_ham_ok2x6, const uint8_t* d_crc_ok2, const int32_t* d_id, int32_t* d_state3, uint8_t* d_kind,
                            uint8_t* d_strong, int32_t* d_tg, int32_t* d_src, void* hip_stream);
int ddn_dpmr_voice_gather(const uint8_t* d_records10, size_t stride_symbols, const int32_t* d_sync_pos, const int32_t* d_n_sync, int n_channels,
                          size_t max_syncs, int inverted, const int32_t* d_fields2x8, const uint8_t* d_valid, uint8_t* d_ambe_fr,
                          uint8_t* d_voiced2, uint8_t* d_muted2, void* hip_stream);
/* (host) dpmr_convert_air_interface_id() (dpmr_voice.c:477-546): the seven base-11 digits the reference prints for a raw 24-bit ID
 * ("1601621"), '*' for ten, NUL-terminated.  Like the reference, a first digit of 11 (IDs >= 11 x 1464100) is written as '0' + 11. */
void ddn_dpmr_air_interface_id(uint32_t id, char out[8]);

/* ---- D-STAR frames behind the loop's syncs (DDN_FSK4_DSTAR, -fd; ddn_dstar.hip) ------------------------------------------------
 * Inputs are the loop's outputs: d_records10 [B][stride_symbols][10], d_counts, d_sync_pos / d_sync_pat [B][max_syncs], d_n_sync and the
 * thresholds each sync left (d_sync_thr5, ddn_fsk4_rx_set_sync_thresholds).  One wavefront per slot c * max_syncs + k.
 * ddn_dstar_header_decode_batch == dstar_header_decode_soft() for every header sync (pattern 2 / 3) whose 660 symbols lie inside the
 *   records: gmsk_soft_symbol_to_viterbi_cost() per symbol against the sync's {center, max, min} (whatever the sync's polarity: a high
 *   symbol costs towards 1), PN descramble (x^7 + x^4 + 1 seeded 0x07), the 24-stride de-interleave, the 4-state soft Viterbi
 *   (K = 3, G = 7, 5) over 330 steps, 328 bits packed LSB first: d_hdr41 [S][41] (flags 0..2, RPT2 3..10, RPT1 11..18, DST 19..26,
 *   SRC 27..38, CRC 39..40), d_hdr_crc_ok [S] (dstar_crc16 over 39 bytes == bytes 39..40), d_valid [S].
 * ddn_dstar_voice_decode_batch == processDSTAR() for every sync whose 1992 voice symbols (for a header sync: 660 symbols later) lie inside
 *   the records: the two-level slice against the sync's center, the 21 voice frames as processMbeFrame receives them, d_ambe_fr
 *   [S][21][4][24] (one bit per byte, the 24 cells the schedule never writes are 0), and processDSTAR_SD() on the 480 slow-data bits
 *   except APRS: d_sd_bytes [S][60] (the packed bytes as the reference prints them), d_sd_kind [S] (0 unknown, 1 header format 0x55,
 *   2 text 0x40, 3 fixed form 0x35), d_sd_hdr41 [S][41] (the truncated-payload reload), d_sd_crc_ok [S] (its CRC in wire order),
 *   d_sd_text [S][60] (dstar_txt as the text handler leaves it - 0x20 fill, characters at their byte positions, byte 59 = 0 - for a text
 *   message or a fixed form that is not "$$CRC", zeros otherwise), d_valid [S].
 * The voice frames are AMBE 3600x2400 frames.  They are handed back, not synthesised: mbe_processAmbe3600x2400Framef stays refused
 * (include/ddn_mbe.h - the 2400 rate's layout and tables are not in the reference tree).  A slot that is not valid is written as zeros. */
int ddn_dstar_header_decode_batch(const uint8_t* d_records10, size_t stride_symbols, const int32_t* d_counts, const int32_t* d_sync_pos,
                                  const uint8_t* d_sync_pat, const int32_t* d_n_sync, const float* d_sync_thr5, int n_channels,
                                  size_t max_syncs, uint8_t* d_hdr41, uint8_t* d_hdr_crc_ok, uint8_t* d_valid, void* hip_stream);
int ddn_dstar_voice_decode_batch(const uint8_t* d_records10, size_t stride_symbols, const int32_t* d_counts, const int32_t* d_sync_pos,
                                 const uint8_t* d_sync_pat, const int32_t* d_n_sync, const float* d_sync_thr5, int n_channels,
                                 size_t max_syncs, uint8_t* d_ambe_fr, uint8_t* d_sd_bytes, uint8_t* d_sd_kind, uint8_t* d_sd_hdr41,
                                 uint8_t* d_sd_crc_ok, uint8_t* d_sd_text, uint8_t* d_valid, void* hip_stream);

/* ---- EDACS control-channel frames behind the loop's syncs (DDN_FSK4_EDACS; ddn_edacs.hip) ------------------------------------------
 * Inputs are the loop's outputs: d_records10 [B][stride_symbols][10], d_counts, d_sync_pos / d_sync_pat [B][max_syncs], d_n_sync and the
 * thresholds each sync left (d_sync_thr5, ddn_fsk4_rx_set_sync_thresholds).  One lane per slot s = c * max_syncs + k.  == edacs()
 * (src/protocol/edacs/edacs-fme.c:2012-2066) for every sync whose 240 symbols lie inside the records:
 *   the two-level bit of each symbol against the sync's center (pattern 1 = POS: symbol > center -> 0; pattern 0 = NEG: -> 1), six 40-bit
 *   words MSB first (edacs_build_raw_frames(), :1973-1990) -> d_raw40 [S][6]; the bitwise majority of words 0, ~1, 2 and of 3, ~4, 5
 *   (edacs_vote_frames(), :157-175) -> d_vote40 [S][2]; each voted word's 28-bit message (bits 39..12) re-encoded with the BCH(40,28)
 *   code, generator x^12 + x^10 + x^8 + x^5 + x^4 + x^3 + 1 (0x1539: edacs_bch(), edacs-bch3.c), compared with the voted word ->
 *   d_bch_ok [S][2], d_frame_ok [S] (both equal; otherwise the reference prints "BCH FAIL"); the two messages with esk_mask << 20 XORed
 *   in (edacs_process_valid_frame(), :1993-2010) -> d_msg28 [S][2] (also on a failed frame, where the reference stops before the XOR);
 *   d_kind [S]: 0 none (frame not good), 1 a standard-mode message (ea_mode 0), 2 an EA message (ea_mode 1), + 2 when it is a site ID:
 *   d_types [S][3] = {MT-A msg_1[27:25], MT-B [24:22], MT-D [21:17]} (:1915-1940) or {MT1 [27:23], MT2 [22:19], 0} (:1265-1284);
 *   the standard site ID (MT-A = 7, MT-B = 7, MT-D 0x08..0x0B): d_site6 [S][6] = {site_id msg_1 & 0x1F, priority (>> 9) & 7, cc_lcn
 *   (>> 12) & 0x1F, SCAT bit 7, failsoft bit 6, auxiliary bit 5} (:1748-1781) - the reference prints "Site ID [%02X][%03d]" of site_id;
 *   the EA site ID (MT1 = 0x1F, MT2 = 0xA): d_site6 = {((msg_1 & 0x7000) >> 7) | (msg_1 & 0x1F), area (msg_1 & 0xFE0) >> 5, 0, 0, 0, 0}
 *   (:944-955).  d_valid [S] = 1 when the 240 symbols were inside the records; a slot that is not valid is written as zeros.
 * ea_mode 0 / 1, esk_mask 0 or 0xA0: -fh = (0, 0), -fH = (0, 0xA0), -fe = (1, 0), -fE = (1, 0xA0).  Everything else edacs() does - the
 * trunking layer (grants, LCN frequencies, tuning, AFS labels), analog voice and ProVoice - stays out. */
int ddn_edacs_frame_decode_batch(const uint8_t* d_records10, size_t stride_symbols, const int32_t* d_counts, const int32_t* d_sync_pos,
                                 const uint8_t* d_sync_pat, const int32_t* d_n_sync, const float* d_sync_thr5, int n_channels,
                                 size_t max_syncs, int ea_mode, int esk_mask, uint64_t* d_raw40, uint64_t* d_vote40, uint8_t* d_bch_ok,
                                 uint8_t* d_frame_ok, uint32_t* d_msg28, uint8_t* d_kind, uint8_t* d_types, int32_t* d_site6,
                                 uint8_t* d_valid, void* hip_stream);

/* CRC of decoded NXDN fields, rows = ddn_fec_nxdn_conv_batch output: kind 0 = SACCH (26 bits + CRC6, nxdn_deperm.c:1246-1261),
 * kind 1 = FACCH1 (80 bits + CRC12, nxdn_dcr_utils.c:21-42); kind + 2 = the same on rows of one bit per byte (what
 * ddn_fec_trellis_decode_batch writes); d_ok [n] = 1 when the field's CRC matches */
int ddn_nxdn_crc_check_batch(const uint8_t* d_bytes, int stride, size_t n, int kind, uint8_t* d_ok, void* hip_stream);

/* ---- DMR data PDUs: the protocol layer behind the dispatched data bursts (ddn_dmr_pdu.hip) ---------------------------------------
 * ddn_dmr_pdu_walk_batch walks each channel's data bursts of a call in air order through what dmr_data_burst_handler()
 * (src/protocol/dmr/dmr_dburst.c:812-845) does with them under dsd_state's running state: the profile under data_conf_data /
 * data_header_format (:105-174), crc_correct and data_block_crc_valid, the rate 3/4 candidate pick against the expected DBSN
 * (:428-468), the DBSN sequence (:651-680), dmr_dheader() (src/protocol/dmr/dmr_block.c:557-618), dmr_block_assembler() types 1 - 3
 * (:1052-1710), the data terminator (dmr_flco.c:319-333); between the bursts dmr_reset_blocks() (dmr_block.c:1714-1748) and the
 * carrier-loss reset (src/engine/engine.c:1957-2000,2041-2063) where the marks say so.  d_state (n_channels x
 * ddn_dmr_pdu_state_bytes(), all zeros = a stream's start) carries both time slots' fields, data_block_crc_valid and the two 3072-byte
 * dmr_pdu_sf rows from call to call: a PDU completes in the call that holds its last burst.
 * Scope: the reference's default options only (aggressive_framesync = 1, dmr_crc_relaxed_default = 0: the RAS override never fires);
 * branding (XPT, Cap+) is taken as unset - CSBK parsing, which sets it, stays on the host; a burst whose slot type did not decode
 * (type > 11) is passed over; everything behind a completed PDU - decryption, LRRP / IP / text / UDT / CSBK message parsing, events -
 * is the caller's.
 * Input, D = n_channels * max_bursts entries, channel c's bursts at c * max_bursts + k for k < d_n_bursts[c] (the layout of
 * ddn_fsk4_chain_results' d_dmr_data_* / d_dmr_r34_* arrays): time slot, data type, the 12 BPTC bytes, the 196 info bits, BPTC
 * irrecoverable errors, the crc flags (bit 0: crc_correct while data_conf_data = 0, bit 1: the confirmed block's CRC9), the
 * unconfirmed rate 3/4 payload, the rate 3/4 pool (ddn_r34_candidate [34] with {CRC9 ok, DBSN} in each entry's two pad bytes) and
 * its length.  Marks, max_marks per channel, each list ascending: d_reset_before[c][j] / d_loss_before[c][j] = the index of the burst
 * the j-th dmr_reset_blocks() / carrier loss of the call precedes (d_n_bursts[c]: behind the last burst). */
typedef struct ddn_dmr_pdu_input {
    int n_channels, max_bursts, max_marks;
    const int32_t* d_n_bursts;       /* [n_channels] */
    const uint8_t* d_slot;           /* [D] */
    const uint8_t* d_type;           /* [D] */
    const uint8_t* d_bytes12;        /* [D][12] */
    const uint8_t* d_info196;        /* [D][196] */
    const uint32_t* d_errs;          /* [D] */
    const uint8_t* d_crc;            /* [D] */
    const uint8_t* d_unconfirmed18;  /* [D][18] */
    const void* d_pool;              /* [D][34] ddn_r34_candidate (include/ddn_hip.h) */
    const int32_t* d_pool_n;         /* [D] */
    const int32_t* d_n_resets;       /* [n_channels] */
    const int32_t* d_reset_before;   /* [n_channels][max_marks] */
    const int32_t* d_n_losses;       /* [n_channels] */
    const int32_t* d_loss_before;    /* [n_channels][max_marks] */
} ddn_dmr_pdu_input;
/* Output.  Per burst [D]: the data_conf_data the burst was read under, data_block_counter before it, crc_correct, the DBSN (0xFF:
 * none), the rate 3/4 pool index chosen (-1: none), and a status byte:
 *   0 ignored (no effect on a PDU)   1 data header accepted      2 data header rejected for its CRC   3 data header with
 *   irrecoverable BPTC errors        4 block filed               5 block filed, PDU completed         6 DBSN sequence error (blocks
 *   reset, no dispatch)              7 MBC longer than 4 blocks  8 data terminator                    9 MBC header filed
 * Per completed PDU, max_pdus slots per channel and call (P; d_n_pdus counts those past P too), slot c * P + j:
 *   d_pdu_kind 1 data / 2 MBC / 3 UDT, d_pdu_slot, d_pdu_burst (index of the burst that completed it), d_pdu_len, d_pdu_bytes [3072]
 *   (zeros behind the length), d_pdu_crc4 {data: CRC32 good (an MNIS header waives it); MBC / UDT: both CRCs good, header CRC good,
 *   blocks CRC16 good, protect flag}, d_pdu_block_crc [128] data_block_crc_valid at completion, d_pdu_header9 {dpf, sap, blocks, poc,
 *   confirmed, p_head, gi, source, target} */
typedef struct ddn_dmr_pdu_output {
    int max_pdus;
    uint8_t* d_burst_conf;     /* [D] */
    int32_t* d_burst_counter;  /* [D] */
    uint8_t* d_burst_crc;      /* [D] */
    uint8_t* d_burst_dbsn;     /* [D] */
    int32_t* d_burst_pick;     /* [D] */
    uint8_t* d_burst_status;   /* [D] */
    int32_t* d_n_pdus;         /* [n_channels] */
    uint8_t* d_pdu_kind;       /* [n_channels][P] */
    uint8_t* d_pdu_slot;       /* [..] */
    int32_t* d_pdu_burst;      /* [..] */
    int32_t* d_pdu_len;        /* [..] */
    uint8_t* d_pdu_bytes;      /* [..][3072] */
    uint8_t* d_pdu_crc4;       /* [..][4] */
    uint8_t* d_pdu_block_crc;  /* [..][128] */
    int32_t* d_pdu_header9;    /* [..][9] */
} ddn_dmr_pdu_output;
size_t ddn_dmr_pdu_state_bytes(void);
int ddn_dmr_pdu_walk_batch(const ddn_dmr_pdu_input* in, void* d_state, const ddn_dmr_pdu_output* out, void* hip_stream);
/* The marks of a call from the receive loop's outputs: dmr_reset_blocks() at a kind-5 event whose slot type or TACT failed or that
 * the colour-code gate rejected (dmr_data_finalize(), dmr_data.c:292-299) and at a kind-8 voice end with a failed TACT or EMB / sync
 * (dmr_bs.c:671-680,937-947), each with the number of dispatched bursts (kind 6, VC 0) ahead of it in the event list; carrier loss at
 * every 1800th symbol in a row of the call's new flags (rows of stride_symbols, from carry_symbols to carry_symbols + d_new[c]) that
 * is neither in frame nor a sync - the loop restarts its count there - placed among the bursts' last symbols (d_burst_start + 143).
 * The run of hunted symbols is carried in d_state. */
int ddn_dmr_pdu_marks_batch(const int32_t* d_events, const int32_t* d_n_events, size_t max_events, const uint8_t* d_flags,
                            size_t stride_symbols, int carry_symbols, const int32_t* d_new, const int32_t* d_burst_start,
                            const int32_t* d_n_bursts, int n_channels, int max_bursts, void* d_state, int32_t* d_reset_before,
                            int32_t* d_n_resets, int32_t* d_loss_before, int32_t* d_n_losses, int max_marks, void* hip_stream);

/* ---- NXDN control and data channels: CAC, FACCH2 / UDCH and the SACCH superframe (ddn_nxdn_ctrl.hip) -----------------------------
 * What nxdn_frame() does with a frame whose LICH names no SACCH / FACCH1 pair, and the state it keeps between frames
 * (src/protocol/nxdn/nxdn_frame.c:117-160,237-263,311-346,488-494; nxdn_deperm.c:164-205,245-340,496-530,610-634,1263-1372;
 * nxdn_dcr_utils.c:44-106; nxdn_element.c:158-200).  Sync slots as ddn_nxdn_frame_gather has them: slot c * max_syncs + k, S =
 * n_channels * max_syncs.
 *
 * ddn_nxdn_ctrl_decode_batch: per slot the LICH is read again from the records (parity, then profile) and the frame classed:
 *   kind 0 none (no whole frame, gate closed, or a channel left to the caller: SACCH / FACCH1 frames, SCCH, FACCH3 / UDCH2, SACCH2,
 *   PICH / TCH)   1 CAC (LICH 0x01, 0x05; bits 16..315)   2 FACCH2 (0x28, 0x29, 0x49; bits 16..363)   3 UDCH (0x2E, 0x2F, 0x4E, 0x4F)
 * Kinds 1..3: de-permutation, 12-in-14 de-puncture, CNXDNConvolution soft decode over 175 / 203 steps with 171 / 199 bits chained
 * back, crc16cac over the 171 bits = 0 / crc15 over bits 0..183 against bits 184..198; where that fails trellis_decode() over the
 * de-punctured hard bits is taken instead, whatever its CRC says (d_fallback = 1), and d_crc_ok is that result's verdict.
 * d_bits208 = the reference's trellis_buf (one bit per byte, zeros behind 171 / 199), d_bytes26 = its m_data (22 / 26 bytes, zeros
 * behind), d_ran = bits 2..7, d_sf = bits 0..1.  d_kind is written for every slot; the other rows of a kind-0 slot stay as they
 * were.  Only the two decoder launches' wanted slots are decoded: a batch without control frames pays for the LICH reads.
 *
 * ddn_nxdn_ctrl_walk_batch: one channel's slots in air order through the state of d_state (n_channels x
 * ddn_nxdn_ctrl_state_bytes(); all zeros is NOT a start: ddn_nxdn_ctrl_state_init sets part_of_frame 0, the segment store and its
 * CRC flags all 1, last RAN none, cac_fail 0).  A slot that is not d_valid is passed over.  Per frame: a LICH with good parity that
 * misses the profile table resets the segment store (a parity failure does not); a SACCH frame takes the soft SACCH where d_sacch_ok,
 * else the greedy retry, through nxdn_handle_sacch(); a FACCH2 / UDCH frame sets part_of_frame = 3 - SF and last RAN on a good CRC,
 * part_of_frame = 0 on a bad one; a CAC sets last RAN on a good CRC and counts consecutive bad ones in cac_fail.  Per slot:
 *   d_sacch_status  0 no SACCH in this frame, 1 segment stored with good CRC, 2 stored with bad CRC, 3 non-superframe good, 4 bad
 *   d_pf            part_of_frame after the frame          d_seq_ok  the sequence rule held ("PF n/4", not "PF X/4"; "PF 1/1")
 *   d_msg_status    0 none, 1 delivered (all four segment CRCs good; a good non-superframe SACCH), 2 completed but a segment was bad
 *   d_msg72         written where d_msg_status != 0 or d_sacch_status is 3 / 4: the four 18-bit segments; a non-superframe SACCH's
 *                   24 bits (message + CRC6) in the first 24, zeros behind
 *   d_last_ran      after the frame, -1 = none             d_cac_fail  after the frame
 * Deviation: above ten consecutive bad CACs the reference resets its symbolizer (thresholds, sample history, sync state) and the
 * counter.  The device cannot hand a decode verdict back into a receive-loop pass that has already run, so the reset is NOT
 * applied: the frame that would trigger it reports d_cac_fail = 11 and the carried counter starts again from 0.  A host that wants
 * the reset has the object resets (ddn_fsk4_rx_reset).  Message parsing (NXDN_Elements_Content_decode), trunking, aliases and the
 * cipher LFSR bookkeeping stay on the host.  A NULL output pointer means that array is not wanted (d_kind, and for the walk d_crc_ok,
 * d_ran and d_sf, are inputs of the later stages and required). */
typedef struct ddn_nxdn_ctrl_input {
    int n_channels;
    size_t max_symbols;              /* row length of d_records10 in symbols */
    size_t max_syncs;
    const uint8_t* d_records10;      /* [n_channels][max_symbols][10] */
    const int32_t* d_counts;         /* [n_channels] records held per row */
    const int32_t* d_sync_pos;       /* [S] */
    const int32_t* d_n_sync;         /* [n_channels] */
    /* the walk only: what ddn_nxdn_frame_gather and the SACCH decoders made of the same slots */
    const uint8_t* d_lich;           /* [S] 7-bit LICH, bit 7 = parity good */
    const uint8_t* d_valid;          /* [S] */
    const uint8_t* d_sacch;          /* [S][4] soft decode, packed */
    const uint8_t* d_sacch_ok;       /* [S] */
    const uint8_t* d_sacch_hard;     /* [S][32] greedy retry, one bit per byte */
    const uint8_t* d_sacch_hard_ok;  /* [S] */
} ddn_nxdn_ctrl_input;
typedef struct ddn_nxdn_ctrl_frames {
    uint8_t* d_kind;      /* [S] */
    uint8_t* d_bits208;   /* [S][208] */
    uint8_t* d_bytes26;   /* [S][26] */
    uint8_t* d_crc_ok;    /* [S] */
    uint8_t* d_fallback;  /* [S] */
    uint8_t* d_ran;       /* [S] */
    uint8_t* d_sf;        /* [S] */
} ddn_nxdn_ctrl_frames;
typedef struct ddn_nxdn_ctrl_messages {
    uint8_t* d_sacch_status; /* [S] */
    uint8_t* d_pf;           /* [S] */
    uint8_t* d_seq_ok;       /* [S] */
    uint8_t* d_msg72;        /* [S][72] */
    uint8_t* d_msg_status;   /* [S] */
    int32_t* d_last_ran;     /* [S] */
    int32_t* d_cac_fail;     /* [S] */
} ddn_nxdn_ctrl_messages;
size_t ddn_nxdn_ctrl_state_bytes(void);
int ddn_nxdn_ctrl_state_init(void* d_state, size_t n_channels, void* hip_stream);
int ddn_nxdn_ctrl_decode_batch(const ddn_nxdn_ctrl_input* in, const ddn_nxdn_ctrl_frames* out, void* hip_stream);
int ddn_nxdn_ctrl_walk_batch(const ddn_nxdn_ctrl_input* in, const ddn_nxdn_ctrl_frames* fr, void* d_state,
                             const ddn_nxdn_ctrl_messages* out, void* hip_stream);

/* ---- DMR MS / direct mode: the bursts behind sync patterns 2..7 (ddn_dmr_ms.hip) ---------------------------------------------------
 * What dmrMSData() and dmrMSBootstrap() + dmrMS() (src/protocol/dmr/dmr_ms.c:420-497, 384-417, 323-381) read behind an MS or
 * direct-mode word at the default options (trunk_enable 0, dmr_stereo 1, inverted_dmr 0).  Both read fixed counts with no early
 * exit - 264 symbols behind a data word (54 + 144 + 66), 1704 behind a voice word (54 + 144 + 9 x 144 + 210; the reference's own
 * tests/protocol/dmr/test_dmr_ms_data.c holds 264, 1506, 1704 and 15 / 18 vocoder calls) - so the receive loop needs no handler:
 * DDN_DMR_MS_LOCK_DATA / _VOICE as its lock_symbols[0] / [1] are all it takes.  p = row index of a sync's last symbol:
 *   data word (patterns 2, 4, 5)   one burst: dibits 0..89 = the hand-over d_pre / d_pre_rel of the sync, 90..143 = records p + 1 ..
 *     p + 54.  dmr_data_sync() (dmr_data.c:117-343) with dmr_stereo = 1, dmr_ms_mode = 1: TACT Hamming(7,4) (fails: status 1), slot
 *     type Golay(20,8) (fails: status 2), no confidence gate, colour code from the slot type, slot 0 - 1 behind the direct-mode TS2
 *     data word - then dmr_data_burst_handler(): the FEC-level results the BS data bursts have (ddn_chain.h, d_dmr_data_*).
 *   voice word (patterns 3, 6, 7)  the bootstrap burst (VC 1) laid out the same way, then five bursts k = 0..4 (VC k + 2) of 144
 *     records from p + 199 + 288 k.  Every burst: three AMBE 3600x2450 frames (dibits 12..47, 48..65 + 90..107, 108..143), its 48
 *     sync-field bits; VC 2..6 file them as embedded signalling and try QR(16,7,6) on the EMB (good: colour code, power bit); at
 *     VC 6 BPTC(128,77) runs over the fragments of VC 2..5 and the 5-bit checksum is checked.  d_voice_tact_ok is what
 *     dmr_ms_decode_tact() computes - Hamming(7,4) over the first seven CACH dibits taken as bits - and the reference ignores.
 * ddn_dmr_ms_walk_batch: one channel's decode list (the syncs whose 54 records are in the row) and the voice unit left open by the
 * previous call (d_state: n_channels x ddn_dmr_ms_state_bytes(), started by ddn_dmr_ms_state_init - all zeros is NOT a start) -> the
 * bursts that end in this call, in air order per list.  A data or bootstrap burst is listed in the call that lists its sync; a later
 * burst of a unit in the call whose row (d_counts records) holds its last symbol - its first is at most 143 records back, so a
 * carry of 144 records or more keeps it whole; a unit may span any number of calls.  d_new is how far the row moves on before the
 * next call.  A burst that finds its list full is counted in d_dropped (running) and written nowhere; the unit goes on.
 *   d_data_start / d_voice_start  row index of the burst's first CACH dibit; down to -89 for a data or bootstrap burst (those dibits
 *                      are the hand-over), DDN_DMR_MS_UNUSED in an unused entry
 *   d_data_sync / d_voice_pre     the sync slot (c * max_syncs + k) whose hand-over opens the burst; -1: a later burst of a unit
 *   d_data_status      0 decoded, 1 TACT failed, 2 slot type failed (the rows of ddn_dmr_ms_data are zeros, d_type 0xFF); d_data_cc
 *                      0xFF unless 0; d_data_gate 0 / -1 is the same verdict as ddn_dmr_ms_data_batch reads it
 *   d_voice_vc         1 bootstrap, 2..6, 0 unused; d_voice_tact_ok / _emb_ok 0xFF for VC 1 (not decoded there), d_voice_emb_cc 0xFF
 *                      and d_voice_power 9 where the EMB did not decode
 *   d_lc_pos           row index of the VC 6 burst's last symbol, -1 unused; d_lc_in128 the 8 x 16 matrix (zeros where unused)
 *   d_cc               the colour code carried per channel (16 until a slot type or an EMB decodes), d_phase the open unit's next
 *                      burst k (5: none open)
 * ddn_dmr_ms_data_batch: gather, Golay(20,8), BPTC(196,96), the data type's CRC / RS(12,9), the rate 3/4 decoders and pool - the
 * BS data-burst stage's kernels on the walk's list.  ddn_dmr_ms_voice_batch: the frames, BPTC(128,77) + checksum per listed link
 * control, and - mbe != NULL, an AMBE 3600x2450 batch of n_channels talk paths - frame FEC, skip marks and synthesis, 3 max_voice
 * frames per path.  One talk path per channel (dmrMS() forces slot 0) whose history streams from call to call.
 * Deviation: the reference keeps one mbe_parms set for slot 0, shared by the MS path and the BS slot-0 path of the same receiver;
 * here the MS talk path is its own, so BS and MS traffic alternating on one channel do not see each other's vocoder history.
 * Not here: message parsing, dmr_sbrc(), late-entry MI, the keystreams, -xr polarity, the reverse-channel word (pattern 8). */
#define DDN_DMR_MS_LOCK_DATA 264
#define DDN_DMR_MS_LOCK_VOICE 1704
#define DDN_DMR_MS_UNUSED INT32_MIN
typedef struct ddn_dmr_ms_input {
    int n_channels;
    size_t max_symbols;          /* row length of d_records10 in symbols */
    size_t max_syncs;
    const uint8_t* d_records10;  /* [n_channels][max_symbols][10] */
    const int32_t* d_counts;     /* [n_channels] records held per row */
    const int32_t* d_new;        /* [n_channels] records the row moves on by before the next call */
    const int32_t* d_sync_pos;   /* [S] */
    const uint8_t* d_sync_pat;   /* [S] */
    const int32_t* d_n_sync;     /* [n_channels] */
    const uint8_t* d_pre;        /* [S][DDN_FSK4_PRE] */
    const uint8_t* d_pre_rel;    /* [S][DDN_FSK4_PRE] */
} ddn_dmr_ms_input;
typedef struct ddn_dmr_ms_bursts { /* the walk's lists: D = n_channels * max_data, V = n_channels * max_voice, L = n_channels * max_lc */
    int max_data, max_voice, max_lc;
    int32_t* d_n_data;         /* [n_channels] */
    int32_t* d_data_start;     /* [D] */
    int32_t* d_data_sync;      /* [D] */
    int32_t* d_data_gate;      /* [D] */
    uint8_t* d_data_pat;       /* [D] sync pattern */
    uint8_t* d_data_slot;      /* [D] */
    uint8_t* d_data_status;    /* [D] */
    uint8_t* d_data_cc;        /* [D] */
    int32_t* d_n_voice;        /* [n_channels] */
    int32_t* d_voice_start;    /* [V] */
    int32_t* d_voice_pre;      /* [V] */
    uint8_t* d_voice_vc;       /* [V] */
    uint8_t* d_voice_tact_ok;  /* [V] */
    uint8_t* d_voice_emb_ok;   /* [V] */
    uint8_t* d_voice_emb_cc;   /* [V] */
    uint8_t* d_voice_power;    /* [V] */
    uint8_t* d_voice_sync48;   /* [V][48] */
    int32_t* d_n_lc;           /* [n_channels] */
    int32_t* d_lc_pos;         /* [L] */
    uint8_t* d_lc_in128;       /* [L][128] */
    int32_t* d_cc;             /* [n_channels] */
    int32_t* d_dropped;        /* [n_channels] */
    int32_t* d_phase;          /* [n_channels] */
} ddn_dmr_ms_bursts;
typedef struct ddn_dmr_ms_data { /* per data burst, as ddn_fsk4_chain_results.d_dmr_data_* / d_dmr_r34_* */
    uint8_t* d_type;               /* [D] 0xFF: not decoded */
    uint8_t* d_info196;            /* [D][196] */
    uint8_t* d_bits96;             /* [D][96] */
    uint8_t* d_bytes12;            /* [D][12] */
    uint32_t* d_errs;              /* [D] */
    uint8_t* d_crc;                /* [D] */
    uint8_t* d_r34_unconfirmed;    /* [D][18] */
    uint8_t* d_r34_confirmed;      /* [D][18] */
    uint8_t* d_r34_confirmed_crc;  /* [D] */
    void* d_r34_pool;              /* [D][34] ddn_r34_candidate (include/ddn_hip.h) */
    int32_t* d_r34_pool_n;         /* [D] */
} ddn_dmr_ms_data;
typedef struct ddn_dmr_ms_voice {
    uint8_t* d_ambe_frames;   /* [V][3][4][24] */
    uint8_t* d_skip;          /* [V][3] 0xFF: no burst in this entry */
    uint8_t* d_lc77;          /* [L][77] */
    uint32_t* d_lc_errs;      /* [L] */
    uint8_t* d_lc_ok;         /* [L] the 5-bit checksum held */
    /* with a vocoder batch: */
    uint8_t* d_ambe_bits;     /* [V][3][49] */
    int32_t* d_ambe_result;   /* [V][3][5] */
    float* d_pcm;             /* [V][3][160] */
} ddn_dmr_ms_voice;
size_t ddn_dmr_ms_state_bytes(void);
int ddn_dmr_ms_state_init(void* d_state, size_t n_channels, void* hip_stream);
int ddn_dmr_ms_walk_batch(const ddn_dmr_ms_input* in, void* d_state, const ddn_dmr_ms_bursts* out, void* hip_stream);
int ddn_dmr_ms_data_batch(const ddn_dmr_ms_input* in, const ddn_dmr_ms_bursts* bursts, const ddn_dmr_ms_data* out, void* hip_stream);
int ddn_dmr_ms_voice_batch(const ddn_dmr_ms_input* in, const ddn_dmr_ms_bursts* bursts, const ddn_dmr_ms_voice* out, void* mbe_batch,
                           void* hip_stream);
#ifdef __cplusplus
}
#endif
#endif
