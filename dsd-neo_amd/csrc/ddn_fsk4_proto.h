// ddn_fsk4_proto.h - the protocols of the fsk4 receive loop, one row per DDN_FSK4_* value (include/ddn_fsk4.h).  This is where a
// protocol is defined: the kernel (Fsk4Cfg<PROTO>, ddn_rx4.hip), its launcher, the host object (ddn_api_rx4.cpp) and the chain
// (ddn_api_chain_fsk4.cpp) all read the row and state none of it again.  Host and device, plain C++17 constexpr; not installed.
#ifndef DDN_FSK4_PROTO_H
#define DDN_FSK4_PROTO_H
#include <stdint.h>

#include "ddn_fsk4.h"
#include "ddn_tables_dpmr.h"
#include "ddn_tables_fsk4.h"

namespace ddn_fsk4 {
// the matched filter's tap table (k_fsk4_matched_filter<NT, SET>); none = the protocol has no filter, use_matched_filter is ignored
enum Taps { TAPS_NONE = -1, TAPS_DMR = 0, TAPS_NXDN48 = 1, TAPS_DPMR = 2 };
// (the loop's in-kernel filter stage needs a length even where it never runs: without a table it is compiled for the shortest one)
constexpr int
taps_len(int set) {
    return set == TAPS_NXDN48 ? DDN_NXDN48_FILTER_TAPS : (set == TAPS_DPMR ? DDN_DPMR_FILTER_TAPS : DDN_DMR_FILTER_TAPS);
}
inline const unsigned int*
taps_bits(int set) { // binary32 bit patterns, nullptr = none
    return set == TAPS_DMR ? ddn_dmr_filter_bits : (set == TAPS_NXDN48 ? ddn_nxdn48_filter_bits : (set == TAPS_DPMR ? ddn_dpmr_filter_bits : nullptr));
}

// type ids only need to be non-zero and distinct per family; these mirror synctype_ids.h + 1
// (DMR; NXDN; YSF :109-110; dPMR FS2 :92,96; D-STAR :44-47; EDACS :85-86 = DDN_EDACS_TYPE_*; M17 :52-63 in its row)
enum {
    T_BS_DATA = 11, T_BS_VOICE_NEG = 12, T_BS_VOICE = 13, T_BS_DATA_NEG = 14, T_MS_VOICE = 33, T_MS_DATA = 34, T_RC_DATA = 35,
    T_NX_POS = 29, T_NX_NEG = 30, T_YSF_POS = 31, T_YSF_NEG = 32, T_DPMR_FS2 = 22, T_DPMR_FS2_INV = 26,
    T_DSTAR_POS = 7, T_DSTAR_NEG = 8, T_DSTAR_HD_POS = 19, T_DSTAR_HD_NEG = 20
};

// One sync pattern: a word as a sign string ('1' = +3, '3' = -3) or its complement, the sync type it is accepted as, the
// lock_symbols[] class behind it, and whether digitize() treats the type as negative polarity (flags bit 4).
struct Pat {
    const char* word;
    bool complement;
    uint8_t type, cls, neg;
};
constexpr int MAX_ROW_PAT = 12;

// sign bits of a word, first symbol highest: bits 0..23 go to DdnFsk4Config::pat_bits, 24..47 (a 48-symbol word) to pat_hi
constexpr uint64_t
word_bits(const char* s, bool complement) {
    uint64_t v = 0;
    for (; *s; s++) {
        v = (v << 1) | ((*s == '1') != complement ? 1u : 0u);
    }
    return v;
}

struct Row {
    const char* name;       // for messages
    int sym_rate;           // symbols/s
    int t_max, warm_len;    // level ring (frame_sync_select_t_max()), symbols of the warm start behind an accepted sync
    bool confirm;           // a sync is accepted on the second consecutive match (NXDN, dsd_frame_sync.c:1507-1556)
    bool dmr_window;        // C4FM left edge 1 once a sync type is held (dsd_symbol.c:197-224)
    bool redigitize;        // dmr_resample_on_sync() (src/dsp/dmr_sync.c:63-131)
    bool m17;               // the words are matched by frame_sync_try_m17()'s rules (m17_hit(), ddn_rx4.hip); pat[] names the outcomes
    Taps taps;
    bool handlers;          // has a handler family (ddn_fsk4h_dev.h); the others read fixed counts behind a sync
    bool inverted_ok;       // ddn_fsk4_rx_config::inverted is accepted
    // out_rate_hz / sym_rate must lie in sps_min..sps_max (sps_whole: with no remainder).  The kernel's per-round hand-off queue and
    // its whole-symbol pass are sized for 8..21 samples per symbol; the longer queue of a protocol below that holds 4-sample symbols
    // and its straight pass at most 11
    int sps_min, sps_max;
    bool sps_whole;
    // MAXW, the longest whole symbol the straight pass takes (samples per symbol + one slip sample): 12 covers 4800 symbols/s at
    // 48 ksps, 22 covers 2400.  by_sps: 12 up to 11 samples per symbol and 22 above; else 12 whatever the rate
    bool maxw_by_sps;
    int lock_symbols[4];    // the defaults of ddn_fsk4_rx_config::lock_symbols, per sync class
    Pat pat[MAX_ROW_PAT];   // in the order of the sync pattern index (include/ddn_fsk4.h)

    constexpr int
    n_pat() const { // as the kernel compares it
        int n = 0;
        while (n < MAX_ROW_PAT && pat[n].word) {
            n++;
        }
        return n;
    }
    constexpr int
    win_len() const { // symbols of the sync window = of a word
        int n = 0;
        while (pat[0].word && pat[0].word[n]) {
            n++;
        }
        return n;
    }
    constexpr int
    maxw(int sps) const {
        return (maxw_by_sps && sps > 11) ? 22 : 12;
    }
};

// both NXDN rows: the frame sync word and the four single-symbol variants the reference also accepts, then their complements
// (include/dsd-neo/core/sync_patterns.h:58-80, src/dsp/dsd_frame_sync.c:1508-1512)
#define DDN_FSK4_NXDN_PATS                                                                                                         \
    {{"3131331131", false, T_NX_POS, 0, 0}, {"3331331131", false, T_NX_POS, 0, 0}, {"3131331111", false, T_NX_POS, 0, 0},          \
     {"3331331111", false, T_NX_POS, 0, 0}, {"3131311131", false, T_NX_POS, 0, 0}, {"3131331131", true, T_NX_NEG, 0, 1},           \
     {"3331331131", true, T_NX_NEG, 0, 1},  {"3131331111", true, T_NX_NEG, 0, 1},  {"3331331111", true, T_NX_NEG, 0, 1},           \
     {"3131311131", true, T_NX_NEG, 0, 1}}
#define DDN_FSK4_M17_OUTCOME(k, type) {"11111111", false, type, (k) < 2 ? 1 : 0, (k) & 1}

constexpr Row kRow[] = {
    {},
    // DMR: 4800 symbols/s on the 4800_4 hunt profile, basic lock (dsd_frame_sync.c:385-392,1102-1314) + dmr_resample_on_sync(): warm
    // start over the 24 sync symbols, re-digitisation of the 66 payload dibits before them.  Words: ETSI TS 102 361-1 table 9.2 (BS /
    // MS / direct-mode sourced data and voice); class 1 = voice.  Pattern 8, tried after the eight: the MS reverse-channel word
    // (sync_patterns.h:74-75; frame_sync_try_dmr_rc_data(), dsd_frame_sync.c:1318-1334) has no voice / data partner (its complement
    // is ETSI-reserved and claimed only under -xr), no digitize() polarity, and class 2 = the 12 dibits dmr_rc.c:39-44 reads beyond the
    // 36 already behind the sync.  lock_symbols: data 120 = 54 live + 66 skipped, voice 54 + 6 superframes' bursts
    {"DMR", 4800, 24, 24, false, true, true, false, TAPS_DMR, true, true, 8, 21, false, true, {120, 54 + 6 * 288, 12, 0},
     {{"313333111331131131331131", false, T_BS_DATA, 0, 0}, {"131111333113313313113313", false, T_BS_VOICE, 1, 0},
      {"311131133313133331131113", false, T_MS_DATA, 0, 0}, {"133313311131311113313331", false, T_MS_VOICE, 1, 0},
      {"331333313111313133311111", false, T_MS_DATA, 0, 0}, {"311311111333113333133311", false, T_MS_DATA, 0, 0},
      {"113111131333131311133333", false, T_MS_VOICE, 1, 0}, {"133133333111331111311133", false, T_MS_VOICE, 1, 0},
      {"131331111133133133311313", false, T_RC_DATA, DDN_FSK4_CLASS_RC, 0}}},
    // NXDN48: 2400 symbols/s on the 2400_4 hunt profile (level ring 12), 10-symbol window, five patterns per polarity, accepted on the
    // second consecutive match (dsd_frame_sync.c:1507-1556), nxdn_filter (src/dsp/dsd_filters.c:348-356); 182 dibits behind a sync
    {"NXDN48", 2400, 12, 10, true, false, false, false, TAPS_NXDN48, true, false, 8, 21, false, true, {182, 0, 0, 0}, DDN_FSK4_NXDN_PATS},
    // NXDN96: NXDN's sync words, two-match confirmation and LICH gate at 4800 symbols/s on the 4800_4 hunt profile (level ring 24,
    // src/dsp/dsd_frame_sync.c:1525-1556,1729-1744) behind the DMR matched filter (symbol_apply_matched_filter(),
    // src/dsp/dsd_symbol.c:323-335); 10 samples per symbol at 48 ksps - the straight pass of 12
    {"NXDN96", 4800, 24, 10, true, false, false, false, TAPS_DMR, true, false, 8, 21, false, false, {182, 0, 0, 0}, DDN_FSK4_NXDN_PATS},
    // M17 (-fz): C4FM lock at 4800 symbols/s without a matched filter (decode_mode_apply_m17(), src/runtime/decode_mode.c:486-510),
    // eight-symbol words matched with one error allowed by frame_sync_try_m17() (src/dsp/dsd_frame_sync.c:865-1100), 8-symbol warm
    // start.  The table names the twelve outcomes, its words only span the window: type ids = synctype_ids.h:52-63 + 1, odd rows
    // negative polarity, class 1 = the preamble (skipDibit(8)), class 0 = a frame or the EOT marker (184 dibits) - dispatch_m17.c:25-68
    {"M17", 4800, 24, 8, false, false, false, true, TAPS_NONE, false, false, 8, 21, false, false, {184, 8, 0, 0},
     {DDN_FSK4_M17_OUTCOME(0, 99), DDN_FSK4_M17_OUTCOME(1, 100), DDN_FSK4_M17_OUTCOME(2, 101), DDN_FSK4_M17_OUTCOME(3, 102),
      DDN_FSK4_M17_OUTCOME(4, 17), DDN_FSK4_M17_OUTCOME(5, 18), DDN_FSK4_M17_OUTCOME(6, 77), DDN_FSK4_M17_OUTCOME(7, 78),
      DDN_FSK4_M17_OUTCOME(8, 9), DDN_FSK4_M17_OUTCOME(9, 10), DDN_FSK4_M17_OUTCOME(10, 87), DDN_FSK4_M17_OUTCOME(11, 88)}},
    // YSF (-fy): the 20-symbol FUSION_SYNC compared exactly in both polarities (frame_sync_try_ysf(), src/dsp/dsd_frame_sync.c:770-797;
    // include/dsd-neo/core/sync_patterns.h:30-31; types = synctype_ids.h:109-110 + 1), 20-symbol warm start, the DMR matched filter
    // once a YSF sync is the last type (src/dsp/dsd_symbol.c:306-309), a fixed count behind a sync (processYSF() reads 100 FICH + 360
    // payload dibits for every frame type but FI = 3 with DT != 1, src/protocol/ysf/ysf.c)
    {"YSF", 4800, 24, 20, false, false, false, false, TAPS_DMR, false, false, 8, 21, false, false, {460, 0, 0, 0},
     {{"31111311313113131131", false, T_YSF_POS, 0, 0}, {"31111311313113131131", true, T_YSF_NEG, 0, 1}}},
    // dPMR (-fm): 2400 symbols/s on the 2400_4 hunt profile (level ring 12), FS2 only, exact over 12 symbols, the plain word or - under
    // -xd (inverted) - its complement as T_DPMR_FS2_INV (frame_sync_try_dpmr(), src/dsp/dsd_frame_sync.c:832-862; include/dsd-neo/core/
    // sync_patterns.h:123-132).  Neither type is a four-level negative type to digitize() (src/core/frames/dsd_dibit.c:916-935): the
    // dibits stay as sliced, processdPMRvoice() XORs them with 2 itself under -xd - neg stays 0.  12-symbol warm start, dpmr_filter once
    // a dPMR type is held (src/dsp/dsd_symbol.c:316-321); 372 dibits behind a sync (dpmr_voice.c:397-425)
    {"dPMR", 2400, 12, 12, false, false, false, false, TAPS_DPMR, false, true, 8, 21, false, true, {372, 0, 0, 0},
     {{"113333131331", false, T_DPMR_FS2, 0, 0}}},
    // D-STAR (-fd): 4800 symbols/s on the 4800_2 hunt profile (level ring 24), no matched filter (symbol_apply_matched_filter() has no
    // D-STAR branch, src/dsp/dsd_symbol.c:300-336), the four 24-symbol words compared exactly (frame_sync_try_dstar(),
    // dsd_frame_sync.c:1452-1503; include/dsd-neo/core/sync_patterns.h:44-47) with the basic lock and a 24-symbol outer-only warm start.
    // The two-level slice (digitize(), src/core/frames/dsd_dibit.c:892-948,1019-1029) belongs to the frame decoders (ddn_dstar.hip),
    // which read the records' symbols against the thresholds the sync left; neg marks the negative words.  Class 1 = a voice sync
    // (processDSTAR(): 21 x 72 + 20 x 24 symbols), class 0 = a header sync (660 more, processDSTAR_HD())
    {"D-STAR", 4800, 24, 24, false, false, false, false, TAPS_NONE, false, false, 8, 21, false, false,
     {DDN_DSTAR_HEADER_SYMBOLS, DDN_DSTAR_VOICE_SYMBOLS, 0, 0},
     {{"313131313133131113313111", false, T_DSTAR_POS, DDN_FSK4_CLASS_VOICE, 0}, {"313131313133131113313111", true, T_DSTAR_NEG, DDN_FSK4_CLASS_VOICE, 1},
      {"131313131333133113131111", false, T_DSTAR_HD_POS, DDN_FSK4_CLASS_DATA, 0}, {"131313131333133113131111", true, T_DSTAR_HD_NEG, DDN_FSK4_CLASS_DATA, 1}}},
    // EDACS (-fh / -fH / -fe / -fE): 9600 symbols/s on the 9600_2 hunt profile, 5 samples per symbol at 48 ksps
    // (decode_mode_apply_edacs_pv(): samplesPerSymbol = 5), level ring 24 (frame_sync_select_t_max(), default branch), no matched filter
    // (no EDACS branch in symbol_apply_matched_filter(), src/dsp/dsd_symbol.c:300-336).  The two 48-symbol words are compared exactly
    // (frame_sync_try_provoice(), dsd_frame_sync.c:1421-1450; include/dsd-neo/core/sync_patterns.h:107-108): EDACS_SYNC is accepted as
    // DSD_SYNC_EDACS_NEG, INV_EDACS_SYNC as DSD_SYNC_EDACS_POS (types = synctype_ids.h:85-86 + 1), with the basic lock and a 48-symbol
    // outer-only warm start (frame_sync_accept_edacs(), :1399-1409).  The sign history is 48 symbols long: bits 0..23 in hist_bits,
    // 24..47 in hist_hi (Fsk4Cfg::wide).  240 symbols behind a sync (edacs_collect_bits()); the two-level slice
    // (store_two_level_dibit(), src/core/frames/dsd_dibit.c:938-948) belongs to ddn_edacs.hip
    {"EDACS", 9600, 24, 48, false, false, false, false, TAPS_NONE, false, false, 5, 10, true, false, {DDN_EDACS_FRAME_SYMBOLS, 0, 0, 0},
     {{"313131313131313131313111333133133131313131313131", false, DDN_EDACS_TYPE_NEG, 0, 1},
      {"313131313131313131313111333133133131313131313131", true, DDN_EDACS_TYPE_POS, 0, 0}}},
};
#undef DDN_FSK4_NXDN_PATS
#undef DDN_FSK4_M17_OUTCOME
constexpr int N_PROTO = (int)(sizeof(kRow) / sizeof(kRow[0])) - 1;
static_assert(N_PROTO == DDN_FSK4_EDACS, "one row per DDN_FSK4_* value");

constexpr bool
known(int protocol) {
    return protocol >= 1 && protocol <= N_PROTO;
}
} // namespace ddn_fsk4
#endif
