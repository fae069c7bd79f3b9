// ddn_p25h_rules.h - the decision rules of the P25 Phase 1 handlers, stated once for both receive loops (ddn_rx.hip serve(),
// ddn_cqrx.hip handler_symbol()): what a decoded NID does to the carried NAC, how long each DUID is read, where a TSDU / data unit
// ends, every word of the events.  Integers only, constexpr, and it compiles for the host (plain g++: tests/test_p25h_rules.py runs
// it against the oracle's orc_p25h_symbol()).  The decoders that feed the rules, and the handlers' source lines: ddn_p25h_dev.h.
#ifndef DDN_P25H_RULES_H
#define DDN_P25H_RULES_H
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define DDN_P25H_HD __host__ __device__ __forceinline__ constexpr
#else
#define DDN_P25H_HD inline constexpr
#endif

namespace ddn_p25h {

enum { PH_IDLE = 0, PH_NID = 1, PH_BODY = 2, PH_TSBK = 3, PH_MPDU = 4 }; // (PH_BODY: a fixed count, the symbol-rate loop's alone)
enum { EV_NID = 1, EV_TSBK = 2, EV_MPDU = 3 };
constexpr int TSBK_SYMBOLS = 101, TSBK_MAX_BLOCKS = 3;
// one decision as the loops log it: events[.] = {position, kind, a, b}, event_data[.] = {d0, d1, d2, d3}
struct Event { int32_t kind, a, b, d0, d1, d2, d3; };

// position of received dibit i inside the de-interleaved block: 49 dibit pairs dealt to 4 lanes round-robin - received order:
// lane 0 pairs (0,4,8,...,48) [13 pairs], lane 1 (1,5,...,45) [12], lane 2 [12], lane 3 [12]
DDN_P25H_HD int
deinterleave98(int i) {
    const int pair_rx = i >> 1;
    int lane = 0, k = pair_rx;
    if (pair_rx >= 13) {
        lane = 1 + (pair_rx - 13) / 12;
        k = (pair_rx - 13) % 12;
    }
    return 2 * (lane + 4 * k) + (i & 1);
}

// trellis output for (state << 2) | next state, src/protocol/p25/p25_12.c:19:
// {2, 12, 1, 15, 14, 0, 13, 3, 9, 7, 10, 4, 5, 11, 6, 8} packed 4 bits each
constexpr uint64_t HALF_RATE_NIBBLES = 0x86B5'4A79'3D0E'F1C2ull;
DDN_P25H_HD int
half_rate_nibble(int idx) {
    return (int)((HALF_RATE_NIBBLES >> (4 * idx)) & 15u);
}
// the table read the other way: (state << 2) | next state of the one branch that emits a nibble, packed 4 bits each
DDN_P25H_HD uint64_t
half_rate_branches_by_nibble() {
    uint64_t inv = 0;
    for (int idx = 0; idx < 16; idx++) {
        inv |= (uint64_t)idx << (4 * half_rate_nibble(idx));
    }
    return inv;
}
DDN_P25H_HD bool
half_rate_nibbles_distinct() {
    unsigned seen = 0;
    for (int idx = 0; idx < 16; idx++) {
        seen |= 1u << half_rate_nibble(idx);
    }
    return seen == 0xFFFFu;
}
static_assert(half_rate_nibbles_distinct(), "half_rate_hard_path_wave: one branch per nibble, or the look-up is not a function");
// skipdibit bookkeeping of tsbk_read_repetition_samples() / p25_mpdu_read_repetition() in closed form.  The counter starts a
// block at sk0 (1..36); a symbol read with the counter at 36 is a status symbol and restarts it, so status symbols sit at
// i0 = 36 - sk0 and every 36 after.
DDN_P25H_HD bool
block_is_status(int sk0, int i, int& data_index) {
    const int i0 = 36 - sk0;
    const int before = (i <= i0) ? 0 : ((i - 1 - i0) / 36 + 1); // status symbols among 0 .. i - 1
    data_index = i - before;
    return i >= i0 && ((i - i0) % 36) == 0;
}
DDN_P25H_HD int
block_counter_after(int sk0, int n_sym, int& n_data) { // the counter after n_sym symbols, and how many of them were data
    const int i0 = 36 - sk0;
    if (n_sym <= i0) {
        n_data = n_sym;
        return sk0 + n_sym;
    }
    const int n_status = (n_sym - 1 - i0) / 36 + 1;
    n_data = n_sym - n_status;
    return n_sym - (i0 + 36 * (n_status - 1));
}
// symbols p25_mpdu_read_repetition() consumes for one repetition starting with the counter at sk0 (98 data dibits, <= 101 reads)
DDN_P25H_HD int
mpdu_block_symbols(int sk0, int& sk_after) {
    int sk = sk0, k = 0, i = 0;
    for (; i < 101; i++) {
        if ((sk / 36) == 0) {
            k++;
        } else {
            sk = 0;
        }
        sk++;
        if (k == 98) {
            i++;
            break;
        }
    }
    sk_after = sk;
    return i;
}
// p25p1_decode_nid_and_duid(): the NAC the decoder's retry is told, state->nac when valid, else p2_cc, else none
DDN_P25H_HD int
observed_nac(int nac, int p2cc) {
    return (nac > 0 && nac < 0xFFF) ? nac : ((p2cc > 0 && p2cc < 0xFFF) ? p2cc : 0);
}
// p25p1_handle_nid_decode_success() on p25p1_nid_decode's {status, nac, duid, errs}: a new NAC that is neither 0 nor 0xFFF replaces
// the carried pair; a failed decode leaves both and has no DUID (0xFF)
struct NidOutcome { int nac, p2cc, duid; Event ev; };
DDN_P25H_HD NidOutcome
nid_outcome(int status, int r_nac, int r_duid, int errs, int nac, int p2cc) {
    int duid = 0xFF;
    if (status > 0) {
        if (r_nac != nac && r_nac != 0 && r_nac != 0xFFF) {
            nac = r_nac;
            p2cc = r_nac;
        }
        duid = r_duid;
    }
    return {nac, p2cc, duid, {EV_NID, status, (r_nac & 0xFFFF) | (duid << 16), status, r_nac, r_duid, errs}};
}
// dispatch_p25p1.c:391-403: symbols read after the NID of a DUID without blocks - HDU, LDU1 / LDU2, TDU, TDULC; undefined / failed: 0
DDN_P25H_HD int
body_symbols(int duid) {
    return duid == 0x0 ? 339 : ((duid == 0x5 || duid == 0xA) ? 807 : (duid == 0x3 ? 15 : (duid == 0xF ? 159 : 0)));
}
// a TSDU (DUID 7) or data unit (DUID 12) is read block by block: TSBK_MAX_BLOCKS / p25_mpdu_context_init() end = 3, the status
// counter 14 dibits past a status symbol.  PH_IDLE: the DUID has no blocks (body_symbols())
struct BlockPhase { int phase, block, end, skipdibit; };
DDN_P25H_HD BlockPhase
block_phase_start(int duid) {
    return {duid == 0x7 ? PH_TSBK : (duid == 0xC ? PH_MPDU : PH_IDLE), 0, TSBK_MAX_BLOCKS, 36 - 14};
}
DDN_P25H_HD int32_t
block_data3(int crc_ok, int sel, int block) { // event-data word 3 of a trellis block: CRC16 good | candidate index << 8 | block << 16
    return (crc_ok & 1) | ((sel & 0xFF) << 8) | (block << 16);
}
DDN_P25H_HD bool
tsbk_block_ends(int block) { // whatever it decodes: known before the decode, so the C4FM loop answers its waiting lane first
    return block + 1 >= TSBK_MAX_BLOCKS;
}
// one TSDU block (words w: byte k = (w[k >> 2] >> (8 * (k & 3))) & 0xFF; sel = the list candidate taken): the TSDU ends on the
// block's last-block flag or with the third block.  Event word b: CRC good | byte 1 << 8 | (last flag << 8 | sel) << 16
struct TsbkOutcome { Event ev; bool last; };
DDN_P25H_HD TsbkOutcome
tsbk_outcome(uint32_t w0, uint32_t w1, uint32_t w2, int crc_ok, int sel, int block) {
    const int flag = (int)((w0 >> 7) & 1u);
    return {{EV_TSBK, block, crc_ok | (int)(((w0 >> 8) & 0xFFu) << 8) | (((flag << 8) | sel) << 16), (int32_t)w0, (int32_t)w1,
             (int32_t)w2, block_data3(crc_ok, sel, block)},
            flag != 0 || tsbk_block_ends(block)};
}
// a data unit's header block, p25_mpdu_update_header_from_first_block(): blks + 1 blocks in all (SAP 61 / 63 with blks > 10: 4);
// aggressive_framesync = 1 keeps the carried `end` on a bad header CRC.  Event word b: end | byte 0 << 16
struct HeaderOutcome { Event ev; int end; };
DDN_P25H_HD HeaderOutcome
header_outcome(uint32_t w0, uint32_t w1, uint32_t w2, int crc_ok, int sel, int end) {
    if (crc_ok) {
        const int sap = (int)((w0 >> 8) & 0x3Fu), blks = (int)((w1 >> 16) & 0x7Fu);
        end = ((sap == 61 || sap == 63) && blks > 10) ? 4 : blks + 1;
    }
    return {{EV_MPDU, crc_ok, (end & 0xFFFF) | (int)((w0 & 0xFFu) << 16), (int32_t)w0, (int32_t)w1, (int32_t)w2, block_data3(crc_ok, sel, 0)},
            end};
}
} // namespace ddn_p25h
#endif
