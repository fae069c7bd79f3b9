// ddn_dmr_pdu.hip - the DMR protocol layer between a dispatched data burst and a completed PDU (include/ddn_fsk4.h:
// ddn_dmr_pdu_walk_batch; include/ddn_chain.h: ddn_dmr_pdu_chain_results), and the per-channel state that carries a PDU across calls.
//
// ddn_dmr_data.hip leaves every dispatched burst at FEC level with both answers where the reference's choice depends on its running
// state.  This file keeps that state and makes the choice, burst by burst in air order, as dmr_data_burst_handler()
// (src/protocol/dmr/dmr_dburst.c:812-845) does:
//   dmr_dburst_profile_resolve() (:105-174) under data_conf_data / data_header_format, the data_p_head clear (:196-198,820-822)
//   crc_correct and data_block_crc_valid[slot][counter] as the handler has them in that state; for rate 3/4
//     dmr_dburst_trellis_choose_candidate_index() (:428-468) over the stored pool against data_dbsn_have / data_dbsn_expected
//   dmr_dburst_update_dbsn_sequence() (:651-680), the sequence error included (dmr_reset_blocks(), no dispatch)
//   the dispatch (:736-771): dmr_dheader() (src/protocol/dmr/dmr_block.c:557-618 with its handlers :281-297,331-387,475-535),
//     dmr_block_assembler() types 1, 2 and 3 (:1052-1114,1157-1180,1423-1451,1462-1582,1622-1710), and the one effect dmr_flco() has
//     on these fields: a readable data terminator (TD_LC, dmr_flco.c:319-333)
// between the bursts: dmr_reset_blocks() (dmr_block.c:1714-1748) where the loop's events say the reference calls it, and the
// carrier-loss reset (no_carrier_reset_dmr_data_blocks() + no_carrier_reset_dmr_misc_state(), src/engine/engine.c:1957-2000,2041-2063:
// data_conf_data, the DBSN expectation and udt_uab_reserved stand).
//   k_dmr_pdu_marks   one wavefront per channel: the call's events -> the resets (dmr_data_finalize(), dmr_data.c:292-299: slot type
//                     or TACT failed, or the colour-code gate rejected the burst; finalize_dmr_bs() / dmrBSBootstrap(), dmr_bs.c:671-680,
//                     937-947: TACT or EMB / sync failed), each with the number of dispatched bursts ahead of it; the call's new flags ->
//                     carrier loss at every 1800th symbol in a row that is neither in frame nor a sync (the count is carried)
//   k_dmr_pdu_walk    one wavefront per channel: the merge of bursts and marks.  The sequencing is wave-uniform; the lanes move the
//                     bytes (a block into the slot's row, a completed row to its PDU slot, the clears), pick the pool entry (a lane
//                     per candidate) and compute the CRCs (a span of bytes per lane, the partial remainders combined).
// Scope: the reference's default options (aggressive_framesync = 1, dmr_crc_relaxed_default = 0: the RAS override never fires),
// branding unset (XPT / Cap+ come from CSBK parsing, which stays on the host), data_block_crc_valid written only below index 127 (the
// reference indexes its [127] row with an unbounded counter), a burst whose slot type did not decode is passed over.  Everything
// behind a completed PDU (decryption, LRRP / IP / text / UDT / CSBK parsing, events) is the caller's.
// Vector stores only, no atomics: one wavefront owns its channel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddn_crc_dev.h"
#include "ddn_device.h"

// What a channel carries from call to call (all zeros = a stream's start: `live` = 0 reads as dsd_init.c / dmr_reset_blocks() leave the
// fields - counters 1, blocks 1, format 7; its size is ddn_dmr_pdu_state_bytes()).
struct DdnDmrPduState {
    int32_t live;
    int32_t hunted;      // symbols hunted in a row behind the last lock when the last call ended (k_dmr_pdu_marks)
    int32_t blocks[2];   // data_header_blocks
    int32_t counter[2];  // data_block_counter
    int32_t byte_ctr[2]; // data_byte_ctr
    int32_t fill[2];     // no byte of sf[slot] at or behind this index is non-zero (what a clear has to touch; a multiple of 4)
    uint32_t src[2], tgt[2]; // dmr_lrrp_source / dmr_lrrp_target
    // data_conf_data, data_header_format, data_header_valid, data_p_head, data_header_sap, data_block_poc, udt_uab_reserved,
    // data_dbsn_have, data_dbsn_expected, dmr_data_target_is_group
    uint8_t conf[2], hfmt[2], hvalid[2], p_head[2], sap[2], poc[2], udt_res[2], dbsn_have[2], dbsn_exp[2], gi[2];
    uint8_t pad[4];
    uint8_t crc_valid[2][128]; // data_block_crc_valid[2][127]
    uint8_t sf[2][3072];       // dmr_pdu_sf
};

namespace {

constexpr int ROW = 24 * 128; // sizeof(state->dmr_pdu_sf[slot])
constexpr int ROW_CLEARED = 24 * 127; // what dmr_clear_superframe_slot() clears of it
// the status byte of a burst (include/ddn_fsk4.h)
enum { ST_IGNORED = 0, ST_HDR_OK, ST_HDR_CRC, ST_HDR_FEC, ST_FILED, ST_PDU, ST_SEQ_ERR, ST_MBC_LONG, ST_TERMINATOR, ST_MBC_HEADER };
enum { KIND_DATA = 1, KIND_MBC = 2, KIND_UDT = 3 };

struct Slot { // one time slot's scalars, wave-uniform
    int blocks, counter, byte_ctr, fill;
    uint32_t src, tgt;
    int conf, hfmt, hvalid, p_head, sap, poc, udt_res, dbsn_have, dbsn_exp, gi;
};

struct Out {
    uint8_t *pdu_kind, *pdu_slot, *pdu_bytes, *pdu_crc4, *pdu_block_crc;
    int32_t *pdu_burst, *pdu_len, *pdu_header9;
    int max_pdus;
};

__device__ __forceinline__ void
slot_defaults(Slot& s) { // dmr_reset_blocks() / dsd_init.c, all but the row and its fill
    s.blocks = 1, s.counter = 1, s.byte_ctr = 0;
    s.src = 0, s.tgt = 0;
    s.conf = 0, s.hfmt = 7, s.hvalid = 0, s.p_head = 0, s.sap = 0, s.poc = 0, s.udt_res = 0, s.dbsn_have = 0, s.dbsn_exp = 0, s.gi = 0;
}

__device__ __forceinline__ void
row_clear(uint8_t* sf, Slot& s, int lane, bool whole) { // only what was written; dmr_clear_superframe_slot() stops 24 bytes short of the row
    uint32_t* w = reinterpret_cast<uint32_t*>(sf);
    const int end = (whole || s.fill < ROW_CLEARED) ? s.fill : ROW_CLEARED;
    for (int i = lane; i < end / 4; i += 64) {
        w[i] = 0;
    }
    s.fill = end == s.fill ? 0 : s.fill;
    __syncthreads();
}

__device__ __forceinline__ void
valid_clear(uint8_t* v, int lane) {
    reinterpret_cast<uint16_t*>(v)[lane] = 0;
}

// a completed row -> the channel's next PDU slot (the first max_pdus of a call are stored, all are counted)
__device__ __forceinline__ void
pdu_emit(const Out& o, size_t ch, int& np, const uint8_t* sf, const uint8_t* valid, const Slot& s, int slot, int burst, int kind, int n,
         int crc, int hdr_crc, int blk_crc, int pf, int lane) {
    n = n < ROW ? n : ROW;
    if (np < o.max_pdus) {
        const size_t po = ch * (size_t)o.max_pdus + (size_t)np;
        uint32_t* dst = reinterpret_cast<uint32_t*>(o.pdu_bytes + po * 3072);
        const uint32_t* src = reinterpret_cast<const uint32_t*>(sf);
        for (int i = lane; i < 768; i += 64) {
            uint32_t w = 4 * i < n ? src[i] : 0u;
            if (4 * i < n && 4 * i + 4 > n) {
                w &= 0xFFFFFFFFu >> (8 * (4 * i + 4 - n)); // little endian: the bytes at and behind n
            }
            dst[i] = w;
        }
        reinterpret_cast<uint16_t*>(o.pdu_block_crc + po * 128)[lane] = reinterpret_cast<const uint16_t*>(valid)[lane];
        if (lane == 0) {
            o.pdu_kind[po] = (uint8_t)kind;
            o.pdu_slot[po] = (uint8_t)slot;
            o.pdu_burst[po] = burst;
            o.pdu_len[po] = n;
            o.pdu_crc4[po * 4 + 0] = (uint8_t)crc;
            o.pdu_crc4[po * 4 + 1] = (uint8_t)hdr_crc;
            o.pdu_crc4[po * 4 + 2] = (uint8_t)blk_crc;
            o.pdu_crc4[po * 4 + 3] = (uint8_t)pf;
        }
        if (lane < 9) {
            const int32_t h[9] = {s.hfmt, s.sap, s.blocks, s.poc, s.conf, s.p_head, s.gi, (int32_t)s.src, (int32_t)s.tgt};
            o.pdu_header9[po * 9 + lane] = h[lane];
        }
    }
    np++;
}

// dmr_block_assembler(): `lane_byte` is the block's byte number `lane` (lanes >= block_len hold nothing), b0 its first byte
__device__ __forceinline__ int
assemble(const Out& o, size_t ch, int& np, uint8_t* sf, uint8_t* valid, Slot& s, int slot, int burst, uint32_t lane_byte, uint32_t b0,
         int block_len, int typ, int lane) {
    const int bc = s.counter;
    int blocks, is_udt = 0;
    if (typ == 1) {
        blocks = s.blocks - 1;
    } else if (typ == 2) {
        blocks = s.counter;
    } else {
        blocks = s.blocks;
        is_udt = 1;
        typ = 2;
    }
    blocks = blocks < 1 ? 1 : (blocks > 127 ? 127 : blocks);
    int st = ST_FILED, lb = 0;
    if (typ == 1) {
        // dmr_block_type1_append_bytes(): saturates at the row's end
        int ctr = s.byte_ctr < ROW ? s.byte_ctr : ROW;
        if (lane < block_len && ctr + lane < ROW) {
            sf[ctr + lane] = (uint8_t)lane_byte;
        }
        ctr = ctr + block_len < ROW ? ctr + block_len : ROW;
        s.byte_ctr = ctr;
        s.fill = s.fill > ((ctr + 3) & ~3) ? s.fill : ((ctr + 3) & ~3);
        __syncthreads();
        if (s.counter == s.blocks && s.hvalid == 1) {
            // dmr_block_type1_update_crc(): the row in swapped-byte order (dmr_block_type1_pack_crc_bits(), :1127-1155 - its skip of
            // the confirmed blocks' DBSN octets compares an even index with block_len - 1 + offset, odd for every profile: it never
            // fires, and the reference's assembler accepts confirmed rows of 10-, 16- and 22-byte blocks whose trailer was made
            // without it: the recorded sequences of tests/golden/dmr_pdu_vectors.json), ComputeCrc32Bit() over all but the last four
            // bytes against those four; an MNIS header waives it
            uint32_t ext = 0, comp = 0;
            if (ctr >= 4) {
                ext = ((uint32_t)sf[ctr - 4] << 24) | ((uint32_t)sf[ctr - 3] << 16) | ((uint32_t)sf[ctr - 2] << 8) | (uint32_t)sf[ctr - 1];
                comp = ddn_crc::wave_crc(ddn_crc::CRC32, ctr - 4, lane, [&](int j) { return (uint32_t)sf[j ^ 1]; }); // (not inverted)
                comp = __builtin_bswap32(comp);
            }
            const int ok = (comp == ext || (s.hfmt == 0xF && s.sap == 1)) ? 1 : 0;
            pdu_emit(o, ch, np, sf, valid, s, slot, burst, KIND_DATA, ctr, ok, 0, 0, 0, lane);
            st = ST_PDU;
            s.hfmt = 7, s.sap = 0, s.hvalid = 0, s.conf = 0, s.poc = 0, s.byte_ctr = 0; // dmr_block_type1_clear_header_state()
        }
    } else {
        if (s.counter > 4) {
            s.counter = 4;
        }
        const int base = bc * block_len;
        if (lane < block_len && base + lane < ROW) {
            sf[base + lane] = (uint8_t)lane_byte;
        }
        {
            const int end = base + block_len < ROW ? base + block_len : ROW;
            s.fill = s.fill > ((end + 3) & ~3) ? s.fill : ((end + 3) & ~3);
        }
        __syncthreads();
        lb = (int)(b0 >> 7);
        int pf = (int)((b0 >> 6) & 1u);
        if (is_udt) { // dmr_block_type2_set_lb_pf()
            pf = 0;
            if (s.udt_res) { // a reserved block count: the message ends where its CRC16 checks
                lb = 0;
                const int mbytes = bc * 12;
                if (mbytes >= 2) { // (bc <= 5: the reference's 6-block buffer is never short)
                    int n = (1 + bc) * block_len;
                    n = n < ROW ? n : ROW;
                    const int eo = 12 * (1 + bc) - 2;
                    const uint32_t ext = ((eo < n ? (uint32_t)sf[eo] : 0u) << 8) | (eo + 1 < n ? (uint32_t)sf[eo + 1] : 0u);
                    const uint32_t comp = ddn_crc::finish(
                        ddn_crc::CCITT16, ddn_crc::wave_crc(ddn_crc::CCITT16, mbytes - 2, lane, [&](int j) { return 12 + j < n ? (uint32_t)sf[12 + j] : 0u; }));
                    if (comp == ext) {
                        lb = 1;
                        blocks = bc;
                    }
                }
            } else {
                lb = blocks == bc ? 1 : 0;
            }
        }
        if (lb == 1 && s.hvalid == 1) {
            if (!(is_udt || (blocks >= 1 && blocks <= 4))) { // dmr_block_type2_length_ok(): no finalize, the counter stands
                valid[0] = 0;
                __syncthreads();
                return ST_MBC_LONG;
            }
            // dmr_block_type2_unpack_bits() / _update_crc(): five blocks of the row at most are looked at; an MBC's CRC16 runs over
            // three continuation blocks' worth of them whatever its length
            int total = (1 + blocks) * block_len;
            total = total < 60 ? total : 60;
            if (is_udt) {
                pf = total > 9 ? (sf[9] >> 6) & 1 : 0; // bit 73
            }
            const int good0 = valid[0];
            const int eo = 12 * (1 + blocks) - 2;
            const uint32_t ext = ((eo < total ? (uint32_t)sf[eo] : 0u) << 8) | (eo + 1 < total ? (uint32_t)sf[eo + 1] : 0u);
            int limit = is_udt ? 12 * blocks : 36;
            limit = limit < 72 ? limit : 72;
            int nb = blocks * 12 - 2;
            nb = nb < 72 ? nb : 72;
            const uint32_t comp = ddn_crc::finish(
                ddn_crc::CCITT16, ddn_crc::wave_crc(ddn_crc::CCITT16, nb, lane, [&](int j) { return (j < limit && 12 + j < total) ? (uint32_t)sf[12 + j] : 0u; }));
            const int good1 = comp == ext ? 1 : 0;
            pdu_emit(o, ch, np, sf, valid, s, slot, burst, is_udt ? KIND_UDT : KIND_MBC, (1 + blocks) * block_len, good0 & good1, good0, good1,
                     pf, lane);
            st = ST_PDU;
        }
    }
    // dmr_block_assembler_finalize()
    if (typ == 1 && s.counter == s.blocks) {
        __syncthreads();
        row_clear(sf, s, lane, false);
        valid[0] = 0;
        s.counter = 1, s.hfmt = 7, s.sap = 0, s.hvalid = 0, s.conf = 0, s.p_head = 0, s.poc = 0, s.byte_ctr = 0, s.udt_res = 0;
    } else if (typ == 2 && lb == 1) {
        __syncthreads();
        row_clear(sf, s, lane, false);
        valid[0] = 0;
        s.counter = 1, s.hfmt = 7, s.sap = 0, s.hvalid = 0, s.conf = 0, s.p_head = 0, s.udt_res = 0;
    } else {
        s.counter++;
    }
    __syncthreads();
    return st;
}

__global__ __launch_bounds__(64) void
k_dmr_pdu_walk(const int32_t* __restrict__ n_bursts, int max_bursts, const uint8_t* __restrict__ bslot, const uint8_t* __restrict__ btype,
               const uint8_t* __restrict__ bytes12, const uint8_t* __restrict__ info196, const uint32_t* __restrict__ errs,
               const uint8_t* __restrict__ crcflags, const uint8_t* __restrict__ unconf18, const uint8_t* __restrict__ pool,
               const int32_t* __restrict__ pool_n, const int32_t* __restrict__ n_resets, const int32_t* __restrict__ reset_before,
               const int32_t* __restrict__ n_losses, const int32_t* __restrict__ loss_before, int max_marks,
               DdnDmrPduState* __restrict__ state, uint8_t* __restrict__ o_conf, int32_t* __restrict__ o_counter, uint8_t* __restrict__ o_crc,
               uint8_t* __restrict__ o_dbsn, int32_t* __restrict__ o_pick, uint8_t* __restrict__ o_status, Out o, int32_t* __restrict__ n_pdus) {
    const int lane = threadIdx.x;
    const size_t ch = blockIdx.x;
    DdnDmrPduState* S = state + ch;
    Slot sl[2];
    if (S->live) {
        for (int q = 0; q < 2; q++) {
            Slot& s = sl[q];
            s.blocks = S->blocks[q], s.counter = S->counter[q], s.byte_ctr = S->byte_ctr[q], s.fill = S->fill[q];
            s.src = S->src[q], s.tgt = S->tgt[q];
            s.conf = S->conf[q], s.hfmt = S->hfmt[q], s.hvalid = S->hvalid[q], s.p_head = S->p_head[q], s.sap = S->sap[q], s.poc = S->poc[q];
            s.udt_res = S->udt_res[q], s.dbsn_have = S->dbsn_have[q], s.dbsn_exp = S->dbsn_exp[q], s.gi = S->gi[q];
            s.fill = (s.fill < 0 ? 0 : (s.fill > ROW ? ROW : s.fill)) & ~3; // (a block that was not written here must not steer a store)
        }
    } else {
        slot_defaults(sl[0]);
        slot_defaults(sl[1]);
        sl[0].fill = sl[1].fill = 0; // (the block arrives zeroed)
    }
    __syncthreads();
    int nb = n_bursts[ch];
    nb = nb < max_bursts ? nb : max_bursts;
    int nr = n_resets[ch], nl = n_losses[ch];
    nr = nr < max_marks ? nr : max_marks;
    nl = nl < max_marks ? nl : max_marks;
    const int32_t* rb = reset_before + ch * (size_t)max_marks;
    const int32_t* lbf = loss_before + ch * (size_t)max_marks;
    int ir = 0, il = 0, np = 0;

    auto reset_blocks = [&]() { // dmr_reset_blocks(): both time slots
        for (int q = 0; q < 2; q++) {
            row_clear(S->sf[q], sl[q], lane, true);
            valid_clear(S->crc_valid[q], lane);
            slot_defaults(sl[q]);
        }
        __syncthreads();
    };
    auto carrier_loss = [&]() {
        for (int q = 0; q < 2; q++) {
            Slot& s = sl[q];
            row_clear(S->sf[q], s, lane, true);
            valid_clear(S->crc_valid[q], lane);
            s.src = 0, s.tgt = 0, s.gi = 0, s.sap = 0, s.p_head = 0, s.poc = 0, s.byte_ctr = 0, s.hvalid = 0;
            s.blocks = 1, s.hfmt = 7, s.counter = 1;
        }
        __syncthreads();
    };

    for (int k = 0; k <= nb; k++) {
        while (ir < nr && (k == nb || rb[ir] <= k)) {
            reset_blocks();
            ir++;
        }
        while (il < nl && (k == nb || lbf[il] <= k)) {
            carrier_loss();
            il++;
        }
        if (k == nb) {
            break;
        }
        const size_t bo = ch * (size_t)max_bursts + (size_t)k;
        const int slot = bslot[bo] & 1, ty = btype[bo];
        Slot s = sl[slot];
        uint8_t* sf = S->sf[slot];
        uint8_t* valid = S->crc_valid[slot];
        const int conf = s.conf;
        int crc = 0, dbsn = -1, pick = -1, st = ST_IGNORED;
        const int counter_before = s.counter;
        if (ty <= 11) {
            const int is_udt = (ty == 7 && s.hfmt == 0) ? 1 : 0;
            if (!(ty == 6 || ty == 7 || ty == 8 || ty == 10 || ty == 11)) {
                s.p_head = 0;
            }
            const uint8_t* by = bytes12 + bo * 12;
            const int flags = crcflags[bo];
            int bptc_errs = 0, block_len = 12;
            uint32_t lane_byte = lane < 12 ? by[lane] : 0u; // the block the assembler gets, a byte per lane
            if (ty <= 7 || ty == 11) {
                bptc_errs = (int)errs[bo];
                if (ty == 7 && conf == 0) {
                    crc = 1;
                } else if (ty == 7) {
                    dbsn = by[0] >> 1;
                    crc = (flags >> 1) & 1;
                    lane_byte = lane < 10 ? by[2 + lane] : 0u;
                    block_len = 10;
                } else {
                    crc = flags & 1;
                }
                if (ty == 4 || ty == 6) {
                    valid[0] = (uint8_t)crc;
                }
            } else if (ty == 8) {
                if (conf == 0) {
                    crc = 1;
                    block_len = 18;
                    lane_byte = lane < 18 ? unconf18[bo * 18 + lane] : 0u;
                } else {
                    // dmr_dburst_trellis_choose_candidate_index(): a lane per candidate; the first tier that holds one, there the
                    // lowest metric, the first entry on a tie
                    int pn = pool_n[bo];
                    pn = pn < 0 ? 0 : (pn > 34 ? 34 : pn);
                    const uint8_t* e = pool + (bo * 34 + (size_t)(lane < pn ? lane : 0)) * 24;
                    const bool have = lane < pn;
                    const uint32_t metric = have ? *reinterpret_cast<const uint32_t*>(e) : 0u;
                    const bool ok9 = have && e[22] != 0, seq = have && s.dbsn_have && e[23] == s.dbsn_exp;
                    const unsigned long long t0 = __ballot(seq && ok9), t1 = __ballot(ok9), t2 = __ballot(seq && !ok9), t3 = __ballot(have);
                    const unsigned long long tier = t0 ? t0 : (t1 ? t1 : (t2 ? t2 : t3));
                    unsigned long long key = ((tier >> lane) & 1ull) ? ((((unsigned long long)(metric ^ 0x80000000u)) << 8) | (unsigned)lane) : ~0ull;
                    for (int sft = 32; sft >= 1; sft >>= 1) {
                        const unsigned long long other = __shfl_xor(key, sft, 64);
                        key = other < key ? other : key;
                    }
                    pick = tier ? (int)(key & 0xFF) : -1;
                    block_len = 16;
                    if (pick >= 0) {
                        const uint8_t* c = pool + (bo * 34 + (size_t)pick) * 24;
                        dbsn = c[4] >> 1;
                        crc = c[22] ? 1 : 0;
                        lane_byte = lane < 16 ? c[4 + 2 + lane] : 0u;
                    } else { // an empty pool leaves the payload all zeros, whose CRC9 checks
                        dbsn = 0;
                        crc = 1;
                        lane_byte = 0;
                    }
                }
            } else if (ty == 10) {
                // dmr_dburst_handle_full(): the info bits as they are, 96 + 96 of them; confirmed: DBSN(7) | CRC9 | 22 bytes
                const uint8_t* in = info196 + bo * 196;
                const int head = conf ? 10 : 12;
                block_len = head + 12;
                lane_byte = 0;
                if (lane < block_len) {
                    const int b0 = lane < head ? (conf ? 16 : 0) + 8 * lane : 100 + 8 * (lane - head);
                    for (int q = 0; q < 8; q++) {
                        lane_byte = (lane_byte << 1) | (uint32_t)(in[b0 + q] & 1);
                    }
                }
                if (conf == 0) {
                    crc = 1;
                } else {
                    dbsn = 0;
                    for (int q = 0; q < 7; q++) {
                        dbsn = (dbsn << 1) | (in[q] & 1);
                    }
                    crc = (flags >> 1) & 1;
                }
            }
            if (dbsn >= 0 && counter_before >= 0 && counter_before < 127) {
                valid[counter_before] = (uint8_t)crc;
            }
            __syncthreads();
            bool dispatch = true;
            if (dbsn >= 0) { // dmr_dburst_update_dbsn_sequence()
                if (!s.dbsn_have) {
                    if (crc == 1) {
                        s.dbsn_exp = (dbsn + 1) & 0x7F;
                        s.dbsn_have = 1;
                    }
                } else if (crc == 1 && dbsn != s.dbsn_exp) {
                    sl[slot] = s;
                    reset_blocks();
                    s = sl[slot];
                    st = ST_SEQ_ERR;
                    dispatch = false;
                } else if (crc == 1) {
                    s.dbsn_exp = (dbsn + 1) & 0x7F;
                }
            }
            const uint32_t b0 = (uint32_t)__shfl((int)lane_byte, 0, 64);
            if (!dispatch) {
            } else if (ty == 2) {
                if (bptc_errs == 0 && (by[0] >> 7) == 0 && (by[0] & 0x3F) == 0x30) { // a readable TD_LC ends the data session
                    s.hfmt = 7, s.sap = 0, s.hvalid = 0, s.conf = 0, s.poc = 0, s.byte_ctr = 0;
                    st = ST_TERMINATOR;
                }
            } else if (ty == 4) {
                s.counter = 0;
                s.hvalid = 1;
                st = assemble(o, ch, np, sf, valid, s, slot, k, lane_byte, b0, 12, 2, lane);
                st = st == ST_FILED ? ST_MBC_HEADER : st;
            } else if (ty == 5) {
                st = assemble(o, ch, np, sf, valid, s, slot, k, lane_byte, b0, 12, 2, lane);
            } else if (ty == 6) { // dmr_dheader()
                const int inherited = s.poc;
                row_clear(sf, s, lane, false);
                s.counter = 1;
                s.poc = 0;
                if (bptc_errs != 0) { // dmr_dheader_reset_irrecoverable()
                    s.hvalid = 0, s.p_head = 0, s.conf = 0, s.counter = 1, s.blocks = 1, s.hfmt = 7;
                    st = ST_HDR_FEC;
                } else if (crc != 1) {
                    st = ST_HDR_CRC;
                } else {
                    s.dbsn_have = 0;
                    s.dbsn_exp = 0;
                    const int h0 = by[0], h1 = by[1], h8 = by[8];
                    const int gi = h0 >> 7, a = (h0 >> 6) & 1, dpf = h0 & 0xF;
                    int sap = h1 >> 4;
                    const int poc = (h1 & 0xF) + (((h0 >> 4) & 1) << 4), s_ab_fin = (((h0 >> 4) & 3) << 4) | (h1 & 0xF);
                    const int udt_format = h1 & 0xF, udt_uab = (h8 & 3) + 1, p_sap = h0 >> 4, p_mfid = h1;
                    if (dpf != 15) {
                        s.tgt = ((uint32_t)by[2] << 16) | ((uint32_t)by[3] << 8) | by[4];
                        s.src = ((uint32_t)by[5] << 16) | ((uint32_t)by[6] << 8) | by[7];
                        s.gi = gi;
                    } else {
                        s.gi = 0;
                    }
                    s.poc = (dpf == 2 || dpf == 3) ? poc : (dpf == 15 ? inherited : 0);
                    s.hfmt = dpf;
                    s.udt_res = (dpf == 0 && udt_format == 5 && udt_uab == 3) ? 1 : 0;
                    if (dpf == 0) { // dmr_dheader_handle_udt(): the header is the message's block 0
                        s.blocks = udt_uab;
                        s.hvalid = 1;
                        s.counter = 0;
                        (void)assemble(o, ch, np, sf, valid, s, slot, k, lane_byte, b0, 12, 3, lane);
                    } else if (dpf == 2 || dpf == 3) {
                        s.blocks = h8 & 0x7F;
                        s.conf = dpf == 3 ? 1 : s.conf;
                    } else if (dpf == 13 || dpf == 14) {
                        s.blocks = s_ab_fin ? s_ab_fin : s.blocks;
                        s.conf = a == 1 ? 1 : s.conf;
                    } else if (dpf == 15) {
                        if (p_mfid == 0x10 && p_sap == 1) { // dmr_dheader_handle_moto_p_head(): ten bytes of the MNIS header open the row
                            if (lane < 10) {
                                sf[lane] = (uint8_t)lane_byte;
                            }
                            s.fill = s.fill > 12 ? s.fill : 12;
                            s.counter++;
                            s.byte_ctr = 10;
                            s.p_head = 1;
                            __syncthreads();
                        } else {
                            s.blocks = s.blocks > 1 ? s.blocks - 1 : s.blocks;
                            s.byte_ctr = 0;
                        }
                        sap = p_sap;
                    }
                    if (dpf != 15) {
                        s.byte_ctr = 0; // dmr_dheader_reset_non_extended()
                    }
                    s.blocks = s.blocks > 127 ? 127 : (s.blocks < 1 ? 1 : s.blocks);
                    if (dpf != 15) {
                        s.hvalid = 1;
                    }
                    s.sap = sap;
                    st = ST_HDR_OK;
                }
            } else if (ty == 7) {
                st = assemble(o, ch, np, sf, valid, s, slot, k, lane_byte, b0, block_len, is_udt ? 3 : 1, lane);
            } else if (ty == 8 || ty == 10) {
                st = assemble(o, ch, np, sf, valid, s, slot, k, lane_byte, b0, block_len, 1, lane);
            }
        }
        sl[slot] = s;
        if (lane == 0) {
            o_conf[bo] = (uint8_t)conf;
            o_counter[bo] = counter_before;
            o_crc[bo] = (uint8_t)crc;
            o_dbsn[bo] = (uint8_t)(dbsn >= 0 ? dbsn : 0xFF);
            o_pick[bo] = pick;
            o_status[bo] = (uint8_t)st;
        }
    }
    // behind the call's last burst: unused entries read as such
    for (int k = nb + lane; k < max_bursts; k += 64) {
        const size_t bo = ch * (size_t)max_bursts + (size_t)k;
        o_conf[bo] = 0;
        o_counter[bo] = 0;
        o_crc[bo] = 0;
        o_dbsn[bo] = 0xFF;
        o_pick[bo] = -1;
        o_status[bo] = ST_IGNORED;
    }
    if (lane == 0) {
        n_pdus[ch] = np;
        S->live = 1;
    }
    if (lane < 2) {
        const Slot s = sl[lane];
        const int q = lane;
        S->blocks[q] = s.blocks, S->counter[q] = s.counter, S->byte_ctr[q] = s.byte_ctr, S->fill[q] = s.fill;
        S->src[q] = s.src, S->tgt[q] = s.tgt;
        S->conf[q] = (uint8_t)s.conf, S->hfmt[q] = (uint8_t)s.hfmt, S->hvalid[q] = (uint8_t)s.hvalid, S->p_head[q] = (uint8_t)s.p_head;
        S->sap[q] = (uint8_t)s.sap, S->poc[q] = (uint8_t)s.poc, S->udt_res[q] = (uint8_t)s.udt_res, S->dbsn_have[q] = (uint8_t)s.dbsn_have;
        S->dbsn_exp[q] = (uint8_t)s.dbsn_exp, S->gi[q] = (uint8_t)s.gi;
    }
}

// One wavefront per channel.  Resets: lane = event of the current chunk of 64; a reset's place = the dispatched bursts ahead of it in
// the event list.  Carrier loss: lane = symbol of the current chunk of the call's new flags; the run of symbols that are neither in
// frame nor a sync is carried in the state, and every 1800th of a run is a loss (the loop restarts its count there), placed by
// position among the bursts' last symbols.
__global__ __launch_bounds__(64) void
k_dmr_pdu_marks(const int32_t* __restrict__ events, const int32_t* __restrict__ n_events, int max_events, const uint8_t* __restrict__ flags,
                size_t stride, int carry, const int32_t* __restrict__ n_new, const int32_t* __restrict__ dstart, const int32_t* __restrict__ dn,
                int max_bursts, DdnDmrPduState* __restrict__ state, int32_t* __restrict__ reset_before, int32_t* __restrict__ n_resets,
                int32_t* __restrict__ loss_before, int32_t* __restrict__ n_losses, int max_marks) {
    const int ch = blockIdx.x, lane = threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    int nbursts = 0, nr = 0;
    const int ne = n_events[ch] < max_events ? n_events[ch] : max_events;
    for (int base = 0; base < ne; base += 64) {
        const int i = base + lane;
        int4 e = make_int4(0, 0, 0, 0);
        if (i < ne) {
            e = *reinterpret_cast<const int4*>(events + ((size_t)ch * max_events + i) * 4);
        }
        const int b = (int)(int16_t)(e.w & 0xFFFF), c = e.w >> 16;
        const bool burst = i < ne && e.y == 6 && (e.w & 0xFFFF) == 0;
        const bool reset = i < ne && ((e.y == 5 && (e.z == 0 || ((c >> 8) & 1))) || (e.y == 8 && (b != 1 || c != 1)));
        const unsigned long long mb = __ballot(burst), mr = __ballot(reset);
        const int k = nr + __popcll(mr & below);
        if (reset && k < max_marks) {
            reset_before[(size_t)ch * max_marks + k] = nbursts + __popcll(mb & below);
        }
        nbursts += __popcll(mb);
        nr += __popcll(mr);
    }
    int run = state[ch].hunted, nl = 0;
    run = run < 0 ? 0 : (run > 1799 ? 1799 : run);
    int nd = dn[ch];
    nd = nd < max_bursts ? nd : max_bursts;
    const int end = (size_t)(carry + n_new[ch]) < stride ? carry + n_new[ch] : (int)stride;
    for (int base = carry; base < end; base += 64) {
        const int i = base + lane;
        const bool busy = i < end && (flags[(size_t)ch * stride + (size_t)i] & 3) != 0;
        const int valid = end - base < 64 ? end - base : 64;
        const unsigned long long m = __ballot(busy) & (valid == 64 ? ~0ull : ((1ull << valid) - 1ull));
        // a run can only reach 1800 in the quiet symbols that open the chunk: behind a busy one it starts again, 63 at the most
        const int lead = m ? __builtin_ctzll(m) : valid;
        if (run + lead >= 1800) {
            const int pos = base + (1800 - run) - 1; // the run's 1800th symbol
            int before = 0;
            for (int j = lane; j < nd; j += 64) {
                before += dstart[(size_t)ch * max_bursts + j] + 143 < pos ? 1 : 0;
            }
            for (int sft = 32; sft >= 1; sft >>= 1) {
                before += __shfl_xor(before, sft, 64);
            }
            if (lane == 0 && nl < max_marks) {
                loss_before[(size_t)ch * max_marks + nl] = before;
            }
            nl++;
            run -= 1800;
        }
        run += lead;
        if (m) { // the quiet symbols behind the chunk's last busy one
            run = valid - 1 - (63 - __builtin_clzll(m));
        }
    }
    if (lane == 0) {
        state[ch].hunted = run;
        n_resets[ch] = nr < max_marks ? nr : max_marks;
        n_losses[ch] = nl < max_marks ? nl : max_marks;
    }
}
} // namespace

extern "C" size_t
ddn_dev_dmr_pdu_state_bytes(void) {
    return sizeof(DdnDmrPduState);
}

extern "C" hipError_t
ddn_dev_dmr_pdu_walk(const int32_t* n_bursts, int n_channels, int max_bursts, const uint8_t* bslot, const uint8_t* btype, const uint8_t* bytes12,
                     const uint8_t* info196, const uint32_t* errs, const uint8_t* crcflags, const uint8_t* unconf18, const void* pool,
                     const int32_t* pool_n, const int32_t* n_resets, const int32_t* reset_before, const int32_t* n_losses,
                     const int32_t* loss_before, int max_marks, void* state, uint8_t* o_conf, int32_t* o_counter, uint8_t* o_crc, uint8_t* o_dbsn,
                     int32_t* o_pick, uint8_t* o_status, uint8_t* pdu_kind, uint8_t* pdu_slot, int32_t* pdu_burst, int32_t* pdu_len,
                     uint8_t* pdu_bytes, uint8_t* pdu_crc4, uint8_t* pdu_block_crc, int32_t* pdu_header9, int max_pdus, int32_t* n_pdus,
                     hipStream_t st) {
    Out o;
    o.pdu_kind = pdu_kind, o.pdu_slot = pdu_slot, o.pdu_bytes = pdu_bytes, o.pdu_crc4 = pdu_crc4, o.pdu_block_crc = pdu_block_crc;
    o.pdu_burst = pdu_burst, o.pdu_len = pdu_len, o.pdu_header9 = pdu_header9, o.max_pdus = max_pdus;
    hipLaunchKernelGGL(k_dmr_pdu_walk, dim3((unsigned)n_channels), dim3(64), 0, st, n_bursts, max_bursts, bslot, btype, bytes12, info196, errs,
                       crcflags, unconf18, (const uint8_t*)pool, pool_n, n_resets, reset_before, n_losses, loss_before, max_marks,
                       (DdnDmrPduState*)state, o_conf, o_counter, o_crc, o_dbsn, o_pick, o_status, o, n_pdus);
    return hipGetLastError();
}

extern "C" hipError_t
ddn_dev_dmr_pdu_marks(const int32_t* events, const int32_t* n_events, int max_events, const uint8_t* flags, size_t stride, int carry,
                      const int32_t* n_new, const int32_t* dstart, const int32_t* dn, int n_channels, int max_bursts, void* state,
                      int32_t* reset_before, int32_t* n_resets, int32_t* loss_before, int32_t* n_losses, int max_marks, hipStream_t st) {
    hipLaunchKernelGGL(k_dmr_pdu_marks, dim3((unsigned)n_channels), dim3(64), 0, st, events, n_events, max_events, flags, stride, carry, n_new,
                       dstart, dn, max_bursts, (DdnDmrPduState*)state, reset_before, n_resets, loss_before, n_losses, max_marks);
    return hipGetLastError();
}
