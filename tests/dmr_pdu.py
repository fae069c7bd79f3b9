"""The DMR protocol layer between a dispatched data burst and a completed PDU, restated: what dmr_data_burst_handler()
(src/protocol/dmr/dmr_dburst.c:812-845) does with the burst's FEC-level results under the running state of dsd_state - the profile
(:105-174), crc_correct and data_block_crc_valid, the rate 3/4 candidate pick against the expected DBSN (:428-468), the DBSN sequence
(:651-680), dmr_dheader() (src/protocol/dmr/dmr_block.c:557-618), dmr_block_assembler() (:1052-1710), the data terminator
(dmr_flco.c:319-333), dmr_reset_blocks() (dmr_block.c:1714-1748) and the carrier-loss reset (src/engine/engine.c:1957-2000,2041-2063).
Default options only: aggressive_framesync = 1, dmr_crc_relaxed_default = 0, no branding.  TEST INFRASTRUCTURE - the product never
imports this.

The input is a list of bursts in air order - dicts as tests/dmr_data.data_burst() makes them, with a "slot" - and marks: (index of
the burst the mark precedes, kind) with kind 0 = dmr_reset_blocks(), 1 = carrier loss; marks_of() reads them off the oracle loop's
event rows and flags."""
import numpy as np

ROW = 24 * 128          # sizeof(state->dmr_pdu_sf[slot])
ROW_CLEARED = 24 * 127  # what dmr_clear_superframe_slot() clears of it

# status byte of a burst
ST_IGNORED, ST_HDR_OK, ST_HDR_CRC, ST_HDR_FEC, ST_FILED, ST_PDU, ST_SEQ_ERR, ST_MBC_LONG, ST_TERMINATOR, ST_MBC_HEADER = range(10)
KIND_DATA, KIND_MBC, KIND_UDT = 1, 2, 3


def crc_ccitt16_bits(bits):
    """dsd_crc_ccitt16_bits() (src/core/util/bit_packing.c:141-155)"""
    crc = 0
    for b in bits:
        fb = ((crc >> 15) & 1) ^ (int(b) & 1)
        crc = (crc << 1) & 0xFFFF
        if fb:
            crc ^= 0x1021
    return crc ^ 0xFFFF


def crc32_bits(bits):
    """ComputeCrc32Bit() (src/protocol/dmr/dmr_utils.c:454-483): the remainder with its four bytes reversed"""
    crc = 0
    for b in bits:
        if ((crc >> 31) & 1) ^ (int(b) & 1):
            crc = ((crc << 1) ^ 0x04C11DB7) & 0xFFFFFFFF
        else:
            crc = (crc << 1) & 0xFFFFFFFF
    return int.from_bytes(crc.to_bytes(4, "big"), "little")


def crc9_ok_zero():
    """a pool that is empty leaves trellis_return all zeros: ComputeCrc9Bit of zeros is 0x1FF, the extracted CRC 0 ^ 0x1FF"""
    return 1


def type1_crc_bits(sf, block_len, ctr, offset, conf):
    """dmr_block_type1_update_crc() (:1157-1180): the row's bits, then dmr_block_type1_pack_crc_bits() (:1127-1155) over them, as
    written - the confirmed-block skip compares an even index with block_len - 1 + offset, which is odd for every profile"""
    bits = list(np.unpackbits(np.asarray(sf[:ctr], np.uint8))) + [0] * 16
    i, j = 0, 0
    while i < ctr:
        if i + 1 < ctr:
            bits[j:j + 8] = [(int(sf[i + 1]) >> (7 - q)) & 1 for q in range(8)]
        bits[j + 8:j + 16] = [(int(sf[i]) >> (7 - q)) & 1 for q in range(8)]
        if i == block_len - 1 + offset and conf == 1:
            i += 2
        i += 2
        j += 16
    return bits


# dmr_dburst_profile_resolve() (:105-174): data type -> (CRC mask, CRC length, PDU length), then what the state changes of it
PROFILES = {0: (0x6969, 16, 12), 1: (0x969696, 24, 12), 2: (0x999999, 24, 12), 3: (0xA5A5, 16, 12), 4: (0xAAAA, 16, 12), 5: (0, 0, 12),
            6: (0xCCCC, 16, 12), 7: (0x0F0, 9, 12), 8: (0x1FF, 9, 18), 9: (0, 0, 0), 10: (0x10F, 9, 24), 11: (0x3333, 16, 12)}


def profile(ty, conf, hfmt):
    """-> dict(crcmask, crclen, pdu_len, pdu_start, udt) for data types 0 .. 11"""
    mask, crclen, n = PROFILES[ty]
    start = 0
    if ty in (7, 8, 10) and conf == 1:
        n, start = n - 2, 2
    return dict(crcmask=mask, crclen=crclen, pdu_len=n, pdu_start=start, udt=int(ty == 7 and hfmt == 0))


def choose_candidate(pool, have, expected):
    """dmr_dburst_trellis_choose_candidate_index() (:428-468) over [(bytes18, metric, crc_ok, dbsn)] -> index (-1: empty pool)"""
    best = [-1, -1, -1, -1]          # crc + dbsn, crc, dbsn, any

    def lower(cur, ci):
        return ci if cur < 0 or pool[ci][1] < pool[cur][1] else cur
    for ci, (_, _, ok, dbsn) in enumerate(pool):
        best[3] = lower(best[3], ci)
        if have and dbsn == expected:
            if ok:
                best[0] = lower(best[0], ci)
            else:
                best[2] = lower(best[2], ci)
        if ok:
            best[1] = lower(best[1], ci)
    for b in best:
        if b >= 0:
            return b
    return -1


class Slot:
    def __init__(self):
        self.conf = self.hvalid = self.p_head = self.sap = self.poc = self.udt_res = self.dbsn_have = self.dbsn_exp = 0
        self.gi = self.src = self.tgt = self.byte_ctr = 0
        self.hfmt, self.blocks, self.counter = 7, 1, 1
        self.crc_valid = np.zeros(127, np.uint8)
        self.sf = np.zeros(ROW, np.uint8)


class Walk:
    """one channel's state; burst() -> the per-burst outputs, completed PDUs collect in .pdus"""

    def __init__(self):
        self.s = [Slot(), Slot()]
        self.pdus = []
        self.k = 0                   # index of the burst at hand (a PDU names the burst that completed it)

    def reset_blocks(self):
        self.s = [Slot(), Slot()]

    def carrier_loss(self):
        """no_carrier_reset_dmr_data_blocks() + no_carrier_reset_dmr_misc_state(): data_conf_data, the DBSN expectation and
        udt_uab_reserved stand"""
        for s in self.s:
            s.src = s.tgt = s.gi = s.sap = s.p_head = s.poc = s.byte_ctr = s.hvalid = 0
            s.blocks, s.hfmt, s.counter = 1, 7, 1
            s.sf[:] = 0
            s.crc_valid[:] = 0

    def mark(self, kind):
        (self.carrier_loss if kind else self.reset_blocks)()

    def _set_valid(self, s, idx, v):
        if 0 <= idx < 127:           # (the reference indexes [127] with an unbounded int: past it nothing is modelled)
            s.crc_valid[idx] = v

    def _emit(self, s, slot, kind, n, crc, hdr_crc, blk_crc, pf, snap):
        n = min(n, ROW)
        by = np.zeros(ROW, np.uint8)
        by[:n] = s.sf[:n]
        self.pdus.append(dict(kind=kind, slot=slot, burst=self.k, n=n, bytes=by, crc=int(crc), hdr_crc=int(hdr_crc), blk_crc=int(blk_crc),
                              pf=int(pf), valid=s.crc_valid.copy(), **snap))

    def _snap(self, s):
        return dict(dpf=s.hfmt, sap=s.sap, blocks=s.blocks, poc=s.poc, confirmed=s.conf, p_head=s.p_head, gi=s.gi, source=s.src, target=s.tgt)

    def _assemble(self, slot, block, block_len, typ):
        """dmr_block_assembler() -> status"""
        s = self.s[slot]
        block = [int(x) for x in block[:block_len]]
        bc = s.counter
        is_udt = 0
        if typ == 1:
            blocks = s.blocks - 1
        elif typ == 2:
            blocks = s.counter
        else:
            blocks, is_udt, typ = s.blocks, 1, 2
        blocks = max(1, min(127, blocks))
        st = ST_FILED
        lb = 0
        if typ == 1:
            offset = 12 if s.p_head == 1 else 0
            ctr = min(s.byte_ctr, ROW)
            for b in block:
                if ctr < ROW:
                    s.sf[ctr] = b
                    ctr += 1
            s.byte_ctr = ctr
            if s.counter == s.blocks and s.hvalid == 1:
                ext = int.from_bytes(bytes(s.sf[ctr - 4:ctr]), "big") if ctr >= 4 else 0
                bits = type1_crc_bits(s.sf, block_len, ctr, offset, s.conf)
                comp = crc32_bits(bits[:ctr * 8 - 32] if ctr >= 4 else [])
                ok = comp == ext or (s.hfmt == 0xF and s.sap == 1)
                self._emit(s, slot, KIND_DATA, ctr, ok, 0, 0, 0, self._snap(s))
                st = ST_PDU
                s.hfmt, s.sap, s.hvalid, s.conf, s.poc, s.byte_ctr = 7, 0, 0, 0, 0, 0       # dmr_block_type1_clear_header_state()
        else:
            if s.counter > 4:
                s.counter = 4
            base = bc * block_len
            for i, b in enumerate(block):
                if base + i < ROW:
                    s.sf[base + i] = b
            lb, pf = block[0] >> 7, (block[0] >> 6) & 1
            if is_udt:
                pf = 0
                if s.udt_res:
                    lb = 0
                    mbits = bc * 96
                    if mbits >= 16:
                        mbits = min(mbits, 576)
                        n = min((1 + bc) * block_len, ROW)
                        bits = list(np.unpackbits(s.sf[:n])) + [0] * (96 * (2 + bc))
                        ext = int("".join(str(int(x)) for x in bits[96 * (1 + bc) - 16:96 * (1 + bc)]), 2)
                        if crc_ccitt16_bits(bits[96:96 + mbits - 16]) == ext:
                            lb, blocks = 1, bc
                else:
                    lb = 1 if blocks == bc else 0
            if lb == 1 and s.hvalid == 1:
                if not (is_udt or 1 <= blocks <= 4):
                    s.crc_valid[0] = 0
                    return ST_MBC_LONG                      # (no finalize: the block counter stands)
                total = min((1 + blocks) * block_len, 60)
                bits = list(np.unpackbits(s.sf[:total])) + [0] * (96 * (2 + blocks))
                if is_udt:
                    pf = bits[73]
                good0 = int(s.crc_valid[0])
                ext = int("".join(str(int(x)) for x in bits[96 * (1 + blocks) - 16:96 * (1 + blocks)]), 2)
                limit = min(96 * blocks, 576) if is_udt else 288
                mbc = bits[96:96 + limit] + [0] * (576 - limit)
                nbits = min(max(blocks * 96 - 16, 0), 576)
                good1 = int(crc_ccitt16_bits(mbc[:nbits]) == ext)
                self._emit(s, slot, KIND_UDT if is_udt else KIND_MBC, (1 + blocks) * block_len, good0 and good1, good0, good1, pf, self._snap(s))
                st = ST_PDU
        # dmr_block_assembler_finalize()
        if typ == 1 and s.counter == s.blocks:
            s.sf[:ROW_CLEARED] = 0
            s.crc_valid[0] = 0
            s.counter, s.hfmt, s.sap, s.hvalid, s.conf, s.p_head, s.poc, s.byte_ctr, s.udt_res = 1, 7, 0, 0, 0, 0, 0, 0, 0
        elif typ == 2 and lb == 1:
            s.sf[:ROW_CLEARED] = 0
            s.crc_valid[0] = 0
            s.counter, s.hfmt, s.sap, s.hvalid, s.conf, s.p_head, s.udt_res = 1, 7, 0, 0, 0, 0, 0
        else:
            s.counter += 1
        return st

    def _dheader(self, slot, by, crc, errs):
        s = self.s[slot]
        inherited = s.poc
        s.sf[:ROW_CLEARED] = 0
        s.counter, s.poc = 1, 0
        if errs != 0:
            s.hvalid = s.p_head = s.conf = 0
            s.counter, s.blocks, s.hfmt = 1, 1, 7
            return ST_HDR_FEC
        if crc != 1:
            return ST_HDR_CRC
        s.dbsn_have = s.dbsn_exp = 0
        b = [int(x) for x in by]
        gi, a, dpf, sap = b[0] >> 7, (b[0] >> 6) & 1, b[0] & 0xF, b[1] >> 4
        poc = (b[1] & 0xF) + (((b[0] >> 4) & 1) << 4)
        s_ab_fin = (((b[0] >> 4) & 3) << 4) | (b[1] & 0xF)
        udt_format, udt_uab = b[1] & 0xF, (b[8] & 3) + 1
        p_sap, p_mfid = b[0] >> 4, b[1]
        if dpf != 15:
            s.src, s.tgt, s.gi = (b[5] << 16) | (b[6] << 8) | b[7], (b[2] << 16) | (b[3] << 8) | b[4], gi
        else:
            s.gi = 0
        if dpf in (2, 3):
            s.poc = poc
        elif dpf == 15:
            s.poc = inherited
        s.hfmt = dpf
        s.udt_res = int(dpf == 0 and udt_format == 5 and udt_uab == 3)
        if dpf == 0:
            s.blocks, s.hvalid, s.counter = udt_uab, 1, 0
            self._assemble(slot, by, 12, 3)
        elif dpf in (2, 3):
            s.blocks = b[8] & 0x7F
            if dpf == 3:
                s.conf = 1
        elif dpf in (13, 14):
            if s_ab_fin:
                s.blocks = s_ab_fin
            if a == 1:
                s.conf = 1
        elif dpf == 15:
            if p_mfid == 0x10 and p_sap == 1:
                s.sf[:10] = by[:10]
                s.counter += 1
                s.byte_ctr, s.p_head = 10, 1
            else:
                if s.blocks > 1:
                    s.blocks -= 1
                s.byte_ctr = 0
            sap = p_sap
        if dpf != 15:
            s.byte_ctr = 0
        s.blocks = max(1, min(127, s.blocks))
        if dpf != 15:
            s.hvalid = 1
        s.sap = sap
        return ST_HDR_OK

    def burst(self, x):
        """-> dict(conf, counter, crc, dbsn, pick, status)"""
        slot, ty = x["slot"] & 1, x["type"]
        s = self.s[slot]
        out = dict(conf=s.conf, counter=s.counter, crc=0, dbsn=0xFF, pick=-1, status=ST_IGNORED)
        if ty > 11:                  # no slot type: nothing of it is modelled
            self.k += 1
            return out
        conf = s.conf
        is_udt = ty == 7 and s.hfmt == 0
        if ty not in (6, 7, 8, 10, 11):
            s.p_head = 0
        by = np.asarray(x["bytes12"], np.uint8)
        flags = int(x["crc"])
        dbsn, crc, pdu, errs = None, 0, by, 0
        if ty in (0, 1, 2, 3, 4, 5, 6, 7, 11):
            errs = int(x["errs"])
            if ty == 7 and conf == 0:
                crc = 1
            elif ty == 7:
                dbsn, crc = int(by[0]) >> 1, (flags >> 1) & 1
                self._set_valid(s, s.counter, crc)
                pdu = by[2:12]
            else:
                crc = flags & 1
            if ty in (4, 6):
                s.crc_valid[0] = crc
        elif ty == 8:
            if conf == 0:
                pdu, crc = np.asarray(x["unconfirmed"], np.uint8), 1
            else:
                pool = x["pool"]
                ci = choose_candidate(pool, s.dbsn_have, s.dbsn_exp)
                out["pick"] = ci
                b18 = np.asarray(pool[ci][0], np.uint8) if ci >= 0 else np.zeros(18, np.uint8)
                crc = int(pool[ci][2]) if ci >= 0 else crc9_ok_zero()
                dbsn = int(b18[0]) >> 1
                self._set_valid(s, s.counter, crc)
                pdu = b18[2:18]
        elif ty == 10:
            info = np.asarray(x["info"], np.uint8)
            if conf == 0:
                pdu, crc = np.packbits(np.concatenate([info[0:96], info[100:196]])), 1
            else:
                dbsn = int("".join(str(int(v)) for v in info[0:7]), 2)
                crc = (flags >> 1) & 1
                self._set_valid(s, s.counter, crc)
                pdu = np.packbits(np.concatenate([info[16:96], info[100:196]]))
        out["crc"] = crc
        if dbsn is not None:
            out["dbsn"] = dbsn
            # dmr_dburst_update_dbsn_sequence()
            if not s.dbsn_have:
                if crc == 1:
                    s.dbsn_exp, s.dbsn_have = (dbsn + 1) & 0x7F, 1
            else:
                if crc == 1 and dbsn != s.dbsn_exp:
                    self.reset_blocks()
                    out["status"] = ST_SEQ_ERR
                    self.k += 1
                    return out
                if crc == 1:
                    s.dbsn_exp = (dbsn + 1) & 0x7F
        if ty == 2:
            if errs == 0 and (int(by[0]) >> 7) == 0 and (int(by[0]) & 0x3F) == 0x30:          # a readable TD_LC
                s.hfmt, s.sap, s.hvalid, s.conf, s.poc, s.byte_ctr = 7, 0, 0, 0, 0, 0
                out["status"] = ST_TERMINATOR
        elif ty == 4:
            s.counter, s.hvalid = 0, 1
            st = self._assemble(slot, by, 12, 2)
            out["status"] = ST_MBC_HEADER if st == ST_FILED else st
        elif ty == 5:
            out["status"] = self._assemble(slot, by, 12, 2)
        elif ty == 6:
            out["status"] = self._dheader(slot, by, crc, errs)
        elif ty == 7:
            out["status"] = self._assemble(slot, pdu, len(pdu), 3 if is_udt else 1)
        elif ty in (8, 10):
            out["status"] = self._assemble(slot, pdu, len(pdu), 1)
        self.k += 1
        return out


def walk(bursts, marks=(), state=None):
    """bursts in air order, marks [(before, kind)] sorted by `before` -> (per-burst outputs, completed PDUs, the state after)"""
    w = state or Walk()
    w.pdus, w.k = [], 0
    marks = list(marks)
    outs, m = [], 0
    for k, x in enumerate(bursts):
        while m < len(marks) and marks[m][0] <= k:
            w.mark(marks[m][1])
            m += 1
        outs.append(w.burst(x))
    for _, kind in marks[m:]:
        w.mark(kind)
    return outs, w.pdus, w


def marks_of(events, flags, burst_pos):
    """the oracle loop's event rows [(pos, kind, a, b, c)] and flags -> marks [(before, kind)]: dmr_reset_blocks() at a kind-5 event
    whose slot type or TACT failed or that the colour-code gate rejected (dmr_data_finalize(), dmr_data.c:292-299) and at a kind-8
    voice end with a failed TACT or EMB / sync (dmr_bs.c:671-680,937-947), in event order between the dispatched bursts; carrier loss
    where 1800 symbols in a row carry no flag (the loop restarts its count there), placed by position among the bursts' last symbols"""
    marks, nb = [], 0
    for (pos, kind, a, b, c) in events:
        if kind == 6 and b == 0:
            nb += 1
        elif kind == 5 and (a == 0 or (c >> 8) & 1):
            marks.append((nb, 0))
        elif kind == 8 and (b != 1 or c != 1):
            marks.append((nb, 0))
    busy = (np.asarray(flags) & 3) != 0
    run = 0
    pos = np.asarray(burst_pos, np.int64)
    for i, f in enumerate(busy):
        run = 0 if f else run + 1
        if run == 1800:
            marks.append((int(np.searchsorted(pos, i, side="left")), 1))
            run = 0
    return sorted(marks, key=lambda t: t[0])


def stream_reference(w, events):
    """the oracle loop's whole-stream output and event rows -> (positions of the dispatched bursts' last symbols, their FEC-level
    dicts, marks, per-burst outputs, completed PDUs): tests/dmr_data.stream_expectation, marks_of and walk in a row"""
    import dmr_data
    data, _ = dmr_data.stream_expectation(w, events)
    pos = [p for p, _, _ in data]
    bursts = []
    for _, slot, x in data:
        b = dict(slot=slot, unconfirmed=np.zeros(18, np.uint8), pool=[])
        b.update(x)
        bursts.append(b)
    marks = marks_of(events, w["fl"], pos)
    outs, pdus, _ = walk(bursts, marks)
    return pos, bursts, marks, outs, pdus
