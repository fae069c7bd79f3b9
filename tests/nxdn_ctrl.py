"""CPU restatement of the NXDN control and data channels (include/ddn_fsk4.h, "NXDN control and data channels"; kernels in
dsd-neo_amd/csrc/ddn_nxdn_ctrl.hip): CAC, FACCH2 / UDCH and the SACCH state machine, as plain code over one frame's 182 dibits and
reliabilities.  The two decoders are the pinned ones (fecgen.oracle_nxdn = CNXDNConvolution soft, rx4.oracle_trellis_decode =
trellis_decode); everything else restates what the reference does (read, not copied):

  src/protocol/nxdn/nxdn_frame.c:117-160 (LICH profiles), :237-263 (profile miss), :311-346 (bit windows), :488-494 (non-superframe)
  nxdn_deperm.c:112-119,164-205 (de-permutation, de-puncture, soft decode + hard retry), :245-340 (SACCH), :496-530 (FACCH2 / UDCH),
  :610-634 (CAC), :1263-1275 (crc16cac), :1299-1372; nxdn_dcr_utils.c:44-106 (crc15, sequence rule); nxdn_element.c:158-200

TEST INFRASTRUCTURE - the product never imports this."""
import numpy as np

import rx4

KIND_NONE, KIND_CAC, KIND_FACCH2, KIND_UDCH = 0, 1, 2, 3
# k_nxdn_lich_profiles: every LICH of the table, those whose frame carries a SACCH, and the channels decoded here
LICH_PROFILE = frozenset([0x01, 0x05, 0x28, 0x29, 0x49, 0x2E, 0x2F, 0x4E, 0x4F, 0x32, 0x33, 0x52, 0x53, 0x34, 0x35, 0x54, 0x55, 0x36, 0x37,
                          0x56, 0x57, 0x20, 0x21, 0x30, 0x31, 0x40, 0x41, 0x50, 0x51, 0x38, 0x39, 0x46, 0x08, 0x48, 0x4A, 0x76, 0x77, 0x75,
                          0x72, 0x73, 0x70, 0x71, 0x6E, 0x6F, 0x68, 0x69, 0x62, 0x63, 0x60, 0x61])
LICH_SACCH = frozenset([0x32, 0x33, 0x52, 0x53, 0x34, 0x35, 0x54, 0x55, 0x36, 0x37, 0x56, 0x57, 0x20, 0x21, 0x30, 0x31, 0x40, 0x41, 0x50,
                        0x51, 0x38, 0x39])
LICH_KIND = {0x01: KIND_CAC, 0x05: KIND_CAC, 0x28: KIND_FACCH2, 0x29: KIND_FACCH2, 0x49: KIND_FACCH2, 0x2E: KIND_UDCH, 0x2F: KIND_UDCH,
             0x4E: KIND_UDCH, 0x4F: KIND_UDCH}
LICH_NON_SUPERFRAME = frozenset([0x20, 0x21, 0x61, 0x40, 0x41])
# kind -> (interleaver columns N, air bits, decoder steps, bits chained back, bytes of m_data)
SHAPE = {KIND_CAC: (25, 300, 175, 171, 22), KIND_FACCH2: (29, 348, 203, 199, 26), KIND_UDCH: (29, 348, 203, 199, 26)}
DEPUNCTURE_14 = (0, 1, 2, None, 3, 4, 5, 6, 7, 8, 9, None, 10, 11)


# ---- checksums --------------------------------------------------------------------------------------------------------------------
def crc16cac(bits):
    """a register of 0xC3EE, message bits shifted in at the low end, x^16 + x^12 + x^5 + 1, inverted at the end"""
    crc = 0xC3EE
    for b in bits:
        crc = ((crc << 1) | int(b)) & 0x1FFFF
        if crc & 0x10000:
            crc = (crc & 0xFFFF) ^ 0x1021
    return (crc ^ 0xFFFF) & 0xFFFF


def crc15(bits):
    """x^15 + x^14 + x^11 + x^10 + x^7 + x^6 + x^2 + 1 from all ones, the message bit meets the register's top"""
    crc = 0x7FFF
    for b in bits:
        fb = ((crc >> 14) & 1) ^ int(b)
        crc = (crc << 1) & 0x7FFF
        if fb:
            crc ^= 0x4CC5
    return crc


def facch2_crc15_payload(trellis_bits):
    return crc15(trellis_bits[:184])


def facch2_crc15_check(trellis_bits):
    return rx4.bits_int(trellis_bits[184:199])


def sacch_part_of_frame(sf):
    return {2: 1, 1: 2, 0: 3}.get(int(sf), 0)


def ran_from_trellis(bits):
    return rx4.bits_int(bits[2:8])


def sequence_is_valid(crc_ok, previous_part, part):
    if not crc_ok:
        return False
    return part == 0 or part == (previous_part + 1) % 4


# ---- one frame ----------------------------------------------------------------------------------------------------------------------
def frame_bits(dibits182, rel182):
    """-> (de-scrambled bits [364], reliabilities [364]: one per dibit, used for both of its bits)"""
    d = (np.asarray(dibits182, np.uint8) & 3) ^ (rx4.nxdn_pn9() << 1)
    return np.stack([d >> 1, d & 1], 1).reshape(-1), np.repeat(np.asarray(rel182, np.uint8), 2)


def lich_of(bits364):
    """-> (7-bit LICH, parity good)"""
    full = rx4.bits_int(bits364[0:16:2])
    lich = full >> 1
    par = sum(full >> k for k in (4, 5, 6, 7)) & 1
    if lich in (0x08, 0x4A, 0x48, 0x46):
        par = sum(full >> k for k in range(1, 8)) & 1
    return lich, (full & 1) == par


def kind_of(lich, parity_ok):
    return LICH_KIND.get(lich, KIND_NONE) if parity_ok and lich in LICH_PROFILE else KIND_NONE


def decoder_rows(bits364, rel364, kind):
    """the rows of the soft decoder and of the greedy one: (symbols = bit << 1 [2 * steps], reliabilities, hard bits); the arrays of
    nxdn_depermute_rel and nxdn_depuncture_12_group_rel one after the other"""
    N, nb, steps, _, _ = SHAPE[kind]
    dep, depr = np.zeros(nb, np.uint8), np.zeros(nb, np.uint8)
    for i in range(nb):
        dep[(i % N) * 12 + i // N] = bits364[16 + i]
        depr[(i % N) * 12 + i // N] = rel364[16 + i]
    hard, rel = [], []
    for g in range(N):
        for m in DEPUNCTURE_14:
            hard.append(0 if m is None else int(dep[12 * g + m]))
            rel.append(0 if m is None else int(depr[12 * g + m]))
    hard, rel = np.array(hard, np.uint8), np.array(rel, np.uint8)
    assert len(hard) == 2 * steps
    return hard << 1, rel, hard


def field_ok(kind, bits):
    if kind == KIND_CAC:
        return crc16cac(bits[:171]) == 0
    return facch2_crc15_payload(bits) == facch2_crc15_check(bits)


def decode_rows(kind, sym, rel, hard):
    """nxdn_deperm_cac_soft / nxdn_deperm_facch2_udch_soft behind the de-puncture -> dict(bits208, bytes26, crc_ok, fallback, ran, sf)"""
    import fecgen
    _, _, steps, nbits, nbytes = SHAPE[kind]
    soft = fecgen.oracle_nxdn(np.ascontiguousarray(sym[None]), np.ascontiguousarray(rel[None]), steps, nbits)[0][0]
    bits = np.zeros(208, np.uint8)
    bits[:8 * len(soft)] = np.unpackbits(soft)
    bits[nbits:] = 0
    ok, fallback = field_ok(kind, bits), 0
    if not ok:
        bits[:] = 0
        bits[:nbits] = rx4.oracle_trellis_decode(np.ascontiguousarray(hard[None]), nbits)[0]
        ok, fallback = field_ok(kind, bits), 1
    by = np.zeros(26, np.uint8)
    by[:nbytes] = np.packbits(bits)[:nbytes]
    return dict(kind=kind, bits208=bits, bytes26=by, crc_ok=int(ok), fallback=fallback, ran=ran_from_trellis(bits), sf=rx4.bits_int(bits[:2]))


def decode_frame(dibits182, rel182):
    """-> dict(kind, lich, parity, [bits208, bytes26, crc_ok, fallback, ran, sf]) of one whole frame"""
    bits, rel = frame_bits(dibits182, rel182)
    lich, par = lich_of(bits)
    kind = kind_of(lich, par)
    out = dict(kind=kind, lich=lich, parity=par)
    if kind:
        out.update(decode_rows(kind, *decoder_rows(bits, rel, kind)))
    return out


def sacch_of(dibits182, rel182):
    """the chain's four SACCH arrays of a frame: (soft [4] packed, soft CRC6 good, greedy retry [32], its CRC6 good)"""
    import fecgen
    _, _, ss, sr, _, _ = rx4.nxdn_frame_fields(np.asarray(dibits182, np.uint8) & 3, rel182)
    soft = fecgen.oracle_nxdn(ss[None].copy(), sr[None].copy(), 36, 32)[0][0]
    hard = rx4.oracle_trellis_decode((ss.reshape(1, 72) >> 1), 32)[0]
    return soft, int(rx4.nxdn_crc_ok(np.unpackbits(soft)[:32], 0)), hard, int(rx4.nxdn_crc_ok(hard, 0))


# ---- the state carried from frame to frame ----------------------------------------------------------------------------------------
class State:
    def __init__(self):
        self.part_of_frame, self.last_ran, self.cac_fail = 0, -1, 0
        self.reset_segments()

    def reset_segments(self):
        self.segment = np.ones((4, 18), np.uint8)
        self.segcrc = [1, 1, 1, 1]

    def copy(self):
        s = State()
        s.part_of_frame, s.last_ran, s.cac_fail = self.part_of_frame, self.last_ran, self.cac_fail
        s.segment, s.segcrc = self.segment.copy(), list(self.segcrc)
        return s


def walk_frame(s, lich_byte, valid, sacch, sacch_ok, sacch_hard, sacch_hard_ok, fr):
    """one slot through the state `s` -> dict(sacch_status, pf, seq_ok, msg72 (None = not written), msg_status, last_ran, cac_fail);
    lich_byte = 7-bit LICH | 0x80 where the parity is good; fr = the slot's decode_frame fields (kind, crc_ok, ran, sf)"""
    status, seq, mst, msg, fails = 0, 0, 0, None, s.cac_fail
    lich = int(lich_byte) & 0x7F
    if valid and (int(lich_byte) & 0x80):
        if lich not in LICH_PROFILE:
            s.reset_segments()
        elif lich in LICH_SACCH:
            t = np.unpackbits(np.asarray(sacch, np.uint8))[:32] if sacch_ok else np.asarray(sacch_hard, np.uint8) & 1
            good = bool(sacch_ok or sacch_hard_ok)
            if not good:
                s.reset_segments()
            if lich in LICH_NON_SUPERFRAME:
                if good:
                    s.last_ran = ran_from_trellis(t)
                s.part_of_frame = 3 if good else 0
                status, seq, mst = (3, 1, 1) if good else (4, 0, 0)
                msg = np.zeros(72, np.uint8)
                msg[:24] = t[8:32]
                s.reset_segments()
            else:
                part = sacch_part_of_frame(rx4.bits_int(t[:2]))
                seq = int(sequence_is_valid(good, s.part_of_frame, part))
                if not seq:
                    s.reset_segments()
                s.part_of_frame = part
                if good:
                    s.last_ran = ran_from_trellis(t)
                s.segcrc[part] = 0 if good else 1
                s.segment[part] = t[8:26]
                status = 1 if good else 2
                if part == 3:
                    mst = 2 if any(s.segcrc) else 1
                    msg = s.segment.reshape(-1).copy()
                    s.reset_segments()
        elif fr["kind"] == KIND_CAC:
            if fr["crc_ok"]:
                s.last_ran, s.cac_fail, fails = fr["ran"], 0, 0
            else:
                fails = s.cac_fail + 1
                s.cac_fail = 0 if fails > 10 else fails       # (where the reference resets its symbolizer: not applied, reported as 11)
        elif fr["kind"] != KIND_NONE:
            if fr["crc_ok"]:
                s.last_ran, s.part_of_frame = fr["ran"], 3 - fr["sf"]
            else:
                s.part_of_frame = 0
    return dict(sacch_status=status, pf=s.part_of_frame, seq_ok=seq, msg72=msg, msg_status=mst, last_ran=s.last_ran, cac_fail=fails)


# ---- a stream: the frames of the oracle loop (chain_fsk4_stream.nxdn_oracle_stream) through decode and walk ---------------------------
_DECODED = {}


def stream_reference(want):
    """want = nxdn_oracle_stream(..) of one channel -> [(position, frame fields, walk fields)] of every whole frame in air order (the
    frames the chain flags valid), one State over the whole stream"""
    key = id(want)
    if key not in _DECODED:
        s, out = State(), []
        for p, k, d, rel, (lich7, par, *_rest) in want["frames"]:
            fr = decode_frame(d, rel)
            assert fr["lich"] == int(lich7) and bool(fr["parity"]) == bool(par)
            so, sok, sh, shok = sacch_of(d, rel)
            out.append((p, fr, walk_frame(s, int(lich7) | (0x80 if par else 0), 1, so, sok, sh, shok, fr)))
        _DECODED[key] = (want, out)
    return _DECODED[key][1]


def delivered(ref):
    """the messages a host sees: [(position of the last frame, last RAN, msg72)] of the slots with msg_status 1"""
    return [(p, w["last_ran"], w["msg72"]) for p, _, w in ref if w["msg_status"] == 1]


# ---- arrays: what ddn_nxdn_ctrl_decode_batch + ddn_nxdn_ctrl_walk_batch leave, from records ---------------------------------------------
FRAME_ARRAYS = dict(kind=(np.uint8, ()), bits208=(np.uint8, (208,)), bytes26=(np.uint8, (26,)), crc_ok=(np.uint8, ()), fallback=(np.uint8, ()),
                    ran=(np.uint8, ()), sf=(np.uint8, ()))
MESSAGE_ARRAYS = dict(sacch_status=(np.uint8, ()), pf=(np.uint8, ()), seq_ok=(np.uint8, ()), msg72=(np.uint8, (72,)), msg_status=(np.uint8, ()),
                      last_ran=(np.int32, ()), cac_fail=(np.int32, ()))
FILL = 0xEE          # what the tests put into every output row first: a row nobody writes keeps it


def blank(B, S):
    """the output arrays of both calls as the tests hand them in"""
    out = {}
    for k, (dt, sh) in list(FRAME_ARRAYS.items()) + list(MESSAGE_ARRAYS.items()):
        out[k] = np.full((B, S) + sh, FILL if dt == np.uint8 else -0x11111112, dt)
    return out


def slot_frame(rec10, counts, c, pos):
    """(dibits [182], reliabilities [182]) behind sync position `pos` of channel c, or None where the row holds no whole frame"""
    max_sym = rec10.shape[1]
    if pos < 0 or not (pos + 182 < int(counts[c]) and pos + 182 < max_sym):
        return None
    return rec10[c, pos + 1:pos + 183, 0] & 3, rec10[c, pos + 1:pos + 183, 1]


def decode_batch(rec10, counts, sync_pos, n_sync, out):
    """rec10 [B][max_symbols][10], sync_pos [B][S] -> writes the frame arrays of `out` as the device call does: kind for every slot, the
    other rows of kinds 1..3 only; returns per slot the decode_frame dict (None: no whole frame)"""
    B, S = sync_pos.shape
    frames = [[None] * S for _ in range(B)]
    for c in range(B):
        for k in range(S):
            fr = None
            if k < int(n_sync[c]):
                f = slot_frame(rec10, counts, c, int(sync_pos[c, k]))
                if f is not None:
                    fr = frames[c][k] = decode_frame(*f)
            out["kind"][c, k] = fr["kind"] if fr else 0
            if fr and fr["kind"]:
                for key in ("bits208", "bytes26", "crc_ok", "fallback", "ran", "sf"):
                    out[key][c, k] = fr[key]
    return frames


def sacch_arrays(rec10, counts, sync_pos, n_sync):
    """the walk's inputs as ddn_nxdn_frame_gather and the chain's SACCH decoders leave them: dict(lich, valid, sacch, sacch_ok, sacch_hard,
    sacch_hard_ok) over [B][S]"""
    B, S = sync_pos.shape
    a = dict(lich=np.zeros((B, S), np.uint8), valid=np.zeros((B, S), np.uint8), sacch=np.zeros((B, S, 4), np.uint8),
             sacch_ok=np.zeros((B, S), np.uint8), sacch_hard=np.zeros((B, S, 32), np.uint8), sacch_hard_ok=np.zeros((B, S), np.uint8))
    for c in range(B):
        for k in range(min(int(n_sync[c]), S)):
            f = slot_frame(rec10, counts, c, int(sync_pos[c, k]))
            if f is None:
                continue
            lich, par = lich_of(frame_bits(*f)[0])
            a["lich"][c, k], a["valid"][c, k] = lich | (0x80 if par else 0), 1
            a["sacch"][c, k], a["sacch_ok"][c, k], a["sacch_hard"][c, k], a["sacch_hard_ok"][c, k] = sacch_of(*f)
    return a


def walk_batch(n_sync, sa, frames_out, states, out):
    """the walk over arrays: sa = sacch_arrays(..), frames_out = the frame arrays decode_batch left (kind, crc_ok, ran, sf are read as the
    device reads them), states [B] of State (advanced in place); writes the message arrays of `out` for the slots below n_sync"""
    B, S = sa["lich"].shape
    for c in range(B):
        for k in range(min(int(n_sync[c]), S)):
            fr = dict(kind=int(frames_out["kind"][c, k]), crc_ok=int(frames_out["crc_ok"][c, k]), ran=int(frames_out["ran"][c, k]),
                      sf=int(frames_out["sf"][c, k]))
            w = walk_frame(states[c], sa["lich"][c, k], sa["valid"][c, k], sa["sacch"][c, k], sa["sacch_ok"][c, k], sa["sacch_hard"][c, k],
                           sa["sacch_hard_ok"][c, k], fr)
            for key, v in w.items():
                if key != "msg72":
                    out[key][c, k] = v
                elif v is not None:
                    out[key][c, k] = v
