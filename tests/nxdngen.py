"""Generator of whole NXDN frames as dibits: frame sync word + LICH + the payload of every channel the control-channel stage reads
(CAC, FACCH2, UDCH) and of the SACCH / FACCH1 frames around them, scrambled (PN9 seed 228).  The transmit side of
src/protocol/nxdn/nxdn_deperm.c and nxdn_frame.c, written from the receive side's tables: K = 5 encoder (generators 0x19 / 0x17, four
flush bits), puncture, interleave.  TEST INFRASTRUCTURE - the product never imports this."""
import numpy as np

import fecgen
import nxdn_ctrl as nc
import rx4

FSW = np.array([int(ch) for ch in rx4.NXDN_POS[0]], np.uint8)        # 3131331131: '1' = +3 (dibit 1), '3' = -3 (dibit 3)
FRAME = 192                                                              # symbols: 10 + 182
LICH_CAC, LICH_FACCH2, LICH_UDCH = 0x01, 0x28, 0x2E
LICH_SACCH_FACCH, LICH_SACCH_VOICE, LICH_SACCH_NSF = 0x30, 0x36, 0x20    # RTCH: SACCH + two FACCH1 / + four voice frames; non-superframe
LICH_OFF_TABLE = 0x02                                                    # good parity, in no row of k_nxdn_lich_profiles
assert LICH_OFF_TABLE not in nc.LICH_PROFILE


def bits_of(v, n):
    return np.array([(int(v) >> (n - 1 - i)) & 1 for i in range(n)], np.uint8)


def _encode(bits):
    """bits + four flush zeros through the K = 5 rate 1/2 encoder"""
    return fecgen.conv_k5_encode(np.concatenate([bits, np.zeros(4, np.uint8)]).astype(np.int64)[None])[0]


def _interleave(dep, rows, cols):
    """the air order of de-permuted bits: the receiver files air bit i at (i % cols) * rows + i // cols"""
    return np.array([dep[(i % cols) * rows + i // cols] for i in range(rows * cols)], np.uint8)


def header8(sf, ran):
    return np.concatenate([bits_of(sf, 2), bits_of(ran, 6)])


def cac_field(ran, msg147, sf=0, bad_crc=False):
    """-> (air bits [300], the 171 bits a decoder should return)"""
    info = np.concatenate([header8(sf, ran), np.asarray(msg147, np.uint8)])
    assert len(info) == 155
    # crc16cac over message + field is 0 where the field holds what the division leaves over message + sixteen zeros
    crc = nc.crc16cac(np.concatenate([info, np.zeros(16, np.uint8)]))
    word = np.concatenate([info, bits_of(crc ^ (0x0400 if bad_crc else 0), 16)])
    assert bad_crc or nc.crc16cac(word) == 0
    enc = _encode(word)                                                  # 175 steps
    kept = np.array([enc[14 * g + j] for g in range(25) for j in range(14) if j not in (3, 11)], np.uint8)
    return _interleave(kept, 12, 25), word


def facch2_field(ran, msg176, sf=3, bad_crc=False):
    """FACCH2 and UDCH share the coding -> (air bits [348], the 199 bits a decoder should return)"""
    info = np.concatenate([header8(sf, ran), np.asarray(msg176, np.uint8)])
    assert len(info) == 184
    word = np.concatenate([info, bits_of(nc.crc15(info) ^ (0x0010 if bad_crc else 0), 15)])
    enc = _encode(word)                                                  # 203 steps
    kept = np.array([enc[14 * g + j] for g in range(29) for j in range(14) if j not in (3, 11)], np.uint8)
    return _interleave(kept, 12, 29), word


def sacch_field(sf, ran, msg18, bad_crc=False):
    """-> (air bits [60], the 32 bits a decoder should return)"""
    info = np.concatenate([header8(sf, ran), np.asarray(msg18, np.uint8)])
    word = np.concatenate([info, bits_of(rx4.nxdn_crc(info, 0) ^ (0x04 if bad_crc else 0), 6)])
    enc = _encode(word)                                                  # 36 steps
    kept = np.array([enc[12 * g + j] for g in range(6) for j in range(12) if j not in (5, 11)], np.uint8)
    return _interleave(kept, 12, 5), word


def facch1_field(msg80):
    """-> air bits [144]"""
    info = np.asarray(msg80, np.uint8)
    word = np.concatenate([info, bits_of(rx4.nxdn_crc(info, 1), 12)])
    enc = _encode(word)                                                  # 96 steps
    kept = np.array([enc[4 * g + j] for g in range(48) for j in range(4) if j != 1], np.uint8)
    return _interleave(kept, 16, 9)


def lich_bits(lich7, bad_parity=False):
    full = int(lich7) << 1
    par = sum(full >> k for k in (4, 5, 6, 7)) & 1
    if lich7 in (0x08, 0x4A, 0x48, 0x46):
        par = sum(full >> k for k in range(1, 8)) & 1
    return bits_of(full | (par ^ (1 if bad_parity else 0)), 8)


def frame(lich7, payload348, bad_parity=False):
    """frame sync word + 182 scrambled dibits: the LICH's eight bits ride the sign of eight +-3 symbols, the payload two bits a dibit"""
    payload348 = np.asarray(payload348, np.uint8)
    assert len(payload348) == 348
    d = np.concatenate([(lich_bits(lich7, bad_parity) << 1) | 1, (payload348[0::2] << 1) | payload348[1::2]]).astype(np.uint8)
    return np.concatenate([FSW, d ^ (rx4.nxdn_pn9() << 1)])


def cac_frame(rng, ran, lich7=LICH_CAC, bad_crc=False, msg=None):
    """-> (dibits [192], expected 171 bits)"""
    msg = rng.integers(0, 2, 147).astype(np.uint8) if msg is None else msg
    air, word = cac_field(ran, msg, bad_crc=bad_crc)
    return frame(lich7, np.concatenate([air, rng.integers(0, 2, 48).astype(np.uint8)])), word


def facch2_frame(rng, ran, lich7=LICH_FACCH2, sf=3, bad_crc=False, msg=None):
    """FACCH2 (lich7 0x28, 0x29, 0x49) or UDCH (0x2E, 0x2F, 0x4E, 0x4F) -> (dibits [192], expected 199 bits)"""
    msg = rng.integers(0, 2, 176).astype(np.uint8) if msg is None else msg
    air, word = facch2_field(ran, msg, sf=sf, bad_crc=bad_crc)
    return frame(lich7, air), word


def sacch_frame(rng, sf, ran, msg18, lich7=LICH_SACCH_FACCH, bad_crc=False, bad_parity=False):
    """a frame with a SACCH segment in front of two FACCH1 fields (random bits behind a voice LICH) -> (dibits [192], expected 32 bits)"""
    air, word = sacch_field(sf, ran, msg18, bad_crc=bad_crc)
    if lich7 in (0x30, 0x31, 0x50, 0x51, 0x20, 0x21, 0x40, 0x41):
        rest = np.concatenate([facch1_field(rng.integers(0, 2, 80).astype(np.uint8)) for _ in range(2)])
    else:
        rest = rng.integers(0, 2, 288).astype(np.uint8)
    return frame(lich7, np.concatenate([air, rest]), bad_parity=bad_parity), word


def vcall_message(src, tg, msg_type=1):
    """a 72-bit SACCH message laid out as the VCALL the tools print: message type in bits 2..7, source unit in bits 24..39, destination in
    bits 40..55"""
    m = np.zeros(72, np.uint8)
    m[2:8], m[24:40], m[40:56] = bits_of(msg_type, 6), bits_of(src, 16), bits_of(tg, 16)
    return m


def superframe(rng, ran, msg72, lich7=LICH_SACCH_FACCH, order=(0, 1, 2, 3), bad=()):
    """the four frames of a superframe (SF 3, 2, 1, 0 = parts 0..3), sent in `order`, the parts in `bad` with a broken CRC6"""
    return [sacch_frame(rng, 3 - p, ran, msg72[18 * p:18 * p + 18], lich7=lich7, bad_crc=p in bad)[0] for p in order]


# ---- the streams the tests run ------------------------------------------------------------------------------------------------------
def control_frames(seed=5, ran=9):
    """One channel's traffic, frame after frame: a control channel (CACs, some with a broken CRC), a traffic channel with superframes in
    and out of order, a LICH off the profile table and one with bad parity between segments, non-superframe SACCHs, FACCH2 / UDCH frames
    - one of them between two segments.  The receive loop drops its lock on a LICH it rejects, hunts through the rest of that frame
    (where random dibits now and then look like a sync word) and accepts the second of two syncs in a row, so five spare frames follow
    each of the two.  -> list of 192-dibit frames"""
    rng = np.random.default_rng(seed)
    idle = lambda: cac_frame(rng, ran)[0]
    msg = lambda k: vcall_message(901 + k, 100 + k)
    fr = [idle() for _ in range(3)]                                          # (the loop accepts from the second sync on)
    fr += [cac_frame(rng, ran, lich7=(LICH_CAC, 0x05)[k & 1])[0] for k in range(14)]
    fr += [cac_frame(rng, ran, bad_crc=True)[0] for _ in range(3)]
    fr += [idle() for _ in range(2)]
    fr += superframe(rng, ran, msg(0))                                        # delivered
    fr += [facch2_frame(rng, ran, lich7=l)[0] for l in (0x28, 0x29, 0x49, 0x28)]
    fr += superframe(rng, ran, msg(1), lich7=LICH_SACCH_VOICE)                # delivered
    fr += [facch2_frame(rng, ran, lich7=l)[0] for l in (0x2E, 0x2F, 0x4E, 0x4F, 0x2E)]
    fr += superframe(rng, ran, msg(2), bad=(1,))                              # completed, not delivered
    fr += superframe(rng, ran, msg(3), order=(0, 2, 1, 3))                    # out of sequence
    s = superframe(rng, ran, msg(4))                                          # a LICH off the table between segments: the store is reset
    fr += s[:2] + [sacch_frame(rng, 1, ran, np.zeros(18, np.uint8), lich7=LICH_OFF_TABLE)[0]] + [idle() for _ in range(5)] + s[2:]
    s = superframe(rng, ran, msg(5))                                          # a parity failure between segments resets nothing
    fr += s[:2] + [sacch_frame(rng, 1, ran, np.zeros(18, np.uint8), bad_parity=True)[0]] + [idle() for _ in range(5)] + s[2:]
    fr += [sacch_frame(rng, 0, ran, rng.integers(0, 2, 18).astype(np.uint8), lich7=LICH_SACCH_NSF)[0] for _ in range(2)]
    fr += [sacch_frame(rng, 0, ran, rng.integers(0, 2, 18).astype(np.uint8), lich7=LICH_SACCH_NSF, bad_crc=True)[0]]
    s = superframe(rng, ran, msg(6))                                          # FACCH2 with SF 2 after part 0: part_of_frame = 1, so
    fr += s[:1] + [facch2_frame(rng, ran, sf=2)[0]] + s[2:]                  # part 2 is in sequence although part 1 never came
    s = superframe(rng, ran, msg(7))                                          # FACCH2 with a broken CRC: part_of_frame = 0, part 2 is not
    fr += s[:2] + [facch2_frame(rng, ran, sf=1, bad_crc=True)[0]] + s[2:]
    fr += superframe(rng, ran, msg(8))                                        # delivered
    fr += superframe(rng, ran, msg(9), lich7=LICH_SACCH_VOICE)                # delivered
    fr += [facch2_frame(rng, ran, lich7=LICH_UDCH, bad_crc=True)[0]]
    fr += [idle() for _ in range(2)]
    return fr


def control_stream(n_frames=None):
    """control_frames (the first n_frames of them) on the air: 120 random dibits for the loop's levels to settle on, the frames, a tail"""
    rng = np.random.default_rng(17)
    return np.concatenate([rng.integers(0, 4, 120).astype(np.uint8)] + control_frames()[:n_frames] + [rng.integers(0, 4, 60).astype(np.uint8)])


def cac_stream(n_frames, seed=6, ran=3):
    """a control channel: every frame a CAC"""
    rng = np.random.default_rng(seed)
    return np.concatenate([cac_frame(rng, ran)[0] for _ in range(n_frames)])


_AIR = {}


def air_batch(which="nxdn96"):
    """control_stream as cu8 I/Q on three channels (chain_fsk4_stream._batch: as sent, delayed, starting later); NXDN96 at 10 samples
    per symbol, NXDN48 a shorter stream at 20"""
    if which not in _AIR:
        import chain_fsk4_stream as cs
        import p25gen
        dib = control_stream()
        if which == "nxdn96":
            L = 10 * len(dib) + 4000
            iq = p25gen.modulate_cu8(dib, L + 3000, sps=10, lead=300, seed=4)
            _AIR[which] = cs._batch(iq, L - L % 6000, 1234, later=1931)
        else:
            dib = control_stream(44)
            L = 20 * len(dib) + 4000
            iq = p25gen.modulate_cu8(dib, L + 6000, sps=20, dev=0.045, lead=600, seed=4)
            _AIR[which] = cs._batch(iq, L - L % 12000, 2345, later=3877)
    return _AIR[which]


# ---- records for the direct calls: frames laid into the loop's 10-byte records without a loop ------------------------------------------
def records(frames_per_channel, max_symbols, rng, rel=None, lead=7):
    """frames_per_channel [B]: lists of 192-dibit frames -> (rec10 [B][max_symbols][10] - byte 0 the dibit under random upper bits, byte 1
    the reliability, the rest noise -, counts [B], sync positions [B] lists: the last symbol of every sync word)"""
    B = len(frames_per_channel)
    rec = rng.integers(0, 256, (B, max_symbols, 10)).astype(np.uint8)
    counts, pos = np.zeros(B, np.int32), []
    for c, frames in enumerate(frames_per_channel):
        p, at = [], lead + c
        rec[c, :, 1] = rng.integers(90, 256, max_symbols) if rel is None else rel
        for f in frames:
            fixed = isinstance(f, tuple)              # (frame, "rel0" / "rel255"): clean dibits whose reliabilities are all 0 / 255
            f, level = (f[0], int(f[1][3:])) if fixed else (f, None)
            assert at + FRAME <= max_symbols
            rec[c, at:at + FRAME, 0] = (rec[c, at:at + FRAME, 0] & 0xFC) | f
            if fixed:
                rec[c, at:at + FRAME, 1] = level
            p.append(at + 9)
            at += FRAME
        counts[c] = at
        pos.append(p)
    return rec, counts, pos


def slot_arrays(pos, S):
    """sync position lists -> (sync_pos [B][S] with -1 behind a channel's syncs, n_sync [B])"""
    sp = np.full((len(pos), S), -1, np.int32)
    for c, p in enumerate(pos):
        sp[c, :len(p)] = p
    return sp, np.array([len(p) for p in pos], np.int32)


_SOFT = {}


def soft_frame(kind):
    """The reference's soft decoder charges a branch that disagrees with the one known bit of a punctured pair 8 - x where its twin is
    charged x, so on CAC and FACCH2 words it loses most clean frames to the retry.  -> (a frame it does decode at reliabilities of 255,
    "rel255"): the first of a fixed series of messages for which it does"""
    if kind not in _SOFT:
        rng = np.random.default_rng(100 + kind)
        for _ in range(4000):
            f = cac_frame(rng, 21)[0] if kind == nc.KIND_CAC else facch2_frame(rng, 22, lich7=(LICH_FACCH2, LICH_UDCH)[kind - 2])[0]
            d = nc.decode_frame(f[10:], np.full(182, 255, np.uint8))
            if d["crc_ok"] and not d["fallback"]:
                _SOFT[kind] = (f, "rel255")
                break
    return _SOFT[kind]


def _mix(rng, n, ran):
    """n CACs and n FACCH2 / UDCH frames between SACCH frames, so that both decoders have n wanted slots, neither of them in a row:
    every third CAC with reliabilities of 0, every fifth FACCH2 with a broken CRC, the second of each a frame the soft decoder takes"""
    fr, msg = [], vcall_message(901, 77)
    for k in range(n):
        c = cac_frame(rng, ran, lich7=(0x01, 0x05)[k & 1], bad_crc=k % 7 == 6)[0]
        fr.append(soft_frame(nc.KIND_CAC) if k == 1 else ((c, "rel0") if k % 3 == 0 else c))
        fr.append(sacch_frame(rng, 3 - k % 4, ran, msg[18 * (k % 4):18 * (k % 4) + 18], lich7=(0x30, 0x36)[k & 1])[0])
        f2 = facch2_frame(rng, ran, lich7=(0x28, 0x2E, 0x49, 0x4F)[k % 4], sf=k % 4, bad_crc=k % 5 == 4)[0]
        fr.append(soft_frame(nc.KIND_FACCH2 + (k >> 1 & 1)) if k in (1, 2) else f2)
    return fr


_DIRECT = {}


def direct_case(name):
    """the inputs of the direct calls (no loop): dict(rec, counts, sync_pos [B][S], n_sync).  Names:
       wanted_N (N = 1, 15, 16, 17, 33)   N CACs and N FACCH2 / UDCH among SACCH frames on one channel (k_k5_nxdn takes 16 words a group)
       only_cac / only_facch2 / only_sacch one decoder, the other, neither has a wanted slot
       sparse                             two wanted slots per decoder in 40, groups of 16 without any between them
       ragged                             n_sync = 0, max_syncs and 2 on three channels
       invalid_mid                        a slot whose frame is not whole between the segments of a superframe
       superframes                        the control stream's frames (every walk rule) on two channels, the second one frame behind"""
    if name in _DIRECT:
        return _DIRECT[name]
    rng = np.random.default_rng(sum(name.encode()))
    ran = 1 + len(name) % 60
    sacch = lambda k: sacch_frame(rng, 3 - k % 4, ran, vcall_message(901, 5)[18 * (k % 4):18 * (k % 4) + 18])[0]
    extra = 0
    if name.startswith("wanted_"):
        chans = [_mix(rng, int(name[7:]), ran)]
    elif name == "only_cac":
        chans = [[cac_frame(rng, ran)[0] for _ in range(5)]]
    elif name == "only_facch2":
        chans = [[facch2_frame(rng, ran, lich7=l)[0] for l in (0x28, 0x2F, 0x49)]]
    elif name == "only_sacch":
        chans = [[sacch(k) for k in range(6)]]
    elif name == "sparse":
        fr = [sacch(k) for k in range(40)]
        fr[3], fr[20] = soft_frame(nc.KIND_CAC), (cac_frame(rng, ran)[0], "rel0")
        fr[18], fr[37] = soft_frame(nc.KIND_UDCH), facch2_frame(rng, ran, lich7=0x4E, bad_crc=True)[0]
        chans = [fr]
    elif name == "ragged":
        chans = [[], _mix(rng, 3, ran), [cac_frame(rng, ran)[0], sacch(0)]]
    elif name == "invalid_mid":
        chans = [[sacch(0), sacch(1), sacch(2), sacch(3), cac_frame(rng, ran)[0]]]
        extra = 1
    elif name == "superframes":
        fr = control_frames()
        chans = [fr, fr[1:]]
    else:
        raise KeyError(name)
    S = max(len(c) for c in chans) + extra
    rec, counts, pos = records(chans, S * FRAME + 64, rng)
    if name == "invalid_mid":            # slot 2 points at a frame the records do not hold to its end
        pos[0].insert(2, int(counts[0]) - 100)
    sp, ns = slot_arrays(pos, S)
    _DIRECT[name] = dict(rec=rec, counts=counts, sync_pos=sp, n_sync=ns)
    return _DIRECT[name]


DIRECT_CASES = ("wanted_1", "wanted_15", "wanted_16", "wanted_17", "wanted_33", "only_cac", "only_facch2", "only_sacch", "sparse", "ragged",
                "invalid_mid", "superframes")
