"""CPU restatement of the reference's D-STAR path (-fd) for the tests: the receive-loop profile, the two-level slice, the radio header
(GMSK soft cost, PN descramble, de-interleave, K = 3 soft Viterbi, CRC-CCITT, fields), the voice-frame gather and the slow data, and a
small encoder for generated transmissions.  TEST INFRASTRUCTURE - the product never imports this.

  sync words, profile   src/dsp/dsd_frame_sync.c:1452-1503, include/dsd-neo/core/sync_patterns.h:44-47, decode_mode.c:393-428
  two-level slice       src/core/frames/dsd_dibit.c:892-948,1019-1029 (digitize(): no soft metric, no payload buffer)
  soft cost             gmsk_soft_symbol_to_viterbi_cost() / llr_to_viterbi_cost(), dsd_dibit.c:1150-1167,1245-1281
  header                src/protocol/dstar/dstar_header.c, dstar_header_utils.c:11-184 (PN x^7 + x^4 + 1 seeded 0x07, 24-stride
                        de-interleave, 4-state soft Viterbi over 330 steps, CRC-16/X25 byte-swapped)
  voice + slow data     src/protocol/dstar/dstar.c:21-66 (21 x 72 voice dibits, 20 x 24 slow-data dibits), dstar_slow_data.c:56-441
The tables (AMBE interleave, slow-data pattern) come from tests/golden/dstar_vectors.json."""
import ctypes as C
import ctypes.util
import json
import os

import numpy as np

import rx4

HERE = os.path.dirname(os.path.abspath(__file__))
VOICE_SYNC = "313131313133131113313111"
HEADER_SYNC = "131313131333133113131111"
# pattern rows of the loop: 0 +voice, 1 -voice, 2 +header, 3 -header (types = synctype_ids.h:44-47 + 1, 0 stays "none")
TYPES = [7, 8, 19, 20]
PAT_VOICE_POS, PAT_VOICE_NEG, PAT_HD_POS, PAT_HD_NEG = 0, 1, 2, 3
HEADER_SYMS, VOICE_SYMS = 660, 1992
FRAMES, SD_FRAMES = 21, 20
CODED, INFO = 660, 330


def inv(s):
    return "".join("1" if c == "3" else "3" for c in s)


WORDS = [VOICE_SYNC, inv(VOICE_SYNC), HEADER_SYNC, inv(HEADER_SYNC)]


def vectors():
    return json.load(open(os.path.join(HERE, "golden", "dstar_vectors.json")))


_V = None


def _tables():
    global _V
    if _V is None:
        v = vectors()
        _V = (np.array(v["interleave_w"], np.int32), np.array(v["interleave_x"], np.int32), np.array(v["sd_scrambler"], np.uint8))
    return _V


def profile(rf_mod=2, lock=None, out_rate=48000):
    """the loop profile ddn_fsk4_rx_create builds for DDN_FSK4_DSTAR (tests/rx4.py's Profile): 4800 symbols/s, level ring 24, the four
    words exact over 24 symbols, 24-symbol warm start, no matched filter, class 0 = header (2652), class 1 = voice (1992)"""
    p = rx4.Profile()
    p.proto, p.handler = rx4.PROTO_P25P1, 0     # (no handler family: fixed counts)
    p.out_rate, p.rf_mod, p.use_filter = out_rate, rf_mod, 0
    p.sym_rate, p.win_len, p.t_max, p.warm_len = 4800, 24, 24, 24
    p.n_pat = 4
    for k in range(4):
        p.pat_bits[k], p.pat_type[k], p.pat_neg[k] = rx4.bits_of(WORDS[k]), TYPES[k], k & 1
        p.pat_class[k] = rx4.CLASS_VOICE if k < 2 else rx4.CLASS_DATA
    taps = rx4._taps("dmr")     # (unused)
    p.nt = len(taps)
    for k, t in enumerate(taps):
        p.taps[k] = t
    lock = lock or [HEADER_SYMS + VOICE_SYMS, VOICE_SYMS, 0, 0]
    for k in range(4):
        p.lock_symbols[k] = lock[k]
    return p


def bits2(sym, center, neg):
    """digitize() for a two-level type: positive -> (symbol > center ? 0 : 1), negative -> the complement"""
    b = (np.asarray(sym, np.float32) > np.float32(center)).astype(np.uint8) ^ 1
    return b ^ (1 if neg else 0)


# ---- soft cost -------------------------------------------------------------------------------------------------------------------
_libm = C.CDLL(ctypes.util.find_library("m"))
_libm.expf.restype = C.c_float
_libm.expf.argtypes = [C.c_float]
F = np.float32


def llr_cost(llr):
    if llr >= F(16.0):
        return 0
    if llr <= F(-16.0):
        return 65535
    p1 = F(1.0) / (F(1.0) + F(_libm.expf(float(llr))))
    q = int(np.rint(F(p1 * F(65535.0))))
    return min(max(q, 0), 65535)


def soft_cost(sym, thr5):
    """gmsk_soft_symbol_to_viterbi_cost() against thr5 = {center, umid, lmid, max, min} (binary32 throughout)"""
    center, mx, mn = F(thr5[0]), F(thr5[3]), F(thr5[4])
    if not (mn < center and center < mx):
        span = F(mx - mn)
        if span < F(1e-3):
            span = F(2.0)
        half = F(span * F(0.5))
        mn, mx = F(center - half), F(center + half)
    mu0 = F(F(0.5) * F(mn + center))
    mu1 = F(F(0.5) * F(center + mx))
    sigma = F(F(mx - mn) / F(4.0))
    if sigma < F(1e-3):
        sigma = F(1e-3)
    inv2 = F(F(0.5) / F(sigma * sigma))
    d0, d1 = F(F(sym) - mu0), F(F(sym) - mu1)
    llr = F(F(F(d1 * d1) - F(d0 * d0)) * inv2)
    return llr_cost(llr)


# ---- header ---------------------------------------------------------------------------------------------------------------------
def pn127():
    reg, out = 0x07, []
    for _ in range(127):
        out.append((reg >> 6) & 1)
        fb = ((reg >> 6) ^ (reg >> 3)) & 1
        reg = ((reg << 1) & 0x7E) | fb
    return np.array(out, np.uint8)


def deinterleave_perm():
    """perm[i] = where coded position i of the air order lands (dstar_deinterleave_soft_costs: out[perm[i]] = in[i])"""
    k, perm = 0, []
    for _ in range(CODED):
        perm.append(k)
        k += 24
        if k >= 672:
            k -= 671
        elif k >= 660:
            k -= 647
    return np.array(perm, np.int32)


def viterbi(costs660):
    """4-state soft Viterbi (G = 7, 5), ties to the first candidate; -> 330 bits"""
    c = [int(v) for v in costs660]
    pm = [0, 0, 0, 0]
    mem = np.zeros((4, INFO), np.uint8)

    def bm(s1, s0, r1, r0):
        return (s1 if r1 == 0 else 0xFFFF - s1) + (s0 if r0 == 0 else 0xFFFF - s0)

    for n in range(INFO):
        s1, s0 = c[2 * n], c[2 * n + 1]
        cand = [(bm(s1, s0, 0, 0) + pm[0], bm(s1, s0, 1, 1) + pm[2]), (bm(s1, s0, 1, 1) + pm[0], bm(s1, s0, 0, 0) + pm[2]),
                (bm(s1, s0, 1, 0) + pm[1], bm(s1, s0, 0, 1) + pm[3]), (bm(s1, s0, 0, 1) + pm[1], bm(s1, s0, 1, 0) + pm[3])]
        new = []
        for st, (a, b) in enumerate(cand):
            if a <= b:
                mem[st, n] = 0
                new.append(a)
            else:
                mem[st, n] = 1
                new.append(b)
        pm = new
    st = int(np.argmin(pm))             # first minimum
    prev = [[0, 0, 1, 1], [2, 2, 3, 3]]
    out = np.zeros(INFO, np.uint8)
    for i in range(INFO - 1, -1, -1):
        out[i] = st & 1
        st = prev[mem[st, i]][st]
    return out


def crc16(data):
    """dstar_crc16: CRC-16/X25 (reflected 0x1021, init / xorout 0xFFFF), returned byte-swapped"""
    crc = 0xFFFF
    for b in bytes(bytearray(data)):
        crc ^= b
        for _ in range(8):
            crc = (crc >> 1) ^ 0x8408 if crc & 1 else crc >> 1
    crc = (~crc) & 0xFFFF
    return ((crc << 8) | (crc >> 8)) & 0xFFFF


def header_from_costs(costs660):
    """-> 41 octets (LSB first) from 660 soft costs in air order"""
    pn = pn127()
    c = np.asarray(costs660, np.int64)
    s = np.where(pn[np.arange(CODED) % 127] == 1, 0xFFFF - c, c)
    d = np.zeros(CODED, np.int64)
    d[deinterleave_perm()] = s
    bits = viterbi(d)
    h = np.zeros(41, np.uint8)
    for i in range(328):
        h[i >> 3] |= int(bits[i]) << (i & 7)
    return h


def header_fields(h41):
    h = bytes(h41) if isinstance(h41, (bytes, bytearray)) else bytes(bytearray(np.asarray(h41, np.uint8)))
    return {"flags": h[0], "rpt2": h[3:11], "rpt1": h[11:19], "dst": h[19:27], "src": h[27:39],
            "crc_ok": crc16(h[:39]) == ((h[39] << 8) | h[40])}


def decode_header(sym660, thr5):
    """dstar_header_decode_soft() -> (41 octets, CRC ok)"""
    h = header_from_costs([soft_cost(s, thr5) for s in np.asarray(sym660, np.float32)])
    return h, header_fields(h)["crc_ok"]


# ---- voice frames + slow data -----------------------------------------------------------------------------------------------------
def voice_gather(dibits1992):
    """processDSTAR(): 21 AMBE frames ambe_fr[4][24] (bit = dibit & 1) and the 480 slow-data dibits as read (a two-level dibit is
    the bit itself)"""
    w, x, _ = _tables()
    b = np.asarray(dibits1992, np.uint8)
    fr = np.zeros((FRAMES, 4, 24), np.uint8)
    sd = np.zeros(480, np.uint8)
    for j in range(FRAMES):
        fr[j, w, x] = b[96 * j:96 * j + 72] & 1
        if j < SD_FRAMES:
            sd[24 * j:24 * j + 24] = b[96 * j + 72:96 * j + 96]
    return fr, sd


def _sanitize(by):
    b = bytearray(by)
    for i in range(1, 60):
        if b[i] < 0x20 or b[i] > 0x7E:
            b[i] = 0x20
        if i < 59 and b[i] == 0x66 and b[i + 1] == 0x66:
            b[i] = 0
        if i == 59 and b[i] == 0x66:
            b[i] = 0
    return b


SD_UNKNOWN, SD_HEADER, SD_TEXT, SD_FIXED = 0, 1, 2, 3


def slow_data(sd480):
    """processDSTAR_SD() without APRS -> dict(bytes = the 60 packed bytes, kind, hdr41, crc_ok, text = dstar_txt's 60 bytes when a
    text message is stored (else None))"""
    _, _, pat = _tables()
    s = (np.asarray(sd480, np.uint8) & 1) ^ pat[np.arange(480) % 24]
    s = s[::-1]
    sdb = bytearray(60)
    for i in range(60):
        v = 0
        for k in range(8):
            v = (v << 1) | int(s[8 * i + k])
        sdb[59 - i] = v
    raw = bytes(sdb)
    ln = (sdb[0] & 0xF) + 1
    hd = bytearray(60)
    j = 0
    for i in range(50):
        j += 1
        hd[i] = sdb[j]
        for m in range(1, 10):
            if j == ln * m - 1:
                j += 1
    hdr41 = bytes(hd[:41])
    crc_ok = ((hd[39] << 8) + hd[40]) == crc16(hd[:39])
    sdb = _sanitize(sdb)
    kind, text = SD_UNKNOWN, None
    if sdb[0] == 0x55:
        kind = SD_HEADER
    elif sdb[0] == 0x35 or sdb[0] == 0x40:
        kind = SD_FIXED if sdb[0] == 0x35 else SD_TEXT
        if not (kind == SD_FIXED and bytes(sdb[1:6]) == b"$$CRC"):
            t = bytearray(b" " * 60)
            for i in range(1, 59):
                if i % 6 and 0x19 < sdb[i] < 0x7F:
                    t[i] = sdb[i]
            t[59] = 0
            text = bytes(t)
    return dict(bytes=raw, kind=kind, hdr41=hdr41, crc_ok=bool(crc_ok), text=text)


def decode_unit(sym, pat, thr5):
    """one sync's unit from the symbols behind it (pattern row pat, thresholds thr5) -> dict(header41, header_crc_ok, ambe, sd)"""
    neg, hd = pat & 1, pat >= 2
    sym = np.asarray(sym, np.float32)
    out = dict(pat=int(pat), header41=None, header_crc_ok=False)
    off = 0
    if hd:
        out["header41"], out["header_crc_ok"] = decode_header(sym[:HEADER_SYMS], thr5)
        off = HEADER_SYMS
    fr, sd = voice_gather(bits2(sym[off:off + VOICE_SYMS], thr5[0], neg))
    out["ambe"], out["sd480"] = fr, sd
    out["sd"] = slow_data(sd)
    return out


def unit_len(pat):
    return VOICE_SYMS + (HEADER_SYMS if pat >= 2 else 0)


def decode_stream(sym, sync_pos, sync_pat, sync_thr):
    """every sync whose unit lies inside the stream -> [(k, decode_unit)]"""
    out = []
    for k, (p, t) in enumerate(zip(sync_pos, sync_pat)):
        a = int(p) + 1
        if a + unit_len(int(t)) <= len(sym):
            out.append((k, decode_unit(sym[a:a + unit_len(int(t))], int(t), sync_thr[k])))
    return out


def text(b):
    return bytes(b).decode("latin-1")


# ---- encoder (generated transmissions) ---------------------------------------------------------------------------------------------
def conv_encode(bits):
    s0 = s1 = 0
    out = []
    for b in bits:
        out += [b ^ s0 ^ s1, b ^ s1]
        s1, s0 = s0, b
    return np.array(out, np.uint8)


def encode_header(h41):
    """41 octets -> the 660 air bits (K = 3 encode of 330 bits, interleave, scramble)"""
    info = np.zeros(INFO, np.uint8)
    for i in range(328):
        info[i] = (int(h41[i >> 3]) >> (i & 7)) & 1
    coded = conv_encode(info)
    air = coded[deinterleave_perm()]            # air[i] = coded[perm[i]]
    return air ^ pn127()[np.arange(CODED) % 127]


def make_header(flags, rpt2, rpt1, dst, src, good_crc=True):
    h = bytearray(41)
    h[0] = flags
    for at, s, n in ((3, rpt2, 8), (11, rpt1, 8), (19, dst, 8), (27, src, 12)):
        h[at:at + n] = s.encode().ljust(n)[:n]
    c = crc16(h[:39]) ^ (0 if good_crc else 0x0101)
    h[39], h[40] = c >> 8, c & 0xFF
    return bytes(h)


def encode_slow_data(sd_bytes60):
    """the inverse of slow_data()'s packing: 60 bytes -> 480 slow-data bits as they come off the air"""
    _, _, pat = _tables()
    bits = np.zeros(480, np.uint8)
    for bi in range(60):
        by = sd_bytes60[59 - bi]
        for k in range(8):
            pos = 479 - (bi * 8 + k)
            bits[pos] = ((by >> (7 - k)) & 1) ^ pat[pos % 24]
    return bits


def compact_to_sd_bytes(compact, marker, fill=0x20):
    """set_compacted_slow_data_bytes() of the reference's unit test: the compact bytes into every byte but each sixth"""
    b = bytearray([fill] * 60)
    b[0] = marker
    ci = 0
    for i in range(1, 60):
        if i % 6 == 0:
            continue
        if ci < len(compact):
            b[i] = compact[ci]
            ci += 1
    return bytes(b)


def encode_voice(ambe_frames, sd480):
    """21 AMBE frames [21][4][24] + 480 slow-data bits -> the 1992 bits behind a voice sync"""
    w, x, _ = _tables()
    out = np.zeros(VOICE_SYMS, np.uint8)
    for j in range(FRAMES):
        out[96 * j:96 * j + 72] = ambe_frames[j][w, x]
        if j < SD_FRAMES:
            out[96 * j + 72:96 * j + 96] = sd480[24 * j:24 * j + 24]
    return out


def bits_to_symbols(bits, neg, level=1.0, center=0.0, rng=None, noise=0.0):
    """two-level symbols whose slice (bits2 with this polarity) gives bits back; optional noise"""
    b = np.asarray(bits, np.uint8) ^ (1 if neg else 0)
    s = np.where(b == 0, center + level, center - level).astype(np.float32)
    if rng is not None and noise > 0:
        s = (s + rng.standard_normal(len(s)) * noise).astype(np.float32)
    return s


def header_air_symbols(h41, neg, level=1.0, center=0.0):
    """the 660 header symbols whose soft costs decode to h41: the cost of a high symbol is near 0xFFFF (bit 1), whatever the
    polarity of the sync (gmsk_soft_symbol_to_viterbi_cost() reads no sync type)"""
    a = encode_header(h41)
    return np.where(a == 1, center + level, center - level).astype(np.float32)
