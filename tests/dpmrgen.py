"""Test-only dPMR voice superframe encoder (the inverse of tests/dpmr.py's decode): CCH fields -> CRC7 -> six Hamming(12,8) words ->
6 x 12 interleave -> x^9 + x^5 + 1 scrambling (seed 0x1FF) -> 36 dibits; colour-code dibits; AMBE 3600x2450 frames through the
36-dibit schedule; whole transmissions (FS2 + 372 dibits per superframe).  TEST INFRASTRUCTURE - the product never imports this.

Hamming(12,8): parity bit 8 + r makes row r of the parity-check matrix the device and the oracle share (ddn_tables_fec3.h) vanish."""
import numpy as np

import dpmr
import rx4

H12_8 = (0x135, 0x26B, 0x4D7, 0x89A)        # ddn_hamming_12_8_H: bit j of a row = code bit j
FIELDS = (("fn", 0, 2), ("half", 2, 12), ("mode", 14, 3), ("version", 17, 2), ("format", 19, 2), ("emergency", 21, 1),
          ("reserved", 22, 1), ("slow", 23, 18))
SYNC = [int(ch) for ch in dpmr.FS2]


def _put(bits, at, n, v):
    for k in range(n):
        bits[at + k] = (int(v) >> (n - 1 - k)) & 1


def cch_bits(fn=0, half=0, mode=0, version=0, format=0, emergency=0, reserved=0, slow=0, crc_good=True):
    """the 48 CCH bits (fields MSB first, CRC7 over bits 0..40 in bits 41..47; crc_good=False flips its last bit)"""
    b = [0] * 48
    v = dict(fn=fn, half=half, mode=mode, version=version, format=format, emergency=emergency, reserved=reserved, slow=slow)
    for name, at, n in FIELDS:
        _put(b, at, n, v[name])
    _put(b, 41, 7, dpmr.crc7(b[:41]) ^ (0 if crc_good else 1))
    return b


def hamming_12_8(d8):
    """8 data bits -> 12-bit code word (bit j = list index j)"""
    w = sum(int(x) << j for j, x in enumerate(d8))
    return [int(x) for x in d8] + [bin(w & h & 0xFF).count("1") & 1 for h in H12_8]


def cch_dibits(bits48, flips=()):
    """48 bits -> 36 dibits; flips = (word, bit) pairs flipped in the code words before interleaving (channel errors)"""
    words = [hamming_12_8(bits48[8 * j:8 * j + 8]) for j in range(6)]
    for j, i in flips:
        words[j][i] ^= 1
    il = [0] * 72
    for j in range(6):
        for i in range(12):
            il[i * 6 + j] = words[j][i]
    s = dpmr.scramble(il)[0]
    return [s[2 * k] * 2 + s[2 * k + 1] for k in range(36)]


def color_dibits(code24):
    """a 24-bit colour-code pattern (MSB first) -> 12 dibits"""
    return [(int(code24) >> (22 - 2 * k)) & 3 for k in range(12)]


def color_pattern(col):
    return [c for c, v in dpmr.vectors()["color_codes"] if v == col][0]


def ambe_dibits(fr):
    """ambe_fr [4][24] -> the 36 dibits the schedule (rx4.ambe2450_map) reads it from"""
    m = rx4.ambe2450_map()
    return [int(fr[m[i, 0], m[i, 1]]) * 2 + int(fr[m[i, 2], m[i, 3]]) for i in range(36)]


def superframe(cch0, cch1, color24, tch):
    """372 dibits: CCH, four TCH frames, colour code, CCH, four TCH frames; cch0 / cch1 = 36 dibits each, tch = 8 x 36 dibits"""
    d = np.zeros(dpmr.FRAME, np.uint8)
    d[dpmr.CCH0:dpmr.CCH0 + 36] = cch0
    d[dpmr.CCH1:dpmr.CCH1 + 36] = cch1
    d[dpmr.CC_AT:dpmr.CC_AT + 12] = color_dibits(color24)
    for f, a in enumerate(dpmr.VOICE_AT):
        d[a:a + 36] = tch[f]
    return d


def transmission(superframes, inverted=False):
    """FS2 + 372 dibits per superframe, back to back; inverted: every dibit ^ 2 (what -xd expects on the air)"""
    d = np.concatenate([np.concatenate([np.array(SYNC, np.uint8), s]) for s in superframes])
    return d ^ 2 if inverted else d
