"""EDACS control-channel test signals: frames as edacs() reads them (two BCH(40,28) codewords, each sent three times with the middle copy
inverted) behind a 48-symbol sync word, and their 9600-baud two-level cu8 I/Q at 48 ksps (5 samples per symbol).  TEST INFRASTRUCTURE."""
import numpy as np

import edacs


def frame_bits(msg1, msg2, flips=()):
    """240 bits: m1, ~m1, m1, m2, ~m2, m2 (40 bits each, MSB first); flips = (copy 0..5, bit 0..39) pairs flipped after encoding"""
    c = [edacs.bch(msg1), edacs.bch(msg2)]
    words = [c[0], ~c[0] & edacs.MASK40, c[0], c[1], ~c[1] & edacs.MASK40, c[1]]
    bits = np.array([(w >> (39 - i)) & 1 for w in words for i in range(40)], np.uint8)
    for j, b in flips:
        bits[40 * j + b] ^= 1
    return bits


def site_id_msg(site_id, priority=0, cc_lcn=1, scat=0, failsoft=0, aux=0, esk_mask=0):
    """a standard-mode site-ID message 1 (MT-A = 7, MT-B = 7, MT-D = 0x08 + (cc_lcn >> 5 is 0) ...) as sent under esk_mask"""
    m = (7 << 25) | (7 << 22) | (0x08 << 17) | ((cc_lcn & 0x1F) << 12) | ((priority & 7) << 9) | (scat << 7) | (failsoft << 6) | (aux << 5)
    m |= site_id & 0x1F
    return m ^ (esk_mask << 20)


def ea_site_id_msg(site_id, area, esk_mask=0):
    """an EA site-ID message 1 (MT1 = 0x1F, MT2 = 0xA) as sent under esk_mask"""
    m = (0x1F << 23) | (0xA << 19) | (((site_id >> 5) & 7) << 12) | ((area & 0x7F) << 5) | (site_id & 0x1F)
    return m ^ (esk_mask << 20)


def symbols(bits240, pat):
    """sync word + frame as signs (+1 = '1' / a high symbol): pattern 1 (+EDACS) sends a 0 high, pattern 0 (-EDACS) a 1"""
    sync = np.array([1 if ch == "1" else -1 for ch in edacs.sync_word(pat)], np.int8)
    hi = bits240 == (1 if pat == edacs.PAT_NEG else 0)
    return np.concatenate([sync, np.where(hi, 1, -1).astype(np.int8)])


def stream(rng, n_frames, pat, gap=(0, 24), msgs=None):
    """frames with idle dotting between them -> (signs, [(msg1, msg2, start symbol of the sync)])"""
    out, meta, at = [], [], 0
    for k in range(n_frames):
        g = int(rng.integers(gap[0], gap[1] + 1))
        out.append(np.tile(np.array([1, -1], np.int8), g // 2 + 1)[:g])
        at += g
        m1, m2 = msgs[k] if msgs else (int(rng.integers(0, 1 << 28)), int(rng.integers(0, 1 << 28)))
        out.append(symbols(frame_bits(m1, m2), pat))
        meta.append((m1, m2, at))
        at += 48 + edacs.FRAME
    return np.concatenate(out), meta


def modulate_cu8(signs, n, sps=5, dev=0.25, lead=211, seed=0, noise=0.02):
    """signs -> uint8 [n, 2]: 2-level FM, lightly smoothed, `lead` idle samples first"""
    rng = np.random.default_rng(seed)
    nrz = np.repeat(signs.astype(np.float64), sps)
    win = np.array([0.25, 0.5, 0.25])
    shaped = np.convolve(nrz, win, mode="same")
    f = np.zeros(n)
    m = min(n - lead, len(shaped))
    f[lead:lead + m] = shaped[:m]
    ph = 0.3 + np.cumsum(f * dev)
    i = 0.8 * np.cos(ph) + rng.normal(0, noise, n)
    q = 0.8 * np.sin(ph) + rng.normal(0, noise, n)
    out = np.empty((n, 2), np.uint8)
    out[:, 0] = np.clip(np.rint(127.5 + 127.5 * i), 0, 255)
    out[:, 1] = np.clip(np.rint(127.5 + 127.5 * q), 0, 255)
    return out
