"""Synthetic DMR MS and direct-mode traffic for the tests of the MS stage: data bursts of every data type and voice units behind the
MS / direct-mode TS1 / TS2 words.  A transmitter keys every other 144-dibit slot, so the air is TDMA frames of 288 dibits - a burst,
then 144 dibits that are not its own (random here).  A voice unit is six frames: the bootstrap burst with the voice word, then five
bursts whose sync field is EMB + 32 bits of embedded signalling - the BPTC(128,77) link control in the fragments the reference reads
(bursts 2..5; the sixth carries none).  The codes are tests/dmrgen.py's (found by search against the oracle's decoders).
TEST INFRASTRUCTURE - the product never imports this."""
import numpy as np

import dmr_ms
import dmrgen
import rx4

WORDS = {2: rx4.DMR_MS_DATA, 3: rx4.DMR_MS_VOICE, 4: rx4.DMR_DM1_DATA, 5: rx4.DMR_DM2_DATA, 6: rx4.DMR_DM1_VOICE, 7: rx4.DMR_DM2_VOICE}
FRAME = 288


def _word_bits(word):
    return [b for ch in word for b in ((1, 1) if ch == "3" else (0, 1))]


def _cach(rng):
    tact = dmrgen.encode(0, [1, 0, int(rng.integers(0, 2)), int(rng.integers(0, 2))])
    cach = np.zeros(24, np.uint8)
    cach[:7] = tact
    cach[7:] = rng.integers(0, 2, 17)
    return [int(cach[rx4.CACH_IL[k]]) for k in range(24)]


def _dibits(bits):
    assert len(bits) == 288
    return np.array([2 * bits[2 * i] + bits[2 * i + 1] for i in range(144)], np.int8)


def burst(pat, cc, dtype, info196, rng, hurt_slot_type=False):
    """one 144-dibit data burst behind sync pattern `pat`; hurt_slot_type: three flips the Golay(20,8) decoder refuses"""
    st = dmrgen.encode(5, dmrgen._bits(cc, 4) + dmrgen._bits(dtype, 4))
    info = list(map(int, info196))
    cach = _cach(rng)
    while True:
        s = st.copy()
        if hurt_slot_type:
            s[rng.choice(20, 3, replace=False)] ^= 1
        d = _dibits(cach + info[:98] + list(s[:10]) + _word_bits(WORDS[pat]) + list(s[10:]) + info[98:])
        if not hurt_slot_type or dmr_ms.data_fields(pat, d)[0] == 2:
            return d


def voice_burst(pat, cc, emb32, rng, lcss=0, hurt_emb=False):
    """one voice burst: pat = a voice word's pattern for the bootstrap burst, None for a burst with EMB (QR(16,7,6) over colour code, PI,
    LCSS) around 32 bits of embedded signalling; hurt_emb: three flips the decoder refuses"""
    voice = [int(x) for x in rng.integers(0, 2, 216)]
    cach = _cach(rng)
    if pat is not None:
        return _dibits(cach + voice[:108] + _word_bits(WORDS[pat]) + voice[108:])
    emb = dmrgen.encode(7, dmrgen._bits(cc, 4) + [int(rng.integers(0, 2))] + dmrgen._bits(lcss, 2))
    while True:
        e = emb.copy()
        if hurt_emb:
            e[rng.choice(16, 3, replace=False)] ^= 1
        d = _dibits(cach + voice[:108] + list(e[:8]) + [int(x) for x in emb32] + list(e[8:]) + voice[108:])
        if not hurt_emb or dmr_ms.voice_fields(2, d, np.zeros((5, 48), np.uint8))["emb_ok"] == 0:
            return d


def voice_unit(pat, cc, lc72, rng, crc5=None, hurt_emb_at=None):
    """six bursts: the bootstrap burst, then VC 2..6 with the link control in VC 2..5"""
    m = dmrgen.bptc_128x77(lc72, crc5)
    cm = [int(m[r, c]) for c in range(16) for r in range(8)]
    out = [voice_burst(pat, cc, None, rng)]
    for k in range(5):
        out.append(voice_burst(None, cc, cm[32 * k:32 * k + 32] if k < 4 else [0] * 32, rng, (1, 3, 3, 2, 0)[k], hurt_emb_at == k))
    return out


def data_info(dtype, rng, **kw):
    """the 196 info bits of a data burst of type dtype, as tests/chain_fsk4_stream.dmr_data_stream builds them"""
    if dtype == 8:
        return dmrgen.r34_info(dmrgen.r34_bytes(rng, **kw))
    if dtype == 10:
        info = rng.integers(0, 2, 196).astype(np.uint8)
        info[96:100] = 0
        c = dmrgen.crc9_confirmed_rate1(info)
        info[7:16] = [(c >> (8 - i)) & 1 for i in range(9)]
        return info
    return dmrgen.bptc_196x96(dmrgen.payload_bits(dtype, rng, **kw))


def air(bursts, rng, lead_frames=0, tail_frames=2):
    """bursts -> dibits: every burst opens a 288-dibit frame whose other half, like the frames in front and behind, is random"""
    out = [rng.integers(0, 4, FRAME * lead_frames).astype(np.int8)]
    for b in bursts:
        out += [b, rng.integers(0, 4, FRAME - 144).astype(np.int8)]
    out.append(rng.integers(0, 4, FRAME * tail_frames).astype(np.int8))
    return np.concatenate(out)


def traffic(seed=77):
    """the chain test's traffic (about 1.9 s): CSBKs, every data type the handler treats differently behind the MS word, direct-mode
    TS1 / TS2 data, a refused slot type, and three voice units - MS (good link control), direct-mode TS1 (wrong checksum), direct-mode
    TS2 (good, one refused EMB) -> (dibits, the link controls sent [(bits72, good)])"""
    rng = np.random.default_rng(seed)
    D = lambda pat, ty, **kw: burst(pat, 5, ty, data_info(ty, rng, **kw), rng)
    lcs = [(rng.integers(0, 2, 72).astype(np.uint8), g) for g in (True, False, True)]
    bad = (int(np.packbits(lcs[1][0]).astype(np.int64).sum()) % 31) ^ 0x0A
    b = [D(2, 3), D(2, 3), D(2, 1), D(2, 2), D(2, 6), D(2, 7, confirmed=True, dbsn=3)]
    b += voice_unit(3, 5, lcs[0][0], rng)
    b += [D(2, 8), D(2, 8, confirmed=True, dbsn=1), D(2, 10), D(5, 3), D(4, 6), burst(2, 5, 3, data_info(3, rng), rng, hurt_slot_type=True)]
    b += voice_unit(6, 5, lcs[1][0], rng, crc5=bad)
    b += [D(5, 7), D(2, 3, good_crc=False)]
    b += voice_unit(7, 9, lcs[2][0], rng, hurt_emb_at=1)
    b += [D(2, 3)]
    return air(b, rng), lcs


_AIR = {}


def air_batch(B=8):
    """cu8 I/Q [B][samples][2] of traffic(): every channel its own delay and noise"""
    import p25gen
    if B not in _AIR:
        dib, _ = traffic()
        L = 10 * len(dib) + 4000
        L -= L % 6000                      # (calls of 2000, 30 and 10 samples divide it)
        _AIR[B] = np.stack([p25gen.modulate_cu8(dib, L, lead=300 + 137 * c, seed=20 + c, noise=0.02) for c in range(B)])
    return _AIR[B]


# ---- records for the batch entry points: no receive loop, the row is the generator's own dibits ---------------------------------------
def records(dib, rng):
    """the loop's 10-byte records of a dibit stream: byte 0 the dibit, byte 1 a reliability, the rest as a loop leaves them unread"""
    rec = np.zeros((len(dib), 10), np.uint8)
    rec[:, 0] = np.asarray(dib, np.uint8) & 3
    rec[:, 1] = rng.integers(60, 256, len(dib))
    return rec


def syncs_of(dib, rng):
    """where an MS / direct-mode word ends and nothing is held: [(p, pattern, hand-over dibits, hand-over reliabilities)] in the order the
    loop would accept them with lock_symbols = dmr_ms.LOCK (a word inside the held stretch is not seen).  The hand-over is the stream's
    own 90 dibits with two of them changed - what re-digitisation may do - so that a consumer reading the records instead shows"""
    s = "".join("3" if d >= 2 else "1" for d in dib)
    out, free = [], 0
    at = 0
    while True:
        hits = [(s.find(w, at), pat) for pat, w in WORDS.items() if s.find(w, at) >= 0]
        if not hits:
            return out
        q, pat = min(hits)
        p = q + 23
        at = q + 1
        if p < 89 or q < free:
            continue
        pre = (np.asarray(dib[p - 89:p + 1], np.uint8) & 3).copy()
        pre[rng.integers(12, 61)] ^= 1
        pre[rng.integers(12, 61)] ^= 2
        out.append((p, pat, pre, rng.integers(60, 256, 90).astype(np.uint8)))
        free = p + 1 + (dmr_ms.LOCK[1] if pat in dmr_ms.VOICE_PATS else dmr_ms.LOCK[0])


def small_traffic(seed=5):
    """the batch tests' traffic (about 3700 dibits): data bursts - one refused, one rate 3/4, one direct-mode TS2 - around one voice unit"""
    rng = np.random.default_rng(seed)
    D = lambda pat, ty, **kw: burst(pat, 3, ty, data_info(ty, rng, **kw), rng)
    lc = rng.integers(0, 2, 72).astype(np.uint8)
    b = [D(2, 3), D(5, 8, confirmed=True, dbsn=2)] + voice_unit(6, 3, lc, rng, hurt_emb_at=2) + [burst(2, 3, 6, data_info(6, rng), rng, hurt_slot_type=True), D(4, 1)]
    return air(b, rng, lead_frames=1, tail_frames=2), lc


def calls_of(rec, syncs, ends, T):
    """what a chain would hand the stage call by call: rec [n][10] and syncs (absolute positions) of one channel, ends = records held
    after each call (the last call is followed by a flush) -> [dict(row [T + new][10], cnt, new, syncs with row positions)]: a row is the
    T records before the call's first new one (zeros in front of the stream), then the new ones; a sync is listed in the first call that
    holds the T records behind it, the rest in the flush"""
    out, base, k = [], 0, 0
    for end in list(ends) + [None]:
        flush = end is None
        new = 0 if flush else end - base
        row = np.zeros((T + new, 10), np.uint8)
        lo = base - T
        src = rec[max(lo, 0):base + new]
        row[T + new - len(src):] = src
        mine = []
        while k < len(syncs) and (flush or syncs[k][0] + T < base + new):
            p, pat, pre, prel = syncs[k]
            mine.append((p - lo, pat, pre, prel))
            k += 1
        out.append(dict(row=row, cnt=T + new, new=new, syncs=mine, lo=lo))
        base += new
    return out
