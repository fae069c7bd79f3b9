"""The CPU side of the P25 Phase 2 chain object's tests (tests/test_chain_p25p2_gpu.py, tests/test_chain_p25p2_short_calls_gpu.py; floors in
tests/test_chain_p25p2_short_calls_traffic.py): the whole-stream reference with the demodulator's blocks cut the way the chain cuts them
(oracle CQPSK front end -> oracle/ddn_oracle_cqrx.c -> tests/p2seq.py -> the vocoder restatement), synthetic voice channels, the short-call
cases, and the comparison of what a chain filed call by call with that reference.  No device, no bindings beyond orc, p2seq, mbe."""
import functools

import numpy as np

import orc
import p2seq

CARRY = 720          # a group = 20 sync dibits + 700: the records the chain carries from call to call
FLUSH_SCAN = 20      # at flush the carried 720 hold at most one more whole group, behind a sync among their first 20

# calls at or below the carry (720 symbols = 5760 samples at 48 kHz) on the capture (96000 samples, run whole): a third of the carry with
# the boundaries off the symbol edges, half the carry, exactly the carry, the carry plus one sample, one demodulator block, one block plus
# the shortest ragged block the demodulator takes
CAPTURE = "iq_p25p2_cc.npz"
CAPTURE_CALLS = [1999, 2880, 5760, 5761, 8192, 8196]
# (samples per symbol, sample rate, samples per call) on a 10-group synthetic voice stream: 29 calls at 1999
VOICE_CALLS = [(8, 48000, 1999), (8, 48000, 5761), (4, 24000, 999), (4, 24000, 2881)]
VOICE_GROUPS = 10
VOICE_SITES = [(0x12345, 0x2A1, 0x3C1), (0xBEE00, 0x164, 0x161), (0x5A5A5, 0x0F3, 0x293)]
FLUSH_CUT = 6        # calls of VOICE_CALLS[0] after which a flush files a group on the first channel and none on the second
VOICE_SHIFT = 777    # samples the second channel lags the first by at 8 samples per symbol (388 at 4)
# the wide case: more channels than a wavefront holds, every one out of step with the others - channel c lags by WIDE_SHIFT * c samples
# (at 97 a channel the last channels lose a third group to the lag and seven of them fall to one good ESS, below the traffic floor; at 47 a
# channel every channel holds the floors and the lags still spread over half a group)
WIDE_B, WIDE_SHIFT, WIDE_CALL, WIDE_PCM = 67, 47, 1999, (0, 1, 63, 64, 66)
WIDE_NOSITE = 65     # the wide case's channel whose seed is 0: no valid site, the scrambled bursts are skipped


def seed44(site):
    w, s, nac = site
    return w * 16777216 + s * 4096 + nac


def oracle_groups(iq, n_call, rate=48000, block_len=8192):
    """-> (symbols, rec4, flags, sync positions, bits [G][1400], llr [G][1400], new symbols per call) of the whole stream: the
    demodulator runs per call in block_len blocks and a shorter last one, like the chain's"""
    x = ((iq.astype(np.float32) - 127.5) * np.float32(1.0 / 127.5)).astype(np.float32)
    fe = orc.OracleCqpskFe(rate=rate, sym_rate=6000)
    per = [fe.run(x[k:k + n_call], block_len) for k in range(0, len(x), n_call)]
    sym = np.concatenate(per)
    rec, fl = orc.OracleCqRx(orc.CQ_P25P2).run(sym)
    pos = [int(p) for p in np.flatnonzero(fl & 2) if p + 700 < len(sym)]
    bits = np.zeros((len(pos), 1400), np.uint8)
    llr = np.zeros((len(pos), 1400), np.int16)
    for k, p in enumerate(pos):
        d = rec[p + 1:p + 701]
        bits[k, 0::2], bits[k, 1::2] = (d[:, 0] >> 1) & 1, d[:, 0] & 1
        llr[k, 0::2], llr[k, 1::2] = d[:, 2], d[:, 3]
    return sym, rec, fl, pos, bits, llr, np.array([len(p) for p in per])


def voice_of_rows(rows, slot):
    """the AMBE frames [F][4][24] of the 4V / 2V rows filed under logical channel `slot`, in air order"""
    fr = [r["fr"][f] for r in rows if r["slot"] == slot and r["action"] in (p2seq.A_4V, p2seq.A_2V)
          for f in range(4 if r["action"] == p2seq.A_4V else 2)]
    return np.array(fr, np.uint8).reshape(-1, 4, 24)


def voice_reference(rows, channel, pcm=True):
    """per logical channel: (parameter bits [F][49], frame results [F][5], pcm [F][160] | None) of the whole stream in one go; talk path
    = channel * 2 + slot, as the chain numbers its vocoder's paths"""
    import ddn
    import mbe
    out = []
    for slot in (0, 1):
        fr = voice_of_rows(rows, slot)
        if not len(fr):
            out.append((np.zeros((0, 49), np.uint8), np.zeros((0, 5), np.int32), np.zeros((0, 160), np.float32) if pcm else None))
            continue
        bits, res, _ = mbe.oracle_frame_decode(ddn.MBE_AMBE, fr, soft=True)
        p = mbe.oracle_process_stream(mbe.OracleVocoder(ddn.MBE_AMBE, 1), ddn.MBE_AMBE, bits, 2 * channel + slot, res) if pcm else None
        out.append((bits, res, p))
    return out


def whole_stream(iq, n_call, wacn, sysid, nac, rate=48000, channel=0, pcm=True, block_len=8192):
    """the reference of one channel, from nothing the device returns: {"n": symbols, "new": per call, "pos": sync positions with 700
    records behind, "bits" / "llr": their groups, "rows": p2seq.run_groups over all of them, "voice": voice_reference() per logical channel}"""
    sym, rec, fl, pos, bits, llr, new = oracle_groups(iq, n_call, rate, block_len)
    rows = p2seq.run_groups(bits, llr, wacn, sysid, nac, p2seq.new_state())
    return {"n": len(sym), "new": new, "pos": pos, "bits": bits, "llr": llr, "rows": rows, "voice": voice_reference(rows, channel, pcm)}


def synthetic_channel(seed, n_groups, site, sps, shift=0):
    """a TDMA channel whose logical channel 0 carries a voice call (4V 4V 4V 4V 2V, valid AMBE 3600x2450 frames planted through the burst
    interleave), a sync in front of every group, as cu8 I/Q at `sps` samples per symbol, delayed by `shift` samples of mid-scale and cut
    back to its length -> (iq u8 [n][2], the planted parameter bits [F][49])"""
    import mbe
    rng = np.random.default_rng(seed)
    frames = []

    def voice():
        b = mbe.random_ambe_bits(rng, ())
        frames.append(b)
        return mbe.ambe_encode(b)
    w, s, nac = site
    gb, gl = p2seq.make_stream(rng, n_groups, w, s, nac, start_sf=4 * (seed % 3), plan=None, voice=voice)
    dib = []
    for g in range(n_groups):
        dib.append(p2seq.SYNC20)
        dib.append((gb[g, 0::2] << 1) | gb[g, 1::2])
    iq = orc.modulate_dqpsk_cu8(np.concatenate(dib), sps, seed=seed)
    if shift:
        iq = np.concatenate([np.full((shift, 2), 127, np.uint8), iq[:len(iq) - shift]])
    return np.ascontiguousarray(iq), np.stack(frames)


@functools.lru_cache(maxsize=None)
def capture_case(n_call, site=True):
    """-> (iq u8 [n_total][2], whole_stream() reference) of the capture run whole at n_call samples per call; site False = seed 0"""
    import p2capture
    from conftest import golden
    iq = np.ascontiguousarray(golden(CAPTURE)["iq"])
    iq = iq[:(len(iq) // n_call) * n_call]
    wsn = (p2capture.WACN, p2capture.SYSID, p2capture.NAC) if site else (0, 0, 0)
    return iq, whole_stream(iq, n_call, *wsn, pcm=False)


def _synthetic_case(n_channels, sps, rate, n_call, shift_of, nosite=(), pcm_on=None, n_streams=None):
    # (n_streams: that many streams are made, channel c takes stream c % n_streams at its own lag - a multiple of three keeps the sites)
    base = [synthetic_channel(k, VOICE_GROUPS, VOICE_SITES[k % 3], sps) for k in range(min(n_channels, n_streams or n_channels))]
    made = []
    for c in range(n_channels):
        q, p = base[c % len(base)]
        d = shift_of(c)
        made.append((np.concatenate([np.full((d, 2), 127, np.uint8), q[:len(q) - d]]), p))
    n_total = (min(len(iq) for iq, _ in made) // n_call) * n_call
    iq = np.ascontiguousarray(np.stack([q[:n_total] for q, _ in made]))
    sites = [(0, 0, 0) if c in nosite else VOICE_SITES[c % 3] for c in range(n_channels)]
    refs = [whole_stream(iq[c], n_call, *sites[c], rate=rate, channel=c, pcm=pcm_on is None or c in pcm_on) for c in range(n_channels)]
    return iq, [p for _, p in made], refs, [0 if c in nosite else seed44(sites[c]) for c in range(n_channels)]


@functools.lru_cache(maxsize=None)
def voice_case(sps, rate, n_call):
    """two channels of two sites, the second lagging by VOICE_SHIFT -> (iq u8 [2][n_total][2], planted bits, references, chain seeds)"""
    return _synthetic_case(2, sps, rate, n_call, lambda c: c * (VOICE_SHIFT * sps // 8))


@functools.lru_cache(maxsize=None)
def wide_case():
    """WIDE_B channels of nine streams, channel c lagging by WIDE_SHIFT * c samples, three sites in rotation and one channel without; PCM
    references on WIDE_PCM only"""
    return _synthetic_case(WIDE_B, 8, 48000, WIDE_CALL, lambda c: WIDE_SHIFT * c, nosite=(WIDE_NOSITE,), pcm_on=WIDE_PCM, n_streams=9)


def wide_clean():
    """the wide case's channels whose reference decode is a contiguous run of the planted frames from its first frame on"""
    iq, planted, refs, seeds = wide_case()
    return [c for c in range(WIDE_B) if seeds[c] and planted_run(refs[c]["voice"][0][0], planted[c])]


def planted_run(bits, planted):
    """the parameter bits that went in come out: `bits` is a contiguous part of what was sent (the first group or two fall before the
    loop's first sync)"""
    if len(bits) < 8:
        return False
    k0 = next((k for k in range(len(planted) - 8) if np.array_equal(planted[k:k + 8], bits[:8])), None)
    return k0 is not None and np.array_equal(bits, planted[k0:k0 + len(bits)])


def widen(iq):
    """cu8 -> cf32 exactly as the chain's cu8 input path scales it, (u8 - 127.5) * (1 / 127.5) in float32: the same samples.  (Dividing by
    127.5 instead rounds 4 samples in 10 one ulp apart, and the demodulator then turns out another soft decision here and there - in
    the oracle as on the device.)"""
    return ((iq.astype(np.float32) - np.float32(127.5)) * np.float32(1.0 / 127.5)).astype(np.float32)


def scan_ranges(new, flush=True):
    """the stream positions [lo, hi) whose syncs every call (and the flush) decodes: a call's row is the 720 carried records and its new
    ones, and a sync is decoded in the call that brings the 720th record behind it"""
    out, base = [], 0
    for n in new:
        out.append((base - CARRY, base - CARRY + int(n)))
        base += int(n)
    if flush:
        out.append((base - CARRY, base - CARRY + FLUSH_SCAN))
    return out


def groups_per_call(ws):
    """how many groups every call of the reference `ws` (and the flush behind them) decodes"""
    return [sum(lo <= p < hi for p in ws["pos"]) for lo, hi in scan_ranges(ws["new"])]


def compare(got, want_rows, c):
    """got = (info [C][G][4][8], payload, ambe_fr, ambe_rel, ess) as P25P2Groups.run() and the chain file them; want_rows = run_groups()
    dicts of channel c (rows in order, four per group, all G groups)"""
    info, pay, fr, rel, ess = got
    G = info.shape[1]
    n = 0
    for k, w in enumerate(want_rows):
        g, ts = divmod(k, 4)
        i = info[c, g, ts]
        tag = (c, g, ts, w["action"])
        assert (i[0], i[1], i[2], i[3], i[4]) == (w["duid"], w["isch"], w["offset"], w["slot"], w["action"]), (tag, i.tolist())
        a = w["action"]
        if a in (p2seq.A_4V, p2seq.A_2V):
            assert i[6] == w["fourv"], tag
            assert np.array_equal(fr[c, g, ts], w["fr"]) and np.array_equal(rel[c, g, ts], w["rel"]), tag
            if a == p2seq.A_2V:
                assert i[5] == w["ec"] and bool(i[7] & 8) == bool(w["ess_ok"]) and np.array_equal(ess[c, g, ts], w["ess"]), (tag, i.tolist(), w["ec"])
        elif a in (p2seq.A_SACCH_S, p2seq.A_SACCH_C, p2seq.A_FACCH_C, p2seq.A_FACCH_S, p2seq.A_LCCH_C, p2seq.A_LCCH_S):
            assert i[5] == w["ec"] and (i[7] & 1) == w["used"] and bool(i[7] & 2) == bool(w["crc12"]), (tag, i.tolist(), w["ec"], w["used"])
            if a not in (p2seq.A_FACCH_C, p2seq.A_FACCH_S):
                assert bool(i[7] & 4) == bool(w["crc16"]), tag
            assert np.array_equal(pay[c, g, ts], w["payload"]), tag
        else:
            assert i[5] == 0 and i[7] == 0 and not pay[c, g, ts].any() and not fr[c, g, ts].any(), tag
        n += 1
    assert n == G * 4
    return n


class Filed:
    """what a chain filed for one channel, call by call (the flush is the last call): new records, groups with their stream positions and
    result rows, dropped syncs, and per logical channel the voice stage's parameter bits and PCM"""

    def __init__(self):
        self.new, self.n_groups, self.dropped, self.pos = [], [], [], []
        self.rows = [[] for _ in range(5)]                 # info [4][8], payload [4][180], ambe_fr [4][4][4][24], ambe_rel, ess [4][96] per group
        self.vbits, self.pcm = ([], []), ([], [])

    def add_call(self, new, n_groups, group_pos, arrays, dropped):
        base = sum(self.new)
        self.new.append(int(new))
        self.n_groups.append(int(n_groups))
        self.dropped.append(int(dropped))
        for g in range(int(n_groups)):
            self.pos.append(base + int(group_pos[g]) - CARRY)
            for k, a in enumerate(arrays):
                self.rows[k].append(np.array(a[g]))

    def add_voice(self, slot, bits, pcm):
        self.vbits[slot].append(np.array(bits))
        self.pcm[slot].append(np.array(pcm))

    def got(self):
        shapes = ((4, 8), (4, 180), (4, 4, 4, 24), (4, 4, 4, 24), (4, 96))
        dt = (np.int32, np.uint8, np.uint8, np.uint8, np.uint8)
        return tuple(np.array(r, d).reshape((1, len(self.pos)) + s) for r, s, d in zip(self.rows, shapes, dt))

    def voice(self, slot):
        return (np.concatenate(self.vbits[slot]).reshape(-1, 49) if self.vbits[slot] else np.zeros((0, 49), np.uint8),
                np.concatenate(self.pcm[slot]).reshape(-1, 160) if self.pcm[slot] else np.zeros((0, 160), np.float32))


def check_filed(filed, want, tag, pcm=True, voice=True, planted=None):
    """every group once, whole and in order: a channel's Filed record against its whole_stream() reference"""
    assert sum(filed.new) == want["n"], (tag, sum(filed.new), want["n"])
    assert filed.dropped[-1] == 0, (tag, filed.dropped)
    assert filed.pos == want["pos"], (tag, filed.pos, want["pos"])
    assert filed.new == want["new"].tolist() + [0] and filed.n_groups == groups_per_call(want), (tag, filed.new, filed.n_groups)
    try:
        compare(filed.got(), want["rows"], 0)
    except AssertionError as e:
        raise AssertionError((tag,) + e.args) from None
    if not voice:
        return
    for slot in (0, 1):
        bits, res, wpcm = want["voice"][slot]
        gb, gp = filed.voice(slot)
        assert np.array_equal(gb, bits), (tag, slot, len(gb), len(bits))
        if pcm:
            assert np.array_equal(gp.view(np.uint32), wpcm.view(np.uint32)), (tag, slot)
    if pcm:
        assert float(np.abs(filed.voice(0)[1]).sum()) > 0, tag                 # logical channel 0 carries the call: not silence
    if planted is not None:
        assert planted_run(filed.voice(0)[0], planted), tag
