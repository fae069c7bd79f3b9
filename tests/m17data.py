"""Test helpers for M17 packet and BERT frames: frame construction with the REFERENCE's own encoder (oracle/_ref: m17_algorithms.c
compiled where it lies), the restatement of processM17PKT() / processM17BRT() and of the state behind them on the oracle's exports
(orc_m17_soft_cost, orc_m17_rand_bit, orc_m17_interleave_index, orc_m17_viterbi_decode, orc_nxdn_conv_decode, orc_m17_crc16), and the
whole-stream decode the device is checked against.  TEST INFRASTRUCTURE - the product never imports this."""
import ctypes as C
import os

import numpy as np

import m17
import orc
import rx4

FILLER = np.array([1, 1, 3, 3], np.int8)         # + + - -: every eight-symbol window of it is three or more signs from each M17 word
LEAD_IN = np.array([1, 3, 1], np.int8)           # ... and behind these three the preamble is matched the right way up


class Prbs9RxState(C.Structure):  # == m17_prbs9_rx_state (src/protocol/m17/m17_algorithms.h)
    _fields_ = [("lfsr", C.c_uint16), ("lock_count", C.c_uint16), ("window_bits", C.c_uint16), ("window_errors", C.c_uint16),
                ("total_bits", C.c_uint32), ("total_errors", C.c_uint32), ("resync_count", C.c_uint32), ("locked", C.c_uint8)]


def _r():
    r = m17._r()
    VP = C.c_void_p
    r.m17_packet_metadata_byte.argtypes = [C.c_uint8, C.c_uint8, VP]
    r.m17_packet_parse_metadata_byte.argtypes = [C.c_uint8, VP, VP]
    r.m17_packet_app_bytes_from_eof.argtypes = [C.c_uint8, C.c_uint8, VP]
    r.m17_packet_build_type1_bits.argtypes = [VP, C.c_uint8, VP]
    r.m17_packet_encode_type1_bits.restype = C.c_uint16
    r.m17_packet_encode_type1_bits.argtypes = [VP, VP, VP]
    r.m17_bert_encode_type1_bits.restype = C.c_uint16
    r.m17_bert_encode_type1_bits.argtypes = [VP, VP, VP]
    r.m17_prbs9_fill_bits.argtypes = [VP, VP, C.c_uint16]
    r.m17_prbs9_rx_init.argtypes = [VP, C.c_uint16]
    r.m17_prbs9_rx_push_bit.argtypes = [VP, C.c_uint8]
    r.CNXDNConvolution_decode.argtypes = [C.c_uint8, C.c_uint8]
    r.CNXDNConvolution_chainback.argtypes = [VP, C.c_uint]
    return r


# ---- frames built by the reference's encoder ------------------------------------------------------------------------------------
def metadata_byte(eof, value):
    b = C.c_uint8(0)
    assert _r().m17_packet_metadata_byte(eof, value, C.byref(b)) == 0
    return int(b.value)


def pkt_frame(chunk25, meta):
    """-> 192 dibits: packet sync word + m17_packet_build_type1_bits / m17_packet_encode_type1_bits (K = 5 encoder, P3, interleave,
    randomise) of 25 chunk bytes and a metadata byte (any value: the invalid ones are test cases)"""
    r = _r()
    bits = np.unpackbits(np.asarray(chunk25, np.uint8))
    assert bits.size == 200
    t1, rnd, fr = np.zeros(216, np.uint8), np.zeros(368, np.uint8), np.zeros(192, np.uint8)
    r.m17_packet_build_type1_bits(bits.ctypes.data, meta, t1.ctypes.data)
    assert r.m17_packet_encode_type1_bits(t1.ctypes.data, rnd.ctypes.data, None) == 368
    r.m17_frame_build_dibits(m17.SYNC_PKT, rnd.ctypes.data, fr.ctypes.data)
    return fr


def packet_bytes(app):
    """application bytes -> the bytes on the air: application + CRC16"""
    app = np.asarray(app, np.uint8)
    c = int(_r().m17_crc16(np.ascontiguousarray(app).ctypes.data, len(app)))
    return np.concatenate([app, np.array([c >> 8, c & 0xFF], np.uint8)])


def packet_frames(total):
    """the bytes on the air -> [192 dibits] per frame: counters 0, 1, .. and the EOF frame with its byte count"""
    total = np.asarray(total, np.uint8)
    n = max(1, (len(total) + 24) // 25)
    pad = np.zeros(25 * n, np.uint8)
    pad[:len(total)] = total
    out = []
    for k in range(n):
        last = k == n - 1
        out.append(pkt_frame(pad[25 * k:25 * k + 25], metadata_byte(1, len(total) - 25 * k) if last else metadata_byte(0, k)))
    return out


class BertTx:
    """the PRBS9 transmitter: frames of 197 bits, the register carried from frame to frame"""

    def __init__(self, lfsr=1):
        self.lfsr = C.c_uint16(lfsr)

    def frame(self, flip=()):
        r = _r()
        t1, rnd, fr = np.zeros(208, np.uint8), np.zeros(368, np.uint8), np.zeros(192, np.uint8)
        r.m17_prbs9_fill_bits(C.byref(self.lfsr), t1.ctypes.data, 197)
        for i in flip:
            t1[i] ^= 1
        assert r.m17_bert_encode_type1_bits(t1.ctypes.data, rnd.ctypes.data, None) == 368
        r.m17_frame_build_dibits(m17.SYNC_BRT, rnd.ctypes.data, fr.ctypes.data)
        return fr, t1[:197].copy()


def filler(n):
    """n symbols no M17 word is matched in, ending with the three the next preamble wants before it"""
    body = np.tile(FILLER, n // 4 + 2)[-(n - 3):]          # (whatever n is, the same symbols stand before the lead-in)
    return np.concatenate([body, LEAD_IN])


def head(src="N0CALL"):
    """preamble + LSF (packet mode)"""
    bits, _ = m17.lsf_bits(m17.encode_callsign("ALL"), m17.encode_callsign(src), type_word=0x0002)
    return [m17.repeating(m17.PREAMBLE), m17.lsf_frame(bits)]


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def parse_metadata(b):
    """m17_packet_parse_metadata_byte -> (rc, eof, value)"""
    if b & 3:
        return -1, 0, 0
    eof, val = (b >> 7) & 1, (b >> 2) & 0x1F
    if eof and (val == 0 or val > 25):
        return -1, 0, 0
    return 0, eof, val


def app_bytes_from_eof(full_frames, last):
    """m17_packet_app_bytes_from_eof -> (rc, application bytes)"""
    if full_frames >= 33 or last == 0 or last > 25:
        return -1, 0
    total = full_frames * 25 + last
    if total < 2:
        return -1, 0
    return 0, total - 2


class Prbs9Rx:
    """m17_prbs9_rx_push_bit on {locked, lfsr, lock_count, window_bits, window_errors, total_bits, total_errors, resyncs}"""

    def __init__(self):
        self.reset()

    def reset(self):
        self.locked, self.lfsr, self.lock_count, self.wbits, self.werr, self.bits, self.errs, self.resyncs = 0, 1, 0, 0, 0, 0, 0, 0

    def state(self):
        return [self.locked, self.lfsr, self.lock_count, self.wbits, self.werr, self.bits, self.errs, self.resyncs]

    def push(self, bit):
        if self.lfsr == 0:
            self.lfsr = 1
        expected = ((self.lfsr >> 8) ^ (self.lfsr >> 4)) & 1
        if self.locked:
            self.lfsr = ((self.lfsr << 1) | expected) & 0x1FF
            self.bits += 1
            self.wbits += 1
            if expected != bit:
                self.errs += 1
                self.werr += 1
            if self.wbits >= 128:
                if self.werr > 18:
                    self.locked, self.lock_count = 0, 0
                    self.resyncs += 1
                self.wbits = self.werr = 0
            return
        self.lock_count = self.lock_count + 1 if expected == bit else 0
        self.lfsr = ((self.lfsr << 1) | bit) & 0x1FF
        if self.lock_count >= 18:
            self.locked, self.wbits, self.werr = 1, 0, 0


_il = None


def _tables():
    global _il
    if _il is None:
        o = m17._o()
        _il = (np.array([o.orc_m17_interleave_index(i) for i in range(368)]), np.array([o.orc_m17_rand_bit(i) for i in range(368)], np.uint8))
    return _il


def pkt_decode(sym184, thr5):
    """processM17PKT() up to its checks: 184 soft symbols + the thresholds the sync left -> (26 bytes, path cost, 420 costs)"""
    o = m17._o()
    o.orc_m17_viterbi_decode.restype = C.c_uint32
    o.orc_m17_viterbi_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    il, rand = _tables()
    t = np.ascontiguousarray(thr5, np.float32)
    rnd = np.array([o.orc_m17_soft_cost(C.c_float(float(sym184[i >> 1])), t.ctypes.data, i & 1) for i in range(368)], np.int64)
    rnd = np.where(rand == 1, 0xFFFF - rnd, rnd)
    bits = rnd[il]
    cost = np.full(420, 0x7FFF, np.uint16)      # P3 = {1, 1, 1, 1, 1, 1, 1, 0}
    keep = np.flatnonzero(np.arange(420) % 8 != 7)
    cost[keep] = bits[:len(keep)]
    assert len(keep) == 368
    by = np.zeros(48, np.uint8)
    pc = o.orc_m17_viterbi_decode(by.ctypes.data, cost.ctypes.data, 420)
    return by[1:27].copy(), int(pc), cost


def brt_symbols(dibits184):
    """hard dibits -> de-randomised, de-interleaved -> P2 to 402 symbol values (bit << 1, the cut bit 0)"""
    o = m17._o()
    d = np.ascontiguousarray(dibits184, np.uint8)
    bits = np.zeros(368, np.uint8)
    o.orc_m17_payload_bits(d.ctypes.data, bits.ctypes.data)
    sym, x = np.zeros(402, np.uint8), 0
    for i in range(402):
        if i % 12 != 11 and x < 368:
            sym[i] = bits[x] << 1
            x += 1
    return sym


def nxdn_chainback(sym, n_steps, n_bits):
    o = m17._o()
    o.orc_nxdn_conv_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    s = np.ascontiguousarray(sym, np.uint8)
    metrics, out = np.zeros(16, np.uint16), np.zeros((n_bits + 7) // 8, np.uint8)
    o.orc_nxdn_conv_decode(s.ctypes.data, None, n_steps, metrics.ctypes.data, out.ctypes.data, n_bits)
    return out


def brt_decode(dibits184):
    """processM17BRT() up to the receiver -> 25 bytes (197 bits, most significant first)"""
    return nxdn_chainback(brt_symbols(dibits184), 201, 197)


class DataState:
    """what the reference carries between frames: state->m17_pkt, m17_pbc_ct and the BERT receiver"""

    def __init__(self):
        self.pkt, self.pbc, self.rx = np.zeros(850, np.uint8), 0, Prbs9Rx()

    def clear(self):
        self.pkt[:] = 0
        self.pbc = 0

    def carrier_loss(self):                                  # no_carrier_reset_m17_and_sample_buffers, engine.c:2169-2184
        self.clear()
        self.rx.reset()

    def eot(self):                                           # dispatch_m17.c:39-50: the count, not the buffer
        self.pbc = 0
        self.rx.reset()

    def packet_frame(self, p26):
        """processM17PKT() :3100-3150 -> (status, completed packet or None)"""
        rc, eof, val = parse_metadata(int(p26[25]))
        if rc:
            self.clear()
            return 1, None
        ptr = min(self.pbc * 25, 825)
        if not eof and val != self.pbc:
            self.clear()
            return 2, None
        app, end = 0, ptr + 25
        if eof:
            rc, app = app_bytes_from_eof(self.pbc, val)
            if rc:
                self.clear()
                return 3, None
            end = ptr + val
        self.pkt[ptr:ptr + 25] = p26[:25]
        if eof:
            app = min(app, 823)
            ok = m17.crc16(self.pkt[:app]) == ((int(self.pkt[app]) << 8) | int(self.pkt[app + 1]))
            done = dict(bytes=self.pkt[:end].copy(), app_len=app, crc_ok=int(ok))
            self.clear()
            return (7 if ok else 6), done
        if self.pbc >= 32:
            self.clear()
            return 5, None
        self.pbc += 1
        return 4, None

    def bert_frame(self, b25):
        for bit in np.unpackbits(np.asarray(b25, np.uint8))[:197]:
            self.rx.push(int(bit))


def decode_stream_data(out):
    """out = OracleFsk4Rx.run() of the M17 profile -> (frames, packets): m17.decode_stream's list, one entry per accepted sync, with
    packet frames carrying pkt26 / cost, BERT frames bits25, every entry pkt_status / pkt_count / brt_state / reset (carrier loss
    applied here), and the completed packets {bytes, app_len, crc_ok, sync} in order.  Carrier loss is read off the loop's own flags:
    it is declared at the 1800th symbol hunted in a row, so it lies before a sync that 1800 or more symbols without a flag precede."""
    frames = m17.decode_stream(out)
    assert len(frames) == len(out["sync_pos"])
    fl = np.asarray(out["fl"])
    busy = np.flatnonzero(fl & 3)
    st, packets = DataState(), []
    for k, f in enumerate(frames):
        pos = f["pos"]
        before = busy[busy < pos]
        hunted = pos - (int(before[-1]) + 1 if len(before) else 0)
        f["reset"] = hunted >= 1800
        if f["reset"]:
            st.carrier_loss()
        f["pkt_status"], f["pkt_count"] = 0, st.pbc
        if f["kind"] == "eot":
            st.eot()
        elif f["kind"] == "pkt":
            f["pkt26"], f["cost"], f["cost420"] = pkt_decode(out["sym"][pos + 1:pos + 185], out["sync_thr"][k])
            f["pkt_status"], done = st.packet_frame(f["pkt26"])
            if done:
                done["sync"] = k
                packets.append(done)
        elif f["kind"] == "brt":
            f["bits25"] = brt_decode(out["rec4"][pos + 1:pos + 185, 0])
            st.bert_frame(f["bits25"])
        f["brt_state"] = st.rx.state()
    return frames, packets


def protocol_of(app):
    """the packet's protocol identifier (M17 specification, packet superframe: one byte; 0x05 = SMS) -> (identifier, text or None)"""
    if len(app) == 0:
        return None, None
    ident = int(app[0])
    text = bytes(app[1:]).split(b"\x00")[0].decode("utf-8", "replace") if ident == 0x05 else None
    return ident, text


# ---- the streams of tests/golden/m17_data_streams.npz (make_golden_m17data.py) through the pinned CPU pipeline -------------------
STREAMS = ("a", "b", "c", "d1", "d2", "e", "f", "g0", "g1", "g2", "g3", "g4", "g5", "h")
GAPS = (1790, 1793, 1795, 1800, 1805, 1810)


def golden_streams():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "m17_data_streams.npz"))
    return {k: g[k] for k in g.files}


def modulate(dibits, seed, tail=1200):
    import p25gen
    return p25gen.modulate_cu8(np.asarray(dibits, np.int8), len(dibits) * 10 + tail, lead=20, seed=seed, noise=0.02)


def channel_dibits(g, names):
    """the named streams one behind the other (a few symbols nothing matches in first: the first preamble is then matched the right way up)"""
    return np.concatenate([filler(24)] + [g[n] for n in names])


CHANNELS = (("a", "b", "d1", "d2", "e", "f", "g0", "g3"), ("c", "h", "g1", "g2", "g4", "g5"), ("a", "h"))   # the third one negated: stream (i)

_cache = {}


def channel_disc(c):
    """discriminator stream of test channel c (0 .. 2) through the pinned front end, all three of one length; computed once"""
    if not _cache:
        g = golden_streams()
        dib = [channel_dibits(g, names) for names in CHANNELS]
        n = max(len(d) for d in dib) * 10 + 1200
        for k, d in enumerate(dib):
            import p25gen
            x = orc.OracleFrontEnd(profile=2).run_cu8(p25gen.modulate_cu8(d, n, lead=20, seed=11 + k, noise=0.02), 8192)
            _cache[k] = -x if k == 2 else x
    return _cache[c]


def batch(B):
    """-> (x [B][n] float32, [(channel, roll)]): the three channels round and round, each round one sample later (rolls 0 .. 9)"""
    plan = [(i % 3, (i // 3) % 10) for i in range(B)]
    return np.stack([np.roll(channel_disc(c), r) for c, r in plan]), plan


_want = {}


def channel_want(c, roll=0, max_sync=None):
    """(oracle loop output, frames, packets) of test channel c rolled by `roll` samples, computed once"""
    if (c, roll) not in _want:
        x = np.roll(channel_disc(c), roll)
        out = rx4.OracleFsk4Rx(rx4.profile(rx4.PROTO_M17)).run(x, max_sync=max_sync or len(x) // 80 + 8)
        _want[(c, roll)] = (out,) + decode_stream_data(out)
    return _want[(c, roll)]


def stream_want(x):
    """the same for any discriminator stream"""
    out = rx4.OracleFsk4Rx(rx4.profile(rx4.PROTO_M17)).run(x, max_sync=len(x) // 80 + 8)
    return (out,) + decode_stream_data(out)
