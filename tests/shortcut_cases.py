"""Traffic for the tests of the half-rate decoder's hard-path short cut (ddn_p25h_dev.h, half_rate_hard_path_wave) and what the
oracle's own records say about every trellis block in it: is it a path of the trellis from state 0 (the hard bits of its 196
LLRs), does it carry a zero LLR - i.e. which side of the short cut the block must take on the device.  Shared by
test_rx_handler_shortcut_gpu.py (C4FM loop) and test_cqrx_shortcut_gpu.py (CQPSK symbol-rate loop)."""
import numpy as np

import fecgen
import orc
import p25gen

NAC = 0x293
SK0 = (22, 15, 8)           # status counter at the start of a TSDU's blocks (36 - 14, then 101 symbols each); a PDU header block: 22


def _positions(n_body):
    """frame positions of the first n_body dibits that are no status symbols (one status symbol after every 35 dibits)"""
    flen = -(-n_body // 35) * 36
    stat = list(range(35, flen, 36))
    return flen, stat, [p for p in range(flen) if p not in stat]


def tsdu(rng, good, nac=NAC):
    """one TSDU of len(good) blocks -> (dibits int8, data_pos [blocks][98] frame positions of each block's dibits as sent).
    Every block is a path of the trellis; good[b] = False gives block b a CRC16 that fails.  The last-block flag (bit 7 of byte 0)
    is set on the last block only, so a block with a bad CRC does not end the TSDU early."""
    nb = len(good)
    body = list(orc.P25_FS_DIBITS) + p25gen.nid_dibits(nac, p25gen.DUID_TSBK)
    for b in range(nb):
        pay = rng.integers(0, 256, 10)
        pay[0] = (int(pay[0]) & 0x7F) | (0x80 if b == nb - 1 else 0)
        c = p25gen.crc16_ccitt(pay) ^ (0 if good[b] else 0x5A5A)
        body += list(p25gen.encode_half_rate(list(pay) + [c >> 8, c & 0xFF]))
    flen, stat, pos = _positions(len(body))
    fr = np.zeros(flen, np.int8)
    fr[pos[:len(body)]] = body
    fr[stat] = 2
    return fr, [pos[56 + 98 * b:56 + 98 * (b + 1)] for b in range(nb)]


def pdu(rng, blks, nac=NAC):
    """a data unit with a good header block and blks random data blocks -> (dibits, data_pos [1][98] of the header block)"""
    fr = p25gen.make_pdu(rng, nac, blks)
    _, _, pos = _positions(56 + 98 * (blks + 1))
    return fr, [pos[56:56 + 98]]


class Stream:
    """frames back to back with short gaps; .dib the dibits, .scale per-symbol amplitude factors"""

    def __init__(self, rng):
        self.rng, self.parts, self.n, self.marks = rng, [], 0, []

    def add(self, frame_and_pos, gap=None):
        fr, pos = frame_and_pos
        self.marks.append([[self.n + p for p in blk] for blk in pos])   # stream positions of every block's dibits
        self.parts.append(fr)
        self.n += len(fr)
        g = int(self.rng.integers(0, 30)) if gap is None else gap
        self.parts.append(np.zeros(g, np.int8))
        self.n += g
        return self.marks[-1]

    def finish(self):
        self.dib = np.concatenate(self.parts)
        self.scale = np.ones(len(self.dib))
        return self

    def push_across(self, at):
        """the dibit at stream position `at` across a decision threshold: an outer level pulled inside the inner threshold, an inner
        one pushed beyond it - its low bit comes out wrong, at full sign and a good margin"""
        self.scale[at] = 0.45 if self.dib[at] in (1, 3) else 2.6

    def modulate(self, n, noise, seed, lead=230, invert=False):
        x = p25gen.modulate_disc(self.dib, lead=lead, noise=noise, seed=seed, scale=self.scale)[:n]
        out = np.zeros(n, np.float32)
        out[:len(x)] = x
        return -out if invert else out


def deinterleave98(i):
    """ddn_p25h_dev.h: received data dibit i -> its place among the 98 de-interleaved ones"""
    pair, lo = i >> 1, i & 1
    lane, k = (0, pair) if pair < 13 else (1 + (pair - 13) // 12, (pair - 13) % 12)
    return 2 * (lane + 4 * k) + lo


def mpdu_block_symbols(sk0):
    """symbols p25_mpdu_read_repetition() reads for one repetition (ddn_p25h_dev.h, mpdu_block_symbols)"""
    sk, k, i = sk0, 0, 0
    while i < 101:
        if sk // 36 == 0:
            k += 1
        else:
            sk = 0
        sk += 1
        i += 1
        if k == 98:
            break
    return i


def block_data_symbols(sk0, n_sym):
    """which of a block's n_sym symbols are data dibits, its status counter starting at sk0 (ddn_p25h_rules.h, block_is_status)"""
    i0 = 36 - sk0
    return [s for s in range(n_sym) if not (s >= i0 and (s - i0) % 36 == 0)]


def classify_block(llr_pairs_rx, sk0):
    """llr_pairs_rx int [n_sym][2]: the LLRs of a block's symbols as received (status symbols included), sk0 its status counter ->
    (is_path, has_zero, bytes12 of the hard path or None)"""
    data = block_data_symbols(sk0, len(llr_pairs_rx))[:98]
    assert len(data) == 98
    dei = np.zeros((98, 2), np.int64)
    for k, s in enumerate(data):
        dei[deinterleave98(k)] = llr_pairs_rx[s]
    l = dei.reshape(49, 4)
    nib = ((l[:, 0] > 0) * 8 + (l[:, 1] > 0) * 4 + (l[:, 2] > 0) * 2 + (l[:, 3] > 0) * 1).astype(np.int64)
    half = fecgen.tables()["half"].astype(np.int64)           # nibble of (state << 2) | next state
    branch = {int(half[i]): i for i in range(16)}
    assert len(branch) == 16
    state, path, st = 0, True, []
    for t in range(49):
        ps, ns = branch[int(nib[t])] >> 2, branch[int(nib[t])] & 3
        path = path and ps == state
        state = ns
        st.append(ns)
    by = None
    if path:
        bits = np.array([[s >> 1, s & 1] for s in st[:48]], np.uint8).reshape(-1)
        by = np.packbits(bits)
    return path, bool((l == 0).any()), by


def oracle_blocks(rec_o, ev_rows, ev_data):
    """every trellis block decision of an oracle run (records int [n][4] {dibit, rel, llr0, llr1}, events (pos, kind, a, b, c), event
    data [n][4]) -> list of dicts {kind, block, pos, path, zero, crc_ok, sel}; checks on the way that a block the short cut may
    take decodes, in the oracle, to the hard path with candidate 0"""
    out = []
    for (pos, kind, a, b, c), d4 in zip(ev_rows, ev_data):
        if kind not in (2, 3):
            continue
        block = (int(d4[3]) >> 16) & 0xFF if kind == 2 else 0
        sk0 = SK0[block] if kind == 2 else 22
        n = 101 if kind == 2 else mpdu_block_symbols(sk0)
        assert pos + 1 - n >= 0
        path, zero, by = classify_block(rec_o[pos + 1 - n:pos + 1, 2:4], sk0)
        crc_ok, sel = int(d4[3]) & 1, (int(d4[3]) >> 8) & 0xFF
        if path and not zero:
            got = np.asarray(d4[:3], np.int32).view(np.uint8)
            if p25gen.crc16_ccitt(by[:10]) == ((int(by[10]) << 8) | int(by[11])):
                assert sel == 0 and crc_ok == 1 and np.array_equal(got, by), (pos, sel, crc_ok, got, by)
            else:           # on to the list decoder: another candidate that passes, or none and the hard path stays
                assert (sel > 0 and crc_ok == 1) or (sel == 0 and crc_ok == 0 and np.array_equal(got, by)), (pos, sel, crc_ok)
        out.append(dict(kind=kind, block=block, pos=pos, path=path, zero=zero, crc_ok=crc_ok, sel=sel))
    return out


# ---- the C4FM loop's cases: one stream per channel --------------------------------------------------------------------------
N_SAMPLES = 40000


def clean_stream(seed):
    """TSDUs of one, two and three good blocks back to back"""
    rng = np.random.default_rng(seed)
    s = Stream(rng)
    while s.n < N_SAMPLES // 10:
        for nb in (1, 2, 3):
            s.add(tsdu(rng, [True] * nb))
    return s.finish()


def bad_crc_stream(seed):
    """a block that is a path of the trellis and fails its CRC16, as the first, second and third block (and alone, and as one of two)"""
    rng = np.random.default_rng(seed)
    s = Stream(rng)
    while s.n < N_SAMPLES // 10:
        for good in ([False, True, True], [True, False, True], [True, True, False], [False], [True, False], [False, False, False]):
            s.add(tsdu(rng, good))
    return s.finish()


# which data dibit of which block is pushed across a threshold, one per TSDU.  Block 0's status symbols are its symbols 14, 50, 86
# (data dibits 13 | 14 on either side of the first), block 1's 21, 57, 93, block 2's 28, 64 and 100 - the phase's last symbol, behind
# data dibit 97.  (No block the loops decode starts with its status counter at 36, i.e. with a status symbol as symbol 0: a TSDU's
# blocks start at 22, 15, 8, a data unit's header block at 22.)
CROSSINGS = [(0, 0), (0, 97), (0, 13), (0, 14), (1, 0), (1, 97), (1, 20), (2, 0), (2, 97), (2, 27), (2, 28)]


def crossing_stream(seed, pdu_too=False):
    """three-block TSDUs, one data dibit of one block across a decision threshold each -> (stream, [(stream position of the block's last
    dibit, block)]); pdu_too: data units as well, header block clean / one dibit across"""
    rng = np.random.default_rng(seed)
    s = Stream(rng)
    hit = []
    s.add(tsdu(rng, [True]), gap=3)          # (the slicer's thresholds settle on the first frame)
    for block, k in CROSSINGS[:9] if not pdu_too else CROSSINGS[9:]:
        m = s.add(tsdu(rng, [True, True, True]), gap=3)
        s.finish()
        hit.append((m[block][k], block))
    if pdu_too:
        for j, blks in enumerate((0, 2, 4, 1, 3)):
            m = s.add(pdu(rng, blks), gap=4)
            if j >= 3:
                hit.append((m[0][[0, 97][j - 3]], 0))
    s.finish()
    for at, _ in hit:
        s.push_across(at)
    return s, hit


def noisy_stream(seed):
    rng = np.random.default_rng(seed)
    s = Stream(rng)
    while s.n < N_SAMPLES // 10:
        s.add(tsdu(rng, [True] * int(rng.integers(1, 4))))
    return s.finish()
