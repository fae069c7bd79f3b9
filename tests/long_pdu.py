"""Long P25 data units (DUID 0xC with more than pdu_blocks data blocks) as the reference reads them, restated on a whole stream:
what ddn_p25_chain_get_long_pdu_results() must report (include/ddn_chain.h).  The input is chain_stream.run_stream()'s answer for one
channel - the loop's own header decisions (event kind 3: header bytes, CRC16, blocks read) and the records - and every data block
behind a long header goes through the oracle's decoders: the half-rate list decoder's candidate 0 (p25_mpdu_decode_r12_block), for
confirmed data the rate 3/4 list decoder's first candidate with a good CRC9, then crc32mbf over the data.  TEST INFRASTRUCTURE."""
import ctypes as C

import numpy as np

import orc
import p25gen

OFF_HDR = 33 + 101          # the header's decision falls 134 symbols behind the sync's last one


def block_rows(a, b):
    """row / stream indices of data block b's 98 payload dibits of the unit whose sync's last symbol is at a"""
    return [a - 23 + n + n // 35 for n in range(56 + 98 * b, 56 + 98 * b + 98)]


def _half_rate(llr):
    o = orc.oracle()
    o.orc_p25_12_soft_llr_list.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    ob, om = np.zeros((8, 12), np.uint8), np.zeros(8, np.uint32)
    assert o.orc_p25_12_soft_llr_list(llr.ctypes.data, ob.ctypes.data, om.ctypes.data, 8) >= 1
    return ob[0].copy()


def _three_quarter(llr):
    o = orc.oracle()
    o.orc_p25_mbf34_list.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    cb, cm = np.zeros((8, 18), np.uint8), np.zeros(8, np.uint32)
    nc = o.orc_p25_mbf34_list(llr.ctypes.data, 8, cb.ctypes.data, cm.ctypes.data)
    assert nc >= 1
    good = [k for k in range(nc) if p25gen.crc9([(int(cb[k, 0]) >> (7 - i)) & 1 for i in range(7)] + list(np.unpackbits(cb[k, 2:])))
            == (((int(cb[k, 0]) & 1) << 8) | int(cb[k, 1]))]
    return cb[good[0] if good else 0].copy(), 1 if good else 0


def expected_units(want, pdu_blocks=8, max_blocks=127):
    """run_stream() answer -> {sync record: dict(header, info (4,), blocks [max_blocks][12], valid, blocks18, crc9)} for every unit
    the reference reads as more than pdu_blocks data blocks; a block whose records run past the stream's end is not decoded"""
    rec4 = want["rec4"]
    cnt = len(want["sym"])
    out = {}
    for e, d in zip(want["events"], want["event_data"]):
        if e[1] != 3:
            continue
        a = int(e[0]) - OFF_HDR
        f = want["frames"].get(a)
        if f is None or "nid" not in f or f["nid"][0] <= 0 or f["nid"][2] != 0xC or not (int(d[3]) & 1):
            continue
        end = int(e[3]) & 0xFFFF
        if end - 1 <= pdu_blocks:
            continue
        hdr = d[:3].copy().view(np.uint8)
        r34 = bool((hdr[0] >> 6) & 1) and (hdr[0] & 0x1F) == 0x16
        blocks = np.zeros((max_blocks, 12), np.uint8)
        valid = np.zeros(max_blocks, np.uint8)
        b18 = np.zeros((max_blocks, 18), np.uint8)
        c9 = np.zeros(max_blocks, np.uint8)
        for b in range(1, min(end - 1, max_blocks) + 1):
            idx = block_rows(a, b)
            if idx[-1] >= cnt:
                break
            llr = np.ascontiguousarray(np.stack([rec4[idx, 2], rec4[idx, 3]], axis=1).reshape(196), np.int16)
            blocks[b - 1] = _half_rate(llr)
            valid[b - 1] = 1
            if r34:
                b18[b - 1], c9[b - 1] = _three_quarter(llr)
        complete = block_rows(a, end - 1)[-1] < cnt
        flags = (4 if r34 else 0) | (0 if complete else 8) | (16 if end - 1 > max_blocks else 0)
        nd = end - 1
        crc = 0
        if not (flags & (8 | 16)):
            flat = np.concatenate([b18[k, 2:] for k in range(nd)]) if r34 else blocks[:nd].reshape(-1)
            nbits = (128 if r34 else 96) * nd - 32
            crc = int(p25gen.crc32mbf(flat, nbits) == int.from_bytes(bytes(flat[-4:].tolist()), "big"))
        out[a] = dict(header=hdr, info=np.array([end, int(valid.sum()), flags, crc], np.int32), blocks=blocks, valid=valid,
                      blocks18=b18, crc9=c9)
    return out


def collect(chain, got):
    """the long units the chain reported for its last call -> got[channel][sync record] (each at most once); returns the per-channel
    unit counts d_n"""
    r = chain.long_pdu_results()
    B, P, MB = chain.B, r.per_channel, r.max_blocks
    n = chain.fetch(r.d_n, np.int32, (B,))
    rec = chain.fetch(r.d_sync_record, np.int64, (B, P))
    hdr = chain.fetch(r.d_header, np.uint8, (B, P, 12))
    info = chain.fetch(r.d_info, np.int32, (B, P, 4))
    blk = chain.fetch(r.d_blocks, np.uint8, (B, P, MB, 12))
    vld = chain.fetch(r.d_block_valid, np.uint8, (B, P, MB))
    b18 = chain.fetch(r.d_blocks18, np.uint8, (B, P, MB, 18))
    c9 = chain.fetch(r.d_crc9_ok, np.uint8, (B, P, MB))
    for c in range(B):
        for k in range(min(int(n[c]), P)):
            g = int(rec[c, k])
            assert g not in got[c], ("unit reported twice", c, g)
            got[c][g] = dict(header=hdr[c, k], info=info[c, k], blocks=blk[c, k], valid=vld[c, k], blocks18=b18[c, k], crc9=c9[c, k])
    return n


def assert_same(got, want, what=""):
    """the device's units of one channel equal the restatement's, field by field"""
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for a, w in want.items():
        g = got[a]
        for k in ("header", "info", "blocks", "valid", "blocks18", "crc9"):
            assert np.array_equal(g[k], w[k]), (what, a, k, g[k] if k in ("header", "info") else None, w[k] if k in ("header", "info") else None)
