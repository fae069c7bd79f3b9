#!/usr/bin/env python3
"""Writes tests/golden/m17_data_streams.npz: M17 packet-mode and BERT transmissions as dibit streams (int8) built with the reference's
own encoder (oracle/_ref), and the bytes that were sent (uint8).  Data only.

  a        preamble, LSF, a one-frame packet with 3 application bytes (an SMS "H"), EOT
  b        total length 25 (one frame, EOF value 25) and total length 26 (two frames, last value 1) back to back, no LSF between
  c        the 823-byte packet: 33 frames
  d1, d2   a four-frame packet whose second frame is lost.  Breaking the sync word alone would leave the loop hunting through 184
           randomised payload symbols, where a one-error match of some eight-symbol word is near certain; so the whole frame is
           replaced by symbols no word matches.  The frames behind it mismatch; the EOF frame finalises a short wrong packet (d1)
           or, with an EOF value of 1, fails the byte-count check (d2)
  e        frames with metadata 0x01 and with an EOF value of 26, then a good one-frame packet.  (The encoder sends the upper six bits
           of the metadata byte, and the decoder's last two come out of the flush: 0x01 is on the air as counter 0.)
  f        one payload bit flipped before encoding: the CRC fails
  g0 .. g5 a packet cut after two frames with no EOT, 1790 / 1793 / 1795 / 1800 / 1805 / 1810 symbols nothing matches in, then preamble
           + LSF + a whole three-frame packet, EOT: both sides of the loop's 1800-symbol carrier-loss count (the preamble is matched at
           its seventh symbol or so: 1793 puts that match on the 1800th hunted symbol, the last one before the loss is declared)
  h        preamble, three clean BERT frames, one with its first 19 type-1 bits flipped, EOT, preamble, two more BERT frames, EOT
  sent_<stream>_<k>  the bytes on the air (application + CRC16) of the stream's k-th packet that was sent whole

Every stream ends with 24 symbols nothing matches in, so they may be played one behind the other.
Run where oracle/_ref is built: python3 tests/golden/make_golden_m17data.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "..", "dsd-neo_amd", "bindings"))


def main():
    import m17
    import m17data as md
    rng = np.random.default_rng(17)
    eot, out = m17.repeating(m17.EOT), {}

    def put(name, parts, sent=()):
        out[name] = np.concatenate(parts + [md.filler(24)]).astype(np.int8)
        for k, s in enumerate(sent):
            out["sent_%s_%d" % (name, k)] = np.asarray(s, np.uint8)

    def rand_packet(n_app):
        return md.packet_bytes(rng.integers(0, 256, n_app).astype(np.uint8))

    sms = md.packet_bytes(np.frombuffer(b"\x05H\x00", np.uint8))
    put("a", md.head() + md.packet_frames(sms) + [eot], [sms])
    p25, p26 = rand_packet(23), rand_packet(24)
    put("b", md.head() + md.packet_frames(p25) + md.packet_frames(p26) + [eot], [p25, p26])
    big = rand_packet(823)
    put("c", md.head() + md.packet_frames(big) + [eot], [big])
    for name, n_app in (("d1", 3 * 25 + 7 - 2), ("d2", 3 * 25 + 1 - 2)):
        fr = md.packet_frames(rand_packet(n_app))
        assert len(fr) == 4
        fr[1] = np.tile(md.FILLER, 48)                                      # (no lead-in: a packet sync follows, not a preamble)
        put(name, md.head() + fr + [eot])
    good = rand_packet(10)
    junk = rng.integers(0, 256, 25).astype(np.uint8)
    put("e", md.head() + [md.pkt_frame(junk, 0x01), md.pkt_frame(junk, 0x80 | (26 << 2))] + md.packet_frames(good) + [eot], [good])
    bad = rand_packet(40)
    hit = bad.copy()
    hit[5] ^= 0x10
    put("f", md.head() + md.packet_frames(hit) + [eot])
    for k, gap in enumerate(md.GAPS):
        cut, whole = rand_packet(70), rand_packet(60)
        put("g%d" % k, md.head() + md.packet_frames(cut)[:2] + [md.filler(gap)] + md.head() + md.packet_frames(whole) + [eot], [whole])
    tx = md.BertTx()
    first = [tx.frame()[0] for _ in range(3)] + [tx.frame(flip=range(19))[0]]
    tx2 = md.BertTx()
    put("h", [m17.repeating(m17.PREAMBLE)] + first + [eot, md.filler(24), m17.repeating(m17.PREAMBLE)] + [tx2.frame()[0] for _ in range(2)] + [eot])
    np.savez_compressed(os.path.join(HERE, "m17_data_streams.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
