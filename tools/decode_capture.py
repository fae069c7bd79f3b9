#!/usr/bin/env python3
"""Decode a dsd-neo I/Q capture (P25 Phase 1, C4FM) with libdsdneo_hip.so and print a per-frame summary - the same facts the
reference's --iq-replay log carries (NAC, DUID, TSBK opcodes with CRC status, LDU1 link control, LDU2 encryption sync,
voice-frame counts).  Everything between the capture file and the printed lines runs through the C-ABI: capture reader,
front end, receive loop, framer gathers, BCH / trellis / CRC / Hamming / Reed-Solomon kernels.

A cu8, cf32 or cs16 capture goes to the device in its own format (the kernels widen it).

usage: python tools/decode_capture.py CAPTURE.iq[.json] [--lock SYMBOLS] [--max-frames N] [--m17] [--nxdn 48|96] [--analog OUT.wav]
       --lock: in-frame symbols after a sync (default 840 = LDU-sized; 156 / 336 suit one- / three-block TSDU control
               channels - dibits read outside the in-frame span carry no soft decisions)
       --m17:  read the capture as M17 (cu8 at 48 kHz) through the fsk4 chain object instead and print a line per completed packet:
               application length, CRC verdict, protocol identifier and, for SMS (0x05), the text
       --nxdn 48|96: read the capture as NXDN48 / NXDN96 (cu8 at 48 kHz) through the fsk4 chain object with the control-channel stage on
               and print a line per delivered SACCH message and per CAC / FACCH2 / UDCH frame: RAN, channel, message type, CRC; the
               reference's NXDN48 capture prints its "VCALL ... Src=901" lines
       --analog OUT.wav: run the capture through the analog FM monitor instead (full_demod()'s audio output kind: de-emphasis 75 us,
               DC block, low_pass_real to 8 kHz where the demod rate is a multiple of it) and write the audio as 16-bit PCM at full
               scale pi - one phase step cannot exceed pi; the reference's consumer-side gains stay with the host"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "dsd-neo_amd", "bindings"))
DUID = {0: "HDU", 3: "TDU", 5: "LDU1", 7: "TSBK", 10: "LDU2", 12: "PDU", 15: "TDULC"}


def decode(path, lock=840, max_frames=64, out=print):
    import numpy as np
    import torch
    import ddn
    l = ddn.lib()
    dev = lambda *sh, dt=torch.uint8: torch.zeros(sh, dtype=dt, device="cuda")
    # ---- capture -> channel-major batch of one
    paths = (C.c_char_p * 1)(path.encode())
    buf, n = C.c_void_p(), C.c_size_t()
    info = (C.c_uint8 * 8192)()
    rc = l.ddn_iq_load_batch(paths, 1, C.byref(buf), C.byref(n), info)
    if rc != 0:
        raise SystemExit("cannot open capture (%d): %s" % (rc, l.ddn_last_error().decode()))
    fmt, rate, base_dec, _, demod_rate = np.frombuffer(bytes(info[:24]), np.uint32)[1:6]
    # capture format (DDN_IQ_FORMAT_*) -> (name, the front end's input format); every capture format goes to the device as it is
    name, in_fmt = {1: ("cu8", ddn.IN_CU8), 2: ("cf32", ddn.IN_CF32), 3: ("cs16", ddn.IN_CS16)}.get(int(fmt), (None, None))
    if name is None:
        raise SystemExit("sample format %d is not a capture format this tool knows (cu8 / cf32 / cs16)" % fmt)
    bps = l.ddn_input_format_bytes(in_fmt)
    n = n.value
    host = np.ctypeslib.as_array(C.cast(buf, C.POINTER(C.c_uint8)), (n * bps,)).copy()
    l.ddn_iq_free(buf)
    out("capture: %d complex samples, %s @ %d Hz, base_decimation %d -> demod %d Hz"
        % (n, name, rate, base_dec, demod_rate))
    passes = int(base_dec).bit_length() - 1
    n -= n % (1 << passes)
    fe = ddn.Batch(1, sample_rate_hz=int(demod_rate), input_format=in_fmt, block_len=8192)
    if passes:
        fe.set_decimation(passes)
    d_iq = torch.from_numpy(host[:n * bps]).cuda()
    nd = n >> passes
    d_disc = dev(1, nd, dt=torch.float32)
    fe.run_device(d_iq.data_ptr(), n, d_disc.data_ptr())
    # ---- discriminator -> records -> frame slots
    rx = ddn.P25Rx(1, out_rate=int(demod_rate), lock_symbols=lock, use_matched_filter=1 if demod_rate == 48000 else 0)
    ms = l.ddn_p25_rx_max_symbols(rx.h, nd)
    rec, fl, cnt = dev(1, ms, 10), dev(1, ms), dev(1, dt=torch.int32)
    assert l.ddn_p25_rx_run(rx.h, d_disc.data_ptr(), nd, rec.data_ptr(), fl.data_ptr(), cnt.data_ptr(), ms, None) == 0
    F = max_frames
    fr = C.c_void_p()
    assert l.ddn_p25p1_framer_create(1, F, C.byref(fr)) == 0
    assert l.ddn_p25p1_framer_index(fr, fl.data_ptr(), cnt.data_ptr(), ms, None) == 0
    args = (rec.data_ptr(), cnt.data_ptr(), ms)
    bits, rel, par, prel, nid = dev(F, 63), dev(F, 63), dev(F), dev(F), dev(F, 4, dt=torch.int32)
    obs = dev(F, dt=torch.int32)
    assert l.ddn_p25p1_framer_gather_nid(fr, *args, bits.data_ptr(), rel.data_ptr(), par.data_ptr(), prel.data_ptr(), None,
                                         None) == 0
    assert l.ddn_p25p1_nid_decode_batch(bits.data_ptr(), rel.data_ptr(), obs.data_ptr(), par.data_ptr(), prel.data_ptr(), 64,
                                        F, nid.data_ptr(), None) == 0
    # trunking blocks
    tsbk, tsbk_ok, tsbk_v = [], [], []
    for b in range(3):
        llr, v = dev(F, 196, dt=torch.int16), dev(F)
        o12, met, ok = dev(F, 12), dev(F, dt=torch.int32), dev(F)
        assert l.ddn_p25p1_framer_gather_trellis_block(fr, b, *args, llr.data_ptr(), None, v.data_ptr(), None) == 0
        assert l.ddn_fec_p25_12_soft_batch(llr.data_ptr(), F, o12.data_ptr(), met.data_ptr(), None) == 0
        assert l.ddn_fec_p25_crc16_batch(o12.data_ptr(), 12, F, ok.data_ptr(), None) == 0
        tsbk.append(o12)
        tsbk_ok.append(ok)
        tsbk_v.append(v)
    # LDU words -> Hamming -> RS
    ldu = {}
    for which, code, nd_ in ((1, 0, 12), (2, 1, 16)):
        w, v, errs = dev(F, 240), dev(F), dev(F * 24)
        d6, p6, st = dev(F, nd_, 6), dev(F, 24 - nd_, 6), dev(F)
        assert l.ddn_p25p1_framer_gather_ldu_words(fr, which, *args, w.data_ptr(), None, v.data_ptr(), None) == 0
        assert l.ddn_fec_hamming_10_6_3_batch(w.data_ptr(), F * 24, errs.data_ptr(), None) == 0
        assert l.ddn_p25p1_framer_pack_ldu_rs(fr, which, w.data_ptr(), d6.data_ptr(), p6.data_ptr(), None) == 0
        assert l.ddn_fec_p25_rs_batch(code, d6.data_ptr(), p6.data_ptr(), F, st.data_ptr(), None) == 0
        ldu[which] = (d6, st, v)
    # voice frames
    first, sc = dev(F * 9, dt=torch.int64), dev(F * 9, dt=torch.int32)
    ifr, isf, ifl, isc = dev(F * 9, 8, 23), dev(F * 9, 8, 23, 2), dev(F * 9), dev(F * 9, dt=torch.int32)
    assert l.ddn_p25p1_framer_imbe_index(fr, ms, first.data_ptr(), sc.data_ptr(), None) == 0
    assert l.ddn_p25p1_imbe_deinterleave_batch(rec.data_ptr(), ms, first.data_ptr(), sc.data_ptr(), F * 9, ifr.data_ptr(),
                                               isf.data_ptr(), ifl.data_ptr(), isc.data_ptr(), None) == 0
    torch.cuda.synchronize()
    ns = np.zeros(1, np.int32)
    pos = np.zeros(F, np.int32)
    assert l.ddn_p25p1_framer_get_syncs(fr, ns.ctypes.data, pos.ctypes.data) == 0
    l.ddn_p25p1_framer_destroy(fr)
    nidh = nid.cpu().numpy()
    val = lambda b: int("".join(str(int(x)) for x in b), 2)
    lines = []
    for k in range(int(ns[0])):
        st_, nac, duid, errs = (int(x) for x in nidh[k])
        head = "sync @%6d  " % pos[k]
        if st_ != 1:
            lines.append(head + "NID undecodable")
            continue
        text = head + "NAC %03X  %-5s" % (nac, DUID.get(duid, "DUID%X" % duid)) + ("  (NID %d bit fixes)" % errs if errs else "")
        if duid in (7, 12):
            for b in range(3):
                if not int(tsbk_v[b][k]):
                    break
                by = tsbk[b][k].cpu().numpy()
                text += "  | blk%d op %02X mfid %02X %s" % (b, by[0] & 0x3F, by[1], "crc ok" if int(tsbk_ok[b][k]) else "CRC ERR")
                if (by[0] & 0x3F) == 0x3B and int(tsbk_ok[b][k]):
                    text += " NET_STS WACN %05X SYS %03X" % ((int(by[3]) << 12) | (int(by[4]) << 4) | (int(by[5]) >> 4),
                                                            ((int(by[5]) & 0xF) << 8) | int(by[6]))
                if by[0] & 0x80:
                    break                                  # last block flag
        elif duid == 5 and int(ldu[1][2][k]):
            d6 = ldu[1][0][k].cpu().numpy()
            lc = d6[::-1].reshape(72)
            ok = int(ldu[1][1][k]) == 0
            text += "  | LC %s: LCO %02X MFID %02X" % ("ok" if ok else "RS ERR", val(lc[2:8]), val(lc[8:16]))
            if ok and val(lc[2:8]) == 0 and val(lc[8:16]) in (0, 1):
                text += "  Group Voice Channel User TG %d SRC %d" % (val(lc[32:48]), val(lc[48:72]))
            text += "  | 9 IMBE frames (%d flagged)" % int((ifl[9 * k:9 * k + 9] != 0).sum())
        elif duid == 10 and int(ldu[2][2][k]):
            hx = ldu[2][0][k].cpu().numpy()
            ok = int(ldu[2][1][k]) == 0
            text += "  | ESS %s: ALGID %02X KID %04X" % ("ok" if ok else "RS ERR", val(list(hx[3]) + list(hx[2][:2])),
                                                          val(list(hx[2][2:]) + list(hx[1]) + list(hx[0])))
            text += "  | 9 IMBE frames (%d flagged)" % int((ifl[9 * k:9 * k + 9] != 0).sum())
        lines.append(text)
    for t in lines:
        out(t)
    return lines


M17_PROTOCOLS = {0x00: "RAW", 0x01: "AX.25", 0x02: "APRS", 0x03: "6LoWPAN", 0x04: "IPv4", 0x05: "SMS", 0x06: "Winlink", 0x07: "TLE"}  # M17 spec


def m17_packet_protocol(app):
    """the protocol identifier in front of a packet's application bytes (M17 specification, packet superframe: one byte below 0x80,
    else a UTF-8 style sequence of two to four bytes, shortest form only, 21 bits at most) -> (identifier, its length), or None where it is malformed
    (what m17_packet_protocol_decode() refuses, src/protocol/m17/m17_parse.c:580-632)"""
    if len(app) == 0:
        return None
    b0 = int(app[0])
    if b0 < 0x80:
        return b0, 1
    for mask, lead, need, low in ((0xE0, 0xC0, 2, 0x80), (0xF0, 0xE0, 3, 0x800), (0xF8, 0xF0, 4, 0x10000)):
        if (b0 & mask) == lead:
            if len(app) < need or any((int(b) & 0xC0) != 0x80 for b in app[1:need]):
                return None
            v = b0 & (~mask & 0xFF)
            for b in app[1:need]:
                v = (v << 6) | (int(b) & 0x3F)
            return (v, need) if low <= v <= 0x1FFFFF else None
    return None


def m17_packet_line(app, crc_ok):
    """one line per completed packet"""
    text = "packet: %3d application bytes, CRC %s" % (len(app), "ok" if crc_ok else "ERR")
    proto = m17_packet_protocol(app)
    if proto is None:
        return text + ", protocol: invalid"
    ident, used = proto
    text += ", protocol %s (0x%02X)" % (M17_PROTOCOLS.get(ident, "reserved / unknown"), ident)
    if ident == 0x05:
        text += ': "%s"' % bytes(bytearray(int(b) for b in app[used:])).split(b"\x00")[0].decode("utf-8", "replace")
    return text


def decode_m17(path, out=print):
    """the capture through ddn_fsk4_chain (protocol M17) in calls of one second + the flush -> a line per completed packet"""
    import numpy as np
    import ddn
    l = ddn.lib()
    paths = (C.c_char_p * 1)(path.encode())
    buf, n = C.c_void_p(), C.c_size_t()
    info = (C.c_uint8 * 8192)()
    rc = l.ddn_iq_load_batch(paths, 1, C.byref(buf), C.byref(n), info)
    if rc != 0:
        raise SystemExit("cannot open capture (%d): %s" % (rc, l.ddn_last_error().decode()))
    fmt, rate, base_dec, _, demod_rate = np.frombuffer(bytes(info[:24]), np.uint32)[1:6]
    if int(fmt) != 1 or int(demod_rate) != 48000 or int(base_dec) != 1:
        raise SystemExit("--m17 takes cu8 captures at 48 kHz (format %d, %d Hz, base_decimation %d)" % (fmt, demod_rate, base_dec))
    host = np.ctypeslib.as_array(C.cast(buf, C.POINTER(C.c_uint8)), (n.value * 2,)).copy().reshape(1, -1, 2)
    l.ddn_iq_free(buf)
    per = 48000
    calls = -(-host.shape[1] // per)
    pad = np.full((1, calls * per, 2), 127, np.uint8)
    pad[:, :host.shape[1]] = host
    ch = ddn.Fsk4ChainC(1, per, ddn.FSK4_M17, rf_mod=0, handlers=0, vocoder=0)
    ch.set_m17_packet_slots(33)
    lines = []

    def take():
        d = ch.m17_data_results()
        P = int(d.max_packets)
        k = min(int(ch.fetch(d.d_n_packets, np.int32, (1,))[0]), P)
        by, ln, ok = ch.fetch(d.d_packet, np.uint8, (1, P, 832)), ch.fetch(d.d_packet_app_len, np.int32, (1, P)), ch.fetch(d.d_packet_crc_ok, np.uint8, (1, P))
        for j in range(k):
            lines.append(m17_packet_line(by[0, j, :int(ln[0, j])], int(ok[0, j])))

    for k in range(calls):
        part = np.ascontiguousarray(pad[:, k * per:(k + 1) * per])
        p = C.c_void_p()
        assert l.ddn_device_alloc(part.nbytes, C.byref(p)) == 0 and l.ddn_device_upload(p, part.ctypes.data, part.nbytes) == 0
        ch.run(p)
        take()
        l.ddn_device_free(p)
    ch.flush()
    take()
    ch.close()
    for t in lines:
        out(t)
    return lines


NXDN_KIND = {1: "CAC", 2: "FACCH2", 3: "UDCH"}


def nxdn_message_line(channel, ran, bits, crc_ok):
    """a line for one NXDN layer-3 message (bits = the message behind the 8 header bits): RAN, channel, message type (bits 2..7 of its
    first byte), CRC; a VCALL (type 0x01) adds its source and destination"""
    val = lambda a, b: int("".join(str(int(v)) for v in bits[a:b]), 2)
    t = val(2, 8)
    text = "RAN %02d %-6s type 0x%02X%s CRC %s" % (ran, channel, t, " VCALL" if t == 1 else "", "ok" if crc_ok else "ERR")
    if t == 1 and crc_ok and len(bits) >= 56:
        text += " Src=%d Dst=%d" % (val(24, 40), val(40, 56))
    return text


def decode_nxdn(path, which, out=print):
    """the capture through ddn_fsk4_chain (NXDN48 / NXDN96, handlers = 1, ddn_fsk4_chain_set_nxdn_ctrl) in calls of one second + the
    flush -> a line per delivered SACCH message and per CAC / FACCH2 / UDCH frame, from the library's own outputs"""
    import numpy as np
    import ddn
    l = ddn.lib()
    paths = (C.c_char_p * 1)(path.encode())
    buf, n = C.c_void_p(), C.c_size_t()
    info = (C.c_uint8 * 8192)()
    rc = l.ddn_iq_load_batch(paths, 1, C.byref(buf), C.byref(n), info)
    if rc != 0:
        raise SystemExit("cannot open capture (%d): %s" % (rc, l.ddn_last_error().decode()))
    fmt, rate, base_dec, _, demod_rate = np.frombuffer(bytes(info[:24]), np.uint32)[1:6]
    if int(fmt) != 1 or int(demod_rate) != 48000 or int(base_dec) != 1:
        raise SystemExit("--nxdn takes cu8 captures at 48 kHz (format %d, %d Hz, base_decimation %d)" % (fmt, demod_rate, base_dec))
    host = np.ctypeslib.as_array(C.cast(buf, C.POINTER(C.c_uint8)), (n.value * 2,)).copy().reshape(1, -1, 2)
    l.ddn_iq_free(buf)
    per = 48000
    calls = -(-host.shape[1] // per)
    pad = np.full((1, calls * per, 2), 127, np.uint8)
    pad[:, :host.shape[1]] = host
    ch = ddn.Fsk4ChainC(1, per, ddn.FSK4_NXDN48 if which == 48 else ddn.FSK4_NXDN96, rf_mod=0 if which == 48 else 2, handlers=1, vocoder=0)
    ch.set_nxdn_ctrl(1)
    lines = []

    def take():
        d = ch.nxdn_ctrl_results()
        S, f, m = int(d.max_syncs), d.frames, d.messages
        u8 = lambda p, *sh: ch.fetch(p, np.uint8, (S,) + sh)
        ns = min(int(ch.fetch(d.d_n_sync, np.int32, (1,))[0]), S)
        kind, bits, ok, ran = u8(f.d_kind), u8(f.d_bits208, 208), u8(f.d_crc_ok), u8(f.d_ran)
        mst, sst, msg, last = u8(m.d_msg_status), u8(m.d_sacch_status), u8(m.d_msg72, 72), ch.fetch(m.d_last_ran, np.int32, (S,))
        valid = u8(d.d_valid)
        for k in range(ns):
            if not valid[k]:
                continue
            if kind[k]:
                lines.append(nxdn_message_line(NXDN_KIND[int(kind[k])], int(ran[k]), bits[k, 8:155 if kind[k] == 1 else 184], int(ok[k])))
            elif mst[k] == 1:
                lines.append(nxdn_message_line("SACCH", int(last[k]), msg[k, :72 if sst[k] == 1 else 18], 1))

    for k in range(calls):
        part = np.ascontiguousarray(pad[:, k * per:(k + 1) * per])
        p = C.c_void_p()
        assert l.ddn_device_alloc(part.nbytes, C.byref(p)) == 0 and l.ddn_device_upload(p, part.ctypes.data, part.nbytes) == 0
        ch.run(p)
        take()
        l.ddn_device_free(p)
    ch.flush()
    take()
    ch.close()
    for t in lines:
        out(t)
    return lines


def decode_analog(path, wav, out=print):
    """the capture through ddn_fm_audio_run in calls of one second -> OUT.wav (ddn_wav_write_s16, full scale pi)"""
    import numpy as np
    import ddn
    l = ddn.lib()
    paths = (C.c_char_p * 1)(path.encode())
    buf, n = C.c_void_p(), C.c_size_t()
    info = (C.c_uint8 * 8192)()
    rc = l.ddn_iq_load_batch(paths, 1, C.byref(buf), C.byref(n), info)
    if rc != 0:
        raise SystemExit("cannot open capture (%d): %s" % (rc, l.ddn_last_error().decode()))
    fmt, rate, base_dec, _, demod_rate = (int(v) for v in np.frombuffer(bytes(info[:24]), np.uint32)[1:6])
    dt, in_fmt = {1: (np.uint8, ddn.IN_CU8), 2: (np.float32, ddn.IN_CF32), 3: (np.int16, ddn.IN_CS16)}.get(fmt, (None, None))
    if dt is None:
        raise SystemExit("sample format %d is not a capture format this tool knows (cu8 / cf32 / cs16)" % fmt)
    bps = l.ddn_input_format_bytes(in_fmt)
    host = np.ctypeslib.as_array(C.cast(buf, C.POINTER(C.c_uint8)), (n.value * bps,)).copy().view(dt).reshape(1, -1, 2)
    l.ddn_iq_free(buf)
    passes = base_dec.bit_length() - 1
    block = 8192 << passes
    audio_rate = 8000 if demod_rate % 8000 == 0 and demod_rate > 8000 else demod_rate
    kw = dict(lpr_fast_hz=demod_rate, lpr_slow_hz=audio_rate) if audio_rate != demod_rate else {}
    fm = ddn.FmAudio(1, sample_rate_hz=demod_rate, input_format=in_fmt, block_len=block, passes=passes, deemph=1, **kw)
    per = block * max(1, (rate // block))                      # about a second, whole blocks: every call but the last ends on a block
    total = host.shape[1] - host.shape[1] % (1 << passes)
    parts = [fm.run_host(host[:, p:min(p + per, total)], min(p + per, total) - p) for p in range(0, total, per)]
    pcm = np.ascontiguousarray(np.concatenate(parts, axis=1)[0]) if parts else np.zeros(0, np.float32)
    fm.close()
    rc = l.ddn_wav_write_s16(wav.encode(), audio_rate, 1, pcm.ctypes.data, pcm.size, float(np.float32(np.pi)))
    if rc != 0:
        raise SystemExit("cannot write %s (%d): %s" % (wav, rc, l.ddn_last_error().decode()))
    out("analog: %d complex samples @ %d Hz (demod %d Hz) -> %d audio samples @ %d Hz, peak %.3f rad -> %s"
        % (total, rate, demod_rate, pcm.size, audio_rate, float(np.abs(pcm).max()) if pcm.size else 0.0, wav))
    return pcm


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("capture")
    ap.add_argument("--lock", type=int, default=840)
    ap.add_argument("--max-frames", type=int, default=64)
    ap.add_argument("--m17", action="store_true")
    ap.add_argument("--analog", metavar="OUT.wav")
    ap.add_argument("--nxdn", type=int, choices=(48, 96))
    a = ap.parse_args()
    if a.nxdn:
        decode_nxdn(a.capture, a.nxdn)
        return
    if a.analog:
        decode_analog(a.capture, a.analog)
        return
    if a.m17:
        decode_m17(a.capture)
        return
    decode(a.capture, a.lock, a.max_frames)


if __name__ == "__main__":
    main()
