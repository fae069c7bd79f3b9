"""CPU: M17 packet and BERT frames.  The restatement (tests/m17data.py) against the compiled reference (oracle/_ref: metadata parse,
EOF byte count, the PRBS9 receiver, the 197-bit chain-back), the reference's BERT known answers, the round trip of every generated
packet through modulator, front end, the oracle's loop and the restatement, what the GPU tests' streams hold (floors), and the three
batch calls' / the chain entries' argument checks without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ddn
import m17data as md
import orc

needs_ref = pytest.mark.skipif(not orc.have_ref(), reason="oracle/_ref not built")


# ---- the restatement against the compiled reference ---------------------------------------------------------------------------------
@needs_ref
def test_metadata_parse_equals_the_reference_over_all_bytes(built):
    r = md._r()
    for b in range(256):
        eof, val = C.c_uint8(0xEE), C.c_uint8(0xEE)
        rc = r.m17_packet_parse_metadata_byte(b, C.byref(eof), C.byref(val))
        got = md.parse_metadata(b)
        assert got[0] == rc, b
        if rc == 0:
            assert (got[1], got[2]) == (eof.value, val.value), b
    for eof in (0, 1):                                  # ... and what the encoder's byte parses back to
        for val in range(32):
            m = C.c_uint8(0)
            if r.m17_packet_metadata_byte(eof, val, C.byref(m)) == 0:
                assert md.parse_metadata(m.value) == (0, eof, val)


@needs_ref
def test_app_bytes_from_eof_equals_the_reference(built):
    r = md._r()
    for ff in range(41):
        for last in range(31):
            app = C.c_uint16(0xEEEE)
            rc = r.m17_packet_app_bytes_from_eof(ff, last, C.byref(app))
            got = md.app_bytes_from_eof(ff, last)
            assert got[0] == rc and (rc != 0 or got[1] == app.value), (ff, last)


def _ref_rx_state(rx):
    return [rx.locked, rx.lfsr, rx.lock_count, rx.window_bits, rx.window_errors, rx.total_bits, rx.total_errors, rx.resync_count]


@needs_ref
def test_prbs9_receiver_equals_the_reference_bit_for_bit(built):
    """random PRBS9 streams with error bursts (long enough to lose lock and find it again): every field after every bit"""
    r = md._r()
    rng = np.random.default_rng(9)
    locks = resyncs = 0
    for trial in range(6):
        lfsr = C.c_uint16(int(rng.integers(1, 512)))
        bits = np.zeros(3000, np.uint8)
        r.m17_prbs9_fill_bits(C.byref(lfsr), bits.ctypes.data, len(bits))
        for _ in range(4):
            a, n = int(rng.integers(0, 2800)), int(rng.integers(1, 120))
            bits[a:a + n] ^= (rng.random(n) < rng.choice([0.1, 0.5, 1.0])).astype(np.uint8)
        rx, mine = md.Prbs9RxState(), md.Prbs9Rx()
        r.m17_prbs9_rx_init(C.byref(rx), 1 if trial % 2 == 0 else 0)        # (0 reads 1)
        for b in bits:
            r.m17_prbs9_rx_push_bit(C.byref(rx), int(b))
            mine.push(int(b))
            assert mine.state() == _ref_rx_state(rx)
        locks += rx.locked
        resyncs += rx.resync_count
    assert locks >= 4 and resyncs >= 3


@needs_ref
def test_chainback_of_197_bits_equals_the_reference(built):
    """orc_nxdn_conv_decode over 201 steps with 197 bits chained back = CNXDNConvolution_init / _start / _decode / _chainback (metrics
    from zero, as the stream frames' decode takes them: the reference's file-static metrics carry what the last decode left)"""
    r = md._r()
    rng = np.random.default_rng(21)
    for trial in range(40):
        if trial < 20:                                                       # hard symbols as the BERT path makes them: 0 / 2
            sym = (rng.integers(0, 2, 402) << 1).astype(np.uint8)
            sym[11::12] = 0
        else:
            sym = rng.integers(0, 3, 402).astype(np.uint8)
        r.CNXDNConvolution_init()
        r.CNXDNConvolution_start()
        for i in range(201):
            r.CNXDNConvolution_decode(int(sym[2 * i]), int(sym[2 * i + 1]))
        want = np.zeros(32, np.uint8)
        r.CNXDNConvolution_chainback(want.ctypes.data, 197)
        got = md.nxdn_chainback(sym, 201, 197)
        assert np.array_equal(np.unpackbits(got)[:197], np.unpackbits(want)[:197]), trial
        assert not np.unpackbits(got)[197:].any()


@needs_ref
def test_bert_frame_round_trip_and_known_answers(built):
    """the reference's known answers (tests/protocol/m17/test_m17_state_dispatch.c:1096-1154) as recorded results, on frames that went
    through its encoder and the restated decode: one clean payload from the default state -> locked, 179 bits, no error; two -> 376;
    locked with the first 19 bits flipped -> one resync, 19 errors, 179 bits counted, 51 bits into the window"""
    tx, st = md.BertTx(), md.DataState()
    for want_bits in (179, 376):
        fr, sent = tx.frame()
        b25 = md.brt_decode(fr[8:])
        assert np.array_equal(np.unpackbits(b25)[:197], sent) and not np.unpackbits(b25)[197:].any()
        st.bert_frame(b25)
        assert st.rx.state()[0] == 1 and st.rx.bits == want_bits and st.rx.errs == 0 and st.rx.resyncs == 0
    tx, st = md.BertTx(), md.DataState()
    st.rx.locked = 1
    fr, sent = tx.frame(flip=range(19))
    st.bert_frame(md.brt_decode(fr[8:]))
    assert (st.rx.locked, st.rx.resyncs, st.rx.errs, st.rx.bits, st.rx.wbits, st.rx.werr) == (1, 1, 19, 179, 51, 0)


# ---- the streams of the GPU tests through the CPU pipeline -----------------------------------------------------------------------------
def _gaps(c):
    """[first, last] dibit index (inside the channel) of every run of filler symbols that stands where frames were left out"""
    g = md.golden_streams()
    at, out = 24, []
    for name in md.CHANNELS[c]:
        if name in ("d1", "d2"):
            out.append((at + 192 * 3, at + 192 * 4 - 1))
        if name[0] == "g":
            out.append((at + 192 * 4, at + 192 * 4 + md.GAPS[int(name[1])] - 1))
        at += len(g[name])
    return out


def test_round_trip_and_traffic_floors(built):
    """every packet the fixture says was sent whole comes back byte for byte with a good CRC, and the streams hold what the GPU tests
    are there to compare: every packet status but the unreachable 5, one-, two- and 33-frame packets, BERT lock / resync / EOT reset,
    both sides of the carrier-loss count (the match on the 1800th hunted symbol among them), no sync inside a filler gap"""
    g = md.golden_streams()
    statuses, good, brt, frames_of = set(), [], [], {}
    near = far = edge = 0
    for c in range(3):
        out, fr, pk = md.channel_want(c)
        pos = np.array([f["pos"] for f in fr])
        for a, b in _gaps(c):       # (dibit i is record i + 2: two symbols of lead and filter delay; a word that ends in the gap's first
            inside = pos[(pos - 2 >= a + 8) & (pos - 2 <= b)]               # eight symbols still holds payload symbols)
            assert len(inside) == 0, (c, a, b, inside)
        statuses |= {f["pkt_status"] for f in fr}
        for p in pk:
            if p["crc_ok"]:
                good.append(bytes(p["bytes"].tolist()))
                frames_of[len(p["bytes"])] = fr[p["sync"]]["pkt_count"] + 1
        if c < 2:
            brt += [f for f in fr if f["kind"] in ("brt", "eot")]
            for k, f in enumerate(fr):
                if f["kind"] == "pre" and k and fr[k - 1]["kind"] == "pkt":            # the preamble behind a cut packet
                    hunted = f["pos"] - (fr[k - 1]["pos"] + 184)
                    far += f["reset"]
                    near += (not f["reset"]) and f["pkt_count"] == 2
                    edge += hunted == 1800 and not f["reset"]
                    assert f["reset"] == (hunted > 1800)
    # (the second packet of g0 .. g3 is lost by design: no carrier loss and the count stands, or the preamble is matched the wrong way
    # up by the first window behind the loss)
    for name in ("sent_a_0", "sent_b_0", "sent_b_1", "sent_c_0", "sent_e_0", "sent_g4_0", "sent_g5_0"):
        assert bytes(g[name].tolist()) in good, name
    assert {1, 2, 3, 4, 6, 7} <= statuses
    assert len(good) >= 3 and {1, 2, 33} <= set(frames_of.values()) and frames_of[825] == 33
    frames = [f for f in brt if f["kind"] == "brt" and f["brt_state"][0]]
    assert len([f for f in brt if f["kind"] == "brt"]) >= 4 and len(frames) >= 4
    assert any(f["brt_state"][7] >= 1 for f in frames)                                # a resync
    ks = [k for k, f in enumerate(brt) if f["kind"] == "eot" and k and brt[k - 1]["kind"] == "brt" and brt[k - 1]["brt_state"][5] > 0]
    assert ks and all(brt[k]["brt_state"] == [0, 1, 0, 0, 0, 0, 0, 0] for k in ks)    # EOT: the receiver starts over
    assert near >= 1 and far >= 2 and edge >= 1, (near, far, edge)
    # stream (i): the negated channel locks the negative words and its BERT receiver sees the same bits
    live = len(md.channel_dibits(g, md.CHANNELS[2]))                                  # (behind it the channel is padded with bare carrier)
    fr2 = [f for f in md.channel_want(2)[1] if f["pos"] < live]
    assert [f["brt_state"] for f in fr2 if f["kind"] == "brt"] == [f["brt_state"] for f in md.channel_want(1)[1] if f["kind"] == "brt"][:6]
    assert all(f["pat"] & 1 for f in fr2)


def test_sms_packet_reads_back(built):
    _, fr, pk = md.channel_want(0)
    assert md.protocol_of(pk[0]["bytes"][:pk[0]["app_len"]]) == (0x05, "H")


@needs_ref
def test_tool_protocol_identifier_parse_equals_the_reference(built):
    """tools/decode_capture.py's host parse of the protocol identifier = m17_packet_protocol_decode() (compiled m17_parse.c) on every
    one- and two-byte head and on random longer ones; the SMS line reads the text"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("decode_capture", os.path.join(ddn.ROOT, "tools", "decode_capture.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)

    class Res(C.Structure):
        _fields_ = [("identifier", C.c_uint32), ("length", C.c_uint8)]

    r = md._r()
    r.m17_packet_protocol_decode.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    rng = np.random.default_rng(2)
    heads = [bytes([a]) for a in range(256)] + [bytes([a, b]) for a in range(0x80, 256) for b in range(0, 256, 3)]
    heads += [bytes(rng.integers(0x80, 256, int(rng.integers(3, 6))).tolist()) for _ in range(3000)]
    heads += [bytes([0xF7, 0xBF, 0xBF, 0xBF]), bytes([0xF0, 0x8F, 0xBF, 0xBF]), bytes([0xE0, 0x9F, 0xBF]), bytes([0xE0, 0xA0, 0x80])]
    for h in heads:
        a, res = np.frombuffer(h, np.uint8).copy(), Res()
        rc = r.m17_packet_protocol_decode(a.ctypes.data, len(a), C.byref(res))
        got = tool.m17_packet_protocol(a)
        assert (got is None) == (rc != 0), h
        if rc == 0:
            assert got == (res.identifier, res.length), h
    g = md.golden_streams()
    assert tool.m17_packet_line(g["sent_a_0"][:3], 1) == 'packet:   3 application bytes, CRC ok, protocol SMS (0x05): "H"'
    assert "CRC ERR" in tool.m17_packet_line(g["sent_c_0"][:823], 0)


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------
NAMES = ("ddn_m17_pkt_decode_batch", "ddn_m17_brt_decode_batch", "ddn_m17_data_assemble_batch", "ddn_m17_data_state_bytes",
         "ddn_fsk4_chain_get_m17_data_results", "ddn_fsk4_chain_set_m17_packet_slots")


def test_symbols_exported_and_declared(built):
    hdr = open(os.path.join(ddn.ROOT, "include", "ddn_fsk4.h")).read() + open(os.path.join(ddn.ROOT, "include", "ddn_chain.h")).read()
    l = C.CDLL(ddn.LIB_PATH)
    for name in NAMES:
        assert name + "(" in hdr and hasattr(l, name) and name in ddn.PROTOTYPES, name
    assert ddn.lib().ddn_m17_data_state_bytes() >= 850 + 4 * 10


def test_ctypes_mirror_matches_the_header(built, tmp_path):
    fields = [f[0] for f in ddn.M17DataChainResults._fields_]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"ddn_chain.h\"\nint main(void) {\n"
                   "    printf(\"%zu\\n\", sizeof(ddn_m17_data_chain_results));\n"
                   + "".join("    printf(\"%%zu\\n\", offsetof(ddn_m17_data_chain_results, %s));\n" % f for f in fields)
                   + "    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ddn.ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(ddn.M17DataChainResults)] + [getattr(ddn.M17DataChainResults, f).offset for f in fields]
    assert got == want, (fields, got, want)


def test_bad_arguments_are_refused_before_any_device_is_touched(built):
    """NULL or out-of-range arguments: DDN_EINVAL with a message, with or without a GPU (the pointers are never followed)"""
    l = ddn.lib()
    p = 0x1000                                           # any non-NULL value

    def pkt(**kw):
        a = dict(rec=p, stride=512, cnt=p, pos=p, pat=p, ns=p, thr=p, B=2, my=8, out=p, st=p, pc=None)
        a.update(kw)
        return l.ddn_m17_pkt_decode_batch(a["rec"], a["stride"], a["cnt"], a["pos"], a["pat"], a["ns"], a["thr"], a["B"], a["my"], a["out"],
                                          a["st"], a["pc"], None)

    def brt(**kw):
        a = dict(rec=p, stride=512, cnt=p, pos=p, pat=p, ns=p, B=2, my=8, out=p, st=p)
        a.update(kw)
        return l.ddn_m17_brt_decode_batch(a["rec"], a["stride"], a["cnt"], a["pos"], a["pat"], a["ns"], a["B"], a["my"], a["out"], a["st"], None)

    def asm(**kw):
        a = dict(pat=p, pos=p, ns=p, adv=None, B=2, my=8, p26=p, pst=p, b25=p, bst=p, state=p, o1=p, o2=p, o3=p, o4=p, o5=p, o6=p, o7=p, o8=p, P=4)
        a.update(kw)
        return l.ddn_m17_data_assemble_batch(a["pat"], a["pos"], a["ns"], a["adv"], a["B"], a["my"], a["p26"], a["pst"], a["b25"], a["bst"],
                                             a["state"], a["o1"], a["o2"], a["o3"], a["o4"], a["o5"], a["o6"], a["o7"], a["o8"], a["P"], None)

    for bad in (dict(rec=None), dict(cnt=None), dict(pos=None), dict(pat=None), dict(ns=None), dict(out=None), dict(st=None), dict(B=0),
                dict(my=0), dict(my=(1 << 24) + 1), dict(stride=0)):
        assert pkt(**bad) == -1 and b"ddn_m17_pkt_decode_batch" in l.ddn_last_error(), bad
        assert brt(**bad) == -1 and b"ddn_m17_brt_decode_batch" in l.ddn_last_error(), bad
    assert pkt(thr=None) == -1
    for bad in (dict(pat=None), dict(pos=None), dict(ns=None), dict(p26=None), dict(pst=None), dict(b25=None), dict(bst=None), dict(state=None),
                dict(o1=None), dict(o2=None), dict(o3=None), dict(o4=None), dict(o5=None), dict(o6=None), dict(o7=None), dict(o8=None),
                dict(B=0), dict(my=0), dict(P=0), dict(P=34), dict(P=-1)):
        assert asm(**bad) == -1 and b"ddn_m17_data_assemble_batch" in l.ddn_last_error(), bad
    assert l.ddn_fsk4_chain_get_m17_data_results(None, C.byref(ddn.M17DataChainResults())) == -1
    assert l.ddn_fsk4_chain_set_m17_packet_slots(None, 4) == -1 and b"ddn_fsk4_chain_set_m17_packet_slots" in l.ddn_last_error()
