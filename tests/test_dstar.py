"""D-STAR (-fd) on the CPU: tests/dstar.py against the reference's own unit-test vectors (tests/golden/dstar_vectors.json, extracted by
tests/golden/make_golden_dstar.py) and the oracle loop with the D-STAR profile on the reference's capture (DECODE_IQ_DSTAR: "SRC: KB7WUK")."""
import numpy as np
import pytest

import dstar
import rx4

V = dstar.vectors()


def test_tables_and_sync_words_match_the_reference():
    assert [V["sync_words"][n]["symbols"] for n in ("DSTAR_SYNC", "INV_DSTAR_SYNC", "DSTAR_HD", "INV_DSTAR_HD")] == dstar.WORDS
    assert [V["sync_words"][n]["type"] + 1 for n in ("DSTAR_SYNC", "INV_DSTAR_SYNC", "DSTAR_HD", "INV_DSTAR_HD")] == dstar.TYPES
    # test_dstar_sync_dispatch.c: the voice types run processDSTAR, the header types processDSTAR_HD (rows 2 / 3 of the loop)
    assert [dstar.TYPES[k] - 1 for k in (0, 1)] == V["dispatch"]["voice"]
    assert [dstar.TYPES[k] - 1 for k in (2, 3)] == V["dispatch"]["header"]
    assert dstar.unit_len(0) == dstar.unit_len(1) == 1992 and dstar.unit_len(2) == dstar.unit_len(3) == 2652
    assert sorted(dstar.deinterleave_perm().tolist()) == list(range(660))
    assert dstar.pn127().sum() == 64          # a maximal-length sequence of period 127


def test_crc16_check_value():
    assert dstar.crc16(V["crc16"]["text"].encode()) == V["crc16"]["crc"]


def test_soft_pipeline_round_trip():
    """test_soft_decode_pipeline: encode, interleave, scramble at 0xF000 / 0x1000, then descramble, de-interleave, decode"""
    r = V["header_roundtrip"]
    info = np.array([(i * r["mul"] + r["add"]) & 1 for i in range(dstar.INFO)], np.uint8)
    coded = dstar.conv_encode(info)
    air = coded[dstar.deinterleave_perm()] ^ dstar.pn127()[np.arange(660) % 127]
    costs = np.where(air == 1, r["soft_one"], r["soft_zero"])
    pn = dstar.pn127()[np.arange(660) % 127]
    d = np.zeros(660, np.int64)
    d[dstar.deinterleave_perm()] = np.where(pn == 1, 0xFFFF - costs, costs)
    assert np.array_equal(dstar.viterbi(d), info)


@pytest.mark.parametrize("case", range(len(V["header_fixture"]["cases"])))
def test_encoded_header_fixture_gives_the_callsigns(case):
    """test_soft_header_decode_extracts_callsigns / test_soft_data_header_preserves_callsigns: the fixture through the soft decode
    with {min, center, max} = {-1, 0, 1}"""
    fx = V["header_fixture"]
    flags = fx["cases"][case]["flags"]
    h = bytearray(41)
    h[0] = flags
    for at, s, n in fx["fields"]:
        h[at:at + n] = s.encode()
    c = dstar.crc16(h[:39])
    h[39], h[40] = c >> 8, c & 0xFF
    sym = dstar.header_air_symbols(bytes(h), neg=0)
    thr = np.array([0.0, 0.5, -0.5, 1.0, -1.0], np.float32)
    got, ok = dstar.decode_header(sym, thr)
    assert ok and bytes(got) == bytes(h)
    f = dstar.header_fields(got)
    norm = lambda b: " ".join(dstar.text(b).split())      # the call state collapses the padding ("N0CALL  /TST" -> "N0CALL /TST")
    assert {k: norm(f[k]) for k in ("rpt2", "rpt1", "dst", "src")} == fx["call"]
    assert ("data" if f["flags"] & 0x80 else "voice") == fx["cases"][case]["kind"]


def test_slow_data_header_in_wire_crc_order():
    sh = V["sd_header"]
    compact = bytearray([sh["fill"]] * 51)
    for at, s, n in sh["fields"]:
        compact[at:at + n] = s.encode()
    for at, v in sh["bytes"]:
        compact[at] = v
    sdb = dstar.compact_to_sd_bytes(compact, sh["marker"], sh["fill"])
    got = dstar.slow_data(dstar.encode_slow_data(sdb))
    assert got["bytes"] == sdb
    assert got["kind"] == dstar.SD_HEADER and got["crc_ok"]
    f = dstar.header_fields(got["hdr41"])
    assert " ".join(dstar.text(f["src"]).split()) == V["header_fixture"]["call"]["src"]
    assert dstar.text(f["dst"]).strip() == V["header_fixture"]["call"]["dst"]


def test_slow_data_text_keeps_byte_after_marker():
    st = V["sd_text"]
    b = bytearray([st["fill"]] * 60)
    for at, v in st["bytes"]:
        b[at] = v
    got = dstar.slow_data(dstar.encode_slow_data(bytes(b)))
    assert got["kind"] == dstar.SD_TEXT
    for at, ch in st["text_at"]:
        assert chr(got["text"][at]) == ch


def test_voice_gather_matches_the_process_test():
    """test_dstar_process.c: its stub hands out dibits (call number & 3); ambe_fr takes dibit & 1 through the schedule, the slow data
    starts with the dibit after the first voice frame; processDSTAR_HD reads the header's soft symbols ((call number + 1) x step) first"""
    p = V["process"]
    assert p["voice_frames"] * p["voice_dibits"] + p["slow_frames"] * p["slow_dibits"] == dstar.VOICE_SYMS
    dib = np.arange(dstar.VOICE_SYMS) & p["dibit_mask"]
    fr, sd = dstar.voice_gather(dib)
    for r, c, v in p["ambe_cells"]:
        assert fr[0, r, c] == v, (r, c)
    first = p["slow_data_first"]
    assert sd[:p["slow_dibits"]].tolist() == [(first["offset"] + i) & first["mask"] for i in range(p["slow_dibits"])]
    h = p["header_soft"]
    soft = (np.arange(dstar.HEADER_SYMS + dstar.VOICE_SYMS, dtype=np.float32) + 1) * np.float32(h["step"])
    header = soft[:dstar.HEADER_SYMS]          # what decode_unit reads as the header behind a header sync
    assert header[0] == h["first"] and header[-1] == h["last"]


def test_two_level_slice_and_cost_polarity():
    thr = np.array([0.0, 0.5, -0.5, 1.0, -1.0], np.float32)
    assert dstar.bits2([1.0, -1.0], 0.0, 0).tolist() == [0, 1]
    assert dstar.bits2([1.0, -1.0], 0.0, 1).tolist() == [1, 0]
    assert dstar.soft_cost(1.0, thr) > 0xF000 and dstar.soft_cost(-1.0, thr) < 0x1000
    assert dstar.soft_cost(100.0, thr) == 65535 and dstar.soft_cost(-100.0, thr) == 0


def test_generated_transmission_round_trip():
    rng = np.random.default_rng(11)
    for neg in (0, 1):
        h = dstar.make_header(0x40, "DIRECT", "RPT1", "CQCQCQ", "W1AW    ID51")
        fr = rng.integers(0, 2, (21, 4, 24)).astype(np.uint8)
        w, x, _ = dstar._tables()
        mask = np.zeros((4, 24), bool)
        mask[w, x] = True
        fr[:, ~mask] = 0
        sdb = dstar.compact_to_sd_bytes(dstar.make_header(0, "A", "B", "C", "W1AW")[:41] + b"  ", 0x55)
        sd = dstar.encode_slow_data(sdb)
        sym = np.concatenate([dstar.header_air_symbols(h, neg), dstar.bits_to_symbols(dstar.encode_voice(fr, sd), neg)])
        u = dstar.decode_unit(sym, 2 + neg, np.array([0.0, 0.5, -0.5, 1.0, -1.0], np.float32))
        assert u["header_crc_ok"] and bytes(u["header41"]) == h
        assert np.array_equal(u["ambe"], fr)
        assert u["sd"]["kind"] == dstar.SD_HEADER and u["sd"]["crc_ok"]


def capture_units(rf_mod):
    disc = rx4.capture_disc("iq_dstar.npz", 1)
    w = rx4.OracleFsk4Rx(dstar.profile(rf_mod)).run(disc)
    return w, dstar.decode_stream(w["sym"], w["sync_pos"], w["sync_pat"], w["sync_thr"])


@pytest.mark.parametrize("rf_mod", [2, 0])
def test_capture_gives_src_kb7wuk(rf_mod):
    """DECODE_IQ_DSTAR (tests/CMakeLists.txt:8951): the oracle loop with the D-STAR profile on the capture's discriminator stream.
    The capture carries the positive words (header syncs first, then voice syncs 2016 symbols apart); "SRC: KB7WUK" comes from the
    slow data's header format with a good CRC - the radio headers behind the two header syncs fail their CRC."""
    w, units = capture_units(rf_mod)
    pats = w["sync_pat"].tolist()
    assert dstar.PAT_HD_POS in pats and dstar.PAT_VOICE_POS in pats
    assert dstar.PAT_VOICE_NEG not in pats and dstar.PAT_HD_NEG not in pats
    srcs = [dstar.text(u["sd"]["hdr41"][27:39]) for _, u in units if u["sd"]["kind"] == dstar.SD_HEADER and u["sd"]["crc_ok"]]
    assert len(srcs) >= 3 and all(s.startswith("KB7WUK") for s in srcs), srcs
    assert not any(u["header_crc_ok"] for _, u in units)


def test_capture_negated_locks_the_negative_words():
    disc = -rx4.capture_disc("iq_dstar.npz", 1)
    w = rx4.OracleFsk4Rx(dstar.profile(2)).run(disc)
    units = dstar.decode_stream(w["sym"], w["sync_pos"], w["sync_pat"], w["sync_thr"])
    assert dstar.PAT_VOICE_NEG in w["sync_pat"].tolist()
    srcs = [dstar.text(u["sd"]["hdr41"][27:39]) for _, u in units if u["sd"]["kind"] == dstar.SD_HEADER and u["sd"]["crc_ok"]]
    assert srcs and all(s.startswith("KB7WUK") for s in srcs), srcs
