"""CPU: the restatement of the NXDN control and data channels (tests/nxdn_ctrl.py) against (a) the answers the reference's own tests
hold (tests/golden/nxdn_ctrl_vectors.json, parsed by tests/golden/make_golden_nxdn_ctrl.py), (b) the generator (tests/nxdngen.py):
every kind decodes to the bits that were encoded, (c) the reference's captures: the NXDN48 one delivers VCALL messages with source 901
and RAN 1 - the string DECODE_IQ_NXDN48 asserts -, the NXDN96 one RAN 0.  Integers throughout: every comparison is equality."""
import json
import os

import numpy as np
import pytest

import nxdn_ctrl as nc
import nxdngen as gen
import rx4

VEC = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nxdn_ctrl_vectors.json")))


def test_crc16cac_answers_of_the_reference(built):
    assert [v["name"] for v in VEC["crc16cac"]] == ["empty", "pattern8", "pattern171"]
    for v in VEC["crc16cac"]:
        assert nc.crc16cac(v["bits"][:v["n"]]) == v["crc"], v["name"]
    assert [v["crc"] for v in VEC["crc16cac"]] == [0x3C11, 0xF862, 0x2608]


def test_crc15_window_rules_of_the_reference(built):
    """the payload CRC runs over bits 0..183, the check field is bits 184..198, the bits behind count for neither"""
    w = VEC["crc15_windows"]
    t = np.zeros(w["row"], np.uint8)
    t[:len(w["payload"])] = w["payload"]
    crc = nc.crc15(t[:184])
    assert (len(w["payload"]), w["check_at"], w["check_len"], w["tail_at"], w["row"]) == (184, 184, 15, 199, 208)
    t[w["check_at"]:w["check_at"] + w["check_len"]] = gen.bits_of(crc, w["check_len"])
    t[w["tail_at"]:w["tail_at"] + w["tail_len"]] = gen.bits_of(w["tail"], w["tail_len"])
    assert nc.facch2_crc15_payload(t) == crc and nc.facch2_crc15_check(t) == crc and nc.field_ok(nc.KIND_FACCH2, t)
    t[w["tail_at"]:] ^= 1
    assert nc.facch2_crc15_payload(t) == crc and nc.facch2_crc15_check(t) == crc and nc.field_ok(nc.KIND_UDCH, t)
    t[100] ^= 1
    assert nc.facch2_crc15_payload(t) != crc and not nc.field_ok(nc.KIND_FACCH2, t)


def test_sequence_rule_part_of_frame_and_ran_of_the_reference(built):
    assert len(VEC["sequence_rule"]) == 6
    for v in VEC["sequence_rule"]:
        assert int(nc.sequence_is_valid(v["crc_ok"], v["previous"], v["part"])) == v["valid"], v
    assert sorted(v["sf"] for v in VEC["part_of_frame"]) == [0, 1, 2, 3]
    for v in VEC["part_of_frame"]:
        assert nc.sacch_part_of_frame(v["sf"]) == v["part"], v
    t = np.zeros(8, np.uint8)
    t[VEC["ran_from_trellis"]["ones"]] = 1
    assert nc.ran_from_trellis(t) == VEC["ran_from_trellis"]["ran"] == 0x29


def test_lich_sets_are_the_loops_gate(built):
    """the profile table restated here is the 128-bit set the receive loop's gate carries (csrc/ddn_fsk4h_dev.h, nxdn_lich_ok)"""
    m = [0x00000122, 0x03FFC303, 0x00FFC743, 0x00EFC30F]
    assert {l for l in range(128) if (m[l >> 5] >> (l & 31)) & 1} == set(nc.LICH_PROFILE)
    assert nc.LICH_SACCH < nc.LICH_PROFILE and set(nc.LICH_KIND) < nc.LICH_PROFILE and not set(nc.LICH_KIND) & nc.LICH_SACCH


@pytest.mark.parametrize("level", [255, 0, None])
def test_every_kind_decodes_to_the_bits_that_were_encoded(built, level):
    """generator -> restatement at reliabilities of 255, of 0 (the soft decoder has nothing to go on: the retry's bits) and mixed"""
    rng = np.random.default_rng(40 + (level or 7))
    rel = lambda: np.full(182, level, np.uint8) if level is not None else rng.integers(60, 256, 182).astype(np.uint8)
    for lich in (0x01, 0x05):
        f, word = gen.cac_frame(rng, 33, lich7=lich)
        d = nc.decode_frame(f[10:], rel())
        assert (d["kind"], d["crc_ok"], d["ran"], d["sf"]) == (nc.KIND_CAC, 1, 33, 0)
        assert np.array_equal(d["bits208"][:171], word) and not d["bits208"][171:].any()
        assert np.array_equal(d["bytes26"][:22], np.packbits(d["bits208"][:176])) and not d["bytes26"][22:].any()
        assert level != 0 or d["fallback"] == 1
    for lich, kind in ((0x28, 2), (0x29, 2), (0x49, 2), (0x2E, 3), (0x2F, 3), (0x4E, 3), (0x4F, 3)):
        f, word = gen.facch2_frame(rng, 5, lich7=lich, sf=lich & 3)
        d = nc.decode_frame(f[10:], rel())
        assert (d["kind"], d["crc_ok"], d["ran"], d["sf"]) == (kind, 1, 5, lich & 3)
        assert np.array_equal(d["bits208"][:199], word) and not d["bits208"][199:].any()
        assert np.array_equal(d["bytes26"], np.packbits(d["bits208"]))
    for sf in range(4):
        msg = rng.integers(0, 2, 18).astype(np.uint8)
        f, word = gen.sacch_frame(rng, sf, 17, msg, lich7=(0x30, 0x36)[sf & 1])
        soft, ok, hard, hok = nc.sacch_of(f[10:], rel())
        assert ok or hok
        assert np.array_equal(np.unpackbits(soft) if ok else hard, word)
    # a broken CRC stays broken through both decodes; a LICH off the table or with bad parity names no channel
    for f in (gen.cac_frame(rng, 1, bad_crc=True)[0], gen.facch2_frame(rng, 1, bad_crc=True)[0]):
        d = nc.decode_frame(f[10:], rel())
        assert d["kind"] and (d["crc_ok"], d["fallback"]) == (0, 1)
    f = gen.sacch_frame(rng, 1, 2, np.zeros(18, np.uint8), lich7=gen.LICH_OFF_TABLE)[0]
    d = nc.decode_frame(f[10:], rel())
    assert (d["kind"], d["lich"], bool(d["parity"])) == (0, gen.LICH_OFF_TABLE, True)
    f = gen.frame(0x01, np.zeros(348, np.uint8), bad_parity=True)
    d = nc.decode_frame(f[10:], rel())
    assert (d["kind"], d["lich"], bool(d["parity"])) == (0, 0x01, False)


def test_the_walk_rule_by_rule(built):
    """the generated traffic's frames (tests/nxdngen.control_frames) straight through the walk: what each passage is there for"""
    rng = np.random.default_rng(9)
    s, log = nc.State(), []
    for f in gen.control_frames():
        d, r = f[10:], np.full(182, 255, np.uint8)
        fr = nc.decode_frame(d, r)
        w = nc.walk_frame(s, fr["lich"] | (0x80 if fr["parity"] else 0), 1, *nc.sacch_of(d, r), fr)
        log.append((fr, w))
    msgs = [(k, w) for k, (fr, w) in enumerate(log) if w["msg_status"]]
    super1 = [w for _, w in msgs if w["msg_status"] == 1 and w["sacch_status"] == 1]
    assert [rx4.bits_int(w["msg72"][24:40]) for w in super1] == [901, 902, 906, 909, 910]       # the parity failure reset nothing: 906
    assert all(w["last_ran"] == 9 and rx4.bits_int(w["msg72"][2:8]) == 1 for w in super1)
    assert [w["sacch_status"] for _, w in msgs if w["sacch_status"] >= 3] == [3, 3]              # (a bad non-superframe SACCH: no message)
    undelivered = [rx4.bits_int(w["msg72"][54:72]) for _, w in msgs if w["msg_status"] == 2]
    assert len(undelivered) == 5                   # a bad segment, out of order, the profile miss, FACCH2 for part 1, a bad FACCH2
    # after a FACCH2 with SF 2 part 2 is in sequence; after a FACCH2 with a broken CRC (part_of_frame 0) it is not
    f2 = [k for k, (fr, w) in enumerate(log) if fr["kind"] == nc.KIND_FACCH2 and log[k - 1][1]["sacch_status"] == 1 and log[k + 1][1]["sacch_status"] == 1]
    assert len(f2) == 2
    assert (log[f2[0]][1]["pf"], log[f2[0] + 1][1]["seq_ok"], log[f2[0] + 1][1]["pf"]) == (1, 1, 2)
    assert (log[f2[1]][1]["pf"], log[f2[1] + 1][1]["seq_ok"], log[f2[1] + 1][1]["pf"]) == (0, 0, 2)
    # cac_fail counts the bad CACs in a row and a good one clears it
    fails = [w["cac_fail"] for fr, w in log if fr["kind"] == nc.KIND_CAC]
    assert max(fails) == 3 and fails[-1] == 0 and fails[fails.index(3) + 1] == 0


def test_cac_fail_reports_11_and_starts_again(built):
    """the documented deviation: where the reference resets its symbolizer the counter alone starts again, and the frame reports 11"""
    s = nc.State()
    bad, good = dict(kind=nc.KIND_CAC, crc_ok=0, ran=0, sf=0), dict(kind=nc.KIND_CAC, crc_ok=1, ran=7, sf=0)
    z4, z32 = np.zeros(4, np.uint8), np.zeros(32, np.uint8)
    seen = [nc.walk_frame(s, 0x81, 1, z4, 0, z32, 0, bad)["cac_fail"] for _ in range(13)]
    assert seen == [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 1, 2] and s.last_ran == -1
    assert nc.walk_frame(s, 0x81, 1, z4, 0, z32, 0, good)["cac_fail"] == 0 and s.last_ran == 7
    assert nc.walk_frame(s, 0x81, 0, z4, 0, z32, 0, bad)["cac_fail"] == 0          # a slot that is not valid is passed over


_CAPTURE = {}


def capture(which):
    """a capture of the reference through the pinned front end, the oracle loop with its handlers and the restatement, once"""
    if which not in _CAPTURE:
        import chain_fsk4_stream as cs
        iq = cs._golden_iq("iq_%s.npz" % which)
        _CAPTURE[which] = nc.stream_reference(cs.nxdn_oracle_stream(iq, len(iq), which))
    return _CAPTURE[which]


def test_nxdn48_capture_delivers_vcall_source_901_ran_1(built):
    """what rx4.nxdn_superframes used to string together in test code now comes out of the walk's rules"""
    ref = capture("nxdn48")
    msgs = nc.delivered(ref)
    vcall = [m for _, ran, m in msgs if rx4.bits_int(m[2:8]) == 1]
    assert len(vcall) >= 4 and all(ran == 1 for _, ran, _ in msgs)
    assert all(rx4.bits_int(m[24:40]) == 901 for m in vcall)
    assert not any(fr["kind"] for _, fr, _ in ref)                    # a voice call: no control frame in it


def test_nxdn96_capture_delivers_ran_0(built):
    ref = capture("nxdn96")
    msgs = nc.delivered(ref)
    assert len(msgs) >= 1 and all(ran == 0 for _, ran, _ in msgs)
