"""dPMR (-fm) on the CPU: the restatement in tests/dpmr.py against the reference's own unit-test vectors, the generated matched
filter against the compiled dpmr_filter, and the profile-driven oracle loop on the reference's dPMR capture."""
import ctypes as C

import numpy as np
import pytest

import dpmr
import orc
import rx4


def test_colour_codes_mask_and_reject():
    v = dpmr.vectors()
    assert len(v["color_codes"]) == 64
    for code, col in v["color_codes"]:
        bits = [(code >> (23 - i)) & 1 for i in range(24)]
        assert dpmr.color_code(bits) == col
        masked = code & ~0x555555
        assert dpmr.color_code([(masked >> (23 - i)) & 1 for i in range(24)]) == col
    for code in v["color_reject"]:
        assert dpmr.color_code([(code >> (23 - i)) & 1 for i in range(24)]) == -1


def test_scrambler_crc_and_air_interface_ids():
    v = dpmr.vectors()
    out, state = dpmr.scramble([0] * v["scrambler"]["in_zero_bits"], v["scrambler"]["seed"])
    assert out == v["scrambler"]["out"] and state == v["scrambler"]["state"]
    assert dpmr.crc7(v["crc7"]["bits"]) == v["crc7"]["crc"] and dpmr.crc7([]) == v["crc7"]["empty"]
    b = np.zeros(48, np.uint8)
    b[v["cch_crc"]["ones_at"]] = 1
    assert dpmr.cch_crc(b) == v["cch_crc"]["crc"]
    for val, s in v["aiid"]:
        assert dpmr.air_interface_id(val) == s
    # de-interleave: output[j * 12 + i] = input[i * 6 + j] (test_dpmr_voice_bridge.c:222-232)
    x = list(range(72))
    y = dpmr.deinterleave(x)
    assert all(y[j * 12 + i] == x[i * 6 + j] for i in range(12) for j in range(6))


def _cch_of(bits48):
    """encode: 48 data bits -> 36 dibits (Hamming(12,8) parity from the generator matrix the oracle's H implies, interleave,
    scramble) - the inverse of dpmr.decode_cch for the rule tests"""
    words = []
    for j in range(6):
        d = [int(x) for x in bits48[8 * j:8 * j + 8]]
        best = None
        for p in range(16):
            w = np.array(d + [(p >> (3 - k)) & 1 for k in range(4)], np.uint8)
            _, dec, ok = dpmr.fec3.oracle_decode(1, w.reshape(1, 12))
            if ok.all() and list(dec.reshape(-1)) == d and dpmr.fec3.oracle_decode(1, w.reshape(1, 12))[0].tolist() == [w.tolist()]:
                best = w
                break
        assert best is not None
        words += best.tolist()
    il = [0] * 72
    for j in range(6):
        for i in range(12):
            il[i * 6 + j] = words[j * 12 + i]
    s = dpmr.scramble(il)[0]
    return [s[2 * k] * 2 + s[2 * k + 1] for k in range(36)]


def _bits(fn, half, mode=0, version=0):
    b = [0] * 48
    b[0:2] = [(fn >> 1) & 1, fn & 1]
    b[2:14] = [(half >> (11 - k)) & 1 for k in range(12)]
    b[14:17] = [(mode >> (2 - k)) & 1 for k in range(3)]
    b[17:19] = [(version >> 1) & 1, version & 1]
    c = dpmr.crc7(b[:41])
    b[41:48] = [(c >> (6 - k)) & 1 for k in range(7)]
    return b


def test_superframe_part_rules_and_voice_halves():
    rng = np.random.default_rng(1)
    for fn0, fn1, kind in ((0, 1, "called"), (2, 3, "calling"), (1, 0, None), (3, 2, None)):
        for mode in (0, 1, 2, 5, 7):
            d = list(rng.integers(0, 4, dpmr.FRAME))
            d[0:36] = _cch_of(_bits(fn0, 0x123, mode))
            d[192:228] = _cch_of(_bits(fn1, 0x456, mode, 3))
            sf = dpmr.superframe(d)
            assert all(c["crc_ok"] and c["ham_ok"] for c in sf["cch"])
            assert sf["id"] == 0x123456 and dpmr.part_rule(sf) == (kind, True)
            assert dpmr.voice_halves(sf) == [mode in (0, 1, 5)] * 2 and sf["cch"][1]["version"] == 3
            # -xd: the same superframe sent inverted reads alike
            assert dpmr.superframe([x ^ 2 for x in d], inverted=1)["id"] == 0x123456


def test_superframe_part_outcomes_match_the_reference_vectors():
    """test_dpmr_voice_bridge.c:261-334: called / calling IDs, a changed calling ID, a weak ID that does not overwrite, unknown
    parts that toggle the next-part value (and leave 0 alone)"""
    st = {"tg": "", "src": "", "next": 0}
    for step in dpmr.vectors()["superframe_parts"]:
        if step["force_next"] is not None:
            st["next"] = step["force_next"]
        dpmr.update_part(st, step["part"])
        for k, v in step["expect"].items():
            assert st[k] == v, (step, st)


def test_voice_halves_match_the_reference_vectors():
    """test_dpmr_voice_bridge.c:118-190: four frames for the half whose mode is 0 / 1 / 5, none for the other; version 3 mutes
    without a key"""
    for g in dpmr.vectors()["voice_halves"]:
        frames, muted = dpmr.voice_plan(g["mode"], g["version"], g["key"])
        assert sum(frames) == g["frames"] and muted == g["muted"], g


def test_generated_taps_equal_compiled_dpmr_filter():
    r = orc.ref()
    if r is None:
        pytest.skip("oracle/_ref not built (the reference tree is absent)")
    r.dpmr_filter.argtypes = [C.c_float, C.c_int]
    r.dpmr_filter.restype = C.c_float
    r.init_rrc_filter_memory()
    taps = np.array(dpmr.dpmr_taps(), np.uint32).view(np.float32)
    x = np.zeros(600, np.float32)
    x[0], x[200], x[201] = 1.0, 0.5, -3.25
    want = np.array([r.dpmr_filter(float(v), 20) for v in x], np.float32)
    r.init_rrc_filter_memory()
    nt = len(taps)
    xp = np.concatenate([np.zeros(nt - 1, np.float32), x])
    got = np.zeros_like(want)
    for n in range(len(x)):
        acc = np.float32(0)
        for i in range(nt):
            acc = np.float32(acc + np.float32(taps[i] * xp[n + i]))
        got[n] = acc
    assert nt == 135 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_capture_reads_src_1601621_under_plain_fm():
    """DECODE_IQ_DPMR (tests/CMakeLists.txt:8950): the reference's dPMR capture through the pinned front end, the oracle loop on
    the plain -fm profile (FS2 as written, no -xd, the GFSK rules the reference's modulation vote settles on) and the
    restatement's identity rules -> "Src=1601621"; once published, every later superframe prints it."""
    disc = rx4.capture_disc("iq_dpmr.npz", 1)
    o = rx4.OracleFsk4Rx(dpmr.profile(0)).run(disc)
    sfs = dpmr.decode_stream(o["rec4"][:, 0], o["sync_pos"], inverted=0)
    srcs = [sf["src"] for _, sf in sfs]
    assert "1601621" in srcs
    first = srcs.index("1601621")
    assert all(s == "1601621" for s in srcs[first:])
    calling = [dpmr.air_interface_id(sf["id"]) for _, sf in sfs if sf["kind"] == "calling" and sf["strong"]]
    assert calling == ["1601621"]
    assert sfs[-1][1]["tg"] == "6038584"


def test_capture_superframes_under_xd():
    """The same capture hunted with -xd's word: superframes 384 symbols apart whose CCHs pass Hamming(12,8) and CRC7, frame
    numbers alternating 0 / 1 and 2 / 3 - the framing, scrambler, de-interleave and CRC layout on real traffic."""
    disc = rx4.capture_disc("iq_dpmr.npz", 1)
    inv = rx4.OracleFsk4Rx(dpmr.profile(1)).run(disc)
    sp = inv["sync_pos"]
    assert len(sp) >= 55 and int(np.sum(np.diff(sp) == dpmr.PERIOD)) >= 50
    sfs = dpmr.decode_stream(inv["rec4"][:, 0], sp, inverted=1)
    good = [sf for _, sf in sfs if sf["cch"][0]["crc_ok"] and sf["cch"][1]["crc_ok"]]
    assert len(good) >= 45
    assert {(sf["cch"][0]["fn"], sf["cch"][1]["fn"]) for sf in good} == {(0, 1), (2, 3)}
    # the same superframes from the negated stream with the plain word
    neg = rx4.OracleFsk4Rx(dpmr.profile(0)).run(-disc)
    assert np.array_equal(neg["sync_pos"], sp)
