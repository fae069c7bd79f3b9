"""The reference's own frame-sync known answers (tests/golden/framesync_vectors.json) replayed on the CPU restatements of the hunting
loops: the M17 matcher and the DMR word table (oracle/ddn_oracle_rx4.c, profiles of tests/rx4.py) and the CQPSK sync + map search
(oracle/ddn_oracle_cqrx.c).  Each case runs twice: from the primed state the reference's test starts from, and in stream form - the
symbols that drive a cold loop into that state, then the tested word (tests/framesync_kat.py).

Where the reference's tests run under other conditions than this project's single-protocol channels, the answers carry over because:

* Every frame type is enabled in the M17 and P25p2 files (tests/dsp/test_frame_sync_m17.c:278-289, test_frame_sync_p25p2_rtl.c:
  275-287).  getFrameSync() tries the matchers of frame_sync_try_protocol_matches() in turn and the first that returns a type wins;
  the other protocols' words are 20 or 24 dibits (D-STAR, X2TDMA, P25, DMR, YSF, NXDN 10 / dPMR 12) and none of them is inside the
  eight-symbol M17 test windows or the fill, and no other protocol's word equals a raw P25p2 / P25p1 sync image.  With
  only M17 enabled the preamble keeps its one-error tolerance (frame_sync_try_m17(), src/dsp/dsd_frame_sync.c:865-903: the
  disambiguation that drops it needs D-STAR, DMR or NXDN96 hunting - that half of test_frame_sync_internal_helpers.c:844-867 is not
  replayed, this project hunts one protocol per channel).
* msize = 1 (the short window).  The level window that gives the M17 test min -1.5 / max +1.5 (:870-888) is the hunting ring, not the
  extrema average: at a sync state->min = (state->min + lmin) / 2 with the test's cleared state (min = max = 0), so it pins the ring's
  estimate lmin = -3, lmax = +3 (src/dsp/dsd_frame_sync.c:2316-2336, frame_sync_level.c).  The test has no symbol history, so no warm
  start follows; this project always has one, and its warm start (dsd_sync_warm_start_thresholds_outer_only) replaces max / min with the
  means of the eight preamble symbols - +3 / -3 again.  The loop's lmin / lmax are checked against 2 x the expected values directly.
  For CQPSK the extrema average (dsd_state_push_minmax_window, msize deep) feeds the scanner centre (max + min) / 2.  With msize 1 it
  holds only the estimate at the sync symbol, whose ring has seen every level of the word: centre 0.  This project's window is 1024
  deep (the reference's default, dsd_init.c:170) and also averages the estimates of the word's first symbols, whose ring has seen only
  some of its levels, so for the two identity-map cases the centre lands near 0 but not within the test's 0.001: those two centre
  values are dropped (their sync type and map are kept).  The rotated maps replace the window with the raw fit
  (frame_sync_apply_p25_cqpsk_raw_fit(), :520-548): their centre and (max + min) / 2 are exact, primed or cold.
* 10 samples per symbol in the M17 file (test_frame_sync_m17.c:166): the same as this project's 48 ksps at 4800 symbols/s, so the
  stream form feeds the test's own sample stream.
"""
import ctypes as C

import numpy as np
import pytest

import framesync_kat as fk
import orc
import rx4

V = fk.vectors()
KAT_THR7 = np.float32([0.0, 2.0, -2.0, 3.0, -3.0, 2.4, -2.4])   # init_m17_sync_case(): center, umid, lmid, max, min, maxref, minref


def _prime(prof, last, pol, thr7):
    r = rx4.OracleFsk4Rx(prof)
    r.o.orc_fsk4rx_prime.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    t = np.ascontiguousarray(thr7, np.float32)
    r.o.orc_fsk4rx_prime(r.st, last, pol, t.ctypes.data)
    return r


def _levels(r):
    out = np.zeros(2, np.float32)
    r.o.orc_fsk4rx_get_levels.argtypes = [C.c_void_p, C.c_void_p]
    r.o.orc_fsk4rx_get_levels(r.st, out.ctypes.data)
    return out


def _syncs(out):
    return list(zip(out["sync_pos"].tolist(), out["sync_pat"].tolist()))


def test_fixture_holds_every_vector():
    assert len(V["m17"]) == 11 and len(V["dmr_rc"]) == 4 and len(V["cqpsk"]) == 7
    assert {c["label"] for c in V["m17"]} >= {"M17 rejects cold EOT", "M17 stream to EOT", "M17 preamble to LSF"}
    assert V["sync_ids"]["DMR_RC_DATA"] == 34 and V["m17_samples_per_symbol"] == fk.SPS


@pytest.mark.parametrize("case", V["m17"], ids=lambda c: c["label"])
def test_m17_primed(case):
    """the reference's call: lastsynctype / m17_polarity / levels as the test sets them, one cold getFrameSync() per step fed the
    pattern and then the fill ('1' when a sync is expected, '3' when none is)"""
    prof = rx4.profile(rx4.PROTO_M17)
    last, pol = case["last"] + 1, case["polarity"]       # this project numbers synctype_ids.h + 1, 0 = none
    for step in case["steps"]:
        want = fk.m17_pat(step["expect"])
        r = _prime(prof, last, pol, KAT_THR7)      # run_one_on_state(): a fresh hunt, lastsynctype and polarity carried
        sym = fk.levels(step["pattern"] + ("1" if want >= 0 else "3") * 300)
        got = _syncs(r.run(fk.samples(sym)))
        if want < 0:
            assert got == [], (case["label"], got)
        else:
            assert got[:1] == [(7, want)], (case["label"], got)     # (every word is eight symbols; the preamble syncs on its first)
            assert prof.pat_type[want] == step["expect"] + 1
            last, pol = prof.pat_type[want], (1 if want == rx4.M17_PRE_POS else pol)


@pytest.mark.parametrize("case", fk.m17_cases(V), ids=lambda c: c["label"])
def test_m17_stream_form(case):
    out = rx4.OracleFsk4Rx(rx4.profile(rx4.PROTO_M17)).run(fk.samples(case["sym"]))
    assert _syncs(out) == case["syncs"], (case["label"], _syncs(out))
    a, b = case["word"]
    in_word = [p for p, _ in _syncs(out) if a <= p <= b]
    assert in_word == ([b] if case["expect"] >= 0 else [])


def test_m17_one_error_preamble_is_the_preamble():
    t = V["m17_tolerance"]
    sym = fk.levels(t["pattern"] + "3" * 40)
    for r in (_prime(rx4.profile(rx4.PROTO_M17), 0, 0, KAT_THR7), rx4.OracleFsk4Rx(rx4.profile(rx4.PROTO_M17))):
        out = r.run(fk.samples(sym))
        assert _syncs(out)[:1] == [(7, fk.m17_pat(t["expect"]))]


def test_m17_short_window_levels_of_the_preamble():
    """test_short_m17_window_estimates_levels_without_warm_start_history: min -1.5 / max +1.5 = (0 + lmin) / 2, (0 + lmax) / 2"""
    t = V["m17_levels"]
    assert list(fk.levels(t["pattern"])) == t["levels"]
    zero7 = np.zeros(7, np.float32)
    r = _prime(rx4.profile(rx4.PROTO_M17), 0, 0, zero7)
    out = r.run(fk.samples(fk.levels(t["pattern"])))
    assert _syncs(out) == [(7, fk.m17_pat(t["expect"]))]
    lmin, lmax = _levels(r)
    assert (0.0 + lmin) / 2 == np.float32(t["min"]) and (0.0 + lmax) / 2 == np.float32(t["max"])
    # the warm start that follows in this project (the test has no history): the means of the eight symbols, the same levels
    assert out["sync_thr"][0][3] == 2 * t["max"] and out["sync_thr"][0][4] == 2 * t["min"]


@pytest.mark.parametrize("inverted", [0, 1])
def test_dmr_rc_word_and_its_polarity(inverted):
    prof = rx4.profile(rx4.PROTO_DMR, inverted=inverted)
    assert prof.n_pat == 9 and prof.pat_type[rx4.DMR_PAT_RC] == V["sync_ids"]["DMR_RC_DATA"] + 1
    assert prof.pat_neg[rx4.DMR_PAT_RC] == 0 and prof.pat_class[rx4.DMR_PAT_RC] == rx4.CLASS_RC and prof.lock_symbols[rx4.CLASS_RC] == 12
    for case in fk.dmr_cases(inverted, V):
        # primed: the KAT's min -3 / max +3, the word alone from a fresh hunt
        r = _prime(prof, 0, 0, KAT_THR7)
        got = _syncs(r.run(fk.samples(fk.levels(case["pattern"]))))
        assert got == ([(23, rx4.DMR_PAT_RC)] if case["pat"] >= 0 else []), (case["label"], got)
        # stream form: a cold loop, a lead-in, the word, fill
        out = rx4.OracleFsk4Rx(prof).run(fk.samples(case["sym"]))
        assert _syncs(out) == case["syncs"], (case["label"], _syncs(out))
        # with the handlers (the reference's plain -fs ones): the RC sync takes the configured count and starts no burst decode
        if not inverted:
            h = rx4.OracleFsk4Rx(rx4.profile(rx4.PROTO_DMR, handler=1))
            hout = h.run(fk.samples(case["sym"]))
            assert _syncs(hout) == case["syncs"]
            if case["pat"] >= 0:
                s = case["syncs"][0][0]
                assert (hout["fl"][s + 1:s + 13] & 1).all() and not (hout["fl"][s + 13:] & 1).any()
                assert h.events.n == 0


def _cq(protocol):
    return orc.OracleCqRx(orc.CQ_P25P2 if protocol == "p25p2" else orc.CQ_P25P1, 700 if protocol == "p25p2" else -1)


@pytest.mark.parametrize("case", V["cqpsk"], ids=lambda c: c["label"])
def test_cqpsk_sync_and_map(case):
    expect_neg = case["expect"] in (V["sync_ids"]["P25P2_NEG"], V["sync_ids"]["P25P1_NEG"])
    for primed in (True, False):
        rx = _cq(case["protocol"])
        if primed:
            rx.o.orc_cqrx_prime.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_float]
            rx.o.orc_cqrx_prime(rx.st, 0.0, -3.0, 3.0)
        raw = [int(c) for c in case["pattern"]]
        rec, fl = rx.run(fk.CQ_LEVEL[raw])
        assert np.flatnonzero(fl & 2).tolist() == [len(raw) - 1], (case["label"], primed)
        assert (fl[-1] >> 4) & 7 == case["map"] and bool(fl[-1] & 4) == expect_neg, (case["label"], primed, fl[-1])
        st = rx.state()
        assert int(st[3]) == case["map"] and int(st[4]) == (2 if expect_neg else 1)
        if case["map"] != 0:
            assert abs(st[0] - case["center"]) <= 0.001 and abs((st[1] + st[2]) / 2 - case["scanner_center"]) <= 0.001, (primed, st)


def test_cqpsk_stream_form_and_negative_dibit_polarity():
    neg = V["cqpsk_neg"]
    for proto in ("p25p2", "p25p1"):
        for case in fk.cq_cases(proto, V):
            rec, fl = _cq(proto).run(case["sym"])
            s = case["sync"]
            assert np.flatnonzero(fl & 2).tolist() == [s] and (fl[s] >> 4) & 7 == case["map"], case["label"]
            if case["expect"] == neg["synctype"] and case["map"] == neg["map"]:
                # the symbol after the sync is at neg["input"]: dibit 1, LLR signs (bit0 0, bit1 1)
                assert fk.np.float32(case["sym"][s + 1]) == neg["input"]
                assert rec[s + 1, 0] == neg["dibit"]
                assert (rec[s + 1, 2] > 0) == bool(neg["llr_bits"][0]) and (rec[s + 1, 3] > 0) == bool(neg["llr_bits"][1])
                assert rec[s + 1, 2] != 0 and rec[s + 1, 3] != 0
    # the dibit decision itself, from the test's slicer state (centre 0, min -3, max +3), map X2400, negative polarity
    o = orc.oracle()
    o.orc_cq_digitize.argtypes = [C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_double, C.c_void_p]
    rx = _cq("p25p2")
    rx.o.orc_cqrx_prime.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_float]
    rx.o.orc_cqrx_prime(rx.st, 0.0, -3.0, 3.0)
    rec4 = np.zeros(4, np.int32)
    o.orc_cq_digitize(C.addressof(rx.st) + orc._cqrx_slicer_offset(), neg["input"], neg["map"], 1, -100.0, rec4.ctypes.data)
    assert rec4[0] == neg["dibit"] and (rec4[2] > 0) == bool(neg["llr_bits"][0]) and (rec4[3] > 0) == bool(neg["llr_bits"][1])
