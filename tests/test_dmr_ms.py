"""CPU: the restatement of dmrMSData() / dmrMSBootstrap() + dmrMS() (tests/dmr_ms.py) against the reference's own counts
(tests/golden/dmr_ms_vectors.json, parsed out of tests/protocol/dmr/test_dmr_ms_data.c by tests/golden/make_golden_dmr_ms.py), and its
two derivations against each other: reading the stream as the reference reads it, and the stage's call-by-call rule."""
import json
import os
import re

import numpy as np
import pytest

import ddn
import dmr_ms
import dmrmsgen as gen
import fec3

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "dmr_ms_vectors.json")))


@pytest.fixture(scope="module")
def stream(built):
    rng = np.random.default_rng(3)
    dib, lcs = gen.traffic()
    rec = gen.records(dib, rng)
    return rec, gen.syncs_of(dib, rng), lcs


def test_the_lock_counts_are_the_reference_s(built, stream):
    """264 behind a data word, 1704 behind a voice word: the restatement's list, the header's constants, and what reading the stream as
    the reference reads it comes to behind every sync"""
    assert dmr_ms.LOCK[0] == GOLD["data"]["symbols"] == 264 and dmr_ms.LOCK[1] == GOLD["bootstrap"]["symbols"] == 1704
    hdr = open(os.path.join(ddn.ROOT, "include", "ddn_fsk4.h")).read()
    assert int(re.search(r"#define DDN_DMR_MS_LOCK_DATA (\d+)", hdr).group(1)) == GOLD["data"]["symbols"]
    assert int(re.search(r"#define DDN_DMR_MS_LOCK_VOICE (\d+)", hdr).group(1)) == GOLD["bootstrap"]["symbols"]
    rec, syncs, _ = stream
    _, _, _, read = dmr_ms.read_stream(rec[:, 0], rec[:, 1], syncs)
    pats = {p: pat for p, pat, _, _ in syncs}
    assert len(read) == len(syncs) == 18
    for p, n in read:
        assert n == (GOLD["bootstrap"]["symbols"] if pats[p] in dmr_ms.VOICE_PATS else GOLD["data"]["symbols"]), (p, n)
    # dmrMS() alone: what follows the bootstrap burst's 54 live dibits and the skip behind them
    assert GOLD["bootstrap"]["symbols"] - 54 - 144 == GOLD["cycle"]["symbols"] == 1506
    assert GOLD["bootstrap"]["skip_total"] == 144 * GOLD["bootstrap"]["skips"] and GOLD["cycle"]["skip_total"] == 144 * GOLD["cycle"]["skips"]


def test_vocoder_calls_and_link_controls_per_unit(built, stream):
    rec, syncs, lcs = stream
    _, voice, lc, _ = dmr_ms.read_stream(rec[:, 0], rec[:, 1], syncs)
    units = sum(pat in dmr_ms.VOICE_PATS for _, pat, _, _ in syncs)
    assert units == 3 and 3 * len(voice) == GOLD["bootstrap"]["vocoder_calls"] * units
    assert sum(v["vc"] > 1 for v in voice) * 3 == GOLD["cycle"]["vocoder_calls"] * units
    assert len(lc) == GOLD["cycle"]["embedded_lc_calls"] * units
    assert [v["vc"] for v in voice] == [1, 2, 3, 4, 5, 6] * units
    for got, (sent, good) in zip(lc, lcs):
        assert got["errs"] == 0 and got["ok"] == int(good) and np.array_equal(got["lc77"][:72], sent)


def test_a_data_burst_is_the_hand_over_then_54_live_dibits(built, stream):
    """the reference's index assertions: payload[0] / [89] are the hand-over's ends, [90] / [143] the live half's, reliabilities alike"""
    rec, syncs, _ = stream
    data, _, _, _ = dmr_ms.read_stream(rec[:, 0], rec[:, 1], syncs)
    by_start = {b["start"]: b for b in data}
    n = 0
    for p, pat, pre, prel in syncs:
        if pat not in dmr_ms.DATA_PATS:
            continue
        b = by_start[p - 89]
        for at, k in GOLD["data"]["payload_from_handover"]:
            assert b["dib"][at] == pre[k] & 3 and b["rel"][at] == prel[k]
        for at, k in GOLD["data"]["payload_from_stream"]:
            assert b["dib"][at] == rec[p + 1 + k, 0]
        for at, k in GOLD["data"]["live_reliability"]:
            assert b["rel"][at] == rec[p + 1 + k, 1]
        n += 1
    assert n == 15


def test_burst_offsets(built, stream):
    """burst k of a unit starts at p + 199 + 288 k by the counts of dibits read and skipped, and the stage's rule says the same"""
    rec, syncs, _ = stream
    _, voice, _, _ = dmr_ms.read_stream(rec[:, 0], rec[:, 1], syncs)
    want = []
    for p, pat, _, _ in syncs:
        if pat in dmr_ms.VOICE_PATS:
            want += [p - 89] + [p + 199 + 288 * k for k in range(5)]
    assert [v["start"] for v in voice] == want
    one = dmr_ms.walk_call(dmr_ms.State(), rec[:, 0], rec[:, 1], len(rec), 0, syncs)
    assert [v["start"] for v in one["voice"]] == want


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for k in x:
            if k in y and k not in ("start", "pos", "pre", "sync", "fec"):
                assert np.array_equal(x[k], y[k]), k


def test_both_derivations_agree(built, stream):
    rec, syncs, _ = stream
    data, voice, lc, _ = dmr_ms.read_stream(rec[:, 0], rec[:, 1], syncs)
    s = dmr_ms.State()
    one = dmr_ms.walk_call(s, rec[:, 0], rec[:, 1], len(rec), 0, syncs)
    _same(one["data"], data)
    _same(one["voice"], voice)
    _same(one["lc"], lc)
    assert [b["start"] for b in one["data"]] == [b["start"] for b in data] and [b["pos"] for b in one["lc"]] == [b["pos"] for b in lc]
    assert s.cc == 5 and s.next == 5 and s.dropped == 0        # the last burst is a CSBK under colour code 5; no unit left open


@pytest.mark.parametrize("step", [1, 3, 200, 1000])
def test_the_walk_does_not_depend_on_the_calls(built, stream, step):
    """rows of 256 carried records + `step` new ones, down to one record a call: the same bursts, each once, at the same place"""
    rec, syncs, _ = stream
    rec, syncs = rec[:7200], [s for s in syncs if s[0] < 7000]
    one = dmr_ms.walk_call(dmr_ms.State(), rec[:, 0], rec[:, 1], len(rec), 0, syncs)
    s, got = dmr_ms.State(), dict(data=[], voice=[], lc=[])
    for c in gen.calls_of(rec, syncs, list(range(step, len(rec) + 1, step)) + ([len(rec)] if len(rec) % step else []), 256):
        o = dmr_ms.walk_call(s, c["row"][:, 0], c["row"][:, 1], c["cnt"], c["new"], c["syncs"])
        for k in got:
            for b in o[k]:
                key = "pos" if k == "lc" else "start"
                b[key] += c["lo"]
                got[k].append(b)
    for k in got:
        _same(got[k], one[k])
        key = "pos" if k == "lc" else "start"
        assert [b[key] for b in got[k]] == [b[key] for b in one[k]], k
    assert len(one["voice"]) == 12 and len(one["lc"]) == 2 and len(one["data"]) >= 12


def test_a_full_list_drops_and_counts(built, stream):
    rec, syncs, _ = stream
    s = dmr_ms.State()
    o = dmr_ms.walk_call(s, rec[:, 0], rec[:, 1], len(rec), 0, syncs, max_data=14, max_voice=17, max_lc=2)
    assert (len(o["data"]), len(o["voice"]), len(o["lc"]), s.dropped) == (14, 17, 2, 3)


def test_hamming_7_4_refuses_nothing(built):
    """The code is perfect: every syndrome names a position, so neither dmr_data_collect_cach() nor dmr_ms_decode_tact() can see a TACT
    fail, whatever is sent.  Status 1 of a data burst and d_voice_tact_ok = 0 are kept because the reference has the branch; no traffic
    reaches them, and tests/test_dmr_ms_traffic.py therefore holds no floor for a failed TACT."""
    words = ((np.arange(128)[:, None] >> np.arange(7)[None, :]) & 1).astype(np.uint8)
    _, _, ok = fec3.oracle_decode(0, words)
    assert ok.all()
