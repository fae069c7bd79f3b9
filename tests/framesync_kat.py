"""The reference's frame-sync known answers (tests/golden/framesync_vectors.json, written by tests/golden/make_golden_framesync.py) as
inputs of this project's receive loops: the stream form of every case - symbols that drive a cold loop into the case's starting state,
then the tested word - with the sync each word must produce.  TEST INFRASTRUCTURE - the product never imports this."""
import json
import os

import numpy as np

import rx4

HERE = os.path.dirname(os.path.abspath(__file__))
SPS = 10                          # 48 ksps at 4800 symbols/s: the KAT's own 10 samples per symbol
M17_FRAME, M17_PRE_LOCK = 184, 8  # lock_symbols of the M17 profile: every frame / EOT, the preamble


def vectors():
    with open(os.path.join(HERE, "golden", "framesync_vectors.json")) as f:
        return json.load(f)


def levels(pattern):
    """sign-dibit string ('1' = +3, '3' = -3) -> symbol levels"""
    return np.array([3.0 if c == "1" else -3.0 for c in pattern], np.float32)


def samples(sym):
    return np.repeat(np.asarray(sym, np.float32), SPS)


def m17_pat(sync_id):
    """a synctype_ids.h value -> the row of the M17 table (flags / sync_pat), -1 for none"""
    return -1 if sync_id < 0 else rx4.M17_TYPES.index(sync_id + 1)


def m17_cases(v=None):
    """-> list of dict(label, sym, syncs [(symbol index, pattern row)], word (first, last symbol of the tested word), expect)"""
    v = v or vectors()
    w, ids = v["m17_words"], v["sync_ids"]
    pre2 = w["M17_PRE"] + w["M17_PRE"]   # the preamble syncs on its first eight symbols; its handler skips the next eight
    prefix = {ids["NONE"]: [], ids["M17_LSF_POS"]: ["LSF"], ids["M17_BRT_POS"]: ["BRT"], ids["M17_STR_POS"]: ["LSF", "STR"],
              ids["M17_PKT_POS"]: ["LSF", "PKT"]}
    out = []
    for case in v["m17"]:
        seq, syncs = "", []
        if len(case["steps"]) == 2:
            assert case["last"] == ids["NONE"] and case["steps"][0]["pattern"] == pre2
            assert m17_pat(case["steps"][0]["expect"]) == rx4.M17_PRE_POS
            words = ["PRE2"]
        else:
            words = (["PRE2"] if case["last"] != ids["NONE"] else []) + prefix[case["last"]]
            assert (case["polarity"] == 1) == bool(words)
        for name in words:        # each prefix word syncs on its last symbol (the preamble on its first eight), then its lock runs
            if name == "PRE2":
                syncs.append((len(seq) + 7, rx4.M17_PRE_POS))
                seq += pre2
            else:
                seq += w["M17_" + name]
                syncs.append((len(seq) - 1, m17_pat(ids["M17_%s_POS" % name])))
                seq += "1" * M17_FRAME
        step = case["steps"][-1]
        first = len(seq)
        seq += step["pattern"]
        pat = m17_pat(step["expect"])
        if pat >= 0:
            syncs.append((len(seq) - 1, pat))
            seq += "1" * (M17_PRE_LOCK if pat < 2 else M17_FRAME)
        seq += "3" * 240                 # no word within one error of an all-minus window follows any of these states
        out.append(dict(label=case["label"], sym=levels(seq), syncs=syncs, word=(first, first + len(step["pattern"]) - 1), expect=pat))
    return out


def dmr_cases(inverted, v=None):
    """the RC vectors of one polarity: 100 symbols of a lead-in no DMR word matches, the word, 300 symbols of minus fill"""
    v = v or vectors()
    lead = "3311" * 25
    out = []
    for case in v["dmr_rc"]:
        if case["inverted"] != inverted:
            continue
        seq = lead + case["pattern"] + "3" * 300
        pat = rx4.DMR_PAT_RC if case["expect"] >= 0 else -1
        last = len(lead) + 23
        out.append(dict(label="%s inverted=%d" % (case["word"], inverted), pattern=case["pattern"], sym=levels(seq), expect=case["expect"], pat=pat,
                        syncs=[(last, pat)] if pat >= 0 else [], word=(len(lead), last)))
    return out


CQ_LEVEL = np.array([1.0, 3.0, -1.0, -3.0], np.float32)   # raw dibit -> the CQPSK demodulator's symbol (the KAT's fake reader)


def cq_cases(protocol, v=None):
    """CQPSK vectors of one protocol ("p25p1" / "p25p2"): the raw pattern from a cold loop, then one symbol at 1.0 (the in-frame
    dibit test_negative_cqpsk_dibit_polarity reads), then fill at +3 (raw '1', the KAT's own fill)"""
    v = v or vectors()
    out = []
    for case in v["cqpsk"]:
        if case["protocol"] != protocol:
            continue
        raw = [int(c) for c in case["pattern"]]
        sym = np.concatenate([CQ_LEVEL[raw], np.float32([1.0]), np.full(1000, 3.0, np.float32)]).astype(np.float32)
        out.append(dict(case, sym=sym, sync=len(raw) - 1))
    return out
