"""The traffic the short-call cases of tests/test_chain_p25p2_short_calls_gpu.py run on, judged by the CPU oracle alone (a chain that
decodes nothing equals a reference that holds nothing).  Capture, at every call size: twelve syncs or more with 700 records behind them and
eight or more SACCH PDUs with a good CRC-12, every one of the capture's known PDUs.  Synthetic voice, every case and every channel of it:
eight syncs or more, ten 4V and two 2V timeslots, two good ESS, forty voice frames on logical channel 0 that are a contiguous run of what
was planted.  At 1999 / 999 samples no call brings as many records as the carry holds and every group crosses three calls or more; the
5760 / 5761 / 2881 cases together land the new-record count on two or more of carry - 1, carry, carry + 1."""
import numpy as np
import pytest

import chain_p25p2_stream as cs
import p2seq
from test_oracle_p25p2_capture import SACCH_OCTETS


def _spans(ws):
    """how many calls the 720 records of every group (sync and body) touch"""
    edge = np.cumsum(ws["new"])
    return [int(np.searchsorted(edge, p + 700, side="right") - np.searchsorted(edge, p - 19, side="right")) + 1 for p in ws["pos"]]


@pytest.mark.parametrize("n_call", cs.CAPTURE_CALLS)
def test_capture_cases_hold_traffic(built, n_call):
    _, ws = cs.capture_case(n_call)
    assert ws["new"].sum() == ws["n"]
    assert len(ws["pos"]) >= 12, ws["pos"]
    sacch = [r for r in ws["rows"] if r["action"] == p2seq.A_SACCH_S and r["crc12"]]
    assert len(sacch) >= 8, len(sacch)
    assert all(bytes(np.packbits(r["payload"])[:12]).hex() in SACCH_OCTETS for r in sacch)
    # the same stream without a valid site: the scrambled bursts are skipped
    _, no = cs.capture_case(n_call, site=False)
    assert no["pos"] == ws["pos"]
    assert all(b["action"] == p2seq.A_NOSITE for a, b in zip(ws["rows"], no["rows"]) if a["action"] == p2seq.A_SACCH_S)
    if n_call == 1999:
        assert ws["new"].max() < cs.CARRY and min(_spans(ws)) >= 3, (ws["new"], _spans(ws))


def test_one_second_calls_hold_more_syncs_than_one_slot(built):
    """the too-few-slots case (max_groups = 1 at 48000 samples a call): two calls or more hold a sync, and eight syncs or more find no slot"""
    _, ws = cs.capture_case(48000)
    per_call = cs.groups_per_call(ws)
    assert sum(n > 0 for n in per_call) >= 2 and sum(max(n - 1, 0) for n in per_call) >= 8, per_call


def test_calls_land_on_the_carry_edges(built):
    seen = set()
    for n_call in (5760, 5761):
        seen |= set(cs.capture_case(n_call)[1]["new"].tolist())
    for sps, rate, n_call in cs.VOICE_CALLS:
        if n_call in (5761, 2881):
            for ws in cs.voice_case(sps, rate, n_call)[2]:
                seen |= set(ws["new"].tolist())
    assert len(seen & {cs.CARRY - 1, cs.CARRY, cs.CARRY + 1}) >= 2, seen


def _voice_floors(ws, planted, tag, short):
    rows = ws["rows"]
    assert ws["new"].sum() == ws["n"]
    assert len(ws["pos"]) >= 8, (tag, ws["pos"])
    assert sum(r["action"] == p2seq.A_4V for r in rows) >= 10, tag
    assert sum(r["action"] == p2seq.A_2V for r in rows) >= 2, tag
    assert sum(r["action"] == p2seq.A_2V and bool(r["ess_ok"]) for r in rows) >= 2, tag
    bits = ws["voice"][0][0]
    assert len(bits) >= 40, (tag, len(bits))
    assert planted is None or cs.planted_run(bits, planted), tag
    if short:
        assert ws["new"].max() < cs.CARRY and min(_spans(ws)) >= 3, (tag, ws["new"], _spans(ws))


@pytest.mark.parametrize("sps,rate,n_call", cs.VOICE_CALLS)
def test_synthetic_voice_cases_hold_traffic(built, sps, rate, n_call):
    iq, planted, refs, seeds = cs.voice_case(sps, rate, n_call)
    for c, ws in enumerate(refs):
        _voice_floors(ws, planted[c], (sps, n_call, c), n_call in (1999, 999))
        assert ws["voice"][0][2] is not None and float(np.abs(ws["voice"][0][2]).sum()) > 0      # the reference PCM is not silence


def test_flush_cut_leaves_a_group_to_the_flush(built):
    """after FLUSH_CUT calls of the first voice case the first channel's last 720 records begin with a sync (within 20) that no call has
    decoded, the second channel's do not; and the flush of the whole run files a group too"""
    iq, planted, refs, seeds = cs.voice_case(*cs.VOICE_CALLS[0])
    hits = []
    for ws in refs:
        total = int(ws["new"][:cs.FLUSH_CUT].sum())
        hits.append([p for p in ws["pos"] if total - cs.CARRY <= p < total - cs.CARRY + cs.FLUSH_SCAN])
    assert len(hits[0]) == 1 and hits[1] == [], hits
    rows = refs[0]["rows"][4 * refs[0]["pos"].index(hits[0][0]):][:4]
    assert any(r["slot"] == 0 and r["action"] in (p2seq.A_4V, p2seq.A_2V) for r in rows)          # it carries voice
    lo, hi = cs.scan_ranges(refs[0]["new"])[-1]
    assert any(lo <= p < hi for p in refs[0]["pos"])


def test_wide_case_holds_traffic_on_every_channel(built):
    """67 channels, channel c lagging by 47 c samples: the floors on every channel with a valid site, and the channels out of step - in
    most calls the new-record counts differ across channels, the sync positions differ from channel to channel, and so does the call
    that files a channel's first group, on both sides of the 64-lane edge"""
    iq, planted, refs, seeds = cs.wide_case()
    assert len(refs) == cs.WIDE_B > 64 and seeds[cs.WIDE_NOSITE] == 0
    first_call = []
    for c, ws in enumerate(refs):
        if c == cs.WIDE_NOSITE:
            assert len(ws["pos"]) >= 8 and all(r["action"] not in (p2seq.A_4V, p2seq.A_2V) for r in ws["rows"])
            assert sum(r["action"] == p2seq.A_NOSITE for r in ws["rows"]) >= 12
        else:
            _voice_floors(ws, None, ("wide", c), True)
        ranges = cs.scan_ranges(ws["new"])
        first_call.append(next(k for k, (lo, hi) in enumerate(ranges) if lo <= ws["pos"][0] < hi))
    # a frame or two of the first group decoded can come out wrong beyond the AMBE code's reach: the planted run is asked of the channels
    # whose reference holds it - all but a few, the ones whose PCM is checked among them
    clean = cs.wide_clean()
    assert len(clean) >= 60 and set(cs.WIDE_PCM) <= set(clean), clean
    news = np.array([ws["new"] for ws in refs])
    assert (news.min(axis=0) != news.max(axis=0)).sum() >= news.shape[1] // 2, news
    assert len({ws["pos"][0] for ws in refs}) >= cs.WIDE_B // 2
    assert len(set(first_call[:64])) >= 2 and len(set(first_call[64:])) >= 2, first_call
    per_call = np.array([cs.groups_per_call(ws) for ws in refs])
    assert (per_call.min(axis=0) != per_call.max(axis=0)).sum() >= 8, per_call          # calls in which some channels file a group and others none
