"""GPU: the P25 Phase 2 chain object (ddn_p25p2_chain) at calls shorter than its carry, against the whole-stream CPU reference
(tests/chain_p25p2_stream.py; the traffic floors of every case are in tests/test_chain_p25p2_short_calls_traffic.py).  Whatever the call
size, every group is decoded once, whole and in order: the sync positions, the timeslot rows, the voice stage's parameter bits and the PCM
of every talk path equal the reference of the stream run in one go - with calls that bring fewer records than the 720 the chain carries
(a group crosses three call boundaries, part of the old carry is carried again), new-record counts on 719 / 720 / 721, channels out of step
with each other, more channels than a wavefront holds, 24 kHz input, cf32 input, too few group slots, and the flush edges."""
import ctypes as C

import numpy as np
import pytest

import chain_p25p2_stream as cs
import ddn
import p2capture
import p2seq

pytestmark = pytest.mark.gpu


def _upload(a):
    p = C.c_void_p()
    assert ddn.lib().ddn_device_alloc(a.nbytes, C.byref(p)) == 0
    assert ddn.lib().ddn_device_upload(p, a.ctypes.data, a.nbytes) == 0
    return p


def _collect(ch, B, filed, voc, tag):
    """what the last run() / flush() left, filed per channel and per talk path"""
    r = ch.results()
    G, cap = r.max_groups, r.voice_frames
    assert r.carry_symbols == cs.CARRY
    new = ch.fetch(r.d_new, np.int32, (B,))
    ng = ch.fetch(r.d_n_groups, np.int32, (B,))
    gp = ch.fetch(r.d_group_pos, np.int32, (B, G))
    dropped = ch.fetch(r.d_dropped_syncs, np.int32, (B,))
    info = ch.fetch(r.d_info, np.int32, (B, G, 4, 8))
    pay = ch.fetch(r.d_payload, np.uint8, (B, G, 4, 180))
    afr = ch.fetch(r.d_ambe_fr, np.uint8, (B, G, 4, 4, 4, 24))
    arel = ch.fetch(r.d_ambe_rel, np.uint8, (B, G, 4, 4, 4, 24))
    ess = ch.fetch(r.d_ess, np.uint8, (B, G, 4, 96))
    assert (ng >= 0).all() and (ng <= G).all(), (tag, ng, G)
    for c in range(B):
        n = int(ng[c])
        filed[c].add_call(new[c], n, gp[c], (info[c], pay[c], afr[c], arel[c], ess[c]), dropped[c])
        # the slots no group was filed in stay empty
        assert (info[c, n:, :, 4] == 0).all() and not pay[c, n:].any() and not afr[c, n:].any() and not arel[c, n:].any() and not ess[c, n:].any(), (tag, c)
    if not voc:
        return G
    vsrc = ch.fetch(r.d_voice_src, np.int32, (2 * B, cap))
    vcnt = ch.fetch(r.d_voice_count, np.int32, (2 * B,))
    vbits = ch.fetch(r.d_voice_bits, np.uint8, (2 * B, cap, 49))
    pcm = ch.fetch(r.d_pcm, np.float32, (2 * B, cap, 160))
    assert (vcnt >= 0).all() and (vcnt <= cap).all(), (tag, vcnt, cap)
    for tp in range(2 * B):
        c, slot = tp >> 1, tp & 1
        # air order: the 4V / 2V timeslots the sequencing filed under this slot
        want_src = [((c * G + g) * 4 + ts) * 4 + f for g in range(int(ng[c])) for ts in range(4)
                    if info[c, g, ts, 3] == slot and info[c, g, ts, 4] in (p2seq.A_4V, p2seq.A_2V)
                    for f in range(4 if info[c, g, ts, 4] == p2seq.A_4V else 2)]
        k = int(vcnt[tp])
        assert k == len(want_src) and vsrc[tp, :k].tolist() == want_src and (vsrc[tp, k:] == -1).all(), (tag, tp)
        filed[c].add_voice(slot, vbits[tp, :k], pcm[tp, :k])
    return G


def _drive(seeds, iq, n_call, voc, tag, **kw):
    """iq [B][n_total][2] (cu8, or float32 with input_format=ddn.IN_CF32) through a chain in calls of n_call samples, then flush"""
    B = len(seeds)
    assert iq.shape[0] == B and iq.shape[1] % n_call == 0
    ch = ddn.P25P2ChainC(seeds, n_call, vocoder=voc, **kw)
    filed = [cs.Filed() for _ in range(B)]
    try:
        for k in range(iq.shape[1] // n_call):
            d = _upload(np.ascontiguousarray(iq[:, k * n_call:(k + 1) * n_call]))
            try:
                ch.run(d)
                G = _collect(ch, B, filed, voc, (tag, k))
            finally:
                ddn.lib().ddn_device_free(d)
        ch.flush()
        G = _collect(ch, B, filed, voc, (tag, "flush"))
        # what was flushed is not decoded again: a second flush files nothing and counts nothing
        ch.flush()
        r = ch.results()
        assert not ch.fetch(r.d_n_groups, np.int32, (B,)).any() and not ch.fetch(r.d_new, np.int32, (B,)).any(), tag
        assert ch.fetch(r.d_dropped_syncs, np.int32, (B,)).tolist() == [f.dropped[-1] for f in filed], tag
    finally:
        ch.close()
    return filed, G


@pytest.mark.parametrize("n_call", cs.CAPTURE_CALLS)
def test_capture_at_short_calls(built, n_call):
    """the reference's own Phase 2 capture as three channels, two with its site and one without"""
    iq, ws = cs.capture_case(n_call)
    _, no_site = cs.capture_case(n_call, site=False)
    seed = cs.seed44((p2capture.WACN, p2capture.SYSID, p2capture.NAC))
    filed, G = _drive([seed, seed, 0], np.broadcast_to(iq, (3,) + iq.shape), n_call, 0, n_call)
    assert G == n_call * 6000 // 48000 // 720 + 3
    for c, want in enumerate((ws, ws, no_site)):
        cs.check_filed(filed[c], want, (n_call, c), voice=False)
    i0, i2 = filed[0].got()[0][0], filed[2].got()[0][0]
    sacch = i0[:, :, 4] == p2seq.A_SACCH_S
    assert sacch.sum() >= 8 and (i2[:, :, 4][sacch] == p2seq.A_NOSITE).all()


@pytest.mark.parametrize("sps,rate,n_call", cs.VOICE_CALLS)
def test_synthetic_voice_at_short_calls(built, sps, rate, n_call):
    """two channels of two sites, the second lagging the first, to PCM - at 48 kHz and at 24 kHz (sample_rate_hz)"""
    iq, planted, refs, seeds = cs.voice_case(sps, rate, n_call)
    filed, G = _drive(seeds, iq, n_call, 1, (sps, n_call), sample_rate_hz=0 if rate == 48000 else rate)
    assert G == n_call * 6000 // rate // 720 + 3
    for c in range(2):
        cs.check_filed(filed[c], refs[c], (sps, n_call, c), planted=planted[c])


def test_cf32_input_equals_the_cu8_reference(built):
    """the same samples widened on the host: everything equals the cu8 run's reference"""
    sps, rate, n_call = cs.VOICE_CALLS[0]
    iq, planted, refs, seeds = cs.voice_case(sps, rate, n_call)
    filed, _ = _drive(seeds, cs.widen(iq), n_call, 1, "cf32", input_format=ddn.IN_CF32)
    for c in range(2):
        cs.check_filed(filed[c], refs[c], ("cf32", c), planted=planted[c])


def test_wide_and_ragged_channels(built):
    """67 channels, every one lagging its neighbour: new-record counts, sync positions and group counts of a call differ across channels
    and across the 64-lane edge.  Positions, rows and parameter bits on every channel, PCM on five of them"""
    iq, planted, refs, seeds = cs.wide_case()
    filed, G = _drive(seeds, iq, cs.WIDE_CALL, 1, "wide")
    assert G == 3
    clean = cs.wide_clean()
    for c in range(cs.WIDE_B):
        cs.check_filed(filed[c], refs[c], ("wide", c), pcm=c in cs.WIDE_PCM, planted=planted[c] if c in clean else None)


def test_too_few_group_slots(built):
    """max_groups = 1 at one-second calls: every call files its first sync only and counts the others; the sequencing state sees only what
    was filed"""
    n_call = 48000
    iq, ws = cs.capture_case(n_call)
    site = (p2capture.WACN, p2capture.SYSID, p2capture.NAC)
    filed, G = _drive([cs.seed44(site), 0], np.broadcast_to(iq, (2,) + iq.shape), n_call, 0, "slots", max_groups=1)
    assert G == 1
    kept, lost, dropped = [], 0, []
    for lo, hi in cs.scan_ranges(ws["new"]):
        here = [k for k, p in enumerate(ws["pos"]) if lo <= p < hi]
        kept += here[:1]
        lost += max(len(here) - 1, 0)
        dropped.append(lost)
    assert len(kept) >= 2 and lost >= 8, (kept, lost)
    for c, wsn in enumerate((site, (0, 0, 0))):
        f = filed[c]
        assert f.new == ws["new"].tolist() + [0]
        assert f.dropped == dropped, (c, f.dropped, dropped)
        assert f.pos == [ws["pos"][k] for k in kept], (c, f.pos)
        want = p2seq.run_groups(ws["bits"][kept], ws["llr"][kept], *wsn, p2seq.new_state())
        cs.compare(f.got(), want, 0)


def test_flush_edges(built):
    iq, ws = cs.capture_case(1999)
    ch = ddn.P25P2ChainC([1, 2, 3], 1999, vocoder=1)
    try:
        ch.flush()                                        # before any run: nothing to do, and still nothing to read
        with pytest.raises(ddn.DdnError):
            ch.results()
        # a stream shorter than the carry: the flush holds no whole group
        d = _upload(np.ascontiguousarray(np.broadcast_to(iq[:1999], (3, 1999, 2))))
        try:
            ch.run(d)
        finally:
            ddn.lib().ddn_device_free(d)
        r = ch.results()
        assert ch.fetch(r.d_new, np.int32, (3,)).tolist() == [int(ws["new"][0])] * 3
        for again in range(2):                            # and a second flush decodes nothing again
            ch.flush()
            r = ch.results()
            assert ch.fetch(r.d_n_groups, np.int32, (3,)).tolist() == [0, 0, 0], again
            assert ch.fetch(r.d_new, np.int32, (3,)).tolist() == [0, 0, 0]
            assert ch.fetch(r.d_dropped_syncs, np.int32, (3,)).tolist() == [0, 0, 0]
            assert ch.fetch(r.d_voice_count, np.int32, (6,)).tolist() == [0] * 6
    finally:
        ch.close()


def test_second_flush_decodes_nothing_again(built):
    """cut after FLUSH_CUT calls the first channel's carry holds a whole group behind a sync among its first 20 records and the second
    channel's does not: the flush files that one group, a second flush right after it none, and counts no sync as dropped"""
    sps, rate, n_call = cs.VOICE_CALLS[0]
    iq, planted, refs, seeds = cs.voice_case(sps, rate, n_call)
    total = int(refs[0]["new"][:cs.FLUSH_CUT].sum())
    want = [p for p in refs[0]["pos"] if total - cs.CARRY <= p < total - cs.CARRY + cs.FLUSH_SCAN]
    ch = ddn.P25P2ChainC(seeds, n_call, vocoder=1)
    try:
        for k in range(cs.FLUSH_CUT):
            d = _upload(np.ascontiguousarray(iq[:, k * n_call:(k + 1) * n_call]))
            try:
                ch.run(d)
            finally:
                ddn.lib().ddn_device_free(d)
        ch.flush()
        r = ch.results()
        assert ch.fetch(r.d_n_groups, np.int32, (2,)).tolist() == [1, 0]
        assert [total - cs.CARRY + int(ch.fetch(r.d_group_pos, np.int32, (2, r.max_groups))[0, 0])] == want
        assert ch.fetch(r.d_voice_count, np.int32, (4,)).sum() > 0
        ch.flush()
        r = ch.results()
        assert ch.fetch(r.d_n_groups, np.int32, (2,)).tolist() == [0, 0]
        assert ch.fetch(r.d_dropped_syncs, np.int32, (2,)).tolist() == [0, 0]
        assert ch.fetch(r.d_voice_count, np.int32, (4,)).tolist() == [0] * 4
        assert not ch.fetch(r.d_payload, np.uint8, (2, r.max_groups, 4, 180)).any()
    finally:
        ch.close()
