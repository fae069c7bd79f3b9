"""Long P25 data units across calls (ddn_p25_chain_set_long_data_units, include/ddn_chain.h): a unit that announces more than
pdu_blocks data blocks is decoded block by block in the calls whose records complete it and reported once, whole, in the call that
brings its last block - against the whole-stream restatement (tests/long_pdu.py) and the data the generator sent.  The switch
changes no existing output."""
import ctypes as C

import numpy as np
import pytest

import chain_stream
import ddn
import long_pdu
import mbe
import orc
import p25gen

pytestmark = pytest.mark.gpu

NAC = 0x293


def _upload(a):
    p = C.c_void_p()
    assert ddn.lib().ddn_device_alloc(a.nbytes, C.byref(p)) == 0
    assert ddn.lib().ddn_device_upload(p, a.ctypes.data, a.nbytes) == 0
    return p


def _dibits(rng, plan, gap=200):
    """plan items: dict -> make_pdu_coded(**dict) (sent), "tsdu" / "voice" / "short" -> a frame of that kind; returns (dibits, sent)"""
    parts = [p25gen.make_frames(rng, 1, NAC, crc=True, blocks=1)[0], np.zeros(160, np.int8)]      # (the slicer settles on this one)
    sent = []
    for kw in plan:
        if kw == "tsdu":
            parts.append(p25gen.make_frames(rng, 1, NAC, crc=True, blocks=int(rng.integers(1, 4)))[0])
        elif kw == "voice":
            bits = mbe.random_imbe_bits(rng, (18,))
            parts.append(p25gen.make_ldus(rng, 2, NAC, np.stack([mbe.imbe_encode(b) for b in bits]))[0])
        elif kw == "short":
            parts.append(p25gen.make_pdu_coded(rng, NAC, blks=int(rng.integers(1, 9)))[0])
        else:
            fr, hdr, data = p25gen.make_pdu_coded(rng, NAC, **kw)
            sent.append((kw, hdr, data))
            parts.append(fr)
        parts.append(np.zeros(gap, np.int8))
    return np.concatenate(parts), sent


def _run(iq, n_call, how="run", max_blocks=127, per_channel=0, modulation=0):
    """calls (+ flush) of a chain with the switch on -> (long units [channel]{sync record: unit}, Collector, d_n per call)"""
    B, n_total = iq.shape[0], iq.shape[1]
    ch = ddn.P25ChainC(B, n_call, modulation=modulation)
    if max_blocks:
        ch.set_long_data_units(max_blocks, per_channel)
    col = chain_stream.Collector(ch) if modulation == 0 else None
    got = [dict() for _ in range(B)]
    ns = []
    for a in range(0, n_total, n_call):
        d = _upload(np.ascontiguousarray(iq[:, a:a + n_call]))
        if how == "run":
            ch.run(d)
        else:
            ch.run_pipelined(d)
        ch.wait()
        ddn.lib().ddn_device_free(d)
        if col:
            col.take()
        ns.append(long_pdu.collect(ch, got))
    ch.flush()
    if col:
        col.take()
    ns.append(long_pdu.collect(ch, got))
    ch.close()
    return got, col, np.array(ns)


def _known_answer(units, sent):
    """the device's units (air order) against what make_pdu_coded sent: header, blocks, CRC9 and CRC32 verdicts"""
    assert len(units) == len(sent), (sorted(units), [s[0] for s in sent])
    for (a, u), (kw, hdr, data) in zip(sorted(units.items()), sent):
        nb = kw["blks"]
        conf = kw.get("confirmed", False)
        assert np.array_equal(u["header"], hdr), (a, kw)
        good32 = 1 if kw.get("good_crc32", True) else 0
        assert tuple(u["info"][:3]) == (nb + 1, nb, 4 if conf else 0) and u["info"][3] in ((good32, 0) if conf else (good32,)), (a, kw, u["info"])
        assert u["valid"][:nb].all() and not u["valid"][nb:].any(), (a, kw)
        if conf:
            # (rate 3/4 has little margin: in a long unit a block the restatement misses as well may fail its CRC9 - then its
            # unit's CRC32 fails too; every block with a good CRC9 is the one sent)
            bad = set(kw.get("bad_crc9_at", ()))
            miss = [b for b in range(nb) if b not in bad and not u["crc9"][b]]
            assert all(u["crc9"][b] == 0 for b in bad) and len(miss) <= 2, (a, kw, miss)
            assert all(np.array_equal(u["blocks18"][b], data[b]) for b in range(nb) if b not in bad and b not in miss), (a, kw)
            assert not miss or u["info"][3] == 0, (a, kw, miss)
        else:
            assert np.array_equal(u["blocks"][:nb], data), (a, kw)


def _three_channels(n_total):
    rng = np.random.default_rng(21)
    plan0 = [dict(blks=9), "short", dict(blks=12), "tsdu", dict(blks=20, good_crc32=False), "short", dict(blks=40), "voice",
             dict(blks=127), "tsdu"]
    plan1 = [dict(blks=9, confirmed=True), "short", dict(blks=20, confirmed=True, bad_crc9_at=(3,)), "tsdu",
             dict(blks=40, confirmed=True, good_crc32=False), "short", dict(blks=20, sap=61), "tsdu", "tsdu"]
    plan2 = ["voice", "tsdu", "voice", "tsdu", "tsdu", "voice", "tsdu"] * 3
    out, sent = [], []
    for c, plan in enumerate((plan0, plan1, plan2)):
        dib, s = _dibits(rng, plan)
        assert len(dib) * 10 + 3000 < n_total
        out.append(p25gen.modulate_cu8(dib, n_total, lead=260 + 97 * c, seed=c, noise=0.02))
        sent.append([x for x in s if x[0].get("sap", 0) != 61])
    return np.stack(out), sent


@pytest.mark.parametrize("n_call", [9000, 48000])
def test_long_units_decode_whole_across_calls(built, n_call):
    n_total = 288000
    iq, sent = _three_channels(n_total)
    got, col, _ = _run(iq, n_call)
    for c in range(3):
        want = chain_stream.run_stream(iq[c], n_call, seed=c, vocoder=False)
        # the records themselves, bit for bit (the loop's long in-frame runs)
        col.voice[c] = []
        chain_stream.check_channel(col, c, dict(want, voice=[]))
        exp = long_pdu.expected_units(want)
        long_pdu.assert_same(got[c], exp, ("channel", c))
        _known_answer(got[c], sent[c])
    assert len(got[2]) == 0 and len(got[0]) == 5 and len(got[1]) == 3


def test_back_to_back_units_and_per_channel_limit(built):
    rng = np.random.default_rng(8)
    dib, sent = _dibits(rng, [dict(blks=9) for _ in range(12)], gap=0)
    n_call = 48000
    iq = p25gen.modulate_cu8(dib, 4 * n_call, lead=260, seed=4, noise=0.02)[None]
    got, _, ns = _run(iq, n_call, per_channel=1)
    exp = long_pdu.expected_units(chain_stream.run_stream(iq[0], n_call, seed=0, vocoder=False))
    assert len(exp) == 12 and int(ns.sum()) == 12 and ns.max() >= 3, ns.ravel()
    # only the first unit of each call is filed
    assert len(got[0]) == int((ns > 0).sum())
    for a, u in got[0].items():
        long_pdu.assert_same({a: u}, {a: exp[a]})
    full, _, ns2 = _run(iq, n_call)
    assert np.array_equal(ns, ns2)
    _known_answer(full[0], sent)


def test_flush_inside_a_unit(built):
    rng = np.random.default_rng(9)
    dib, sent = _dibits(rng, ["tsdu", dict(blks=9), dict(blks=40)])
    n_call = 9000
    # the stream ends about half way through the 40-block unit (4212 dibits, then the 200-dibit gap), on a call boundary
    cut = (len(dib) - 200 - 2106 + 260) * 10 // n_call * n_call
    iq = p25gen.modulate_cu8(dib, len(dib) * 10 + 3000, lead=260, seed=5, noise=0.02)[None, :cut]
    got, _, _ = _run(iq, n_call)
    exp = long_pdu.expected_units(chain_stream.run_stream(iq[0], n_call, seed=0, vocoder=False))
    long_pdu.assert_same(got[0], exp)
    (a9, u9), (a40, u40) = sorted(got[0].items())
    assert tuple(u9["info"]) == (10, 9, 0, 1)
    nd = int(u40["info"][1])
    assert 5 < nd < 40 and tuple(u40["info"]) == (41, nd, 8, 0), u40["info"]
    assert u40["valid"][:nd].all() and not u40["valid"][nd:].any()
    assert np.array_equal(u40["blocks"][:nd], sent[1][2][:nd])


def _snapshot(ch):
    """every array of ddn_p25_chain_results of the last call, as bytes"""
    r = ch.results()
    B, S, V, st, E = ch.B, ch.B * ch.F, ch.B * ch.Fv * 9, ch.stride, ch.E
    NE, NB = B * r.pdu_per_channel, B * r.pdu_per_channel * r.pdu_blocks
    sizes = dict(d_records10=B * st * 10, d_flags=B * st, d_counts=4 * B, d_new=4 * B, d_events=16 * B * E, d_n_events=4 * B,
                 d_event_data=16 * B * E, d_n_syncs=4 * B, d_dropped_syncs=4 * B, d_sync_pos=4 * S, d_nid4=16 * S, d_tsbk=36 * S,
                 d_tsbk_crc=3 * S, d_lsd_bits=32 * S, d_lsd_ok=2 * S, d_hdu_rs_data=120 * S, d_hdu_rs_status=S, d_tdulc_rs_data=72 * S,
                 d_tdulc_rs_status=S, d_n_pdu=4 * B, d_pdu_slot=4 * NE, d_pdu_header=12 * NE, d_pdu_info=16 * NE, d_pdu_blocks=12 * NB,
                 d_pdu_block_valid=NB, d_pdu_blocks18=18 * NB, d_pdu_crc9_ok=NB, d_n_ldu=4 * B, d_imbe_bits=88 * V, d_imbe_result=20 * V,
                 d_pcm=640 * V, d_synth_result=20 * V)
    out = {k: ch.fetch(getattr(r, k), np.uint8, (n,)) for k, n in sizes.items()}
    for i, (w, d, s) in enumerate(((240, 72, 1), (240, 96, 1))):
        out["words%d" % i] = ch.fetch(r.d_ldu_words[i], np.uint8, (w * S,))
        out["rs%d" % i] = ch.fetch(r.d_ldu_rs_data[i], np.uint8, (d * S,))
        out["rss%d" % i] = ch.fetch(r.d_ldu_rs_status[i], np.uint8, (s * S,))
    out["_dims"] = np.array([r.stride_symbols, r.pdu_per_channel, r.pdu_blocks])
    # (the framer's sync slots beyond a channel's count are scratch, never written: compared up to the count)
    ns = np.minimum(out["d_n_syncs"].view(np.int32), ch.F)
    pos = out["d_sync_pos"].view(np.int32).reshape(B, ch.F)
    out["d_sync_pos"] = np.concatenate([pos[c, :ns[c]] for c in range(B)])
    return out


@pytest.mark.parametrize("how", ["run", "pipelined"])
def test_switch_changes_no_existing_output(built, how):
    rng = np.random.default_rng(13)
    n_call, calls = 24000, 5
    plan = [dict(blks=20), "voice", "tsdu", "short", dict(blks=9, confirmed=True), "voice", "short", dict(blks=12), "tsdu"]
    iq = np.stack([p25gen.modulate_cu8(_dibits(rng, plan)[0], n_call * calls, lead=260 + 53 * c, seed=c, noise=0.03) for c in range(2)])
    chs = [ddn.P25ChainC(2, n_call), ddn.P25ChainC(2, n_call)]
    chs[1].set_long_data_units(127, 0)
    seen = 0
    for k in range(calls + 1):
        snaps = []
        for ch in chs:
            if k < calls:
                d = _upload(np.ascontiguousarray(iq[:, k * n_call:(k + 1) * n_call]))
                if how == "run":
                    ch.run(d)
                else:
                    ch.run_pipelined(d)
                ch.wait()
                ddn.lib().ddn_device_free(d)
            else:
                ch.flush()
            snaps.append(_snapshot(ch))
        for name in snaps[0]:
            assert np.array_equal(snaps[0][name], snaps[1][name]), (k, name)
        seen += int(chs[1].fetch(chs[1].long_pdu_results().d_n, np.int32, (2,)).sum())
    assert seen >= 4, seen
    r = chs[0].long_pdu_results()
    assert r.max_blocks == 0 and not r.d_n
    for ch in chs:
        ch.close()


def test_cqpsk_long_units(built):
    rng = np.random.default_rng(17)
    dib, sent = _dibits(rng, [dict(blks=20), "tsdu", dict(blks=40), "tsdu"])
    n_call = 24000
    iq = orc.modulate_dqpsk_cu8(dib, 10, seed=2, noise=0.02, lead=400)
    n_total = -(-len(iq) // n_call) * n_call
    iq = np.concatenate([iq, np.full((n_total - len(iq), 2), 127, np.uint8)])
    got, _, _ = _run(np.stack([iq, iq]), n_call, how="pipelined", modulation=1)
    for c in range(2):
        _known_answer(got[c], sent)
    assert got[0].keys() == got[1].keys()


class _PartView:
    """a chain object the mixed chain owns (not destroyed here)"""

    def __init__(self, h, B):
        self.h, self.B = h, B

    def fetch(self, ptr, dtype, shape):
        a = np.zeros(shape, dtype)
        assert ddn.lib().ddn_device_download(a.ctypes.data, ptr, a.nbytes) == 0
        return a

    def long_pdu_results(self):
        r = ddn.P25LongPduResults()
        assert ddn.lib().ddn_p25_chain_get_long_pdu_results(self.h, C.byref(r)) == 0
        return r


def test_mixed_chain_part_matches_a_chain_of_its_own(built):
    n_call, calls = 48000, 3
    iq, sent = _three_channels(n_call * 6)
    iq = np.ascontiguousarray(iq[:2, :n_call * calls])
    m = ddn.MixedChainC(2, 1, 1, n_call)
    l = ddn.lib()
    h = l.ddn_mixed_chain_part(m.h, 0)
    assert l.ddn_p25_chain_set_long_data_units(h, 127, 0) == 0
    view = _PartView(h, 2)
    quiet = _upload(np.full((1, n_call, 2), 127, np.uint8))
    got = [dict(), dict()]
    for k in range(calls):
        d = _upload(np.ascontiguousarray(iq[:, k * n_call:(k + 1) * n_call]))
        m.run(d, quiet, quiet)
        m.wait()
        l.ddn_device_free(d)
        long_pdu.collect(view, got)
    assert l.ddn_p25_chain_flush(h) == 0
    long_pdu.collect(view, got)
    l.ddn_device_free(quiet)
    m.close()
    own, _, _ = _run(iq, n_call)
    for c in range(2):
        long_pdu.assert_same(got[c], own[c], ("channel", c))
    assert len(own[0]) >= 3 and len(own[1]) >= 1
