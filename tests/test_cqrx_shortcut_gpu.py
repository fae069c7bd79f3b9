"""The hard-path short cut ahead of the half-rate decoder in the CQPSK symbol-rate loop (ddn_cqrx.hip half_rate_select, ddn_p25h_dev.h
half_rate_hard_path_wave): records, flags and the handlers' events and payloads equal the oracle's (oracle/ddn_oracle_cqrx.c) and equal
the same run with the short cut switched off (ddn_cq_rx_set_debug_flags bit 1), across a call boundary inside a TSDU's second block.
Same cases as test_rx_handler_shortcut_gpu.py, as symbols: clean TSDUs of one to three blocks in both polarities, trellis paths
with a failing CRC16 in every block index, one data dibit across a decision threshold, data-unit header blocks, noisy traffic picked
on the CPU from the oracle's LLRs; what the oracle's records say about every block is asserted before anything is compared."""
import functools
from collections import Counter

import numpy as np
import pytest

import orc
import shortcut_cases as sc

LEVEL = np.array([1.0, 3.0, -1.0, -3.0])      # dibit -> symbol level (identity map)
NOISE_SIGMA, NOISE_SEEDS = 0.33, (3110, 3058, 3020)   # picked on the CPU: see test_traffic_exercises_both_sides_of_the_short_cut
LEAD = 40


def _symbols(stream, noise, seed, invert=False):
    rng = np.random.default_rng(seed)
    d = np.concatenate([rng.integers(0, 4, LEAD), stream.dib.astype(np.int64) & 3, rng.integers(0, 4, 30)])
    scale = np.concatenate([np.ones(LEAD), stream.scale, np.ones(30)])
    if invert:
        d = d ^ 2
    return (LEVEL[d] * scale + noise * rng.standard_normal(len(d))).astype(np.float32)


def _oracle(s):
    rx = orc.OracleCqRx(orc.CQ_P25P1, -1, -100.0)
    rec, fl = rx.run(s)
    rows, data = rx.events.rows(), rx.events.data()
    return dict(rec=rec, fl=fl, rows=rows, evd=data, blocks=sc.oracle_blocks(rec, rows, data))


@functools.lru_cache(maxsize=None)
def _case():
    cross_a, hit_a = sc.crossing_stream(3)
    cross_b, hit_b = sc.crossing_stream(4, pdu_too=True)
    clean = sc.clean_stream(1)
    streams = [_symbols(clean, 0.12, 1), _symbols(clean, 0.12, 2, invert=True), _symbols(sc.bad_crc_stream(2), 0.12, 3),
               _symbols(cross_a, 0.12, 4), _symbols(cross_b, 0.12, 5, invert=True)]
    streams += [_symbols(sc.noisy_stream(sd), NOISE_SIGMA, sd, invert=(k == 1)) for k, sd in enumerate(NOISE_SEEDS)]
    for s in streams:
        s.setflags(write=False)
    return streams, [_oracle(s) for s in streams], (hit_a, hit_b), clean


def _assert_traffic(want, hits):
    for c in (0, 1):
        b = want[c]["blocks"]
        assert len(b) >= 20 and all(v["path"] and not v["zero"] and v["crc_ok"] and v["sel"] == 0 for v in b), c
        assert Counter(v["block"] for v in b)[2] >= 3 and Counter(v["block"] for v in b)[1] >= 6
    b = want[2]["blocks"]
    assert sum(v["path"] and not v["zero"] for v in b) >= len(b) - 1
    bad = Counter(v["block"] for v in b if not v["crc_ok"])
    assert bad[0] >= 3 and bad[1] >= 3 and bad[2] >= 3 and sum(v["crc_ok"] for v in b) >= 6
    for c, hit, with_pdu in ((3, hits[0], False), (4, hits[1], True)):
        b = want[c]["blocks"]
        n_tsdu_hits = len(hit) - (2 if with_pdu else 0)
        assert Counter(v["block"] for v in b if v["kind"] == 2 and not v["path"]) == Counter(blk for _, blk in hit[:n_tsdu_hits]), c
        assert all(v["crc_ok"] for v in b)
        if with_pdu:
            assert [v["path"] for v in b if v["kind"] == 3] == [True, True, True, False, False]
            assert [r[3] & 0xFFFF for r in want[c]["rows"] if r[1] == 3] == [1, 3, 5, 2, 4]     # blks + 1, read from the decoded header
    noisy = [v for c in (5, 6, 7) for v in want[c]["blocks"]]
    paths = sum(v["path"] for v in noisy)
    assert len(noisy) >= 60 and 0.2 * len(noisy) <= paths <= 0.8 * len(noisy), (len(noisy), paths)
    assert sum(v["path"] and v["zero"] for v in noisy) >= 3     # paths the short cut must leave to the decoder proper
    assert sum(v["path"] and not v["zero"] for v in noisy) >= 12


def test_traffic_exercises_both_sides_of_the_short_cut(built):
    streams, want, hits, clean = _case()
    _assert_traffic(want, hits)


def _run(streams, cuts, dbg):
    """-> per channel (records, flags, events with stream-wide positions); cuts: per-channel call boundaries [B][k]"""
    import ddn
    B = len(streams)
    rx = ddn.CqRx(B, ddn.CQ_P25P1, 0, 0.0, debug_flags=dbg)
    recs, fls, evs = [[] for _ in range(B)], [[] for _ in range(B)], [[] for _ in range(B)]
    done = [0] * B
    for k in range(len(cuts[0]) + 1):
        upto = [cuts[c][k] if k < len(cuts[c]) else len(streams[c]) for c in range(B)]
        take = [u - d for u, d in zip(upto, done)]
        blk = np.zeros((B, max(take)), np.float32)
        for c in range(B):
            blk[c, :take[c]] = streams[c][done[c]:upto[c]]
        rec, fl, cnt, ev = rx.run(blk, take)
        for c in range(B):
            assert cnt[c] == take[c]
            recs[c].append(rec[c, :take[c]])
            fls[c].append(fl[c, :take[c]])
            evs[c] += [(p + done[c], kd, a, b, d4) for (p, kd, a, b, d4) in ev[c]]
        done = upto
    rx.close()
    return [(np.concatenate(recs[c]), np.concatenate(fls[c]), evs[c]) for c in range(B)]


def _check(got, s, w, tag):
    rec, fl, ev = got
    n = len(s)
    assert np.array_equal(fl[:n] & 0x7F, w["fl"]), (tag, np.flatnonzero((fl[:n] & 0x7F) != w["fl"])[:5])
    assert np.array_equal(rec[:n, 0:2].astype(np.int32), w["rec"][:, 0:2]), (tag, "dibit / reliability")
    assert np.array_equal(rec[:n, 2:6].copy().view(np.int16).reshape(n, 2).astype(np.int32), w["rec"][:, 2:4]), (tag, "llr")
    assert np.array_equal(rec[:n, 6:10].copy().view(np.uint32).reshape(-1), s.view(np.uint32)), (tag, "symbol")
    assert len(ev) == len(w["rows"]), (tag, len(ev), len(w["rows"]))
    for (pos, kind, a, b, d4), (wp, wk, wa, wb, wc), wd in zip(ev, w["rows"], w["evd"]):
        assert (pos, kind) == (wp, wk) and np.array_equal(d4, wd), (tag, pos, kind, wp, wk, d4, wd)
        if kind == 1:
            assert a == wa and (b & 0xFFFF) == (wb & 0xFFFF) and ((b >> 16) & 0xFF) == (wc & 0xFF), (tag, "nid")


@pytest.mark.gpu
def test_short_cut_against_the_oracle_and_switched_off(built):
    streams, want, hits, clean = _case()
    _assert_traffic(want, hits)
    # every channel in three calls; channel 0's boundaries fall in the middle of the second block of two three-block TSDUs
    three = [m for m in clean.marks if len(m) == 3]
    cuts = [[len(s) // 3 + 7 * c, 2 * len(s) // 3 + 5 * c] for c, s in enumerate(streams)]
    cuts[0] = [LEAD + three[k][1][49] for k in (1, 2)]
    blk1 = [v["pos"] for v in want[0]["blocks"] if v["block"] == 1]
    for cut in cuts[0]:
        assert any(0 < p - cut < 60 for p in blk1), (cut, blk1)
    on, off = _run(streams, cuts, 0), _run(streams, cuts, 1)
    for c, s in enumerate(streams):
        assert np.array_equal(on[c][0], off[c][0]) and np.array_equal(on[c][1], off[c][1]) and len(on[c][2]) == len(off[c][2]), c
        for e0, e1 in zip(on[c][2], off[c][2]):
            assert e0[:4] == e1[:4] and np.array_equal(e0[4], e1[4]), (c, e0, e1)
        _check(on[c], s, want[c], c)
