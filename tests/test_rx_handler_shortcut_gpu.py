"""The handler wave's short cut for clean trellis blocks and its early answer for a TSDU's third block (ddn_rx.hip serve(),
ddn_p25h_dev.h half_rate_hard_path_wave): records, flags, counts, events and event data of one workgroup (eight channels) equal the
oracle's (oracle/ddn_oracle_handlers.c) and equal the same run with both switched off (ddn_p25_rx_set_debug_flags, the sign bit).

Channels: clean TSDUs of one, two and three blocks in both polarities; blocks that are trellis paths with a failing CRC16 as first,
second and third block; one data dibit pushed across a decision threshold (first, last, beside a status symbol - block 2's last
symbol, index 100, is one); data-unit header blocks clean and with one bad dibit; noisy traffic whose seed and sigma were picked on
the CPU from the oracle's LLRs.  What the oracle's records say about every block (path or not, zero LLR or not) is asserted before
anything is compared, so traffic that exercises one side of the short cut only cannot pass.

A block whose status counter starts at 36 (a status symbol as its symbol 0) is not among the cases: the loops never decode one - a
TSDU's blocks start at 22, 15 and 8, a data unit's header block at 22 (serve(): sk0 = 36 - 14, then block_counter_after())."""
import functools
from collections import Counter

import numpy as np
import pytest

import orc
import shortcut_cases as sc

OFF = -2**31            # ddn_p25_rx_set_debug_flags: the sign bit = no short cut, no early answer
N = sc.N_SAMPLES
NOISE_SIGMA, NOISE_SEEDS = 2000.0, (1057, 1058, 1059)   # picked on the CPU: see test_traffic_exercises_both_sides_of_the_short_cut


def _oracle(x):
    rx = orc.OracleP25Rx(lock_symbols=-1, use_filter=1)
    sym, rec, fl = rx.run(x)
    rows, data = rx.events.rows(), rx.events.data()
    ev = [[e[0], e[1], e[2], (e[3] & 0xFFFF) | ((e[4] & 0xFFFF) << 16)] for e in rows]
    return dict(sym=sym, rec=rec, fl=fl, ev=np.array(ev, np.int64).reshape(-1, 4), evd=data, blocks=sc.oracle_blocks(rec, rows, data))


@functools.lru_cache(maxsize=None)
def _case():
    """-> (x f32 [8][N], oracle results per channel, hits of the two crossing channels); computed once, never written to"""
    cross_a, hit_a = sc.crossing_stream(3)
    cross_b, hit_b = sc.crossing_stream(4, pdu_too=True)
    clean = sc.clean_stream(1)
    rows = [clean.modulate(N, 80.0, 1), clean.modulate(N, 80.0, 2, invert=True), sc.bad_crc_stream(2).modulate(N, 80.0, 3),
            cross_a.modulate(N, 80.0, 4), cross_b.modulate(N, 80.0, 5, invert=True)]
    rows += [sc.noisy_stream(sd).modulate(N, NOISE_SIGMA, sd, invert=(k == 1)) for k, sd in enumerate(NOISE_SEEDS)]
    x = np.stack(rows)
    x.setflags(write=False)
    return x, [_oracle(x[c]) for c in range(len(rows))], (hit_a, hit_b)


def _assert_traffic(want, hits):
    """what the cases are there for, read off the oracle's own records and decisions"""
    for c in (0, 1):                                  # clean, both polarities: every block a path with a good CRC, all three block indices
        b = want[c]["blocks"]
        assert len(b) >= 20 and all(v["path"] and not v["zero"] and v["crc_ok"] and v["sel"] == 0 for v in b), c
        assert Counter(v["block"] for v in b)[2] >= 3 and Counter(v["block"] for v in b)[1] >= 6
    b = want[2]["blocks"]                             # paths with a bad CRC in every block index, the list decoder's answer kept
    assert sum(v["path"] and not v["zero"] for v in b) >= len(b) - 1      # (but the block the end of the call cuts short)
    bad = Counter(v["block"] for v in b if not v["crc_ok"])
    assert bad[0] >= 3 and bad[1] >= 3 and bad[2] >= 3 and sum(v["crc_ok"] for v in b) >= 6
    for c, hit, with_pdu in ((3, hits[0], False), (4, hits[1], True)):   # one dibit across a threshold: exactly those blocks are no paths
        b = want[c]["blocks"]
        n_tsdu_hits = sum(1 for _ in hit) - (2 if with_pdu else 0)
        assert Counter(v["block"] for v in b if v["kind"] == 2 and not v["path"]) == Counter(blk for _, blk in hit[:n_tsdu_hits]), c
        assert all(v["crc_ok"] for v in b)            # (the decoder proper repairs the one dibit)
        if with_pdu:
            hdr = [v for v in b if v["kind"] == 3]
            assert [v["path"] for v in hdr] == [True, True, True, False, False]
            ends = want[c]["ev"][want[c]["ev"][:, 1] == 3][:, 3] & 0xFFFF
            assert list(ends) == [1, 3, 5, 2, 4]      # blks + 1, read from the decoded header
    noisy = [v for c in (5, 6, 7) for v in want[c]["blocks"]]
    paths = sum(v["path"] for v in noisy)
    assert len(noisy) >= 60 and 0.2 * len(noisy) <= paths <= 0.8 * len(noisy), (len(noisy), paths)
    assert sum(v["path"] and v["zero"] for v in noisy) >= 3     # paths the short cut must leave to the decoder proper
    assert sum(v["path"] and not v["zero"] for v in noisy) >= 12


def test_traffic_exercises_both_sides_of_the_short_cut(built):
    x, want, hits = _case()
    _assert_traffic(want, hits)


def _check(rec, fl, cnt, events, n_events, event_data, c, w):
    k = int(cnt[c])
    assert k == len(w["sym"]), (c, k, len(w["sym"]))
    r4, sy = orc.unpack_records10(rec[c, :k])
    bad = np.flatnonzero(fl[c, :k] != w["fl"])
    assert bad.size == 0, (c, bad[:5])
    assert np.array_equal(sy.view(np.uint32), w["sym"].view(np.uint32)), c
    assert np.array_equal(r4, w["rec"]), c
    ne = int(n_events[c])
    mask = np.array([-1, -1, -1, 0xFFFFFFFF])
    got = events[c, :ne].astype(np.int64) & mask
    assert ne == len(w["ev"]) and np.array_equal(got, w["ev"] & mask), (c, got[:6], w["ev"][:6])
    bad = np.flatnonzero((event_data[c, :ne] != w["evd"]).any(axis=1))
    assert bad.size == 0, (c, bad[:4], event_data[c, bad[:2]], w["evd"][bad[:2]])


def _run(x, cpw, fil, dbg, splits=None):
    import ddn
    B = x.shape[0]
    rx = ddn.P25Rx(B, use_matched_filter=1, channels_per_wave=cpw, handlers=True, max_events=512, filter_in_loop=bool(fil), debug_flags=dbg)
    splits = splits or [0, x.shape[1]]
    recs, fls, evs, evds = [[[] for _ in range(B)] for _ in range(4)]
    base = np.zeros(B, np.int64)
    for a, b in zip(splits[:-1], splits[1:]):
        rec, fl, cnt = rx.run(x[:, a:b])
        for c in range(B):
            recs[c].append(rec[c, :cnt[c]])
            fls[c].append(fl[c, :cnt[c]])
            e = rx.events[c, :rx.n_events[c]].astype(np.int64)
            e[:, 0] += base[c]
            evs[c].append(e)
            evds[c].append(rx.event_data[c, :rx.n_events[c]])
            base[c] += cnt[c]
    return [(np.concatenate(recs[c]), np.concatenate(fls[c]), np.concatenate(evs[c]), np.concatenate(evds[c])) for c in range(B)]


def _compare(out, out_off, want):
    for c, (rec, fl, ev, evd) in enumerate(out):
        for a, b in zip(out[c], out_off[c]):          # the same run with the short cut and the early answer switched off
            assert np.array_equal(a, b), c
        _check(rec[None], fl[None], [len(rec)], ev[None], [len(ev)], evd[None], 0, want[c])


@pytest.mark.gpu
@pytest.mark.parametrize("cpw,fil", [(8, 0), (8, 1), (4, 0), (16, 0)])
def test_short_cut_and_early_answer_against_the_oracle_and_switched_off(built, cpw, fil):
    x, want, hits = _case()
    _assert_traffic(want, hits)
    _compare(_run(x, cpw, fil, 0), _run(x, cpw, fil, OFF), want)


@pytest.mark.gpu
def test_decision_phase_split_by_a_call_boundary(built):
    """a three-block TSDU whose second block straddles the call boundary: the history ring, the handler words and the status counter
    are carried, the third block's early answer comes in the second call"""
    x, want, hits = _case()
    clean = sc.clean_stream(1)
    three = [m for m in clean.marks if len(m) == 3]
    cuts = [230 + 10 * three[k][1][49] + 3 for k in (1, 2)]       # the middle of block 1 of the second and third such TSDU
    ev = want[0]["ev"]
    for cut in cuts:                                  # the boundary falls inside a phase that ends in a block-1 decision
        after = ev[ev[:, 0] >= cut // 10 - 30][0]
        assert after[1] == 2 and after[2] == 1 and 0 < after[0] - (cut // 10 - 30) < 101, (cut, after)
    splits = [0] + cuts + [N]
    _compare(_run(x, 8, 0, 0, splits), _run(x, 8, 0, OFF, splits), want)
