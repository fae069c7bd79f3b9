"""GPU: the handler rules (dsd-neo_amd/csrc/ddn_p25h_rules.h) that no other device test reaches, in both loops, one workgroup each,
against the oracle: records, flags, events and event data.  A NID with NAC 0 and one with NAC 0xFFF decode and are refused as the
carried NAC; that the carried pair stayed what it was shows in the frame after each - a "probe" whose NID has all twelve NAC bits
wrong, which p25p1_nid_decode only decodes by its retry with the observed NAC (oracle/ddn_oracle_block.c; alone, from a fresh
state, the probe fails).  The symbol-rate loop also: a probe after a carrier loss (the observed NAC is p2_cc), a data unit with a bad
header CRC, one under the SAP 61 cap, and a NID that spells an undefined DUID."""
import functools

import numpy as np
import pytest

import orc
import p25gen

NAC = 0x293


def _probe():
    fr = p25gen.make_tdu(NAC)
    fr[24:30] ^= 3                          # the NAC's six dibits (none of them the status symbol at 35)
    return fr


def _dibits(rng, cq):
    gap = lambda n=12: rng.integers(0, 4, n)
    parts = [p25gen.make_frames(rng, 1, NAC, crc=True, blocks=1)[0], gap(), p25gen.make_tdu(0x000), gap(), _probe(), gap(),
             p25gen.make_tdu(0xFFF), gap(), _probe(), gap()]
    if not cq:      # (the C4FM loop's slicer thresholds settle on a first frame)
        parts = [p25gen.make_frames(rng, 1, NAC, crc=True, blocks=2)[0], gap()] + parts
    if cq:
        parts += [gap(1900), _probe(), gap(), p25gen.make_pdu(rng, NAC, 3, good_crc=False), gap(), p25gen.make_pdu(rng, NAC, 12, sap=61),
                  gap(), p25gen.frame_with_duid(rng, NAC, 0x9, 40), gap()]
    return np.concatenate([np.asarray(p) & 3 for p in parts])


def _assert_nids(nids, cq):
    """nids: the oracle's NID events as (status, nac, effective duid) in order"""
    want = [(NAC, 7), (0x000, 3), (NAC, 3), (0xFFF, 3), (NAC, 3)] + ([(NAC, 3), (NAC, 12), (NAC, 12)] if cq else [])
    assert [(n, d) for s, n, d in nids[:len(want)]] == want and all(s > 0 for s, _, _ in nids[:len(want)]), nids
    if cq:
        assert nids[len(want)][0] <= 0 and nids[len(want)][2] == 0xFF, nids     # the undefined DUID: refused by the decoder


# ---- k_cq_rx ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cq_case():
    import test_cqrx_gpu as t
    streams = []
    for c in range(4):
        rng = np.random.default_rng(700 + c)
        streams.append(t.symbols_of(np.concatenate([rng.integers(0, 4, 40), _dibits(rng, True), rng.integers(0, 4, 40)]), rng, noise=0.15,
                                    invert=(c == 1)))
    return streams, [t.run_oracle(s, orc.CQ_P25P1) for s in streams]


def test_cq_traffic_reaches_the_rules():
    """on the CPU: what the oracle decodes in the streams below, and that the probe alone fails"""
    import test_cqrx_gpu as t
    streams, want = _cq_case()
    for rec, fl, ev in want:
        _assert_nids([(a, b & 0xFFF, c & 0xFF) for (pos, kind, a, b, c), d4 in ev if kind == 1], True)
        hdr = [(a, b) for (pos, kind, a, b, c), d4 in ev if kind == 3]
        assert hdr == [(0, 3), (1, 4)], hdr                 # bad header CRC: the default end stays; SAP 61 with 12 blocks: 4
    rng = np.random.default_rng(5)
    alone = t.run_oracle(t.symbols_of(np.concatenate([rng.integers(0, 4, 40), _probe() & 3, rng.integers(0, 4, 40)]), rng, noise=0.15), orc.CQ_P25P1)
    assert len(alone[2]) == 1 and alone[2][0][0][1] == 1 and alone[2][0][0][2] <= 0, alone[2]


@pytest.mark.gpu
def test_cq_rx_refused_nacs_carrier_loss_header_rules(built):
    import ddn
    import test_cqrx_gpu as t
    streams, want = _cq_case()
    rec, fl, ev = t.run_gpu_in_calls(streams, ddn.CQ_P25P1, cuts=(0.07, 0.5))      # (the first cut falls between the refused NAC and its probe)
    for c, s in enumerate(streams):
        t.check_channel(rec[c], fl[c], ev[c], s, want[c][0], want[c][1], want[c][2], c)
        for (pos, kind, a, b, d4), ((wp, wk, wa, wb, wc), wd) in zip(ev[c], want[c][2]):   # every word of every event
            assert (a, b & 0xFFFF, (b >> 16) & 0xFFFF) == (wa, wb & 0xFFFF, wc & 0xFFFF), (c, pos, kind)


# ---- k_p25_rxw ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _c4fm_case():
    import test_rx_handlers_gpu as t
    n = 10000
    x = np.zeros((8, n), np.float32)
    for c in range(8):
        s = p25gen.modulate_disc(_dibits(np.random.default_rng(800 + c), False), lead=200 + 13 * c, noise=80.0, seed=c)[:n]
        x[c, :len(s)] = s
    x[5] *= -1.0
    return x, [t._oracle(x[c], 1) for c in range(8)]


def test_c4fm_traffic_reaches_the_rules():
    x, want = _c4fm_case()
    for sym_o, rec_o, fl_o, ev_o, evd_o in want:
        _assert_nids([(int(e[2]), int(e[3]) & 0xFFF, (int(e[3]) >> 16) & 0xFF) for e in ev_o if e[1] == 1][1:], False)


@pytest.mark.gpu
@pytest.mark.parametrize("cpw", [4, 8])
def test_p25_rxw_refused_nacs(built, cpw):
    import ddn
    import test_rx_handlers_gpu as t
    x, want = _c4fm_case()
    rx = ddn.P25Rx(cpw, use_matched_filter=1, channels_per_wave=cpw, handlers=True, max_events=64)
    rec, fl, cnt = rx.run(x[:cpw])
    for c in range(cpw):
        t._check(rec, fl, cnt, rx.events, rx.n_events, c, want[c], rx.event_data)
