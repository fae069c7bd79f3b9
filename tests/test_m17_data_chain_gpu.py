"""M17 packet mode and BERT through the chain object (ddn_fsk4_chain, protocol M17): cu8 I/Q of streams (c) - the 33-frame packet -,
(g) - a cut packet, a gap either side of the carrier-loss count, a whole packet - and (h) - BERT - in one call, in three calls and in
calls of 1500 samples (150 symbols: shorter than the 256-symbol carry), each followed by the flush, against the whole-stream
restatement (tests/m17data.py) frame for frame; the LSF / LICH results of the same runs against m17.decode_stream as before."""
import ctypes as C

import numpy as np
import pytest

import chain_fsk4_stream as cs
import ddn
import m17data as md

pytestmark = pytest.mark.gpu

L = 72000                        # samples per channel: a multiple of 3 and of 1500, past the longest stream (c: 6960 symbols)
NAMES = ("c", "g1", "g4", "h")   # g1: the preamble matched on the 1800th hunted symbol (no carrier loss), g4: past it

_iq = {}


def _streams():
    if not _iq:
        g = md.golden_streams()
        import p25gen
        _iq["x"] = np.stack([p25gen.modulate_cu8(md.channel_dibits(g, (name,)), L, lead=20, seed=31 + k, noise=0.02) for k, name in enumerate(NAMES)])
    return _iq["x"]


def _run_chain(x, n, slots=None):
    """-> (units [B]: (absolute sync position, the M17 results + the data results of the slot), packets [B]: (call, absolute position of
    the EOF frame's sync, bytes [832], app_len, crc_ok), calls)"""
    B = x.shape[0]
    ch = ddn.Fsk4ChainC(B, n, ddn.FSK4_M17, rf_mod=0, handlers=0, vocoder=0)
    if slots:
        ch.set_m17_packet_slots(slots)
    units, packets = [[] for _ in range(B)], [[] for _ in range(B)]
    base = np.zeros(B, np.int64)
    calls = [0]

    def take():
        r, d = ch.results(), ch.m17_data_results()
        S, T, P = int(r.max_syncs), int(r.carry_symbols), int(d.max_packets)
        assert int(d.max_syncs) == S and P == (slots or 4)
        f = ch.fetch
        ns, pos, new = f(r.d_n_sync, np.int32, (B,)), f(r.d_sync_pos, np.int32, (B, S)), f(r.d_new, np.int32, (B,))
        u = dict(pat=f(r.d_sync_pat, np.uint8, (B, S)), thr=f(r.d_sync_thr5, np.float32, (B, S, 5)), lsf=f(r.d_m17_lsf30, np.uint8, (B, S, 30)),
                 lst=f(r.d_m17_lsf_status, np.uint8, (B, S)), cost=f(r.d_m17_lsf_cost, np.uint32, (B, S)), l6=f(r.d_m17_lich6, np.uint8, (B, S, 6)),
                 cnt=f(r.d_m17_lich_cnt, np.uint8, (B, S)), fp=f(r.d_m17_fn_payload18, np.uint8, (B, S, 18)), st=f(r.d_m17_str_status, np.uint8, (B, S)),
                 ll=f(r.d_m17_lich_lsf30, np.uint8, (B, S, 30)), lls=f(r.d_m17_lich_status, np.uint8, (B, S)),
                 p26=f(d.d_pkt26, np.uint8, (B, S, 26)), pf=f(d.d_pkt_frame_status, np.uint8, (B, S)), pc=f(d.d_pkt_cost, np.uint32, (B, S)),
                 b25=f(d.d_bits25, np.uint8, (B, S, 25)), bf=f(d.d_brt_frame_status, np.uint8, (B, S)), pst=f(d.d_pkt_status, np.uint8, (B, S)),
                 pcnt=f(d.d_pkt_count, np.uint8, (B, S)), bst=f(d.d_brt_state, np.int32, (B, S, 8)))
        npk, pk, plen = f(d.d_n_packets, np.int32, (B,)), f(d.d_packet, np.uint8, (B, P, 832)), f(d.d_packet_app_len, np.int32, (B, P))
        pok, pslot = f(d.d_packet_crc_ok, np.uint8, (B, P)), f(d.d_packet_slot, np.int32, (B, P))
        for c in range(B):
            for k in range(int(ns[c])):
                units[c].append((int(base[c]) + int(pos[c, k]) - T, {key: v[c, k] for key, v in u.items()}))
            assert int(npk[c]) <= P
            for j in range(int(npk[c])):
                packets[c].append((calls[0], int(base[c]) + int(pos[c, pslot[c, j]]) - T, pk[c, j].copy(), int(plen[c, j]), int(pok[c, j])))
            base[c] += int(new[c])
        calls[0] += 1

    info = {}
    cs.drive(ch, x, n, take, info)
    ch.close()
    cs.check_info(info)
    return units, packets, info


def _check_data(units_c, packets_c, want, n, new):
    out, fr, pk = want
    total = len(out["sym"])
    assert [p for p, _ in units_c] == [f["pos"] for f in fr]
    n_pkt = n_brt = 0
    for (p, g), f in zip(units_c, fr):
        if f["kind"] == "pkt":
            assert g["pf"] == 1 and np.array_equal(g["p26"], f["pkt26"]) and int(g["pc"]) == f["cost"], p
            n_pkt += 1
        else:
            assert g["pf"] == 0, (p, f["kind"])
        if f["kind"] == "brt":
            assert g["bf"] == 1 and np.array_equal(g["b25"], f["bits25"]), p
            n_brt += 1
        else:
            assert g["bf"] == 0, (p, f["kind"])
        assert (int(g["pst"]), int(g["pcnt"])) == (f["pkt_status"], f["pkt_count"] if f["kind"] == "pkt" else 0), (p, f["kind"])
        if f["kind"] == "brt":                       # (the receiver's fields are written behind BERT frames)
            assert g["bst"].tolist() == f["brt_state"], p
    assert len(packets_c) == len(pk)
    ends = np.cumsum(new)                         # symbols of the stream the chain held after each call
    for (call, p, by, app, ok), q in zip(packets_c, pk):
        end = len(q["bytes"])
        assert p == fr[q["sync"]]["pos"] and np.array_equal(by[:end], q["bytes"]) and not by[end:].any()
        assert (app, ok) == (q["app_len"], q["crc_ok"])
        # completed in the call that holds the frame's last symbol: a sync is handed out once the carry behind it is in the row
        first = int(np.searchsorted(ends, p + 1 + 256, side="left"))
        assert call == min(first, len(new) - 1), (call, first, p)
    return n_pkt, n_brt


@pytest.mark.parametrize("n", [L, L // 3, 1500])
def test_streams_through_the_chain_object(built, n):
    x = _streams()
    units, packets, info = _run_chain(x, n)
    g = md.golden_streams()
    tot = np.zeros(2, np.int64)
    for c, name in enumerate(NAMES):
        w = rx4_want(x[c], n)
        lsfs = cs.m17_check_chain_channel([(p, u) for p, u in units[c]], (w[0], w[1]))     # LSF, stream frames, LICH: unchanged
        tot += _check_data(units[c], packets[c], w, n, info["new"][:, c])
    assert tot[0] >= 33 + 2 * 5 and tot[1] >= 6, tot
    big = [q for q in packets[0] if q[4] == 1 and q[3] == 823]
    assert len(big) == 1 and np.array_equal(big[0][2][:825], g["sent_c_0"])               # the 823 sent bytes (+ CRC)
    assert [q[4] for q in packets[1]] == [0] and [q[4] for q in packets[2]] == [1]        # g1: the count stood; g4: carrier loss, good
    assert np.array_equal(packets[2][0][2][:62], g["sent_g4_0"])


_w = {}


def rx4_want(xc, n):
    import rx4
    key = (xc.ctypes.data, n)
    if key not in _w:
        disc = cs.front_end_disc(xc, n, 2)
        out = rx4.OracleFsk4Rx(rx4.profile(rx4.PROTO_M17)).run(disc, max_sync=4096)
        _w[key] = (out,) + md.decode_stream_data(out)
    return _w[key]


def test_packet_slots_and_the_getter_know_their_chain(built):
    """1 .. 33 slots before the first run, DDN_EINVAL otherwise; the getter refuses any other protocol; one slot stores the first
    packet of a call and counts the rest"""
    l = ddn.lib()
    ch = ddn.Fsk4ChainC(1, 4800, ddn.FSK4_DMR, rf_mod=2, handlers=0, vocoder=0)
    assert l.ddn_fsk4_chain_get_m17_data_results(ch.h, C.byref(ddn.M17DataChainResults())) == -1 and b"M17" in l.ddn_last_error()
    assert l.ddn_fsk4_chain_set_m17_packet_slots(ch.h, 4) == -1
    ch.close()
    ch = ddn.Fsk4ChainC(1, 4800, ddn.FSK4_M17, rf_mod=0, handlers=0, vocoder=0)
    for bad in (0, -1, 34, 1 << 20):
        assert l.ddn_fsk4_chain_set_m17_packet_slots(ch.h, bad) == -1 and b"1 .. 33" in l.ddn_last_error()
    for good in (1, 33, 2):
        assert l.ddn_fsk4_chain_set_m17_packet_slots(ch.h, good) == 0
    assert ch.m17_data_results().max_packets == 2
    p = cs.upload(l, np.full((1, 4800, 2), 127, np.uint8))
    ch.run(p)
    assert l.ddn_fsk4_chain_set_m17_packet_slots(ch.h, 4) == -1                          # it has run
    l.ddn_device_free(p)
    ch.close()
