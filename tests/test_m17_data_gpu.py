"""M17 packet and BERT frames on the device behind the device loop: ddn_m17_pkt_decode_batch, ddn_m17_brt_decode_batch and
ddn_m17_data_assemble_batch against the restatement (tests/m17data.py) on the oracle loop's output, slot for slot, on the streams of
tests/golden/m17_data_streams.npz (built with the reference's encoder; what they hold is asserted in tests/test_m17_data.py)."""
import ctypes as C

import numpy as np
import pytest

import ddn
import m17data as md

pytestmark = pytest.mark.gpu


def _data_calls(g, B, P, advance=None):
    """the three batch calls on one loop call's device outputs -> numpy arrays"""
    import torch
    l = ddn.lib()
    my = g["my"]
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    p = lambda t: t.data_ptr()
    o = dict(p26=z((B, my, 26), torch.uint8), pf=z((B, my), torch.uint8), pc=z((B, my), torch.int32), b25=z((B, my, 25), torch.uint8),
             bf=z((B, my), torch.uint8), state=z((B, l.ddn_m17_data_state_bytes()), torch.uint8), pst=z((B, my), torch.uint8),
             pcnt=z((B, my), torch.uint8), bst=z((B, my, 8), torch.int32), packet=z((B, P, 832), torch.uint8), plen=z((B, P), torch.int32),
             pok=z((B, P), torch.uint8), pslot=z((B, P), torch.int32), np_=z((B,), torch.int32))
    assert l.ddn_m17_pkt_decode_batch(p(g["rec"]), g["ms"], p(g["cnt"]), p(g["spos"]), p(g["spat"]), p(g["ns"]), p(g["thr"]), B, my, p(o["p26"]),
                                      p(o["pf"]), p(o["pc"]), None) == 0, l.ddn_last_error()
    assert l.ddn_m17_brt_decode_batch(p(g["rec"]), g["ms"], p(g["cnt"]), p(g["spos"]), p(g["spat"]), p(g["ns"]), B, my, p(o["b25"]), p(o["bf"]),
                                      None) == 0, l.ddn_last_error()
    assert l.ddn_m17_data_assemble_batch(p(g["spat"]), p(g["spos"]), p(g["ns"]), advance, B, my, p(o["p26"]), p(o["pf"]), p(o["b25"]), p(o["bf"]),
                                         p(o["state"]), p(o["pst"]), p(o["pcnt"]), p(o["bst"]), p(o["packet"]), p(o["plen"]), p(o["pok"]),
                                         p(o["pslot"]), p(o["np_"]), P, None) == 0, l.ddn_last_error()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _check_channel(o, c, want, ns, P):
    """channel c of the device arrays = the restatement; -> (packet frames, BERT frames, completed packets) compared"""
    out, fr, pk = want
    assert ns == len(fr)
    n_pkt = n_brt = 0
    for k, f in enumerate(fr):
        if f["kind"] == "pkt":
            assert o["pf"][c, k] == 1 and np.array_equal(o["p26"][c, k], f["pkt26"]), (c, k)
            assert int(o["pc"][c, k].view(np.uint32)) == f["cost"], (c, k)
            n_pkt += 1
        else:
            assert o["pf"][c, k] == 0, (c, k)
        if f["kind"] == "brt":
            assert o["bf"][c, k] == 1 and np.array_equal(o["b25"][c, k], f["bits25"]), (c, k)
            n_brt += 1
        else:
            assert o["bf"][c, k] == 0, (c, k)
        assert int(o["pst"][c, k]) == f["pkt_status"] and int(o["pcnt"][c, k]) == (f["pkt_count"] if f["kind"] == "pkt" else 0), (c, k, f["kind"])
        if f["kind"] == "brt":                       # (the receiver's fields are written behind BERT frames)
            assert o["bst"][c, k].tolist() == f["brt_state"], (c, k)
    assert int(o["np_"][c]) == len(pk)
    for j, q in enumerate(pk[:P]):
        end = len(q["bytes"])
        assert np.array_equal(o["packet"][c, j, :end], q["bytes"]) and not o["packet"][c, j, end:].any(), (c, j)
        assert (int(o["plen"][c, j]), int(o["pok"][c, j]), int(o["pslot"][c, j])) == (q["app_len"], q["crc_ok"], q["sync"]), (c, j)
    return n_pkt, n_brt, len(pk)


@pytest.mark.parametrize("B", [3, 67])
def test_packet_and_bert_frames_equal_the_restatement(built, B):
    """B = 3: the three test channels; B = 67 (past one block of the per-channel walk): the same round and round, a sample later each
    round.  The loop on the device, then the three calls: chunk bytes, statuses, counts, path costs, BERT bits, all eight receiver
    fields, the completed packets with length and verdict"""
    from test_m17_gpu import _device_loop
    x, plan = md.batch(B)
    g = _device_loop(x)
    P = 8
    o = _data_calls(g, B, P)
    ns = g["ns"].cpu().numpy()
    spos = g["spos"].cpu().numpy()
    tot = np.zeros(3, np.int64)
    for c, (base, roll) in enumerate(plan):
        want = md.channel_want(base, roll, max_sync=g["my"])
        assert np.array_equal(spos[c, :ns[c]], want[0]["sync_pos"]), c
        tot += _check_channel(o, c, want, int(ns[c]), P)
    assert tot[0] >= 60 * (B // 3) and tot[1] >= 12 * (B // 3) and tot[2] >= 9 * (B // 3), tot
    if B == 3:          # what was sent, from device arrays alone: the SMS of stream (a), the 823 bytes of stream (c)
        g0 = md.golden_streams()
        assert md.protocol_of(o["packet"][0, 0, :o["plen"][0, 0]]) == (0x05, "H") and o["pok"][0, 0] == 1
        assert o["pok"][1, 0] == 1 and o["plen"][1, 0] == 823 and np.array_equal(o["packet"][1, 0, :825], g0["sent_c_0"])


def test_one_packet_slot_counts_what_it_does_not_store(built):
    """stream (b) with max_packets = 1: the second packet is not stored, d_n_packets says 2, both EOF frames read status 7"""
    import orc
    from test_m17_gpu import _device_loop
    g0 = md.golden_streams()
    d = md.channel_dibits(g0, ("b",))
    x = orc.OracleFrontEnd(profile=2).run_cu8(md.modulate(d, seed=3), 8192)[None, :]
    g = _device_loop(x)
    o = _data_calls(g, 1, 1)
    out, fr, pk = md.stream_want(x[0])
    assert int(g["ns"].cpu().numpy()[0]) == len(fr) and len(pk) == 2
    assert int(o["np_"][0]) == 2 and [int(v) for v in o["pst"][0, :len(fr)] if v >= 6] == [7, 7]
    assert np.array_equal(o["packet"][0, 0, :25], g0["sent_b_0"]) and o["plen"][0, 0] == 23 and o["pok"][0, 0] == 1
    assert int(o["pslot"][0, 0]) == pk[0]["sync"]
    _check_channel(o, 0, (out, fr, pk), len(fr), 1)


def test_walk_on_made_up_frames(built):
    """ddn_m17_data_assemble_batch alone on frame arrays no air interface yields (metadata bytes with the low bits set, EOF values of 0
    and 26 .. 31, counters out of turn, positions either side of the carrier-loss count, EOT markers), 130 channels, two calls with the
    state carried: statuses, counts, receiver fields and packets = the restatement"""
    import torch
    l = ddn.lib()
    rng = np.random.default_rng(44)
    B, my, P, calls = 130, 48, 33, 2
    st = [md.DataState() for _ in range(B)]
    hunt = np.zeros(B, np.int64)
    state = torch.zeros((B, l.ddn_m17_data_state_bytes()), dtype=torch.uint8, device="cuda")
    seen = set()
    for call in range(calls):
        pat, pos = np.zeros((B, my), np.uint8), np.zeros((B, my), np.int32)
        p26, pf = rng.integers(0, 256, (B, my, 26)).astype(np.uint8), np.zeros((B, my), np.uint8)
        b25, bf = rng.integers(0, 256, (B, my, 25)).astype(np.uint8), np.zeros((B, my), np.uint8)
        b25[:, :, 24] &= 0xF8
        ns = rng.integers(my - 8, my + 1, B).astype(np.int32)
        adv = rng.integers(3000, 9000, B).astype(np.int32)
        want = [[] for _ in range(B)]
        done = [[] for _ in range(B)]
        for c in range(B):
            at = int(hunt[c])
            for k in range(int(ns[c])):
                r = rng.random()
                gap = int(rng.choice([0, 7, 1799, 1800, 1801, 2500])) if rng.random() < 0.15 else 7
                at += gap
                s = st[c]
                if at - int(hunt[c]) >= 1800:
                    s.carrier_loss()
                pos[c, k] = at
                cnt, status = s.pbc, 0
                if r < 0.05:
                    pat[c, k] = 2 + (c & 1)
                    s.eot()
                elif r < 0.10:
                    pat[c, k] = c & 1
                elif r < 0.25:
                    pat[c, k] = 6 + (c & 1)
                    bf[c, k] = rng.random() < 0.9
                    if bf[c, k]:
                        s.bert_frame(b25[c, k])
                else:
                    pat[c, k] = 10 + (c & 1)
                    pf[c, k] = rng.random() < 0.95
                    q = rng.random()
                    if q < 0.70:
                        p26[c, k, 25] = (s.pbc & 31) << 2                       # the counter in turn
                    elif q < 0.85:
                        p26[c, k, 25] = 0x80 | (int(rng.integers(0, 32)) << 2)  # EOF, any value
                    if pf[c, k]:
                        status, fin = s.packet_frame(p26[c, k])
                        if fin:
                            fin["sync"] = k
                            done[c].append(fin)
                want[c].append((status, cnt if pat[c, k] >= 10 and pf[c, k] else 0, s.rx.state() if pat[c, k] in (6, 7) and bf[c, k] else None))
                seen.add(status)
                hunt[c] = at + (8 if pat[c, k] < 2 else 184) + 1
                at = int(hunt[c])
            hunt[c] -= int(adv[c])
        t = lambda a: torch.from_numpy(a).cuda()
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
        d = dict(pat=t(pat), pos=t(pos), ns=t(ns), adv=t(adv), p26=t(p26), pf=t(pf), b25=t(b25), bf=t(bf))
        o = dict(pst=z((B, my), torch.uint8), pcnt=z((B, my), torch.uint8), bst=z((B, my, 8), torch.int32), packet=z((B, P, 832), torch.uint8),
                 plen=z((B, P), torch.int32), pok=z((B, P), torch.uint8), pslot=z((B, P), torch.int32), np_=z((B,), torch.int32))
        p = lambda v: v.data_ptr()
        assert l.ddn_m17_data_assemble_batch(p(d["pat"]), p(d["pos"]), p(d["ns"]), p(d["adv"]), B, my, p(d["p26"]), p(d["pf"]), p(d["b25"]),
                                             p(d["bf"]), p(state), p(o["pst"]), p(o["pcnt"]), p(o["bst"]), p(o["packet"]), p(o["plen"]),
                                             p(o["pok"]), p(o["pslot"]), p(o["np_"]), P, None) == 0, l.ddn_last_error()
        torch.cuda.synchronize()
        o = {k: v.cpu().numpy() for k, v in o.items()}
        for c in range(B):
            for k, (status, cnt, rx) in enumerate(want[c]):
                assert (int(o["pst"][c, k]), int(o["pcnt"][c, k])) == (status, cnt), (call, c, k)
                assert rx is None or o["bst"][c, k].tolist() == rx, (call, c, k)
            assert int(o["np_"][c]) == len(done[c])
            for j, q in enumerate(done[c][:P]):
                end = len(q["bytes"])
                assert np.array_equal(o["packet"][c, j, :end], q["bytes"]) and not o["packet"][c, j, end:].any(), (call, c, j)
                assert (int(o["plen"][c, j]), int(o["pok"][c, j]), int(o["pslot"][c, j])) == (q["app_len"], q["crc_ok"], q["sync"])
    assert {0, 1, 2, 3, 4, 6} <= seen
