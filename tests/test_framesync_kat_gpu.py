"""GPU: the reference's frame-sync known answers (tests/golden/framesync_vectors.json) in stream form on the device hunting loops -
the M17 matcher and the DMR word table of ddn_fsk4_rx (ddn_rx4.hip) and the CQPSK sync + map search of ddn_cq_rx (ddn_cqrx.hip).
Every case of a family is one channel of one batch (the DMR polarity is a batch setting: one batch per polarity).  Each channel equals
the CPU oracle bit for bit, and the device's own sync records give the known answer: sync type (pattern row), map index, and for M17
the levels behind the thresholds the preamble leaves.  The fsk4 loop runs under one and several channels per wave, and every call
split falls inside a tested word.  Why the answers carry over to this project's conditions: tests/test_oracle_framesync_kat.py."""
import numpy as np
import pytest

import ddn
import framesync_kat as fk
import orc
import rx4
from test_cqrx_gpu import check_channel as cq_check_channel
from test_cqrx_gpu import run_gpu_in_calls, run_oracle
from test_rx4_gpu import check_channel

pytestmark = pytest.mark.gpu

V = fk.vectors()


def _device_calls(rx, x, cuts):
    """x [B][n] through the device loop in calls split at the sample indices `cuts`; per call the host copies of its outputs and the
    thresholds every sync left (ddn_fsk4_rx_set_sync_thresholds)"""
    import torch
    l = ddn.lib()
    B = x.shape[0]
    outs = []
    for a, b in zip([0] + list(cuts), list(cuts) + [x.shape[1]]):
        n = b - a
        d = torch.from_numpy(np.ascontiguousarray(x[:, a:b])).cuda()
        ms, my = l.ddn_fsk4_rx_max_symbols(rx.h, n), l.ddn_fsk4_rx_max_syncs(rx.h, n)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
        rec, fl, pay = z((B, ms, 10), torch.uint8), z((B, ms), torch.uint8), z((B, ms, 2), torch.uint8)
        cnt, ns, spos = z((B,), torch.int32), z((B,), torch.int32), z((B, my), torch.int32)
        spat, pre, prel = z((B, my), torch.uint8), z((B, my, 90), torch.uint8), z((B, my, 90), torch.uint8)
        thr = z((B, my, 5), torch.float32)
        p = lambda t: t.data_ptr()
        assert l.ddn_fsk4_rx_set_sync_thresholds(rx.h, p(thr)) == 0
        assert l.ddn_fsk4_rx_run(rx.h, p(d), n, p(rec), p(fl), p(pay), p(cnt), ms, p(spos), p(spat), p(pre), p(prel), p(ns), my, None) == 0
        torch.cuda.synchronize()
        h = lambda t: t.cpu().numpy()
        outs.append(dict(rec=h(rec), fl=h(fl), pay=h(pay), cnt=h(cnt), n_sync=h(ns), sync_pos=h(spos), sync_pat=h(spat), pre=h(pre),
                         pre_rel=h(prel), thr=h(thr), my=my, a=a, b=b))
    assert l.ddn_fsk4_rx_set_sync_thresholds(rx.h, None) == 0
    return outs


def _run_family(cases, gpu_proto, prof_fn, cpw, handlers=False, inverted=0):
    """-> per channel: the syncs [(stream symbol index, pattern row)] and their thresholds, after the bit-exact check against the oracle"""
    n = max(len(c["sym"]) for c in cases) * fk.SPS
    x = np.zeros((len(cases), n), np.float32)
    for k, c in enumerate(cases):
        s = fk.samples(c["sym"])
        x[k, :len(s)] = s
        x[k, len(s):] = s[-1]                       # (the fill goes on: a constant level no word matches)
    cuts = sorted({c["word"][0] * fk.SPS + 45 for c in cases})    # inside every tested word
    rx = ddn.Fsk4Rx(len(cases), gpu_proto, inverted=inverted, handlers=handlers)
    assert ddn.lib().ddn_fsk4_rx_set_channels_per_wave(rx.h, cpw) == 0
    outs = _device_calls(rx, x, cuts)
    cpu = [rx4.OracleFsk4Rx(prof_fn()) for _ in cases]
    res = []
    for k in range(len(cases)):
        syncs, thr, base = [], [], 0
        for o in outs:
            want = cpu[k].run(x[k, o["a"]:o["b"]], max_sync=o["my"])
            check_channel(o, k, want)
            ns = int(o["n_sync"][k])
            assert np.array_equal(o["thr"][k, :ns].view(np.uint32), want["sync_thr"].view(np.uint32)), (cases[k]["label"], o["a"])
            syncs += [(base + int(p), int(q)) for p, q in zip(o["sync_pos"][k, :ns], o["sync_pat"][k, :ns])]
            thr += list(o["thr"][k, :ns])
            base += int(o["cnt"][k])
        res.append((syncs, thr))
    rx.close()
    return res


@pytest.mark.parametrize("cpw", [1, 4])
def test_m17_transitions_on_the_device(built, cpw):
    cases = fk.m17_cases(V)
    res = _run_family(cases, ddn.FSK4_M17, lambda: rx4.profile(rx4.PROTO_M17), cpw)
    for c, (syncs, thr) in zip(cases, res):
        assert syncs == c["syncs"], (c["label"], syncs)
        a, b = c["word"]
        assert [p for p, _ in syncs if a <= p <= b] == ([b] if c["expect"] >= 0 else []), c["label"]
        for (p, q), t in zip(syncs, thr):
            if q == rx4.M17_PRE_POS:
                # the KAT's short-window levels (min -1.5 / max +1.5 = half the ring's estimate from a cleared state) behind the
                # thresholds the preamble leaves: the warm start over the same eight symbols gives the estimate itself
                assert t[3] == 2 * V["m17_levels"]["max"] and t[4] == 2 * V["m17_levels"]["min"] and t[0] == 0.0, (c["label"], t)


@pytest.mark.parametrize("cpw", [1, 4])
def test_m17_one_error_preamble_on_the_device(built, cpw):
    t = V["m17_tolerance"]
    case = dict(label="one-error preamble", sym=fk.levels(t["pattern"] + "3" * 300), word=(0, 7))
    (syncs, _), = _run_family([case], ddn.FSK4_M17, lambda: rx4.profile(rx4.PROTO_M17), cpw)
    assert syncs == [(7, fk.m17_pat(t["expect"]))]


@pytest.mark.parametrize("cpw", [1, 4])
@pytest.mark.parametrize("inverted", [0, 1])
def test_dmr_rc_word_on_the_device(built, cpw, inverted):
    cases = fk.dmr_cases(inverted, V)
    res = _run_family(cases, ddn.FSK4_DMR, lambda: rx4.profile(rx4.PROTO_DMR, inverted=inverted), cpw, inverted=inverted)
    for c, (syncs, _) in zip(cases, res):
        assert syncs == c["syncs"], (c["label"], syncs)
        assert [q for _, q in syncs] == ([rx4.DMR_PAT_RC] if c["expect"] == V["sync_ids"]["DMR_RC_DATA"] else [])


@pytest.mark.parametrize("cpw", [1, 4])
def test_dmr_rc_word_with_the_handlers(built, cpw):
    """handler mode (handler = 1): the RC sync holds the configured 12 symbols, starts no burst decode, raises no event"""
    cases = fk.dmr_cases(0, V)
    res = _run_family(cases, ddn.FSK4_DMR, lambda: rx4.profile(rx4.PROTO_DMR, handler=1), cpw, handlers=True)
    for c, (syncs, _) in zip(cases, res):
        assert syncs == c["syncs"], (c["label"], syncs)


def test_cqpsk_sync_and_map_on_the_device(built):
    neg = V["cqpsk_neg"]
    for proto, gp, op in (("p25p2", ddn.CQ_P25P2, orc.CQ_P25P2), ("p25p1", ddn.CQ_P25P1, orc.CQ_P25P1)):
        cases = fk.cq_cases(proto, V)
        streams = [c["sym"] for c in cases]
        L = len(streams[0])
        rec, fl, ev = run_gpu_in_calls(streams, gp, cuts=((cases[0]["sync"] - 9.5) / L,))    # a call split inside the word
        for k, c in enumerate(cases):
            wr, wf, we = run_oracle(streams[k], op)
            cq_check_channel(rec[k], fl[k], ev[k], streams[k], wr, wf, we, c["label"])
            s = c["sync"]
            f = fl[k]
            assert np.flatnonzero(f & 2).tolist() == [s], c["label"]
            is_neg = c["expect"] in (V["sync_ids"]["P25P2_NEG"], V["sync_ids"]["P25P1_NEG"])
            assert (int(f[s]) >> 4) & 7 == c["map"] and bool(f[s] & 4) == is_neg, (c["label"], f[s])
            if c["expect"] == neg["synctype"] and c["map"] == neg["map"]:
                llr = rec[k][s + 1, 2:6].copy().view(np.int16)
                assert rec[k][s + 1, 0] == neg["dibit"] and (llr[0] > 0) == bool(neg["llr_bits"][0]) and (llr[1] > 0) == bool(neg["llr_bits"][1])
