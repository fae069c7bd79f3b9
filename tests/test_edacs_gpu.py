"""EDACS (-fh / -fH / -fe / -fE) on the device: DDN_FSK4_EDACS as the fsk4 loop's eighth protocol against the restated 9600_2 hunt
(tests/edacs_rx.c) bit for bit, and ddn_edacs_frame_decode_batch against tests/edacs.py field for field, on the reference's capture (as
sent: -EDACS words; I/Q swapped: +EDACS words) and on generated streams."""
import numpy as np
import pytest

import ddn
import edacs
import edacsgen
import orc
import rx4
from test_rx4_gpu import check_channel

pytestmark = pytest.mark.gpu


def _batch(disc, B):
    """copies of the capture: plain, negated (the +EDACS words), delayed behind noise, after silence"""
    n = len(disc)
    rng = np.random.default_rng(5)
    x = np.zeros((B, n), np.float32)
    for c in range(B):
        d = 29 * c
        x[c, :d] = rng.standard_normal(d) * 300
        x[c, d:] = disc[:n - d]
    x[1] = -x[1]
    if B > 3:
        x[3, :20000] = 0
    return x


def _check_loop(x, cuts, rf_mod=2, cpw=0):
    B = x.shape[0]
    gpu = ddn.Fsk4Rx(B, ddn.FSK4_EDACS, rf_mod=rf_mod, use_matched_filter=1)     # (ignored: EDACS has no matched filter)
    if cpw:
        assert ddn.lib().ddn_fsk4_rx_set_channels_per_wave(gpu.h, cpw) == 0
    cpu = [edacs.LoopRx(rf_mod) for _ in range(B)]
    pats = [[] for _ in range(B)]
    for a, b in zip(cuts[:-1], cuts[1:]):
        got = gpu.run_host(x[:, a:b])
        for c in range(B):
            want = cpu[c].run(x[c, a:b], max_sync=got["sync_pos"].shape[1])
            check_channel(got, c, want)
            pats[c] += want["sync_pat"].tolist()
            assert np.array_equal(gpu.thresholds(c).view(np.uint32), cpu[c].thresholds().view(np.uint32)), (c, a)
    gpu.close()
    return pats


@pytest.mark.parametrize("cpw", [0, 1, 4, 16])
@pytest.mark.parametrize("rf_mod", [2, 0])
def test_edacs_loop_bit_exact_on_the_capture_with_call_splits(built, cpw, rf_mod):
    disc = rx4.capture_disc("iq_edacs.npz", 3)
    x = _batch(disc, 4)
    n = x.shape[1]
    pats = _check_loop(x, [0, 4097, 4097 + 63, 30000, 30001, 61000, n], rf_mod, cpw)
    assert pats[0].count(edacs.PAT_NEG) >= 60 and edacs.PAT_POS not in pats[0]
    assert pats[1].count(edacs.PAT_POS) >= 60 and edacs.PAT_NEG not in pats[1]


def test_edacs_loop_bit_exact_on_generated_streams(built):
    """generated frames of both polarities in whole and ragged calls, at 48 and at 96 ksps (the straight passes of 10 samples)"""
    rng = np.random.default_rng(21)
    fe = orc.OracleFrontEnd(profile=3)
    rows = []
    for c in range(6):
        signs, _ = edacsgen.stream(rng, 30, c & 1, gap=(0, 60))
        iq = edacsgen.modulate_cu8(signs, 48000 * 2, lead=100 + 37 * c, seed=c)
        rows.append(fe.run_cu8(iq, 8192))
    x = np.stack(rows).astype(np.float32)
    pats = _check_loop(x, [0, 48000, x.shape[1]])
    assert all(len(p) >= 25 for p in pats), [len(p) for p in pats]
    rng2 = np.random.default_rng(3)
    cuts = np.sort(rng2.choice(np.arange(1, x.shape[1]), 9, replace=False)).tolist()
    _check_loop(x, [0] + cuts + [x.shape[1]], cpw=2)
    # 96 ksps: 10 samples per symbol (every sample repeated), where the loop's bulk passes run
    y = np.repeat(x, 2, axis=1)
    B = y.shape[0]
    gpu = ddn.Fsk4Rx(B, ddn.FSK4_EDACS, rf_mod=2, out_rate=96000)
    cpu = [edacs.LoopRx(2, out_rate=96000) for _ in range(B)]
    for a, b in ((0, 70001), (70001, y.shape[1])):
        got = gpu.run_host(y[:, a:b])
        for c in range(B):
            want = cpu[c].run(y[c, a:b], max_sync=got["sync_pos"].shape[1])
            check_channel(got, c, want)
    gpu.close()


def _device_loop(x, rf_mod=2):
    import torch
    l = ddn.lib()
    B, n = x.shape
    d = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    rx = ddn.Fsk4Rx(B, ddn.FSK4_EDACS, rf_mod=rf_mod)
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
    rx.close()
    return dict(rec=rec, cnt=cnt, ns=ns, spos=spos, spat=spat, thr=thr)


def _decode(o, ea_mode=0, esk_mask=0):
    import torch
    l = ddn.lib()
    B, my = o["spos"].shape
    z = lambda shape, dt=torch.uint8: torch.full(shape, 0x5A, dtype=dt, device="cuda")      # poison: every slot must be written
    raw, vote = z((B, my, 6), torch.int64), z((B, my, 2), torch.int64)
    bok, fok, msg, kind = z((B, my, 2)), z((B, my)), z((B, my, 2), torch.int32), z((B, my))
    types, site, valid = z((B, my, 3)), z((B, my, 6), torch.int32), z((B, my))
    p = lambda t: t.data_ptr()
    assert l.ddn_edacs_frame_decode_batch(p(o["rec"]), o["rec"].shape[1], p(o["cnt"]), p(o["spos"]), p(o["spat"]), p(o["ns"]), p(o["thr"]),
                                          B, my, ea_mode, esk_mask, p(raw), p(vote), p(bok), p(fok), p(msg), p(kind), p(types), p(site),
                                          p(valid), None) == 0
    torch.cuda.synchronize()
    h = lambda t: t.cpu().numpy()
    return dict(raw40=h(raw).view(np.uint64), vote40=h(vote).view(np.uint64), bch_ok=h(bok), frame_ok=h(fok), msg28=h(msg).view(np.uint32),
                kind=h(kind), types=h(types), site6=h(site), valid=h(valid))


def _check_slots(o, got, ea_mode=0, esk_mask=0):
    """every slot of every channel against the restatement on the same records and thresholds -> the decoded slots"""
    rec, cnt, ns = o["rec"].cpu().numpy(), o["cnt"].cpu().numpy(), o["ns"].cpu().numpy()
    spos, spat, thr = o["spos"].cpu().numpy(), o["spat"].cpu().numpy(), o["thr"].cpu().numpy()
    B, my = spos.shape
    out = [[] for _ in range(B)]
    for c in range(B):
        sym = rec[c, :int(cnt[c]), 6:10].copy().view(np.float32).reshape(-1)
        for k in range(my):
            if k < ns[c]:
                want = edacs.decode_slot(sym, int(spos[c, k]), int(spat[c, k]), thr[c, k], ea_mode, esk_mask)
            else:
                want = edacs.decode_slot(sym, -1, 0, thr[c, k])
            for key, v in want.items():
                assert np.array_equal(np.asarray(got[key][c, k]).astype(np.int64).reshape(-1),
                                      np.asarray(v, dtype=np.uint64).astype(np.int64).reshape(-1)), (c, k, key)
            if want["valid"]:
                out[c].append(want)
    return out


@pytest.mark.parametrize("mode", sorted(edacs.MODES))
def test_edacs_kernel_on_the_capture(built, mode):
    """DECODE_IQ_EDACS (tests/CMakeLists.txt:8958-8963): every frame BCH-good and under -fh a standard site ID 2, "Site ID [02][002]",
    on plain, negated and delayed copies; every mode field for field with the restatement"""
    ea, esk = edacs.MODES[mode]
    disc = rx4.capture_disc("iq_edacs.npz", 3)
    o = _device_loop(_batch(disc, 3))
    frames = _check_slots(o, _decode(o, ea, esk), ea, esk)
    for c in range(3):
        assert len(frames[c]) >= 60 and all(f["frame_ok"] for f in frames[c]), c
        if mode == "-fh":
            sites = {edacs.site_line(f["site6"][0]) for f in frames[c] if f["kind"] == 3}
            assert sites == {"Site ID [02][002]"}, (c, sites)


@pytest.mark.parametrize("mode", sorted(edacs.MODES))
def test_edacs_kernel_on_generated_frames(built, mode):
    """generated frames come back exactly under every mode; an error in one copy of a bit is voted out; errors in two copies of the same
    bit fail the BCH check"""
    ea, esk = edacs.MODES[mode]
    rng = np.random.default_rng(7 + ea * 2 + (esk != 0))
    fe = orc.OracleFrontEnd(profile=3)
    B, F = 4, 24
    sent, rows = [], []
    for c in range(B):
        pat = c & 1
        msgs, frames = [], []
        for k in range(F):
            m1 = (edacsgen.ea_site_id_msg(int(rng.integers(0, 256)), int(rng.integers(0, 128)), esk) if ea else
                  edacsgen.site_id_msg(int(rng.integers(0, 32)), int(rng.integers(0, 8)), int(rng.integers(0, 32)), esk_mask=esk)) \
                if k % 3 == 0 else int(rng.integers(0, 1 << 28))
            m2 = int(rng.integers(0, 1 << 28))
            kind = k % 3                       # 0 clean, 1 one bad copy per bit position, 2 two bad copies of one bit
            flips = []
            if kind == 1:
                for h in range(2):
                    flips += [(3 * h + int(rng.integers(0, 3)), int(b)) for b in rng.choice(40, 6, replace=False)]
            elif kind == 2:
                h, b = int(rng.integers(0, 2)), int(rng.integers(0, 40))
                flips = [(3 * h, b), (3 * h + 1, b)]
            msgs.append((m1, m2, kind))
            frames.append(edacsgen.symbols(edacsgen.frame_bits(m1, m2, flips), pat))
            frames.append(np.tile(np.array([1, -1], np.int8), 8))
        signs = np.concatenate(frames)
        rows.append(fe.run_cu8(edacsgen.modulate_cu8(signs, len(signs) * 5 + 1000, lead=300 + 11 * c, seed=c), 8192))
        sent.append(msgs)
    o = _device_loop(np.stack(rows).astype(np.float32))
    frames = _check_slots(o, _decode(o, ea, esk), ea, esk)
    for c in range(B):
        assert len(frames[c]) == F, (c, len(frames[c]))
        for f, (m1, m2, kind) in zip(frames[c], sent[c]):
            if kind == 2:
                assert not f["frame_ok"] and f["kind"] == 0
                continue
            assert f["frame_ok"] and f["vote40"] == [edacs.bch(m1), edacs.bch(m2)]
            assert f["msg28"] == [m1 ^ (esk << 20), m2 ^ (esk << 20)]
        for k in range(0, F, 3):                  # the site-ID frames
            assert frames[c][k]["kind"] == (4 if ea else 3), (c, k)
